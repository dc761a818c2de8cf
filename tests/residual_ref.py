"""The contract of xgpu_batch_residual (include/xevd_hip.h) restated in numpy: from the SoA arrays of a CU batch and a residual
arena (the CPU oracle's, cases.run_cpu) to the three picture-shaped planes, and from those to every output form.  Test infrastructure only."""
import numpy as np

MODE_INTRA, MODE_IBC = 0, 6


def ats_inter_of(batch, i):
    """ats_inter_info of CU i as the backend reads it: of an inter CU only (idx | pos << 4), else 0"""
    if batch.get("ats_inter") is None or int(batch["pred_mode"][i]) in (MODE_INTRA, MODE_IBC):
        return 0
    return int(batch["ats_inter"][i])


def tu_rect(w, h, ai):
    """the coded TU inside a w x h CU -> (x, y, w, h): the CU, or one half (idx 1 vertical split, 2 horizontal) or quarter (3, 4) of it, at its start (pos 0)
    or end (pos 1)"""
    idx, pos = ai & 15, ai >> 4
    if idx in (1, 3):
        tw = w >> (2 if idx == 3 else 1)
        return (w - tw if pos else 0), 0, tw, h
    if idx in (2, 4):
        th = h >> (2 if idx == 4 else 1)
        return 0, (h - th if pos else 0), w, th
    return 0, 0, w, h


def planes(batch, arena, width, height):
    """-> [Y (height x width), Cb, Cr (height / 2 x width / 2)] int16: r(c, x, y), 0 where nothing is coded.  Per CU, in order Y, Cb, Cr, a component block is
    in the arena only with its cbf bit, row stride = the block's width; the block of an ATS-inter CU is its TU.  Inside a local dual tree luma comes from the
    luma-only CUs (tree 1) and chroma from the chroma-only CU (tree 2): their cbf bits say so by themselves (a luma-only CU has no chroma bit, a chroma-only
    CU no luma bit)."""
    arena = np.asarray(arena, np.int16)
    out = [np.zeros((height, width), np.int16), np.zeros((height // 2, width // 2), np.int16), np.zeros((height // 2, width // 2), np.int16)]
    tree, cbf_sub = batch.get("tree"), batch.get("cbf_sub")
    for i in range(len(batch["x"])):
        x, y, w, h = int(batch["x"][i]), int(batch["y"][i]), 1 << int(batch["log2w"][i]), 1 << int(batch["log2h"][i])
        cbf = int(batch["cbf"][i]) & 7
        if tree is not None:
            assert not (tree[i] == 1 and cbf & 6) and not (tree[i] == 2 and cbf & 1)
        tx, ty, tw, th = tu_rect(w, h, ats_inter_of(batch, i))
        off = int(batch["coef_off"][i])
        for c in range(3):
            if not (cbf >> c) & 1:
                continue
            s = 1 if c else 0
            bw, bh = tw >> s, th >> s
            blk = arena[off:off + bw * bh].reshape(bh, bw).copy()
            off += bw * bh
            if (w > 64 or h > 64) and cbf_sub is not None:      # 64x64 (chroma 32x32) sub-blocks without coefficients hold nothing
                for sb in range(4):
                    si, sj = sb & 1, sb >> 1
                    if si * 64 >= w or sj * 64 >= h:
                        continue
                    if not (int(cbf_sub[i]) >> (4 * c + sb)) & 1:
                        blk[(sj * 64) >> s:(sj * 64 + 64) >> s, (si * 64) >> s:(si * 64 + 64) >> s] = 0
            out[c][(y + ty) >> s:(y + ty + th) >> s, (x + tx) >> s:(x + tx + tw) >> s] = blk
    return out


def yuv420(pl, crop=(0, 0, 0, 0)):
    """XGPU_RESID_YUV420, tight: the flat int16 array Y, Cb, Cr of the cropped picture"""
    cl, cr, ct, cb = crop
    h, w = pl[0].shape
    return np.concatenate([pl[0][ct:h - cb, cl:w - cr].ravel(), pl[1][ct // 2:(h - cb) // 2, cl // 2:(w - cr) // 2].ravel(),
                           pl[2][ct // 2:(h - cb) // 2, cl // 2:(w - cr) // 2].ravel()])


def f444(pl, bd_luma, bd_chroma, crop=(0, 0, 0, 0), dtype=np.int16, interleaved=False):
    """XGPU_RESID_444_*: [3, H, W] (interleaved: [H, W, 3]), chroma replicated c[(y + crop_top) >> 1][(x + crop_left) >> 1]; int16: the value; float32:
    float32(r) * 2^-B; float16: that rounded to nearest even"""
    cl, cr, ct, cb = crop
    h, w = pl[0].shape
    yy, xx = np.arange(ct, h - cb), np.arange(cl, w - cr)
    full = [pl[0][yy][:, xx], pl[1][yy >> 1][:, xx >> 1], pl[2][yy >> 1][:, xx >> 1]]
    if np.dtype(dtype) == np.int16:
        out = np.stack(full)
    else:
        scale = [np.float32(2.0 ** -bd_luma), np.float32(2.0 ** -bd_chroma), np.float32(2.0 ** -bd_chroma)]
        out = np.stack([(p.astype(np.float32) * s).astype(np.float32) for p, s in zip(full, scale)]).astype(dtype)
    return np.ascontiguousarray(out.transpose(1, 2, 0)) if interleaved else out


def energy(pl):
    """XGPU_RESID_ENERGY: [3, h_scu, w_scu] float32 - sum |r| over the unit's 4x4 luma samples, and over its 2x2 Cb and Cr samples"""
    h, w = pl[0].shape
    a = [np.abs(p.astype(np.int64)) for p in pl]
    return np.stack([a[0].reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3)), a[1].reshape(h // 4, 2, w // 4, 2).sum(axis=(1, 3)),
                     a[2].reshape(h // 4, 2, w // 4, 2).sum(axis=(1, 3))]).astype(np.float32)


def bits(a):
    """the bit patterns of a float array (so that +0.0 and -0.0 compare unequal)"""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
