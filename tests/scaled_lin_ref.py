"""numpy restatement of the scaled output filtered in linear light (include/xevd_hip.h xgpu_pic_output_device_scaled_lin / _rois_lin),
in float32, one rounded operation at a time.  Written from the contract, not from the kernel:

The source is the picture minus the crop (for the batch: the rectangle), Ws x Hs luma samples; nothing outside it reaches a result.
1. per source pixel at luma resolution: every sample DRA-mapped (where dra is given) and clipped to [0, 2^B - 1]; chroma upsampled on the source's own chroma
   plane, edge-clamped there - "nearest", or "linear" with chroma_loc's quarter weights and (sum + 8) >> 4 (colour_ref.upsample); the integer R'G'B' code at the
   coding depth by the U16 form's matrix (colour_ref.ycbcr_to_rgb); L_c = lin[code_c], float32.
2. vertical pass, the luma row table (xgpu_scale_taps, subsampling 1, siting 0) for all three channels: T_c(x, o) = sum over k ascending of
   float32(qy[o][k]) * L_c(x, first[o] + k); the accumulator starts as the first product, every multiply and every add rounded to float32 on its own.
3. horizontal pass, the luma column table: V_c(ox, o) = (sum over k ascending of float32(qx[ox][k]) * T_c(first[ox] + k, o)) * 2^-28, rounded the same way.
4. (V_R, V_G, V_B) take the place of the three lin[...] values of the colour transform (colour_cm_ref.transform), and its steps from the
   primaries matrix on run unchanged; integers rint(q * (2^D - 1)), floats q; then bgr and the scaled output's normalise (scale_ref.normalise).
5. batch: image i of a stretched batch is the single call with the crop set to rectangle i; with letterbox the inner part and the pad follow roi_ref - the pad is
   a value of the destination space, normalised and never transformed.
The tap loops are explicit: np.sum sums pairwise."""
import numpy as np

import colour_cm_ref as cmr
import colour_ref as cr
import roi_ref
import scale_ref as sr

U8, U16 = sr.U8, sr.U16
STRETCH, LETTERBOX = roi_ref.STRETCH, roi_ref.LETTERBOX


def rgb_codes(planes, bd, matrix=1, full_range=False, chroma_loc=0, upsample="linear", crop=(0, 0, 0, 0), dra=None):
    """step 1 up to the code: decoded [Y, U, V] of the whole picture -> [3][Hs][Ws] int64 R'G'B' codes at the coding depth"""
    planes = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        planes = cr.dra_apply(planes, dra)
    y, u, v = (np.clip(p, 0, (1 << bd) - 1) for p in cr.crop_planes(planes, crop))
    h, w = y.shape
    return cr.ycbcr_to_rgb(y, cr.upsample(u, w, h, upsample, chroma_loc), cr.upsample(v, w, h, upsample, chroma_loc), bd, matrix, full_range, U16).astype(np.int64)


def vertical(lin, rows):
    """lin [Hs][Ws] float32 -> T [Hd][Ws]"""
    out = np.empty((len(rows), lin.shape[1]), np.float32)
    for o, (first, q) in enumerate(rows):
        acc = np.float32(q[0]) * lin[first]
        for k in range(1, len(q)):
            acc = acc + np.float32(q[k]) * lin[first + k]
        out[o] = acc
    return out


def horizontal(mid, rows):
    """T [Hd][Ws] float32 -> V [Hd][Wd]"""
    out = np.empty((mid.shape[0], len(rows)), np.float32)
    for o, (first, q) in enumerate(rows):
        acc = np.float32(q[0]) * mid[:, first]
        for k in range(1, len(q)):
            acc = acc + np.float32(q[k]) * mid[:, first + k]
        out[:, o] = acc * np.float32(2.0 ** -28)
    return out


def filtered_linear(codes, size, tab, filt=sr.BILINEAR, lib=None):
    """steps 1 (the lookup) to 3: codes [3][Hs][Ws] -> V [3][Hd][Wd] float32"""
    hs, ws = codes.shape[1:]
    yl, _, xl, _ = sr.make_tables(ws, hs, size[1], size[0], filt, 0, lib)
    lin = np.asarray(tab["lin"], np.float32)
    return np.stack([horizontal(vertical(lin[codes[c]], yl), xl) for c in range(3)])


def from_linear(e, tab, dtype, bd):
    """step 4's transform: linear light of the source primaries [3, ...] float32 -> uint8 / uint16, or float32 before any f16 / bf16 rounding.  The lines of
    colour_cm_ref.transform behind its lookup, on its own helpers."""
    e = [np.asarray(c, np.float32) for c in e]
    p = [cmr._dot(tab["matrix"][r], e) for r in range(3)] if tab["use_matrix"] else e
    if tab["tone"] is not None:
        yl = cmr.clip01(cmr._dot(tab["luma"], e))
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(yl > 0, cmr.curve_eval(tab["tone"], yl) / np.where(yl > 0, yl, np.float32(1)), np.float32(0)).astype(np.float32)
    else:
        s = np.float32(tab["scale"])
    out = []
    for c in range(3):
        q = cmr.clip01((p[c] * s).astype(np.float32))
        if tab["encode"] is not None:
            q = cmr.curve_eval(tab["encode"], q)
        if dtype in (U8, U16):
            m = np.float32((1 << cr.out_depth(dtype, bd)) - 1)
            q = np.rint((q * m).astype(np.float32)).astype(np.uint8 if dtype == U8 else np.uint16)
        out.append(q)
    return np.stack(out)


def finish(v, bd, tab, dtype=U8, bgr=False, mean=None, inv_std=None):
    """step 4, for V that filtered_linear has made (a test that wants several dtypes of one size filters once)"""
    out = from_linear(v, tab, dtype, bd)
    if bgr:
        out = out[::-1]
    if mean is not None or inv_std is not None:
        assert dtype not in (U8, U16)
        out = sr.normalise(out, np.zeros(3, np.float32) if mean is None else mean, np.ones(3, np.float32) if inv_std is None else inv_std)
    return np.ascontiguousarray(out)


def convert(planes, bd, size, tab, filt=sr.BILINEAR, matrix=1, full_range=False, chroma_loc=0, upsample="linear", dtype=U8, crop=(0, 0, 0, 0), dra=None,
            bgr=False, mean=None, inv_std=None, lib=None):
    """decoded [Y, U, V] of the whole picture through tables `tab` (abi.colour_tables) -> [3][Hd][Wd] in output channel order: uint8 / uint16 for the integer
    dtypes, float32 (before any f16 / bf16 rounding) otherwise"""
    codes = rgb_codes(planes, bd, matrix, full_range, chroma_loc, upsample, crop, dra)
    return finish(filtered_linear(codes, size, tab, filt, lib), bd, tab, dtype, bgr, mean, inv_std)


def batch(planes, bd, size, rois, tab, fit=STRETCH, pad=0.0, crop=(0, 0, 0, 0), dtype=U8, mean=None, inv_std=None, **kw):
    """-> [N][3][Hd][Wd]; rois: (x, y, w, h) inside the picture minus crop; the pad value is roi_ref's - a value of the destination space, never transformed"""
    hd, wd = size
    h, w = np.asarray(planes[0]).shape
    fill = roi_ref.pad_elements(pad, dtype, mean, inv_std)
    out = []
    for x, y, rw, rh in rois:
        ix, iy, wi, hi = roi_ref.inner(rw, rh, wd, hd, fit)
        rect = (crop[0] + x, w - crop[0] - x - rw, crop[2] + y, h - crop[2] - y - rh)      # the rectangle as a crop of the whole picture
        part = convert(planes, bd, (hi, wi), tab, dtype=dtype, crop=rect, mean=mean, inv_std=inv_std, **kw)
        img = np.empty((3, hd, wd), part.dtype)
        img[:] = fill.astype(part.dtype).reshape(3, 1, 1)
        img[:, iy:iy + hi, ix:ix + wi] = part
        out.append(img)
    return np.stack(out)
