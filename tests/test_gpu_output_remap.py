"""GPU suite for xgpu_pic_output_device_remap / XgpuDecoder.pic_output_remapped / StreamDecoder.pictures(remap=): N coordinate grids of one picture - one node
per pixel, or a mesh with a node every 2^k pixels - as a batch of images from one launch, against the restatement of the contract (tests/remap_ref.py), against
the warped output (an affine grid is the warp, bit for bit) and against the plain output where those two agree.  Every comparison is bit for bit, with the
conventions of test_gpu_output_scaled.py."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_io
import remap_ref as mr
import test_gpu_output_scaled as ts
import test_gpu_output_warp as tw
import warp_ref as wr
from test_gpu_output_rois import check_batch
from xevd_amd import abi

pytestmark = pytest.mark.gpu

W, H = 320, 200
SIZE = (48, 64)
SIZES = ((48, 64), (50, 70), (2, 2), (5, 65), (9, 129))      # across the 64-column tile, a height that is no multiple of 4, (dw - 1) >> k changing at 64 | 65, 128 | 129
MEAN, STD, NORM = tw.MEAN, tw.STD, tw.NORM
Q = 65536
TRIPLES = tw.TRIPLES
INV, I32_MAX = mr.INVALID, (1 << 31) - 1


def lens_for(size, ws=W, hs=H):
    """a barrel lens whose undistorted view of size (H, W) covers most of a ws x hs picture"""
    hd, wd = size
    return dict(fx=ws * 0.9, fy=ws * 0.9, cx=ws / 2 - 0.3, cy=hs / 2 + 0.2, k1=-0.28, k2=0.09, p1=0.002, p2=-0.0015, k3=-0.01,
                nfx=wd * 0.8, nfy=ws * 0.8 * hd / hs, ncx=(wd - 1) / 2, ncy=(hd - 1) / 2)


def make_grids(lib, size, k, seed, ws=W, hs=H):
    """-> (int32 grids [5, gh, gw, 2], float32 grids [6, gh, gw, 2]): a smooth lens mesh; the same plus noise of a few samples; a mesh that leaves the picture
    on all four sides; a grid of extremes; a grid with invalid nodes, single ones and a full row; for float32 also NaN, +-inf, +-1e30 and -0.0"""
    rng = np.random.default_rng(seed)
    (gh, gw), (hd, wd) = mr.grid_dims(size, k), size
    lens = abi.remap_from_lens(lib, lens_for(size, ws, hs), size, k)
    assert lens.shape == (gh, gw, 2) and (lens != INV).all()
    noisy = (lens.astype(np.int64) + rng.integers(-3 * Q, 3 * Q + 1, lens.shape)).astype(np.int32)
    ox, oy = np.meshgrid(np.arange(gw, dtype=np.int64) << k, np.arange(gh, dtype=np.int64) << k)      # 20 samples beyond the picture at the image's four edges
    leaves = np.stack([-20 * Q + ox * ((ws + 39) * Q // (wd - 1)) + oy * 2000, -15 * Q - ox * 1300 + oy * ((hs + 29) * Q // (hd - 1))], axis=-1).astype(np.int32)
    edge = [INV + 1, I32_MAX, 0, -1, 127, -129, ((ws - 1) << 16) - 1, (ws - 1) << 16, ((ws - 1) << 16) + 128, ((ws - 1) << 16) + 127, ((hs - 1) << 16) - 129,
            (hs - 1) << 16, ((hs - 1) << 16) + 128, (ws - 2) << 16, ((hs - 2) << 16) + 32768]
    extremes = rng.choice(np.asarray(edge, np.int64), size=lens.shape).astype(np.int32)
    holes = noisy.copy()
    for _ in range(max(1, gh * gw // 40)):
        holes[rng.integers(gh), rng.integers(gw), rng.integers(2)] = INV
    holes[gh // 2, :, rng.integers(2)] = INV
    if gh * gw <= 4:      # leave at least one valid node in the smallest grids
        holes = noisy.copy()
        holes[0, 0, 0] = INV
    i32 = np.stack([lens, noisy, leaves, extremes, holes])
    f32 = (i32.astype(np.float64) / 65536).astype(np.float32)
    f32[3] = rng.choice(np.asarray([-1e30, 1e30, 0.0, -0.0, ws - 1 - 2.0 ** -9, ws - 1 + 2.0 ** -9, ws - 1, hs - 1, hs - 1 + 0.002, 32767.5, -32768.0, 1e-40,
                                    0.5 / 65536, -1.5 / 65536], np.float32), size=lens.shape)
    f32[4][(holes == INV).any(axis=-1)] = np.nan
    special = f32[1].copy()
    flat = special.reshape(-1)
    vals = np.asarray([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0], np.float32)
    for n, at in enumerate(rng.choice(flat.size, size=min(flat.size, max(2, flat.size // 20)), replace=False)):
        flat[at] = vals[n % len(vals)]
    return i32, np.concatenate([f32, special[None]])


def run(dec, pic, planes, bd, grids, size, k, layout="rgb", code=abi.OUT_U8, channels_last=False, normalise=False, samples=1, border="clamp", pad=None, what="", **kw):
    """one batch and its comparison with the restatement; kw: matrix, full_range, chroma_loc, crop, dra, bgr"""
    if pad is None:
        pad = (17, 0, 200) if code in (abi.OUT_U8, abi.OUT_U16) else (0.25, -0.5, 0.447)
    norm = dict(mean=MEAN, std=STD) if normalise else {}
    t = dec.pic_output_remapped(pic, grids, size, step=k, layout=layout, channels_last=channels_last, dtype=ts.torch_dtype(code), samples=samples, border=border,
                                pad=pad, **norm, **kw)
    assert tuple(t.shape) == ((len(grids), *size, 3) if channels_last else (len(grids), 3, *size))
    exp = mr.batch(planes, bd, size, grids, k, samples, mr.PAD if border == "pad" else mr.CLAMP, pad, layout=layout, dtype=code, **(NORM if normalise else {}), **kw)
    check_batch(t, exp, code, channels_last, what or (str(grids.dtype), size, k, layout, code, channels_last, normalise, samples, border, kw))
    return t


@pytest.mark.parametrize("k", [0, 1, 4, 6])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_restatement(bd, k):
    planes = ts.random_planes(W, H, bd, seed=800 + bd, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        for grids in make_grids(dec.lib, SIZE, k, 810 + k):
            assert len(grids) == (5 if grids.dtype == np.int32 else 6)
            for samples in (1, 2, 4):
                for border in ("clamp", "pad"):
                    for layout, code, normalise in TRIPLES:
                        run(dec, pic, planes, bd, grids, SIZE, k, layout=layout, code=code, normalise=normalise, samples=samples, border=border)
        for size in SIZES[1:]:
            for grids in make_grids(dec.lib, size, k, 820 + k + size[1]):
                for samples, border, (layout, code, normalise) in ((1, "pad", TRIPLES[0]), (2, "clamp", TRIPLES[1]), (4, "pad", TRIPLES[2]), (4, "clamp", TRIPLES[0])):
                    run(dec, pic, planes, bd, grids, size, k, layout=layout, code=code, normalise=normalise, samples=samples, border=border)
    finally:
        dec.close()


def test_an_affine_grid_is_the_warp_bit_for_bit():
    """the interpolation of an affine function is exact and the derivatives are the map's linear part: xgpu_remap_from_warp of the warp test's maps, all of which
    stay inside +-32767 samples at every node, gives pic_output_warped's batch at every step and S"""
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=831, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        for k in (0, 3, 6):
            grids = np.stack([abi.remap_from_warp(dec.lib, m, SIZE, k) for m in tw.MAPS])
            assert int(np.abs(grids.astype(np.int64)).max()) < 32767 << 16
            for samples in (1, 2, 4):
                for border in ("clamp", "pad"):
                    for code in (abi.OUT_U8, abi.OUT_U16, abi.OUT_F32):
                        pad = (17, 0, 200) if code != abi.OUT_F32 else (0.25, -0.5, 0.447)
                        kw = dict(dtype=ts.torch_dtype(code), samples=samples, border=border, pad=pad)
                        a = dec.pic_output_remapped(pic, grids, SIZE, step=k, **kw)
                        b = dec.pic_output_warped(pic, tw.maps_array(), SIZE, **kw)
                        assert np.array_equal(ts.tensor_bits(a, code), ts.tensor_bits(b, code)), (k, samples, border, code)
    finally:
        dec.close()


def test_the_identity_grid_is_the_plain_output():
    import torch
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=833, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        for k in (0, 4):
            grid = torch.from_numpy(abi.remap_from_warp(dec.lib, wr.IDENTITY, (H, W), k)).to("cuda:0")
            for loc in range(6):
                for layout, code in (("yuv444", abi.OUT_U16), ("rgb", abi.OUT_U8)):
                    t = dec.pic_output_remapped(pic, grid, (H, W), step=k, layout=layout, dtype=ts.torch_dtype(code), chroma_loc=loc)
                    plain = dec.pic_output_tensor(pic, layout=layout, dtype=ts.torch_dtype(code), upsample="linear", chroma_loc=loc)
                    warped = dec.pic_output_warped(pic, tw.maps_array([wr.IDENTITY]), (H, W), layout=layout, dtype=ts.torch_dtype(code), chroma_loc=loc)
                    torch.cuda.synchronize()
                    assert torch.equal(t[0], plain) and torch.equal(t, warped), (k, layout, code, loc)
            # the same grid in float32
            t = dec.pic_output_remapped(pic, (grid.to(torch.float64) / 65536).to(torch.float32), (H, W), step=k, dtype=torch.uint8)
            plain = dec.pic_output_tensor(pic, dtype=torch.uint8, upsample="linear")
            torch.cuda.synchronize()
            assert torch.equal(t[0], plain), k
    finally:
        dec.close()


def test_layouts_dtypes_sitings_and_dra():
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=835, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        i32, f32 = make_grids(dec.lib, SIZE, 3, 836)
        run(dec, pic, planes, bd, i32, SIZE, 3, layout="rgb", code=abi.OUT_F16, channels_last=True, normalise=True, samples=2, border="pad", bgr=True)
        run(dec, pic, planes, bd, f32, SIZE, 3, layout="yuv444", code=abi.OUT_BF16, channels_last=False, samples=1, border="pad", full_range=True)
        run(dec, pic, planes, bd, i32, SIZE, 3, layout="yuv444", code=abi.OUT_U8, channels_last=True, samples=4)
        run(dec, pic, planes, bd, f32, SIZE, 3, layout="rgb", code=abi.OUT_U16, channels_last=True, samples=1, border="pad", matrix=9, full_range=True, pad=(0, 1023, 512))
        for loc in range(6):
            crop = (2 * loc, 4, 6, 2 * loc)
            g = make_grids(dec.lib, SIZE, loc, 840 + loc, W - crop[0] - crop[1], H - crop[2] - crop[3])[loc & 1]
            run(dec, pic, planes, bd, g, SIZE, loc, layout="yuv444", code=abi.OUT_U16, samples=1 + (loc & 1), chroma_loc=loc, crop=crop)
    finally:
        dec.close()
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    h, w = planes[0].shape
    dec, pic = ts.open_picture(planes, 10)
    try:
        luts = d["three_ranges_idx58_luts"]
        i32, f32 = make_grids(dec.lib, SIZE, 2, 847, w, h)
        run(dec, pic, planes, 10, i32, SIZE, 2, layout="yuv444", code=abi.OUT_U16, samples=2, dra=luts, what="dra yuv444")
        i32, f32 = make_grids(dec.lib, SIZE, 0, 848, w - 6, h - 2)
        run(dec, pic, planes, 10, f32, SIZE, 0, code=abi.OUT_F32, normalise=True, samples=1, border="pad", dra=luts, matrix=9, crop=(2, 4, 0, 2), what="dra rgb")
    finally:
        dec.close()


def test_the_crop_is_a_wall():
    bd = 10
    crop = (16, 24, 8, 12)
    a = ts.random_planes(W, H, bd, seed=851, rails=True)
    b = ts.random_planes(W, H, bd, seed=852)
    for pa, pb, s in zip(a, b, (1, 2, 2)):      # the same samples inside the crop, others everywhere else
        hh, ww = pa.shape
        pb[crop[2] // s:hh - crop[3] // s, crop[0] // s:ww - crop[1] // s] = pa[crop[2] // s:hh - crop[3] // s, crop[0] // s:ww - crop[1] // s]
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    ws, hs = W - crop[0] - crop[1], H - crop[2] - crop[3]
    got = []
    for planes in (a, b):
        dec, pic = ts.open_picture(planes, bd)
        try:
            for k, samples, (layout, code) in ((4, 1, ("yuv444", abi.OUT_U16)), (0, 4, ("rgb", abi.OUT_U8))):
                grids = make_grids(dec.lib, SIZE, k, 853 + k, ws, hs)[0]      # among them the mesh that leaves the source on all four sides, and the extremes
                t = run(dec, pic, planes, bd, grids, SIZE, k, layout=layout, code=code, samples=samples, border="clamp", crop=crop, chroma_loc=1)
                got.append(t.cpu().numpy())
        finally:
            dec.close()
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])


def test_out_with_batch_stride_padded_rows_and_a_grid_pitch():
    import torch
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=857)
    dec, pic = ts.open_picture(planes, bd)
    hd, wd = SIZE
    try:
        for cl, code, off, k, fmt in ((False, abi.OUT_U8, 7, 4, 0), (False, abi.OUT_F32, 3, 0, 1), (True, abi.OUT_F16, 5, 1, 0)):
            grids = make_grids(dec.lib, SIZE, k, 858 + k)[fmt]
            n, (gh, gw) = len(grids), mr.grid_dims(SIZE, k)
            # the grids a pitch above tight apart, behind an offset that keeps them 8-byte aligned; canaries in every gap
            one, gstride, goff = gh * gw * 2, gh * gw * 2 + 6, 4
            canary = 0x5A5A5A5A if fmt == 0 else float(np.float32(-7.25))
            gbuf = torch.full((goff + n * gstride + 10,), canary, dtype=torch.int32 if fmt == 0 else torch.float32, device="cuda:0")
            gview = torch.as_strided(gbuf, (n, gh, gw, 2), (gstride, gw * 2, 2, 1), goff)
            gview.copy_(torch.from_numpy(grids))
            before = gbuf.clone()
            dt = ts.torch_dtype(code)
            fill = 0xA5 if code == abi.OUT_U8 else -3.0
            pad = 9 if code == abi.OUT_U8 else 0.5
            pitch = (3 * wd if cl else wd) + 13                       # elements between rows
            image = (hd if cl else 3 * hd) * pitch
            stride = image + 37                                       # elements between images
            buf = torch.full((off + n * stride + 11,), fill, dtype=dt, device="cuda:0")
            view = torch.as_strided(buf, (n, hd, wd, 3) if cl else (n, 3, hd, wd), (stride, pitch, 3, 1) if cl else (stride, hd * pitch, pitch, 1), off)
            out = dec.pic_output_remapped(pic, gview, SIZE, step=k, channels_last=cl, dtype=dt, samples=2, border="pad", pad=pad, out=view)
            assert out is view
            check_batch(view, mr.batch(planes, bd, SIZE, grids, k, 2, mr.PAD, pad, dtype=code), code, cl, ("out", cl, code, k))
            untouched = torch.ones(buf.numel(), dtype=torch.bool, device="cuda:0")
            torch.as_strided(untouched, view.shape, view.stride(), off).fill_(False)
            assert int(untouched.sum()) == buf.numel() - view.numel()
            assert bool((buf[untouched] == fill).all()), (cl, code)      # every gap between rows and images, and the tail behind the last image
            assert torch.equal(gbuf.view(torch.int32), before.view(torch.int32))      # the grids and the canaries between them
            # a tight batch gives the same bytes
            tight = dec.pic_output_remapped(pic, grids, SIZE, step=k, channels_last=cl, dtype=dt, samples=2, border="pad", pad=pad)
            assert np.array_equal(ts.tensor_bits(tight, code), ts.tensor_bits(view, code))
            for wrong in (torch.as_strided(gbuf, (n, gh, gw, 2), (gstride + 1, gw * 2, 2, 1), goff), torch.as_strided(gbuf, (n, gh, gw, 2), (one - 2, gw * 2, 2, 1), goff),
                          gview[:, :, :, :1], gview.cpu(), gview.to(torch.int64), gview.permute(0, 2, 1, 3)):
                with pytest.raises(ValueError):
                    dec.pic_output_remapped(pic, wrong, SIZE, step=k)
        # one grid [gh, gw, 2] is a batch of one
        g = make_grids(dec.lib, SIZE, 2, 861)[0][1]
        t = dec.pic_output_remapped(pic, g, SIZE, step=2)
        check_batch(t, mr.batch(planes, bd, SIZE, g[None], 2), abi.OUT_U8, what="one grid")
    finally:
        dec.close()


def test_refusals_queue_nothing():
    import torch
    bd = 8
    planes = ts.random_planes(W, H, bd, seed=863)
    dec, pic = ts.open_picture(planes, bd)
    lib = dec.lib
    try:
        k = 4
        grids = make_grids(lib, SIZE, k, 864)[0]
        n = len(grids)
        d_grid = torch.from_numpy(grids).to("cuda:0")
        fmt, sc, rp = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_scale_params(SIZE[1], SIZE[0]), abi.make_remap_params(step_log2=k)
        image = 3 * SIZE[0] * SIZE[1] * 2
        need = abi.output_remap_size(lib, fmt, sc, rp, n, W, H, bd)
        gneed = abi.remap_grid_size(lib, sc, rp, n)
        assert need == n * image and gneed == grids.nbytes
        t = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        host = np.zeros(need, np.uint8)
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(f=fmt, s=sc, r=rp, g=None, gs=gneed, p=None, ds=need, count=n):
            return lib.xgpu_pic_output_device_remap(dec.ctx, pic, None, C.byref(f), C.byref(s), C.byref(r), C.c_void_p(d_grid.data_ptr() if g is None else g), gs, count,
                                                    C.c_void_p(t.data_ptr() if p is None else p), ds, stream_h)

        assert call(p=host.ctypes.data) == -101                     # the destination is host memory
        assert call(ds=need - 1) == -101                            # dst_size too short
        assert call(p=t.data_ptr() + 1) == -101                     # not aligned to the 2-byte element
        assert call(gs=gneed - 1) == -101                           # grid_size too short
        assert "pic_output_device_remap" in lib.xgpu_last_error(dec.ctx).decode()
        assert call(g=grids.ctypes.data) == -101                    # the grid is host memory
        assert call(g=d_grid.data_ptr() + 4, gs=gneed - 8) == -101  # the grid is not aligned to its 8-byte node
        assert call(g=0) == -101
        assert call(count=0) == -101 and call(count=abi.MAX_ROIS + 1) == -101
        assert call(count=n + 1) == -101                            # one grid more than grid_size and dst_size hold
        for bad in (dict(step_log2=7), dict(step_log2=-1), dict(step_log2=k, grid_format=2), dict(step_log2=k, samples=3), dict(step_log2=k, border=2),
                    dict(step_log2=k, pad=0.5), dict(step_log2=k, border=abi.WARP_PAD, pad=-1), dict(step_log2=k, grid_pitch=grids[0].nbytes + 4),
                    dict(step_log2=k, grid_pitch=grids[0].nbytes - 8), dict(step_log2=k, image_pitch=image + 1)):
            assert call(r=abi.make_remap_params(**bad)) == -101, bad
        assert call(r=abi.make_remap_params(step_log2=k, grid_pitch=grids[0].nbytes + 8)) == -101      # valid, but the grids no longer fit grid_size
        assert call(r=abi.make_remap_params(step_log2=k, image_pitch=image + 2)) == -101               # valid, but the batch no longer fits dst_size
        assert call(r=abi.make_remap_params(step_log2=0)) == -101                                      # a per-pixel grid does not fit either
        assert call(s=abi.make_scale_params(SIZE[1], SIZE[0], filter=abi.SCALE_AREA)) == -101
        assert call(s=abi.make_scale_params(SIZE[1], 1)) == -104 and call(s=abi.make_scale_params(16385, SIZE[0])) == -104
        assert call(f=abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)) == -101
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all()
        for wrong in (dict(border="wrap"), dict(samples=3), dict(layout="nv12"), dict(pad=0.5), dict(dtype=torch.uint8, mean=MEAN), dict(step=7), dict(step=3)):
            with pytest.raises(ValueError):
                dec.pic_output_remapped(pic, d_grid, SIZE, **{"step": k, **wrong})
        with pytest.raises(ValueError):
            dec.pic_output_remapped(pic, grids.astype(np.int64), SIZE, step=k)
        assert call() == 0                                          # and the context still works
        check_batch(t[:need].view(torch.int16).view(n, 3, *SIZE), mr.batch(planes, bd, SIZE, grids, k, dtype=abi.OUT_U16), abi.OUT_U16, what="after the refusals")
    finally:
        dec.close()


def test_golden_stream_and_a_side_stream():
    """StreamDecoder.pictures(tensor=, size=, remap=, remap_step=) gives, for every picture, the restatement on that picture's planes - with one grid made once on
    the device and with a callable; a call on a non-default torch stream, read on that stream without any synchronisation in between, sees the finished images"""
    import torch
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))["bytes"].tobytes()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]
    w, h = ref[0][0]["width"], ref[0][0]["height"]
    lib = abi.load()
    size, k = (24, 32), 3
    i32, f32 = make_grids(lib, size, k, 871, w, h)
    opts = dict(dtype=torch.float32, matrix=1, full_range=False, chroma_loc=0, crop=(0, 0, 0, 0), dra=None, samples=2, border="pad", pad=0.447)
    d_grid = torch.from_numpy(i32).to("cuda:0")
    got = [(p, t) for p, t in StreamDecoder(data).pictures(tensor=opts, size=size, mean=MEAN, std=STD, remap=d_grid, remap_step=k)]
    assert len(got) == len(ref) > 1
    for (p, t), (_, planes) in zip(got, ref):
        assert tuple(t.shape) == (len(i32), 3, *size)
        check_batch(t, mr.batch(planes, p["bit_depth"], size, i32, k, 2, mr.PAD, 0.447, dtype=abi.OUT_F32, **NORM), abi.OUT_F32, what=("stream", p["poc"]))

    def per_picture(p):      # a float32 grid per pixel that changes with the picture, as a numpy array the binding uploads
        return (f32[abs(p["poc"]) % len(f32)] + np.float32(0.25 * (abs(p["poc"]) % 4)))[None]

    f32 = make_grids(lib, (16, 16), 0, 872, w, h)[1]
    out = StreamDecoder(data).output_order(tensor=dict(dtype=torch.uint8, channels_last=True), size=(16, 16), remap=per_picture)
    by_poc = {p["poc"]: planes for p, planes in ref}
    assert len(out) == len(ref)
    for p, a in out:
        exp = np.moveaxis(mr.batch(by_poc[p["poc"]], p["bit_depth"], (16, 16), per_picture(p), 0), 1, -1)
        assert np.array_equal(a, exp), p["poc"]
    for wrong in (dict(remap=d_grid), dict(tensor={}, remap=d_grid), dict(tensor={}, size=size, remap=d_grid, rois=[(0, 0, 16, 16)]),
                  dict(tensor={}, size=size, remap=d_grid, warp=[wr.IDENTITY])):
        with pytest.raises(ValueError):
            next(iter(StreamDecoder(data).pictures(**wrong)))
    # a side stream and the null stream, batches of changing size, the warp call between them
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=873, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    plan = [((40, 72), 0, 0), (SIZE, 4, 1), ((100, 30), 6, 0), ((40, 72), 1, 1)]
    try:
        grids = [make_grids(dec.lib, s, kk, 874 + kk)[fm] for s, kk, fm in plan]
        sums = [[int(v) for v in mr.batch(planes, bd, s, g, kk, 2, dtype=abi.OUT_U16).astype(np.int64).sum(axis=(1, 2, 3))] for (s, kk, _), g in zip(plan, grids)]
        side = torch.cuda.Stream(device=0)
        for stream in (side, torch.cuda.default_stream(0)):
            res, warps = [], []
            with torch.cuda.stream(stream):
                for (s, kk, _), g in zip(plan, grids):
                    t = dec.pic_output_remapped(pic, torch.from_numpy(g).to("cuda:0", non_blocking=True), s, step=kk, dtype=torch.int16, samples=2)
                    res.append(t.to(torch.int64).sum(dim=(1, 2, 3)))
                    del t
                    warps.append(dec.pic_output_warped(pic, tw.maps_array(tw.MAPS[:2]), SIZE, dtype=torch.int16).to(torch.int64).sum())
            stream.synchronize()
            assert [[int(v) for v in g] for g in res] == sums
            assert len({int(v) for v in warps}) == 1
    finally:
        dec.close()
