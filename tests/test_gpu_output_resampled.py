"""GPU suite for xgpu_pic_output_device_resampled / _rois_resampled, XgpuDecoder.pic_output_resampled and StreamDecoder.pictures(resample=): the bicubic resize
written by the device into torch tensors, against the numpy restatement of the contract (tests/resample_ref.py) applied to the uploaded planes with the library's
own tap tables (which the CPU suite pins to the Fraction restatement).  Every comparison is bit for bit, with the conventions of test_gpu_output_scaled.py."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import golden_io
import resample_ref as rf
import roi_ref as rr
import test_gpu_output_rois as tr
import test_gpu_output_scaled as ts
from xevd_amd import abi

pytestmark = pytest.mark.gpu

KERNELS = {"catmull-rom": rf.CATMULL_ROM, "cubic-0.75": rf.CUBIC_075, "mitchell": rf.MITCHELL}
MEAN, STD = ts.MEAN, ts.STD
NORM = dict(mean=np.asarray(MEAN, np.float32), inv_std=ts.inv_std(STD))


def run(dec, pic, planes, bd, size, layout="rgb", kernel="catmull-rom", antialias=True, code=abi.OUT_U8, channels_last=False, normalise=False, rois=None,
        fit=None, pad=None, census=None, what="", **kw):
    """one call - the single picture, or with rois the batch - and its comparison; kw: matrix, full_range, chroma_loc, crop, dra, bgr"""
    norm = dict(mean=MEAN, std=STD) if normalise else {}
    t = dec.pic_output_resampled(pic, size, kernel=kernel, antialias=antialias, rois=rois, fit=fit, pad=pad, layout=layout, channels_last=channels_last,
                                 dtype=ts.torch_dtype(code), **norm, **kw)
    ref = dict(layout=layout, kernel=KERNELS[kernel], antialias=antialias, dtype=code, lib=dec.lib, census=census, **(NORM if normalise else {}), **kw)
    what = what or (size, layout, kernel, antialias, code, channels_last, normalise, fit, pad, kw)
    if rois is None:
        ts.check(t, rf.convert(planes, bd, size, **ref), code, channels_last, what)
    else:
        tr.check_batch(t, rf.batch(planes, bd, size, rois, rr.LETTERBOX if fit == "letterbox" else rr.STRETCH, 0.0 if pad is None else pad, **ref), code, channels_last, what)
    return t


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_grid_edges_kernels_and_depths(bd):
    """a 70 x 38 source (its width no multiple of 8) to 70 x 30 and to 150 x 37: widths above 64 that are no multiples of 64, heights that are no multiples
    of 4, one axis reduced while the other is enlarged - every kernel, with and without antialias"""
    planes = ts.random_planes(80, 48, bd, seed=500 + bd, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    crop = (4, 6, 6, 4)
    try:
        for size, kernel, antialias in itertools.product(((30, 70), (37, 150)), KERNELS, (True, False)):
            run(dec, pic, planes, bd, size, "yuv444", kernel, antialias, abi.OUT_U16, crop=crop)      # the filtered samples themselves
            run(dec, pic, planes, bd, size, "rgb", kernel, antialias, abi.OUT_U8, crop=crop)
        run(dec, pic, planes, bd, (37, 150), "rgb", "catmull-rom", True, abi.OUT_F32, normalise=True, crop=crop)
    finally:
        dec.close()


def test_every_layout_dtype_and_chroma_location():
    bd = 10
    planes = ts.random_planes(144, 88, bd, seed=521, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        for layout, cl, code in itertools.product(("rgb", "yuv444"), (False, True), ts.DT_NAMES):
            integer = code in (abi.OUT_U8, abi.OUT_U16)
            run(dec, pic, planes, bd, (50, 100), layout, "catmull-rom", True, code, cl, normalise=not integer and cl, bgr=layout == "rgb" and not cl)
        run(dec, pic, planes, bd, (50, 100), "rgb", "mitchell", True, abi.OUT_F16, True, normalise=True, bgr=True)      # the normalise follows the output order
        for loc in range(6):
            run(dec, pic, planes, bd, (61, 200), "yuv444", "cubic-0.75", False, abi.OUT_U16, chroma_loc=loc)
            run(dec, pic, planes, bd, (30, 40), "rgb", "catmull-rom", True, abi.OUT_U8, chroma_loc=loc, matrix=9, full_range=bool(loc & 1))
    finally:
        dec.close()


def test_dra_picture():
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    h, w = planes[0].shape
    dec, pic = ts.open_picture(planes, 10)
    try:
        for name in ("three_ranges_idx58", "five_ranges_idx40"):
            luts = d[f"{name}_luts"]
            run(dec, pic, planes, 10, (h // 3, w // 3), "yuv444", "catmull-rom", True, abi.OUT_U16, dra=luts, what=(name, "yuv444"))
            run(dec, pic, planes, 10, (h // 2 + 3, w + 10), "rgb", "cubic-0.75", False, abi.OUT_F32, dra=luts, crop=(2, 4, 0, 2), matrix=9, normalise=True, what=(name, "rgb"))
            run(dec, pic, planes, 10, (40, 40), "rgb", "mitchell", True, abi.OUT_U8, dra=luts, rois=[(0, 0, w - 6, h - 2), (w - 40, h - 20, 34, 18)], fit="letterbox", pad=7,
                crop=(2, 4, 0, 2), what=(name, "rois"))
    finally:
        dec.close()


def test_padded_rows_and_a_larger_buffer():
    import torch
    bd = 10
    planes = ts.random_planes(256, 144, bd, seed=523)
    dec, pic = ts.open_picture(planes, bd)
    hd, wd = 54, 97
    try:
        for cl, code in ((False, abi.OUT_U8), (False, abi.OUT_F32), (True, abi.OUT_F16)):
            dt = ts.torch_dtype(code)
            fill = 7 if code == abi.OUT_U8 else 3.0
            big = torch.full((hd, wd + 13, 3) if cl else (3, hd, wd + 13), fill, dtype=dt, device="cuda:0")
            view = big[:, 5:5 + wd, :] if cl else big[:, :, 5:5 + wd]
            out = dec.pic_output_resampled(pic, (hd, wd), channels_last=cl, dtype=dt, out=view)
            assert out is view
            ts.check(view, rf.convert(planes, bd, (hd, wd), dtype=code, lib=dec.lib), code, cl, ("pitch", cl, code))
            rest = torch.cat([(big[:, :5, :] if cl else big[:, :, :5]).flatten(), (big[:, 5 + wd:, :] if cl else big[:, :, 5 + wd:]).flatten()])
            assert bool((rest == fill).all())
        # an element-aligned, not 16-byte-aligned slot of a byte buffer, the bytes around it untouched
        n = 3 * hd * wd
        buf = torch.full((n + 40,), 0xA5, dtype=torch.uint8, device="cuda:0")
        dec.pic_output_resampled(pic, (hd, wd), kernel="mitchell", out=buf[23:23 + n].view(3, hd, wd))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[23:23 + n].reshape(3, hd, wd), rf.convert(planes, bd, (hd, wd), kernel=rf.MITCHELL, dtype=abi.OUT_U8, lib=dec.lib))
        assert (host[:23] == 0xA5).all() and (host[23 + n:] == 0xA5).all()
        for bad in (buf[:n].view(3, wd, hd), buf[:n].view(3, hd, wd).to(torch.int16), torch.empty((3, hd, wd), dtype=torch.uint8)):
            with pytest.raises(ValueError):
                dec.pic_output_resampled(pic, (hd, wd), out=bad)
    finally:
        dec.close()


def test_reduction_by_64_takes_two_rows_per_workgroup():
    """4096 x 64 to 64 x 32: a row of the horizontal pass stages (64 + 4) * 64 luma samples and half of that for either chroma plane - more than a quarter of
    48 KB, so a workgroup holds two rows, not four"""
    bd = 10
    planes = ts.random_planes(4096, 64, bd, seed=541, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        per_row = 0
        for n, s, planes_of in ((4096, 1, 1), (2048, 2, 2)):
            first, count, _ = abi.resample_taps(dec.lib, n, s, 0, 64, rf.CATMULL_ROM, True)
            per_row += planes_of * 2 * (((int(first[63]) + int(count[63]) + 7) & ~7) - (int(first[0]) & ~7))
        assert 12 * 1024 < per_row <= 24 * 1024
        run(dec, pic, planes, bd, (32, 64), "yuv444", "catmull-rom", True, abi.OUT_U16)
        run(dec, pic, planes, bd, (32, 64), "rgb", "mitchell", True, abi.OUT_F32, normalise=True)
        run(dec, pic, planes, bd, (32, 64), "rgb", "cubic-0.75", False, abi.OUT_U8)      # the same shape through four rows per workgroup: no antialias, a window of 4
    finally:
        dec.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_overshoot_is_clipped_after_the_second_pass(bd):
    """a one-sample checker on the rails, enlarged 8 times with the sharpest kernel: both passes overshoot - the intermediate leaves [0, 4 (2^B - 1)] and the
    second pass leaves [0, 2^B - 1] before its clip - and the census of the restatement says so"""
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:16, 0:16]
    luma = (((yy + xx) & 1) * top).astype(np.int16)
    planes = [luma, luma[:8, :8].copy(), (top - luma[:8, :8]).astype(np.int16)]
    dec, pic = ts.open_picture(planes, bd)
    try:
        census = {}
        run(dec, pic, planes, bd, (128, 128), "yuv444", "cubic-0.75", True, abi.OUT_U16, census=census)
        assert census["mid"][0] < 0 and census["mid"][1] > 4 * top, census
        assert census["raw"][0] < 0 and census["raw"][1] > top, census
        run(dec, pic, planes, bd, (128, 128), "rgb", "cubic-0.75", False, abi.OUT_U8)
    finally:
        dec.close()


def test_same_size_is_the_picture():
    """destination = source: the Keys kernels interpolate, so the Y plane of the output is the picture's luma bit for bit"""
    import torch
    for bd in (8, 12):
        planes = ts.random_planes(144, 88, bd, seed=547 + bd, rails=True)
        dec, pic = ts.open_picture(planes, bd)
        try:
            for kernel, antialias in itertools.product(("catmull-rom", "cubic-0.75"), (True, False)):
                t = run(dec, pic, planes, bd, (88, 144), "yuv444", kernel, antialias, abi.OUT_U16)
                assert np.array_equal(t[0].cpu().numpy().view(np.uint16), planes[0].view(np.uint16)), (bd, kernel, antialias)
                crop = (2, 6, 4, 2)
                t = dec.pic_output_resampled(pic, (82, 136), kernel=kernel, antialias=antialias, layout="yuv444", dtype=torch.int16, crop=crop)
                assert np.array_equal(t[0].cpu().numpy(), planes[0][4:86, 2:138]), (bd, kernel, antialias, "crop")
        finally:
            dec.close()


W, H = 320, 200
# overlapping, one repeated, one touching the picture's corner (an 8-fold enlargement there)
ROIS = [(0, 0, W, H), (40, 30, 160, 50), (40, 30, 160, 50), (100, 0, 20, 200), (W - 8, H - 6, 8, 6)]
SIZE = (48, 64)


def test_rois_stretch_equal_the_single_call():
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=557, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        for (kernel, antialias), (layout, code, normalise) in itertools.product((("catmull-rom", True), ("cubic-0.75", False), ("mitchell", True)),
                                                                                 (("rgb", abi.OUT_U8, False), ("yuv444", abi.OUT_U16, False), ("rgb", abi.OUT_F32, True))):
            t = run(dec, pic, planes, bd, SIZE, layout, kernel, antialias, code, normalise=normalise, rois=ROIS)
            norm = dict(mean=MEAN, std=STD) if normalise else {}
            for i, r in enumerate(ROIS):
                one = dec.pic_output_resampled(pic, SIZE, kernel=kernel, antialias=antialias, layout=layout, dtype=ts.torch_dtype(code), crop=tr.rect_crop(r), **norm)
                assert np.array_equal(ts.tensor_bits(t[i], code), ts.tensor_bits(one, code)), (kernel, layout, code, i)
    finally:
        dec.close()


def test_rois_letterbox_pad_and_image_pitch():
    import torch
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=563, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    rois = ROIS[:4] + [(2, 2, 64, 64)]      # (the corner's 8 x 6 would letterbox to 64 x 48 all the same)
    try:
        inners = [rr.inner(r[2], r[3], SIZE[1], SIZE[0]) for r in rois]
        assert inners[1] == (0, 14, 64, 20) and inners[3] == (29, 0, 5, 48) and inners[4] == (8, 0, 48, 48)
        t = run(dec, pic, planes, bd, SIZE, rois=rois, fit="letterbox", pad=114)
        got = t.cpu().numpy()
        for i, (x, y, wi, hi) in enumerate(inners):      # pad everywhere but in the inner part, and the inner part is the single call at the inner size
            mask = np.ones(got[i].shape, bool)
            mask[:, y:y + hi, x:x + wi] = False
            assert (got[i][mask] == 114).all()
            one = dec.pic_output_resampled(pic, (hi, wi), crop=tr.rect_crop(rois[i]))
            assert np.array_equal(got[i][:, y:y + hi, x:x + wi], one.cpu().numpy()), i
        run(dec, pic, planes, bd, SIZE, "rgb", "cubic-0.75", False, abi.OUT_F32, normalise=True, rois=rois, fit="letterbox", pad=0.447)
        run(dec, pic, planes, bd, SIZE, "rgb", "mitchell", True, abi.OUT_F16, True, normalise=True, bgr=True, rois=rois, fit="letterbox", pad=(0.1, 0.447, 0.9))
        run(dec, pic, planes, bd, SIZE, "yuv444", "catmull-rom", True, abi.OUT_U16, rois=rois, fit="letterbox", pad=(64, 512, 1023), chroma_loc=3)
        # an image wider than one workgroup's 64 columns, the inner part starting inside the first one and ending inside the last
        run(dec, pic, planes, bd, (50, 150), "rgb", "catmull-rom", True, abi.OUT_F32, rois=[(2, 2, 64, 64), (40, 30, 160, 50), (0, 0, 64, 200)], fit="letterbox", pad=0.5)
        run(dec, pic, planes, bd, (150, 50), "yuv444", "cubic-0.75", True, abi.OUT_U16, rois=[(2, 2, 64, 64), (100, 0, 20, 200)], fit="letterbox", pad=9)
        # out= with a batch stride and padded rows at an odd element offset: image_pitch and row_pitch, the surroundings untouched
        n, (hd, wd) = len(rois), SIZE
        pitch = wd + 13
        stride = 3 * hd * pitch + 37
        buf = torch.full((7 + n * stride + 11,), 0xA5, dtype=torch.uint8, device="cuda:0")
        view = torch.as_strided(buf, (n, 3, hd, wd), (stride, hd * pitch, pitch, 1), 7)
        assert dec.pic_output_resampled(pic, SIZE, rois=rois, fit="letterbox", pad=9, out=view) is view
        tr.check_batch(view, rf.batch(planes, bd, SIZE, rois, rr.LETTERBOX, 9, lib=dec.lib), abi.OUT_U8, what="out")
        untouched = torch.ones(buf.numel(), dtype=torch.bool, device="cuda:0")
        torch.as_strided(untouched, view.shape, view.stride(), 7).fill_(False)
        assert int(untouched.sum()) == buf.numel() - view.numel() and bool((buf[untouched] == 0xA5).all())
    finally:
        dec.close()


def test_streams_alternating_sizes_and_calls():
    """two streams in turn on one context, two sizes in turn - the cached block is replaced call by call and the intermediate regrows -, the batch and the old
    scaled call between them; no synchronisation between a call and the reduction that reads its tensor"""
    import torch
    bd = 10
    pa = ts.random_planes(320, 176, bd, seed=569)
    pb = ts.random_planes(320, 176, bd, seed=571, rails=True)
    dec, pic_a = ts.open_picture(pa, bd)
    try:
        pic_b = dec.pic_alloc()
        dec.pic_upload(pic_b, pb)
        sizes = ((40, 72), (150, 300))
        sums = {(k, s): int(rf.convert(p, bd, s, dtype=abi.OUT_U16, lib=dec.lib).astype(np.int64).sum()) for k, p in (("a", pa), ("b", pb)) for s in sizes}
        rois = [(0, 0, 320, 176), (100, 20, 64, 48)]
        roi_sum = int(rf.batch(pa, bd, sizes[0], rois, dtype=abi.OUT_U16, lib=dec.lib).astype(np.int64).sum())
        order = [("a", sizes[0]), ("b", sizes[1]), ("a", sizes[0]), ("a", sizes[0]), ("b", sizes[1]), ("a", sizes[1]), ("b", sizes[0])]
        streams = (torch.cuda.Stream(device=0), torch.cuda.Stream(device=0), torch.cuda.default_stream(0))
        got, extra = [], []
        for i, (k, s) in enumerate(order):
            with torch.cuda.stream(streams[i % 3]):
                got.append(dec.pic_output_resampled(pic_a if k == "a" else pic_b, s, dtype=torch.int16).to(torch.int64).sum())
                if i == 2:      # a batch and the triangle filter's call share the intermediate with the cached block's calls
                    extra.append(dec.pic_output_resampled(pic_a, sizes[0], rois=rois, dtype=torch.int16).to(torch.int64).sum())
                    extra.append(dec.pic_output_tensor(pic_a, dtype=torch.int16, size=sizes[0]).to(torch.int64).sum())
        torch.cuda.synchronize()
        assert [int(g) for g in got] == [sums[o] for o in order]
        import scale_ref as sr
        assert [int(e) for e in extra] == [roi_sum, int(sr.convert(pa, bd, sizes[0], dtype=abi.OUT_U16, lib=dec.lib).astype(np.int64).sum())]
        # the C ABI's stream = NULL: the context's own stream
        fmt, rs = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_resample_params(72, 40)
        t = torch.zeros((3, 40, 72), dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        assert dec.lib.xgpu_pic_output_device_resampled(dec.ctx, pic_a, None, C.byref(fmt), C.byref(rs), C.c_void_p(t.data_ptr()), t.numel() * 2, None) == 0
        dec.sync()
        ts.check(t, rf.convert(pa, bd, (40, 72), dtype=abi.OUT_U16, lib=dec.lib), abi.OUT_U16, what="null stream")
    finally:
        dec.close()


def test_refusals_queue_nothing_and_the_filter_argument_keeps_its_two_names():
    import torch
    bd = 8
    planes = ts.random_planes(256, 128, bd, seed=577)
    dec, pic = ts.open_picture(planes, bd)
    lib = dec.lib
    try:
        fmt, rs = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_resample_params(100, 60)
        need = lib.xgpu_output_resampled_size(C.byref(fmt), C.byref(rs), 256, 128, bd)
        assert need == 3 * 60 * 100 * 2
        t = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        host = np.zeros(need, np.uint8)
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(f, s, p=None, n=need):
            return lib.xgpu_pic_output_device_resampled(dec.ctx, pic, None, C.byref(f), C.byref(s), C.c_void_p(t.data_ptr() if p is None else p), n, stream_h)

        assert call(fmt, rs, host.ctypes.data) == -101              # host memory
        assert call(fmt, rs, n=need - 1) == -101                    # too short
        assert call(fmt, rs, t.data_ptr() + 1) == -101              # not aligned to the 2-byte element
        assert b"pic_output_device_resampled" in lib.xgpu_last_error(dec.ctx)
        assert call(fmt, abi.make_resample_params(3, 60)) == -104   # below 1 / 64 of 256
        assert call(fmt, abi.make_resample_params(100, 1025)) == -104
        assert call(fmt, abi.make_resample_params(100, 60, 3)) == -101
        bad = abi.make_resample_params(100, 60)
        bad.antialias = 2
        assert call(fmt, bad) == -101
        assert call(fmt, abi.make_resample_params(100, 60, mean=MEAN, std=STD)) == -101      # normalise into integers
        ra, rp = abi.make_rois([(0, 0, 64, 64), (1, 0, 64, 64)]), abi.make_roi_params()
        assert lib.xgpu_pic_output_device_rois_resampled(dec.ctx, pic, None, C.byref(fmt), C.byref(rs), C.byref(rp), ra, 2, C.c_void_p(t.data_ptr()), need, stream_h) == -101
        assert lib.xgpu_pic_output_device_rois_resampled(dec.ctx, pic, None, C.byref(fmt), C.byref(rs), None, None, 0, C.c_void_p(t.data_ptr()), need, stream_h) == -101
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all()
        for name in ("bicubic", "catmull-rom", "lanczos"):      # pic_output_tensor's filter keeps its two names
            with pytest.raises(ValueError):
                dec.pic_output_tensor(pic, size=(60, 100), filter=name)
        assert call(fmt, rs) == 0                                   # and the context still works
        ts.check(t[:need].view(torch.int16).view(3, 60, 100), rf.convert(planes, bd, (60, 100), dtype=abi.OUT_U16, lib=lib), abi.OUT_U16, what="after the refusals")
    finally:
        dec.close()


def test_golden_stream_through_the_player():
    """a committed stream through StreamDecoder.pictures(resample=..., size=...): every picture is what pic_output_resampled gives for its decoded planes, and the
    restatement of them"""
    import torch
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))["bytes"].tobytes()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]
    opts = dict(dtype=torch.float32, matrix=1, full_range=False, chroma_loc=0, crop=(0, 0, 0, 0), dra=None)
    got = [t for _, t in StreamDecoder(data).pictures(tensor=opts, size=(48, 64), mean=MEAN, std=STD, resample="bicubic")]
    assert len(got) == len(ref) > 1
    bd = ref[0][0]["bit_depth"]
    dec, pic = ts.open_picture(ref[0][1], bd)
    try:
        for t, (p, planes) in zip(got, ref):
            assert tuple(t.shape) == (3, 48, 64)
            dec.pic_upload(pic, planes)
            one = dec.pic_output_resampled(pic, (48, 64), kernel="bicubic", dtype=torch.float32, mean=MEAN, std=STD)
            assert np.array_equal(ts.tensor_bits(t, abi.OUT_F32), ts.tensor_bits(one, abi.OUT_F32)), p["poc"]
            ts.check(t, rf.convert(planes, bd, (48, 64), dtype=abi.OUT_F32, lib=dec.lib, **NORM), abi.OUT_F32, what=("stream", p["poc"]))
    finally:
        dec.close()
    # a kernel and antialias through the dict, with host rectangles, in output order
    rois = [(0, 0, 64, 64), (2, 2, 32, 48)]
    out = StreamDecoder(data).output_order(tensor=dict(opts, dtype=torch.uint8), size=(30, 44), rois=rois, fit="letterbox", pad=3,
                                           resample=dict(kernel="cubic-0.75", antialias=False))
    planes_of = {p["poc"]: planes for p, planes in ref}
    lib = abi.load()
    for p, t in out:
        exp = rf.batch(planes_of[p["poc"]], bd, (30, 44), rois, rr.LETTERBOX, 3, kernel=rf.CUBIC_075, antialias=False, lib=lib)
        assert np.array_equal(t, exp), p["poc"]
