"""GPU suite for xgpu_pic_output_device_rois / XgpuDecoder.pic_output_tensor(size=, rois=) / StreamDecoder.pictures(rois=): several rectangles of one
picture resized into a batch of images by one call, against the restatement of the contract (tests/roi_ref.py on tests/scale_ref.py) and, image by image,
against the single-image call with the crop set to the rectangle.  Every comparison is bit for bit, with the conventions of test_gpu_output_scaled.py
(integers as they are, float32 by its bit pattern, float16 / bfloat16 by the bit pattern of the restatement's float32 rounded to nearest even)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import colour_ref as cr
import golden_io
import roi_ref as rr
import scale_ref as sr
import test_gpu_output_scaled as ts
from xevd_amd import abi

pytestmark = pytest.mark.gpu

W, H = 320, 200
SIZE = (48, 64)
WIDE, TALL, SQUARE = (40, 30, 160, 50), (100, 0, 20, 200), (2, 2, 64, 64)
ROIS = [(0, 0, W, H), (312, 194, 8, 6), WIDE, WIDE, TALL, SQUARE]      # the whole picture, an 8x enlargement in the corner, a duplicate, overlaps
MEAN, STD = ts.MEAN, ts.STD
NORM = dict(mean=np.asarray(MEAN, np.float32), inv_std=ts.inv_std(STD))


def rect_crop(r, w=W, h=H):
    x, y, rw, rh = r
    return (x, w - x - rw, y, h - y - rh)


def check_batch(t, exp, code, channels_last=False, what=""):
    """tensor t [N, ...] against the restatement exp [N][3][H][W], bit for bit"""
    if channels_last:
        exp = np.moveaxis(exp, 1, -1)
    exp = ts.bits(np.ascontiguousarray(exp), code)
    got = ts.tensor_bits(t, code)
    assert got.shape == exp.shape, what
    for i in range(len(exp)):
        bad = int((got[i] != exp[i]).sum())
        assert bad == 0, f"{what}: image {i}: {bad} of {exp[i].size} elements differ"


def run(dec, pic, planes, bd, rois, size=SIZE, layout="rgb", filt="bilinear", code=abi.OUT_U8, channels_last=False, normalise=False, fit="stretch", pad=0.0, what="",
        **kw):
    norm = dict(mean=MEAN, std=STD) if normalise else {}
    t = dec.pic_output_tensor(pic, layout=layout, channels_last=channels_last, dtype=ts.torch_dtype(code), size=size, filter=filt, rois=rois, fit=fit, pad=pad,
                              **norm, **kw)
    assert tuple(t.shape) == ((len(rois), *size, 3) if channels_last else (len(rois), 3, *size))
    exp = rr.batch(planes, bd, size, rois, rr.LETTERBOX if fit == "letterbox" else rr.STRETCH, pad, layout=layout, filt=ts.FILTERS[filt], dtype=code, lib=dec.lib,
                   **(NORM if normalise else {}), **kw)
    check_batch(t, exp, code, channels_last, what or (size, layout, filt, code, channels_last, normalise, fit, pad, kw))
    return t


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_stretch_equals_the_restatement_and_the_single_call(bd):
    planes = ts.random_planes(W, H, bd, seed=300 + bd, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        for filt in ts.FILTERS:
            for layout, code, normalise in (("rgb", abi.OUT_U8, False), ("yuv444", abi.OUT_U16, False), ("rgb", abi.OUT_F32, True)):
                t = run(dec, pic, planes, bd, ROIS, layout=layout, filt=filt, code=code, normalise=normalise)
                norm = dict(mean=MEAN, std=STD) if normalise else {}
                for i, r in enumerate(ROIS):      # image by image: the existing call with the crop set to the rectangle
                    one = dec.pic_output_tensor(pic, layout=layout, dtype=ts.torch_dtype(code), size=SIZE, filter=filt, crop=rect_crop(r), **norm)
                    assert np.array_equal(ts.tensor_bits(t[i], code), ts.tensor_bits(one, code)), (filt, layout, code, i)
    finally:
        dec.close()


def test_reduction_by_64_and_same_size():
    import torch
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=311, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        for filt in ts.FILTERS:
            run(dec, pic, planes, bd, [(0, 0, 320, 192), (0, 8, 320, 192)], size=(3, 5), layout="yuv444", filt=filt, code=abi.OUT_U16)
            run(dec, pic, planes, bd, [(0, 0, 320, 192)], size=(3, 5), layout="rgb", filt=filt, code=abi.OUT_F32, normalise=True)
        # 1:1: the unscaled output with linear upsampling, as for the single-image call
        r = (8, 8, 64, 48)
        for layout, code, loc in (("yuv444", abi.OUT_U16, 0), ("rgb", abi.OUT_U8, 0), ("yuv444", abi.OUT_U16, 3)):
            t = dec.pic_output_tensor(pic, layout=layout, dtype=ts.torch_dtype(code), size=SIZE, rois=[r, r], chroma_loc=loc)
            plain = dec.pic_output_tensor(pic, layout=layout, dtype=ts.torch_dtype(code), upsample="linear", crop=rect_crop(r), chroma_loc=loc)
            torch.cuda.synchronize()
            assert torch.equal(t[0], plain) and torch.equal(t[1], plain), (layout, code, loc)
    finally:
        dec.close()


def test_letterbox():
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=313, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    rois = [WIDE, TALL, SQUARE]
    try:
        # where the inner parts lie (and abi.roi_inner says so): 64 x 20 at (0, 14); 5 x 48 at (29, 0) - odd; 48 x 48 at (8, 0)
        inners = [abi.roi_inner(dec.lib, r, SIZE) for r in rois]
        assert inners == [(0, 14, 64, 20), (29, 0, 5, 48), (8, 0, 48, 48)] == [rr.inner(r[2], r[3], SIZE[1], SIZE[0]) for r in rois]
        t = run(dec, pic, planes, bd, rois, code=abi.OUT_U8, fit="letterbox", pad=114)
        got = t.cpu().numpy()
        for i, (x, y, wi, hi) in enumerate(inners):      # pad everywhere but in the inner part, and the inner part is the single call at the inner size
            mask = np.ones(got[i].shape, bool)
            mask[:, y:y + hi, x:x + wi] = False
            assert (got[i][mask] == 114).all()
            one = dec.pic_output_tensor(pic, size=(hi, wi), crop=rect_crop(rois[i]))
            assert np.array_equal(got[i][:, y:y + hi, x:x + wi], one.cpu().numpy()), i
        for filt in ts.FILTERS:
            run(dec, pic, planes, bd, rois, code=abi.OUT_U8, filt=filt, fit="letterbox", pad=(0, 114, 255))
            run(dec, pic, planes, bd, rois, code=abi.OUT_F32, filt=filt, normalise=True, fit="letterbox", pad=0.447)
            run(dec, pic, planes, bd, rois, code=abi.OUT_F16, filt=filt, channels_last=True, bgr=True, normalise=True, fit="letterbox", pad=(0.1, 0.447, 0.9))
            run(dec, pic, planes, bd, rois, layout="yuv444", code=abi.OUT_U16, filt=filt, fit="letterbox", pad=(64, 512, 1023))
        for loc in range(6):
            run(dec, pic, planes, bd, [TALL, WIDE], layout="yuv444", code=abi.OUT_U16, fit="letterbox", pad=3, chroma_loc=loc)
            run(dec, pic, planes, bd, [TALL], code=abi.OUT_U8, fit="letterbox", pad=7, chroma_loc=loc, matrix=9, full_range=bool(loc & 1))
        # an image wider than one workgroup's 64 columns, the inner part starting inside the first one and ending inside the last
        run(dec, pic, planes, bd, [SQUARE, WIDE, (0, 0, 64, 200)], size=(50, 150), code=abi.OUT_F32, fit="letterbox", pad=0.5)
        run(dec, pic, planes, bd, [SQUARE, TALL], size=(150, 50), layout="yuv444", code=abi.OUT_U16, fit="letterbox", pad=9)
    finally:
        dec.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_every_layout_and_dtype(bd):
    planes = ts.random_planes(W, H, bd, seed=317 + bd, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    rois = [(0, 0, W, H), TALL, (312, 194, 8, 6)]
    try:
        for layout, cl, code in itertools.product(("rgb", "yuv444"), (False, True), ts.DT_NAMES):
            integer = code in (abi.OUT_U8, abi.OUT_U16)
            run(dec, pic, planes, bd, rois, layout=layout, code=code, channels_last=cl, fit="letterbox", pad=(17, 0, 200) if integer else (0.25, -0.5, 1.0),
                normalise=not integer and cl)
            run(dec, pic, planes, bd, rois, layout=layout, code=code, channels_last=cl, filt="area", bgr=layout == "rgb")
    finally:
        dec.close()


def test_dra_picture():
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    h, w = planes[0].shape
    dec, pic = ts.open_picture(planes, 10)
    rois = [(0, 0, w, h), (2, 2, w // 2 & ~1, h // 4 & ~1), (w - 34, h - 18, 34, 18)]
    try:
        for name in ("three_ranges_idx58", "five_ranges_idx40"):
            luts = d[f"{name}_luts"]
            run(dec, pic, planes, 10, rois, size=(h // 3, w // 3), layout="yuv444", code=abi.OUT_U16, dra=luts, what=(name, "yuv444"))
            inside = [(0, 0, w - 6, h - 2), rois[1], (w - 40, h - 20, 34, 18)]      # of the picture minus the crop
            run(dec, pic, planes, 10, inside, size=(40, 40), code=abi.OUT_F32, filt="area", dra=luts, matrix=9, normalise=True, fit="letterbox", pad=0.5,
                crop=(2, 4, 0, 2), what=(name, "rgb"))
    finally:
        dec.close()


def test_out_with_batch_stride_padded_rows_and_odd_offsets():
    import torch
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=331)
    dec, pic = ts.open_picture(planes, bd)
    rois = [WIDE, TALL, SQUARE, (0, 0, W, H)]
    n, (hd, wd) = len(rois), SIZE
    try:
        for cl, code, off in ((False, abi.OUT_U8, 7), (False, abi.OUT_F32, 3), (True, abi.OUT_F16, 5)):
            dt = ts.torch_dtype(code)
            fill = 0xA5 if code == abi.OUT_U8 else -3.0
            pitch = (3 * wd if cl else wd) + 13                       # elements between rows
            image = (hd if cl else 3 * hd) * pitch
            stride = image + 37                                       # elements between images
            buf = torch.full((off + n * stride + 11,), fill, dtype=dt, device="cuda:0")
            view = torch.as_strided(buf, (n, hd, wd, 3) if cl else (n, 3, hd, wd), (stride, pitch, 3, 1) if cl else (stride, hd * pitch, pitch, 1), off)
            out = dec.pic_output_tensor(pic, channels_last=cl, dtype=dt, size=SIZE, rois=rois, fit="letterbox", pad=9 if code == abi.OUT_U8 else 0.5, out=view)
            assert out is view
            check_batch(view, rr.batch(planes, bd, SIZE, rois, rr.LETTERBOX, 9 if code == abi.OUT_U8 else 0.5, dtype=code, lib=dec.lib), code, cl, ("out", cl, code))
            untouched = torch.ones(buf.numel(), dtype=torch.bool, device="cuda:0")
            torch.as_strided(untouched, view.shape, view.stride(), off).fill_(False)
            assert int(untouched.sum()) == buf.numel() - view.numel()
            assert bool((buf[untouched] == fill).all()), (cl, code)
        # a contiguous batch, and one image (any batch stride)
        t = torch.empty((n, 3, hd, wd), dtype=torch.uint8, device="cuda:0")
        assert dec.pic_output_tensor(pic, size=SIZE, rois=rois, out=t) is t
        check_batch(t, rr.batch(planes, bd, SIZE, rois, lib=dec.lib), abi.OUT_U8, what="contiguous out")
        check_batch(dec.pic_output_tensor(pic, size=SIZE, rois=rois[:1], out=t[2:3]), rr.batch(planes, bd, SIZE, rois[:1], lib=dec.lib), abi.OUT_U8, what="one image")
        for bad in (t[:3], t.to(torch.int16), torch.as_strided(t, t.shape, (hd * wd, hd * wd, wd, 1)), t.permute(0, 1, 3, 2)):
            with pytest.raises(ValueError):
                dec.pic_output_tensor(pic, size=SIZE, rois=rois, out=bad)
    finally:
        dec.close()


def test_streams_changing_batches_and_the_single_call_between():
    """a side stream and the null stream; batches of 1, 6, 2, 9 rectangles at changing sizes (the descriptor block and the intermediate regrow), the old
    single-image call between them on the same context (its cached tap tables stay right), no synchronisation before the reduction that reads each result"""
    import torch
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=337, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    nine = ROIS + [(64, 64, 128, 96), (0, 100, 320, 100), (200, 20, 40, 60)]
    plan = [(nine[:1], (40, 72)), (ROIS, SIZE), (nine[4:6], (100, 30)), (nine, (24, 40)), (nine[:1], (40, 72)), (ROIS, (60, 60))]
    single = (40, 72)
    try:
        sums = [[int(v) for v in rr.batch(planes, bd, s, r, rr.LETTERBOX, 5, dtype=cr.U16, lib=dec.lib).astype(np.int64).sum(axis=(1, 2, 3))] for r, s in plan]
        single_sum = int(sr.convert(planes, bd, single, dtype=cr.U16, lib=dec.lib, crop=(2, 4, 6, 8)).astype(np.int64).sum())
        side = torch.cuda.Stream(device=0)
        for stream in (side, torch.cuda.default_stream(0)):
            got, ones = [], []
            with torch.cuda.stream(stream):
                for r, s in plan:
                    t = dec.pic_output_tensor(pic, dtype=torch.int16, size=s, rois=r, fit="letterbox", pad=5)
                    got.append(t.to(torch.int64).sum(dim=(1, 2, 3)))
                    del t
                    ones.append(dec.pic_output_tensor(pic, dtype=torch.int16, size=single, crop=(2, 4, 6, 8)).to(torch.int64).sum())
            stream.synchronize()
            assert [[int(v) for v in g] for g in got] == sums
            assert [int(v) for v in ones] == [single_sum] * len(plan)
        # the C ABI's stream = NULL: the context's own stream
        fmt, sc, rp = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_scale_params(SIZE[1], SIZE[0]), abi.make_roi_params()
        t = torch.zeros((len(ROIS), 3, *SIZE), dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        assert dec.lib.xgpu_pic_output_device_rois(dec.ctx, pic, None, C.byref(fmt), C.byref(sc), C.byref(rp), abi.make_rois(ROIS), len(ROIS),
                                                   C.c_void_p(t.data_ptr()), t.numel() * 2, None) == 0
        dec.sync()
        check_batch(t, rr.batch(planes, bd, SIZE, ROIS, dtype=cr.U16, lib=dec.lib), abi.OUT_U16, what="null stream")
    finally:
        dec.close()


def test_refusals_queue_nothing():
    import torch
    bd = 8
    planes = ts.random_planes(W, H, bd, seed=347)
    dec, pic = ts.open_picture(planes, bd)
    lib = dec.lib
    try:
        fmt, sc, rp = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_scale_params(SIZE[1], SIZE[0]), abi.make_roi_params()
        image = 3 * SIZE[0] * SIZE[1] * 2
        need = lib.xgpu_output_rois_size(C.byref(fmt), C.byref(sc), C.byref(rp), abi.make_rois(ROIS), len(ROIS), W, H, bd)
        assert need == len(ROIS) * image
        t = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        host = np.zeros(need, np.uint8)
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(rois=ROIS, f=fmt, s=sc, r=rp, p=None, n=need, count=None):
            return lib.xgpu_pic_output_device_rois(dec.ctx, pic, None, C.byref(f), C.byref(s), C.byref(r), abi.make_rois(rois), len(rois) if count is None else count,
                                                   C.c_void_p(t.data_ptr() if p is None else p), n, stream_h)

        def err():
            return lib.xgpu_last_error(dec.ctx).decode()

        assert call(p=host.ctypes.data) == -101                     # host memory
        assert call(n=need - 1) == -101                             # too short for the batch
        assert call(p=t.data_ptr() + 1) == -101                     # not aligned to the 2-byte element
        assert "pic_output_device_rois" in err()
        assert call(count=0) == -101 and call(count=abi.MAX_ROIS + 1) == -101
        assert call(ROIS[:3] + [(1, 0, 16, 16)] + ROIS[3:]) == -101 and "roi 3" in err()
        assert call([(0, 0, 16, 16), (310, 0, 16, 16)]) == -101 and "roi 1" in err()
        assert call(ROIS[:2] + [(0, 0, 6, 8)]) == -104 and "roi 2" in err()      # 6 columns to 64
        assert call(r=abi.make_roi_params(fit=3)) == -101
        assert call(r=abi.make_roi_params(abi.FIT_LETTERBOX, 256)) == -101
        assert call(r=abi.make_roi_params(abi.FIT_LETTERBOX, 0.5)) == -101
        assert call(r=abi.make_roi_params(image_pitch=image - 2)) == -101
        assert call(r=abi.make_roi_params(image_pitch=image + 2)) == -101      # the batch no longer fits the destination
        assert call(s=abi.make_scale_params(SIZE[1], SIZE[0], mean=MEAN, std=STD)) == -101
        assert call(f=abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)) == -101
        assert call(f=abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, matrix=2)) == -104
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all()
        for bad in (dict(rois=ROIS), dict(size=SIZE, rois=ROIS, colour=dict(dst_transfer=13)), dict(size=SIZE, rois=ROIS, fit="pad"), dict(size=SIZE, rois=[]),
                    dict(size=SIZE, rois=[(1, 1, 15, 15)]), dict(size=SIZE, rois=[(300, 190, 40, 40)]), dict(size=SIZE, rois=ROIS, layout="nv12"),
                    dict(size=SIZE, rois=ROIS, fit="letterbox", pad=0.5), dict(size=SIZE, fit="letterbox"), dict(size=SIZE, pad=3), dict(snap=True)):
            with pytest.raises(ValueError):
                dec.pic_output_tensor(pic, **bad)
        with pytest.raises(ValueError, match="roi 1 "):
            dec.pic_output_tensor(pic, size=SIZE, rois=[SQUARE, (3, 2, 16, 16)])
        assert call() == 0                                          # and the context still works
        check_batch(t[:need].view(torch.int16).view(len(ROIS), 3, *SIZE), rr.batch(planes, bd, SIZE, ROIS, dtype=cr.U16, lib=lib), abi.OUT_U16, what="after the refusals")
        # snap=True: odd boxes grow outward to even and are cut at the picture's edge
        boxes = [(1, 1, 15, 15), (300, 190, 40, 40), (-5, 33, 21, 10)]
        snapped = [(0, 0, 16, 16), (300, 190, 20, 10), (0, 32, 16, 12)]
        a = dec.pic_output_tensor(pic, size=(16, 16), rois=boxes, snap=True)
        check_batch(a, rr.batch(planes, bd, (16, 16), snapped, lib=lib), abi.OUT_U8, what="snap")
    finally:
        dec.close()


def test_golden_stream_with_rectangles_per_picture():
    """a committed stream through StreamDecoder.pictures(tensor=, size=, rois=callable): the callable sees every picture's parameters"""
    import torch
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))["bytes"].tobytes()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]
    opts = dict(dtype=torch.float32, matrix=1, full_range=False, chroma_loc=0, crop=(0, 0, 0, 0), dra=None)
    lib = abi.load()

    def boxes(p):      # a grid of tiles, and a box that moves with the picture
        k = 2 * (abs(p["poc"]) % 8)
        return abi.tile_rois(p["width"], p["height"], p["width"] // 2 & ~1, p["height"] // 2 & ~1) + [(k, k, 32, 24 + k)]

    got = [(p, t) for p, t in StreamDecoder(data).pictures(tensor=opts, size=(24, 32), mean=MEAN, std=STD, rois=boxes, fit="letterbox", pad=0.447)]
    assert len(got) == len(ref) > 1
    for (p, t), (_, planes) in zip(got, ref):
        assert tuple(t.shape) == (5, 3, 24, 32)
        check_batch(t, rr.batch(planes, p["bit_depth"], (24, 32), boxes(p), rr.LETTERBOX, 0.447, dtype=cr.F32, lib=lib, **NORM), abi.OUT_F32, what=("stream", p["poc"]))
    # a fixed list, integers, channels last; output_order delivers numpy arrays
    tiles = abi.tile_rois(ref[0][0]["width"], ref[0][0]["height"], 64, 64)
    out = StreamDecoder(data).output_order(tensor=dict(opts, dtype=torch.uint8, channels_last=True), size=(16, 16), rois=tiles)
    by_poc = {p["poc"]: planes for p, planes in ref}
    for p, a in out:
        exp = np.moveaxis(rr.batch(by_poc[p["poc"]], p["bit_depth"], (16, 16), tiles, lib=lib), 1, -1)
        assert np.array_equal(a, exp), p["poc"]
    for bad in (dict(rois=tiles), dict(tensor=opts, rois=tiles), dict(tensor=opts, size=(16, 16), fit="letterbox")):
        with pytest.raises(ValueError):
            next(iter(StreamDecoder(data).pictures(**bad)))
