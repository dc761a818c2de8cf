"""GPU suite for xgpu_pic_output_device_rois_dev / XgpuDecoder.pic_output_tensor(size=, rois=<tensor on the device>): boxes a detector left on the GPU, snapped,
described and given their tap tables by k_rois_prepare, with no host read.  The contract is equality, bit for bit, with the host-box call
(xgpu_pic_output_device_rois, which test_gpu_output_rois.py pins against the restatement) on the rectangle every box was snapped to; the statuses, the rectangles
used and their inner parts against tests/roi_dev_ref.py; the tap tables of the device's row builder against xgpu_scale_taps and tests/scale_ref.py."""
import itertools
import os

import numpy as np
import pytest

import golden_io
import roi_dev_ref as rd
import roi_ref as rr
import scale_ref as sr
import test_gpu_output_scaled as ts
from xevd_amd import abi

pytestmark = pytest.mark.gpu

W, H, BD = 192, 128, 10
MEAN, STD = ts.MEAN, ts.STD
# the whole picture, a 2 x 2 box in each corner, boxes touching each edge, a duplicate, two that overlap - and several seeded ones (boxes())
FIXED = [(0, 0, W, H), (0, 0, 2, 2), (W - 2, 0, 2, 2), (0, H - 2, 2, 2), (W - 2, H - 2, 2, 2), (0, 40, 30, 50), (150, 30, 42, 60), (60, 0, 70, 20), (50, 100, 80, 28),
         (50, 100, 80, 28), (40, 30, 64, 48), (72, 54, 64, 48)]
_cache = {}


def boxes(seed=9, n=5, lo=4):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        bw, bh = int(rng.integers(lo, 50)) * 2, int(rng.integers(lo, 40)) * 2
        out.append((int(rng.integers(0, (W - bw) // 2 + 1)) * 2, int(rng.integers(0, (H - bh) // 2 + 1)) * 2, bw, bh))
    return out


def picture(w=W, h=H, bd=BD):
    """one seeded picture per size, shared by the tests (the planes are never written)"""
    if (w, h, bd) not in _cache:
        _cache[(w, h, bd)] = ts.random_planes(w, h, bd, seed=w + bd, rails=True)
    return _cache[(w, h, bd)]


def device_boxes(rows, dtype):
    import torch
    return torch.tensor(np.asarray(rows), dtype=dtype, device="cuda:0")


def against_host(dec, pic, t, res, kw, what):
    """every image with status OK equals image i of the host-box call on the rectangles used, and inner is abi.roi_inner's; -> the statuses"""
    import torch
    res = res.cpu().numpy()
    ok = [i for i in range(len(res)) if res[i, 0] == rd.OK]
    used = [tuple(int(v) for v in res[i, 1:5]) for i in ok]
    fit = abi.FIT_LETTERBOX if kw.get("fit") == "letterbox" else abi.FIT_STRETCH
    for i, u in zip(ok, used):
        assert tuple(res[i, 5:9]) == abi.roi_inner(dec.lib, u, kw["size"], fit), (what, i)
    if ok:
        host = dec.pic_output_tensor(pic, rois=used, **kw)
        torch.cuda.synchronize()
        for k, i in enumerate(ok):
            assert torch.equal(t[i], host[k]), (what, "image", i, used[k])
    return [int(v) for v in res[:, 0]]


def test_tables_of_the_device_row_builder():
    """xgpu_test_scale_taps_device == xgpu_scale_taps == scale_ref.taps: down, up, identity, a ratio near 64, the 8x enlargement limit, the narrowest output"""
    dec, _ = ts.open_picture(picture(96, 64, 8), 8)
    try:
        for (n, N), filt, (s, half) in itertools.product(((128, 24), (24, 128), (64, 64), (130, 3), (2, 16), (96, 2)), (sr.BILINEAR, sr.AREA),
                                                         ((1, 0), (2, 0), (2, 1), (2, 2))):
            what = (n, N, filt, s, half)
            host = abi.scale_taps(dec.lib, n, s, half, N, filt)
            got = abi.scale_taps_device(dec.lib, dec.ctx, n, s, half, N, filt, extra=2)
            if isinstance(host, int):
                assert got == host == -104, what          # (a chroma plane of 130 to 3: beyond 1 / 64)
                continue
            first, count, w = got
            assert np.array_equal(first, host[0]) and np.array_equal(count, host[1]), what
            assert np.array_equal(w[:, :-2], host[2]) and (w[:, -2:] == 0).all(), what          # every weight, and zeros behind count up to the stride
            assert sr.table_rows(first, count, w) == sr.taps(n, s, half, N, filt), what
    finally:
        dec.close()


def test_equal_to_the_host_box_call():
    import torch
    planes = picture()
    dec, pic = ts.open_picture(planes, BD)
    batch = FIXED + boxes()
    assert len(batch) >= 12
    t_boxes = device_boxes(batch, torch.int32)
    luts = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))["three_ranges_idx58_luts"]
    forms = (dict(layout="rgb", dtype=torch.float32, mean=MEAN, std=STD), dict(layout="rgb", dtype=torch.uint8, channels_last=True),
             dict(layout="yuv444", dtype=torch.int16))
    try:
        for fit, form, filt, loc in itertools.product(("stretch", "letterbox"), forms, ("bilinear", "area"), (0, 1)):
            kw = dict(form, size=(16, 16), fit=fit, filter=filt, chroma_loc=loc, pad=0.25 if form["dtype"] == torch.float32 else 77)
            t, res = dec.pic_output_tensor(pic, rois=t_boxes, results=True, **kw)
            assert tuple(res.shape) == (len(batch), 9) and res.dtype == torch.int32
            # no box of this set is refused, and even boxes inside the picture are used as they are
            assert np.array_equal(res.cpu().numpy(), rd.results(batch, rd.XYWH_I32, (H, W), (16, 16), rr.LETTERBOX if fit == "letterbox" else rr.STRETCH)), kw
            assert against_host(dec, pic, t, res, kw, kw) == [rd.OK] * len(batch)
            assert [tuple(r[1:5]) for r in res.cpu().numpy().tolist()] == batch
        kw = dict(layout="yuv444", dtype=torch.int16, size=(16, 16), fit="letterbox", pad=3, dra=luts)
        t, res = dec.pic_output_tensor(pic, rois=t_boxes, results=True, **kw)
        assert against_host(dec, pic, t, res, kw, "dra") == [rd.OK] * len(batch)
    finally:
        dec.close()


@pytest.mark.parametrize("w,h,bd", [(W, H, BD), (96, 64, 8)])
def test_both_formats_and_snapping(w, h, bd):
    """fractional F32 corners and odd I32 boxes: used is abi.roi_snap's, the images are the host-box call's on used; an image wider than one workgroup's 64 columns"""
    import torch
    planes = picture(w, h, bd)
    dec, pic = ts.open_picture(planes, bd)
    rng = np.random.default_rng(w)
    xyxy, xywh = [], []
    for _ in range(8):
        bw, bh = rng.uniform(26, w * 0.6), rng.uniform(14, h * 0.6)
        x, y = rng.uniform(-6, w - bw + 6), rng.uniform(-6, h - bh + 6)
        xyxy.append([float(np.float32(v)) for v in (x, y, x + bw, y + bh)])
        xywh.append([int(x) | 1, int(y), int(bw) | 1, int(bh) | 1])
    xyxy += [[10.0, 4.0, 50.0, 30.0], [10.5, 4.5, 50.5, 30.5], [10.999, 4.999, 50.999, 30.999], [-3.25, -0.5, 40.0, float(h) + 7.5]]
    try:
        for rows, dtype, fmt in ((xyxy, torch.float32, rd.XYXY_F32), (xywh, torch.int32, rd.XYWH_I32)):
            for fit, size in (("letterbox", (20, 150)), ("stretch", (24, 70))):
                kw = dict(dtype=torch.uint8, size=size, fit=fit, pad=114)
                t, res = dec.pic_output_tensor(pic, rois=device_boxes(rows, dtype), results=True, **kw)
                got = res.cpu().numpy()
                for i, b in enumerate(rows):
                    status, used = abi.roi_snap(dec.lib, b, (h, w), fmt)
                    assert status == rd.OK and (int(got[i, 0]), tuple(got[i, 1:5])) == (status, used), (fmt, i, b)
                assert np.array_equal(got, rd.results(rows, fmt, (h, w), size, rr.LETTERBOX if fit == "letterbox" else rr.STRETCH)), (fmt, fit)
                assert against_host(dec, pic, t, res, kw, (fmt, fit)) == [rd.OK] * len(rows)
        assert any(tuple(r) != tuple(int(v) for v in b) for r, b in zip(got[:, 1:5], xywh))      # the odd boxes did move
    finally:
        dec.close()


def test_statuses_and_pad_images():
    import torch
    planes = picture()
    dec, pic = ts.open_picture(planes, BD)
    good = [[8.0, 8.0, 40.0, 60.0], [100.0, 20.0, 164.0, 84.0], [20.5, 30.5, 60.0, 70.0], [0.0, 0.0, 64.0, 64.0]]
    nan = float("nan")
    rows = [good[0], [nan, 0.0, 30.0, 30.0], good[1], [50.0, 50.0, 50.0, 90.0], good[2], [10.0, 10.0, 76.0, 40.0], good[3], [10.0, 10.0, 12.0, 50.0]]
    # NaN; no column; 66 wide with max_roi 64 x 64; 2 columns stretched to 32 (letterboxed, the box keeps its 2 columns and is served)
    stretched = [rd.OK, rd.INVALID, rd.OK, rd.EMPTY, rd.OK, rd.TOO_LARGE, rd.OK, rd.RATIO]
    try:
        for form, pad in ((dict(dtype=torch.float32, mean=MEAN, std=STD), (0.1, 0.447, 0.9)), (dict(dtype=torch.uint8), (0, 114, 255)),
                          (dict(dtype=torch.float16, channels_last=True, mean=MEAN, std=STD, bgr=True), 0.5)):
            for fit in ("stretch", "letterbox"):
                kw = dict(form, size=(32, 32), fit=fit, pad=pad)
                t, res = dec.pic_output_tensor(pic, rois=device_boxes(rows, torch.float32), results=True, max_roi=(64, 64), **kw)
                assert np.array_equal(res.cpu().numpy(), rd.results(rows, rd.XYXY_F32, (H, W), (32, 32), rr.LETTERBOX if fit == "letterbox" else rr.STRETCH, (64, 64)))
                expect = stretched if fit == "stretch" else stretched[:7] + [rd.OK]
                assert against_host(dec, pic, t, res, kw, (form, fit)) == expect          # the boxes between the refused ones are served as ever
                code = {torch.float32: abi.OUT_F32, torch.uint8: abi.OUT_U8, torch.float16: abi.OUT_F16}[form["dtype"]]
                norm = dict(mean=np.asarray(MEAN, np.float32), inv_std=ts.inv_std(STD)) if "mean" in form else {}
                fill = ts.bits(rr.pad_elements(pad, code, **norm), code)
                got = ts.tensor_bits(t, code)
                for i, st in enumerate(expect):
                    if st != rd.OK:      # the whole image is the pad value, channel by channel
                        img = got[i] if form.get("channels_last") else np.moveaxis(got[i], 0, -1)
                        assert (img == fill.reshape(1, 1, 3)).all(), (form, fit, i)
        # the whole 192-wide picture to a width of 2: 96 columns to one
        rows = [(0, 0, 64, 64), (0, 0, W, H), (1, 1, 61, 63)]
        kw = dict(dtype=torch.uint8, size=(8, 2), pad=9)
        t, res = dec.pic_output_tensor(pic, rois=device_boxes(rows, torch.int32), results=True, **kw)
        assert np.array_equal(res.cpu().numpy(), rd.results(rows, rd.XYWH_I32, (H, W), (8, 2)))
        assert against_host(dec, pic, t, res, kw, "width 2") == [rd.OK, rd.RATIO, rd.OK]
        assert bool((t[1] == 9).all())
    finally:
        dec.close()


def test_count_and_missing_results():
    import torch
    planes = picture(96, 64, 8)
    dec, pic = ts.open_picture(planes, 8)
    rows = [(2, 2, 40, 30), (1, 1, 33, 17), (50, 20, 46, 44), (0, 0, 96, 64), (10, 10, 20, 20), (3, 3, 9, 9), (60, 40, 30, 20), (5, 40, 70, 21)]
    t_boxes = device_boxes(rows, torch.int32)
    kw = dict(dtype=torch.float32, size=(24, 40), fit="letterbox", pad=0.5, mean=MEAN, std=STD)
    try:
        for count, live in ((3, 3), (0, 0), (100, 8), (-4, 0), (8, 8)):
            out = torch.full((8, 3, 24, 40), -7.0, dtype=torch.float32, device="cuda:0")
            cnt = torch.tensor([count], dtype=torch.int32, device="cuda:0")
            t, res = dec.pic_output_tensor(pic, rois=t_boxes, count=cnt, results=True, out=out, **kw)
            assert t is out
            assert np.array_equal(res.cpu().numpy(), rd.results(rows, rd.XYWH_I32, (64, 96), (24, 40), rr.LETTERBOX, count=count))
            assert against_host(dec, pic, t, res, kw, ("count", count)) == [rd.OK] * live + [rd.UNUSED] * (8 - live)
            assert bool((out[live:] == -7.0).all()), count          # not an element of an unused image is written
            # without the results the images are the same
            again = torch.full((8, 3, 24, 40), -7.0, dtype=torch.float32, device="cuda:0")
            assert dec.pic_output_tensor(pic, rois=t_boxes, count=cnt, out=again, **kw) is again
            assert torch.equal(again, out), count
        for bad in (dict(rois=t_boxes.cpu()), dict(rois=t_boxes.to(torch.int64)), dict(rois=t_boxes[:, :3]), dict(rois=t_boxes.t()[:, :4]), dict(rois=t_boxes.view(-1)),
                    dict(rois=t_boxes, count=torch.tensor([3], dtype=torch.int32)), dict(rois=t_boxes, count=3), dict(rois=t_boxes, snap=True),
                    dict(rois=t_boxes, colour=dict(dst_transfer=13)), dict(rois=t_boxes, max_roi=(66, 96)), dict(rois=rows, results=True), dict(rois=rows, max_roi=(8, 8)),
                    dict(rois=t_boxes, dtype=torch.uint8, pad=0.5, mean=None, std=None, fit="stretch")):
            with pytest.raises(ValueError):
                dec.pic_output_tensor(pic, **{**kw, **bad})
    finally:
        dec.close()


def test_ordered_behind_the_boxes_without_a_host_read():
    """the boxes come out of torch arithmetic on the current stream right before the call, which runs on another stream behind wait_stream; then the two ROI
    calls and the scaled call alternate on the context"""
    import torch
    planes = picture()
    dec, pic = ts.open_picture(planes, BD)
    base = np.array([[4, 6, 30, 20], [30, 10, 60, 51], [1, 1, 95, 63], [33, 5, 15, 40]], np.int32)          # doubled: even, and inside the 192 x 128 picture
    final =[tuple(int(v) for v in r) for r in base * 2]
    kw = dict(dtype=torch.int16, layout="yuv444", size=(20, 70), fit="letterbox", pad=5)
    side = torch.cuda.Stream(device=0)
    try:
        expect = dec.pic_output_tensor(pic, rois=final, **kw).clone()
        one = dec.pic_output_tensor(pic, dtype=torch.int16, size=(20, 70), crop=(2, 4, 6, 8)).clone()
        torch.cuda.synchronize()
        for _ in range(2):
            stale = torch.zeros((4, 4), dtype=torch.int32, device="cuda:0")
            busy = torch.ones((1024, 1024), device="cuda:0")
            busy = busy @ busy                                                     # the stream is busy when the boxes are queued
            t_boxes = stale + torch.tensor(base, device="cuda:0") * 2            # ... and they are made right here, on the current stream
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                t, res = dec.pic_output_tensor(pic, rois=t_boxes, results=True, **kw)
                sums = t.to(torch.int64).sum()
                host = dec.pic_output_tensor(pic, rois=final, **kw)
                scaled = dec.pic_output_tensor(pic, dtype=torch.int16, size=(20, 70), crop=(2, 4, 6, 8))
                t2 = dec.pic_output_tensor(pic, rois=t_boxes, **kw)
            side.synchronize()
            assert torch.equal(t, expect) and torch.equal(t2, expect) and torch.equal(host, expect) and torch.equal(scaled, one)
            assert int(sums) == int(expect.to(torch.int64).sum())
            assert [tuple(r[1:5]) for r in res.cpu().numpy().tolist()] == final
    finally:
        dec.close()


def test_largest_ratio_fits_the_lds_bound():
    """max_roi = the picture; 128 rows to 2 and 192 columns to 3, the inner part at column 73 of a 150-wide image: the span 64 image columns reach is measured
    against the bound the LDS was sized with, and passes"""
    import torch
    planes = picture()
    dec, pic = ts.open_picture(planes, BD)
    try:
        assert rr.inner(W, H, 150, 2) == (73, 0, 3, 2)
        for filt, dtype in (("bilinear", torch.int16), ("area", torch.uint8)):
            kw = dict(dtype=dtype, layout="yuv444", size=(2, 150), fit="letterbox", pad=1, filter=filt)
            rows = [(0, 0, W, H), (0, 0, W, 2), (20, 0, 128, H)]
            t, res = dec.pic_output_tensor(pic, rois=device_boxes(rows, torch.int32), results=True, max_roi=(H, W), **kw)
            assert np.array_equal(res.cpu().numpy(), rd.results(rows, rd.XYWH_I32, (H, W), (2, 150), rr.LETTERBOX))
            assert against_host(dec, pic, t, res, kw, filt) == [rd.OK] * 3
            assert tuple(res[0, 5:9].tolist()) == (73, 0, 3, 2)
    finally:
        dec.close()
