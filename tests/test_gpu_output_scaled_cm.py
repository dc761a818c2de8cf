"""GPU suite for xgpu_pic_output_device_scaled_cm / xgpu_pic_output_device_rois_cm / XgpuDecoder.pic_output_scaled_cm / StreamDecoder.pictures(tensor=, size=,
to=): the resized, colour-managed, normalised picture (or batch of rectangles) written by the device, against the restatement of INTEGRATION.md section 8m
(tests/scaled_cm_ref.py, fed with the library's own colour and tap tables) and against consequences that do not lean on it.  Every comparison is bit for bit,
with the conventions of test_gpu_output_scaled.py."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import colour_cm_ref as cmr
import colour_ref as cr
import golden_io
import scale_ref as sr
import scaled_cm_ref as scm
import test_gpu_output_rois as tr
import test_gpu_output_scaled as ts
from test_gpu_output_cm import PQ_TO_SRGB, TRANSFORMS, tables
from test_gpu_output_device import golden_planes, open_picture
from xevd_amd import abi

pytestmark = pytest.mark.gpu

ALL = (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32)
MEAN, STD = ts.MEAN, ts.STD
NORM = dict(mean=np.asarray(MEAN, np.float32), inv_std=ts.inv_std(STD))
REDUCED, ENLARGED = (60, 100), (133, 230)      # (H, W); the second: four 64-column strips with a ragged last one, a height that is no multiple of 4


def run(dec, pic, planes, bd, size, colour, tab, code=abi.OUT_U8, channels_last=False, normalise=False, filt="bilinear", ycc=None, what="", **kw):
    """one call and its comparison; kw: matrix, full_range, chroma_loc, crop, dra, bgr; ycc: the filtered planes of (size, filt, chroma_loc, crop) made before"""
    norm = dict(mean=MEAN, std=STD) if normalise else {}
    t = dec.pic_output_scaled_cm(pic, size, colour, channels_last=channels_last, dtype=ts.torch_dtype(code), filter=filt, **norm, **kw)
    ref_norm = NORM if normalise else {}
    if ycc is None:
        exp = scm.convert(planes, bd, size, tab, filt=ts.FILTERS[filt], dtype=code, lib=dec.lib, **ref_norm, **kw)
    else:
        exp = scm.from_ycbcr(*ycc, bd, tab, matrix=kw.get("matrix", 1), dtype=code, bgr=kw.get("bgr", False), **ref_norm)
    ts.check(t, exp, code, channels_last, what or (size, code, channels_last, normalise, filt, kw))
    return t


@pytest.mark.parametrize("name", sorted(TRANSFORMS))
@pytest.mark.parametrize("case", ["base_p_8b", "base_p_10b", "base_p_12b"])
def test_bit_exact_every_dtype_layout_and_size(case, name):
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    colour = TRANSFORMS[name]
    try:
        tab = tables(dec, colour, bd)
        for size in (REDUCED, ENLARGED, planes[0].shape):
            ycc = sr.scaled_ycbcr(planes, bd, size, lib=dec.lib)
            for code, cl in itertools.product(ALL if size == REDUCED else (abi.OUT_U8, abi.OUT_F32), (False, True)):
                run(dec, pic, planes, bd, size, colour, tab, code, cl, ycc=ycc, matrix=9, what=(case, name, size, code, cl))
    finally:
        dec.close()


def test_normalise_bgr_area_crop_and_chroma_loc():
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    try:
        tab = tables(dec, PQ_TO_SRGB, bd)
        for code, cl, bgr, filt in ((abi.OUT_F32, False, False, "bilinear"), (abi.OUT_F16, True, True, "area"), (abi.OUT_BF16, False, True, "bilinear"),
                                    (abi.OUT_F32, True, True, "area")):
            run(dec, pic, planes, bd, (40, 52), PQ_TO_SRGB, tab, code, cl, normalise=True, filt=filt, bgr=bgr, matrix=9)
        for code, filt in ((abi.OUT_U8, "area"), (abi.OUT_U16, "bilinear")):
            run(dec, pic, planes, bd, (30, 44), PQ_TO_SRGB, tab, code, bgr=True, filt=filt)
        for crop, code, cl in (((2, 4, 2, 0), abi.OUT_U8, False), ((6, 0, 4, 6), abi.OUT_F32, True), ((6, 0, 4, 6), abi.OUT_U16, False)):
            run(dec, pic, planes, bd, (33, 70), PQ_TO_SRGB, tab, code, cl, crop=crop, chroma_loc=3, normalise=code == abi.OUT_F32)
    finally:
        dec.close()


def test_padded_rows_and_an_odd_element_offset():
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    h, w = 37, 70
    try:
        tab = tables(dec, PQ_TO_SRGB, bd)
        ycc = sr.scaled_ycbcr(planes, bd, (h, w), lib=dec.lib)
        for code, cl in itertools.product((abi.OUT_U8, abi.OUT_U16, abi.OUT_F32), (False, True)):      # a padded row pitch: the padding untouched
            pitch = (3 * w if cl else w) + 7
            buf = torch.full((h, pitch) if cl else (3, h, pitch), 77, dtype=ts.torch_dtype(code), device="cuda:0")
            out = buf[:, :3 * w].unflatten(1, (w, 3)) if cl else buf[:, :, :w]
            dec.pic_output_scaled_cm(pic, (h, w), PQ_TO_SRGB, channels_last=cl, dtype=ts.torch_dtype(code), out=out)
            ts.check(out, scm.from_ycbcr(*ycc, bd, tab, dtype=code), code, cl, ("pitch", code, cl))
            pad = buf[:, 3 * w:] if cl else buf[:, :, w:]
            assert (pad.cpu().numpy() == 77).all(), ("pitch", code, cl)
        for code in (abi.OUT_U8, abi.OUT_F16, abi.OUT_F32):      # a destination one element into an allocation: neither end is overrun
            n = 3 * h * w
            buf = torch.full((n + 2,), 77, dtype=ts.torch_dtype(code), device="cuda:0")
            out = buf[1:1 + n].view(3, h, w)
            dec.pic_output_scaled_cm(pic, (h, w), PQ_TO_SRGB, dtype=ts.torch_dtype(code), out=out)
            ts.check(out, scm.from_ycbcr(*ycc, bd, tab, dtype=code), code, False, ("offset", code))
            ends = buf.cpu()
            assert float(ends[0]) == 77 and float(ends[-1]) == 77, ("offset", code)
    finally:
        dec.close()


@pytest.mark.parametrize("case", ["base_p_8b", "base_p_10b"])
def test_source_size_is_the_full_size_colour_managed_call(case):
    """(a) no restatement: destination size = source size gives pic_output_tensor(colour=, upsample="linear"), for the integer dtypes and every chroma_loc"""
    import torch
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    try:
        for loc, dtype, name in itertools.product(range(6), (torch.uint8, torch.int16), ("pq2020_srgb709_tone", "hlg2020_linear709")):
            full = dec.pic_output_tensor(pic, dtype=dtype, chroma_loc=loc, upsample="linear", matrix=9, colour=TRANSFORMS[name])
            same = dec.pic_output_scaled_cm(pic, planes[0].shape, TRANSFORMS[name], dtype=dtype, chroma_loc=loc, matrix=9)
            assert torch.equal(full, same), (case, loc, dtype, name)
    finally:
        dec.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_flat_pictures_keep_the_full_size_value_at_any_size(bd):
    """(b) no restatement: a flat picture at code 0, at 2^B - 1 and at mid grey gives the full-size colour-managed value of that pixel everywhere - black under
    the tone curve, the Y = 0 division guard and both rails"""
    import torch
    w, h = 128, 64
    flat = lambda code: [np.full(s, code, np.int16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]      # noqa: E731
    dec, pic = open_picture(flat(0), bd)
    try:
        for code in (0, (1 << bd) - 1, 1 << (bd - 1)):
            dec.pic_upload(pic, flat(code))
            for name, dtype in itertools.product(("pq2020_srgb709_tone", "srgb709_pq2020"), (torch.float32, torch.uint8)):
                one = dec.pic_output_tensor(pic, dtype=dtype, colour=TRANSFORMS[name])[:, 0, 0].clone()
                for size, filt in (((9, 11), "bilinear"), ((70, 130), "bilinear"), ((7, 66), "area")):
                    t = dec.pic_output_scaled_cm(pic, size, TRANSFORMS[name], dtype=dtype, filter=filt)
                    assert torch.equal(t, one.reshape(3, 1, 1).expand(3, *size)), (bd, code, name, dtype, size)
    finally:
        dec.close()


def test_null_transform_through_the_c_entries_is_the_plain_call():
    """(c) cm = NULL: the bytes of xgpu_pic_output_device_scaled / _rois, for RGB and for a layout a transform would refuse"""
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    lib = dec.lib
    try:
        sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        sc = abi.make_scale_params(70, 37, mean=MEAN, std=STD)
        rois = [(0, 0, 64, 48), (20, 10, 100, 40)]
        ra, rp = abi.make_rois(rois), abi.make_roi_params(abi.FIT_LETTERBOX, 0.5)
        for layout in (abi.OUT_RGB_PLANAR, abi.OUT_YUV444_INTERLEAVED):
            fmt = abi.make_output_format(layout, abi.OUT_F32)
            need = lib.xgpu_output_scaled_size(C.byref(fmt), C.byref(sc), *planes[0].shape[::-1], bd)
            a = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda:0")
            b = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda:0")
            assert lib.xgpu_pic_output_device_scaled(dec.ctx, pic, None, C.byref(fmt), C.byref(sc), C.c_void_p(a.data_ptr()), need, sh) == 0
            assert lib.xgpu_pic_output_device_scaled_cm(dec.ctx, pic, None, C.byref(fmt), C.byref(sc), None, C.c_void_p(b.data_ptr()), need, sh) == 0
            torch.cuda.synchronize()
            assert torch.equal(a, b), layout
            need = lib.xgpu_output_rois_size(C.byref(fmt), C.byref(sc), C.byref(rp), ra, 2, *planes[0].shape[::-1], bd)
            a = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda:0")
            b = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda:0")
            assert lib.xgpu_pic_output_device_rois(dec.ctx, pic, None, C.byref(fmt), C.byref(sc), C.byref(rp), ra, 2, C.c_void_p(a.data_ptr()), need, sh) == 0
            assert lib.xgpu_pic_output_device_rois_cm(dec.ctx, pic, None, C.byref(fmt), C.byref(sc), C.byref(rp), ra, 2, None, C.c_void_p(b.data_ptr()), need, sh) == 0
            torch.cuda.synchronize()
            dec.sync()
            assert torch.equal(a, b), layout
    finally:
        dec.close()


def _span_bytes(lib, w, wd):
    """the bytes of LDS one destination row of one 64-column strip stages, from xgpu_scale_taps: Y, Cb and Cr from the 8-aligned first sample of column 0 to the
    8-aligned end of column 63, 16-bit samples"""
    total = 0
    for n, sub, planes_of in ((w, 1, 1), (w // 2, 2, 2)):
        first, count, _ = abi.scale_taps(lib, n, sub, 0, wd)
        total += planes_of * 2 * (((int(first[min(63, wd - 1)]) + int(count[min(63, wd - 1)]) + 7) & ~7) - (int(first[0]) & ~7))
    return total


@pytest.mark.parametrize("w", [2048, 4096])
def test_long_spans_leave_fewer_rows_per_workgroup(w):
    """12 bit, a tone and an encode table, 64 destination columns.  2048 columns: the tables and four rows of spans together pass 64 KB (computed here from
    xgpu_scale_taps) - the case that forces fewer rows per workgroup on a kernel that keeps its tables in LDS.  The kernel that was kept reads them from global
    memory and holds spans only, by the plain passes' 48 KB rule, so 4096 columns is the case where it runs fewer rows.  Both are the restatement's bit for bit."""
    bd, h, size = 12, 16, (8, 64)
    planes = ts.random_planes(w, h, bd, seed=812, rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        tab = tables(dec, PQ_TO_SRGB, bd)
        assert tab["tone"] is not None and tab["encode"] is not None
        table_bytes = 4 * (len(tab["lin"]) + len(tab["tone"]) + len(tab["encode"]))
        per_row = _span_bytes(dec.lib, w, size[1])
        assert table_bytes + 4 * per_row > 64 * 1024, (table_bytes, per_row)
        if w == 4096:
            assert 2 * per_row <= 48 * 1024 < 4 * per_row, per_row
        for code, cl in ((abi.OUT_U16, False), (abi.OUT_F32, True)):
            run(dec, pic, planes, bd, size, PQ_TO_SRGB, tab, code, cl, normalise=code == abi.OUT_F32)
        rois = [(0, 0, w, h), (2, 2, w - 8, 12)]
        t = dec.pic_output_scaled_cm(pic, size, PQ_TO_SRGB, rois=rois, dtype=ts.torch_dtype(abi.OUT_U16))
        tr.check_batch(t, scm.batch(planes, bd, size, rois, tab, dtype=abi.OUT_U16, lib=dec.lib), abi.OUT_U16, what="rois")
    finally:
        dec.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_rectangles_stretch_and_letterbox(bd):
    import torch
    planes = ts.random_planes(tr.W, tr.H, bd, seed=500 + bd, rails=True)
    dec, pic = open_picture(planes, bd)
    colour = PQ_TO_SRGB if bd == 10 else TRANSFORMS["srgb709_pq2020"]
    try:
        tab = tables(dec, colour, bd)
        for code, cl, fit, pad, norm in ((abi.OUT_U8, False, "stretch", None, False), (abi.OUT_F32, True, "letterbox", (0.25, 0.5, 0.75), True),
                                         (abi.OUT_U16, False, "letterbox", 7, False), (abi.OUT_F16, False, "letterbox", 0.447, True),
                                         # every dtype in either layout: the batch kernels' instances come from one dispatch
                                         (abi.OUT_U8, True, "letterbox", 200, False), (abi.OUT_U16, True, "letterbox", 3, False),
                                         (abi.OUT_F16, True, "letterbox", (0.25, 0.5, 0.75), False), (abi.OUT_BF16, False, "letterbox", 0.447, True),
                                         (abi.OUT_BF16, True, "letterbox", (0.25, 0.5, 0.75), True), (abi.OUT_F32, False, "stretch", None, False)):
            kw = dict(mean=MEAN, std=STD) if norm else {}
            t = dec.pic_output_scaled_cm(pic, tr.SIZE, colour, rois=tr.ROIS, fit=fit, pad=pad, channels_last=cl, dtype=ts.torch_dtype(code), **kw)
            assert tuple(t.shape) == ((len(tr.ROIS), *tr.SIZE, 3) if cl else (len(tr.ROIS), 3, *tr.SIZE))
            exp = scm.batch(planes, bd, tr.SIZE, tr.ROIS, tab, scm.LETTERBOX if fit == "letterbox" else scm.STRETCH, 0.0 if pad is None else pad, dtype=code,
                            lib=dec.lib, **(NORM if norm else {}))
            tr.check_batch(t, exp, code, cl, (bd, code, cl, fit, pad))
            if fit == "letterbox":      # the wide rectangle's top rows are the pad value as it was given: normalised like a pixel, never transformed
                img = t[2].movedim(-1, 0) if cl else t[2]
                fill = tr.rr.pad_elements(pad, code, **(NORM if norm else {}))
                got = ts.tensor_bits(img[:, 0, :].contiguous(), code)
                assert (got == ts.bits(np.broadcast_to(fill.reshape(3, 1), got.shape), code)).all(), (bd, code, "pad")
            if fit == "stretch":        # each image is the single call on its rectangle
                for i, r in enumerate(tr.ROIS):
                    one = dec.pic_output_scaled_cm(pic, tr.SIZE, colour, crop=tr.rect_crop(r), dtype=ts.torch_dtype(code))
                    assert torch.equal(t[i], one), (bd, i)
    finally:
        dec.close()


def test_table_cache_shared_with_the_full_size_call():
    """full-size A, scaled A, scaled B, full-size B, scaled A on one context: every call gets its own transform's tables; and a context at another depth"""
    import torch
    A, B = TRANSFORMS["pq2020_srgb709_tone"], TRANSFORMS["hlg2020_linear709"]
    for case in ("base_p_10b", "base_p_12b"):
        planes, bd = golden_planes(case)
        dec, pic = open_picture(planes, bd)
        try:
            ta, tb = tables(dec, A, bd), tables(dec, B, bd)
            ycc = sr.scaled_ycbcr(planes, bd, REDUCED, lib=dec.lib)
            got = [dec.pic_output_tensor(pic, dtype=torch.int16, colour=A), dec.pic_output_scaled_cm(pic, REDUCED, A, dtype=torch.int16),
                   dec.pic_output_scaled_cm(pic, REDUCED, B, dtype=torch.int16), dec.pic_output_tensor(pic, dtype=torch.int16, colour=B),
                   dec.pic_output_scaled_cm(pic, REDUCED, A, dtype=torch.int16),
                   dec.pic_output_scaled_cm(pic, REDUCED, B, rois=[(0, 0, *planes[0].shape[::-1])], dtype=torch.int16)[0]]
            exp = [cmr.convert(planes, bd, ta, dtype=cr.U16), scm.from_ycbcr(*ycc, bd, ta, dtype=cr.U16), scm.from_ycbcr(*ycc, bd, tb, dtype=cr.U16),
                   cmr.convert(planes, bd, tb, dtype=cr.U16), scm.from_ycbcr(*ycc, bd, ta, dtype=cr.U16), scm.from_ycbcr(*ycc, bd, tb, dtype=cr.U16)]
            for i, (t, e) in enumerate(zip(got, exp)):
                ts.check(t, e, abi.OUT_U16, what=(case, i))
        finally:
            dec.close()


def test_refusals_queue_nothing_and_the_context_goes_on():
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    lib = dec.lib
    w, h = planes[0].shape[::-1]
    try:
        rgb = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8)
        yuv = abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_U8)
        sc, tiny = abi.make_scale_params(64, 48), abi.make_scale_params(w * 8 + 2, 48)
        ra, rp = abi.make_rois([(0, 0, 64, 48), (20, 10, 100, 40)]), abi.make_roi_params()
        odd = abi.make_rois([(1, 0, 64, 48), (20, 10, 100, 40)])
        need = 2 * 3 * 64 * 48
        dst = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda:0")
        sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        good = PQ_TO_SRGB
        for fmt, s, colour, rc in ((rgb, sc, dict(good, src_transfer=17), -104), (rgb, sc, dict(good, dst_primaries=11), -104), (rgb, sc, dict(good, src_peak=-1.0), -101),
                                   (yuv, sc, good, -101), (yuv, sc, dict(good, src_transfer=17), -101),      # the layout before the transform
                                   (rgb, tiny, dict(good, src_peak=-1.0), -104), (yuv, tiny, good, -104)):      # the plain call's refusal before either
            c = abi.make_colour_transform(**colour)
            assert lib.xgpu_pic_output_device_scaled_cm(dec.ctx, pic, None, C.byref(fmt), C.byref(s), C.byref(c), C.c_void_p(dst.data_ptr()), need, sh) == rc, colour
            assert b"pic_output_device_scaled_cm" in lib.xgpu_last_error(dec.ctx)
            assert lib.xgpu_output_scaled_cm_check(C.byref(fmt), C.byref(s), C.byref(c), w, h, bd) == rc
            rc_rois = lib.xgpu_pic_output_device_rois_cm(dec.ctx, pic, None, C.byref(fmt), C.byref(s), C.byref(rp), ra, 2, C.byref(c), C.c_void_p(dst.data_ptr()), need, sh)
            assert rc_rois == (rc if s is sc else -104), colour
            assert b"pic_output_device_rois_cm" in lib.xgpu_last_error(dec.ctx)
        c = abi.make_colour_transform(**dict(good, src_transfer=17))      # the batch's own refusal (an odd rectangle) before the transform's
        assert lib.xgpu_pic_output_device_rois_cm(dec.ctx, pic, None, C.byref(rgb), C.byref(sc), C.byref(rp), odd, 2, C.byref(c), C.c_void_p(dst.data_ptr()), need, sh) == -101
        c = abi.make_colour_transform(**good)
        assert lib.xgpu_pic_output_device_scaled_cm(dec.ctx, pic, None, C.byref(rgb), C.byref(sc), C.byref(c), C.c_void_p(dst.data_ptr()), 100, sh) == -101      # too small
        torch.cuda.synchronize()
        dec.sync()
        assert (dst.cpu().numpy() == 0x5A).all()
        # pic_output_tensor keeps refusing the combination; the context still works
        for bad in (dict(size=(48, 64), colour=good), dict(size=(48, 64), colour=good, rois=[(0, 0, 64, 48)])):
            with pytest.raises(ValueError):
                dec.pic_output_tensor(pic, **bad)
        with pytest.raises(ValueError):
            dec.pic_output_scaled_cm(pic, (48, 64), good, rois=torch.zeros((1, 4), dtype=torch.int32, device="cuda:0"))
        run(dec, pic, planes, bd, (48, 64), good, tables(dec, good, bd), abi.OUT_U8)
    finally:
        dec.close()


def test_golden_stream_to_linear_light_at_model_size():
    """a committed stream through StreamDecoder.pictures(tensor=, size=, to=, mean=, std=), and once more with rois=: every picture is the restatement of its
    decoded planes"""
    import torch
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))["bytes"].tobytes()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]
    opts = dict(dtype=torch.float32, matrix=1, full_range=False, chroma_loc=0, crop=(0, 0, 0, 0), dra=None)
    lib = abi.load()
    fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16)

    def tab_of(p):
        t = abi.colour_tables(lib, fmt, abi.make_colour_transform(**StreamDecoder.colour_transform(p["colour"], "linear-bt709")), p["bit_depth"])
        assert isinstance(t, dict), t
        return t
    got = [t for _, t in StreamDecoder(data).pictures(tensor=opts, size=(64, 96), to="linear-bt709", mean=MEAN, std=STD)]
    assert len(got) == len(ref) > 1
    for t, (p, planes) in zip(got, ref):
        assert tuple(t.shape) == (3, 64, 96)
        ts.check(t, scm.convert(planes, p["bit_depth"], (64, 96), tab_of(p), dtype=cr.F32, lib=lib, **NORM), abi.OUT_F32, what=("stream", p["poc"]))

    def boxes(p):
        k = 2 * (abs(p["poc"]) % 8)
        return [(0, 0, p["width"], p["height"]), (k, k, 64, 40 + k)]
    got = [(p, t) for p, t in StreamDecoder(data).pictures(tensor=opts, size=(64, 96), to="linear-bt709", mean=MEAN, std=STD, rois=boxes, fit="letterbox", pad=0.447)]
    assert len(got) == len(ref)
    for (p, t), (_, planes) in zip(got, ref):
        assert tuple(t.shape) == (2, 3, 64, 96)
        exp = scm.batch(planes, p["bit_depth"], (64, 96), boxes(p), tab_of(p), scm.LETTERBOX, 0.447, dtype=cr.F32, lib=lib, **NORM)
        tr.check_batch(t, exp, abi.OUT_F32, what=("stream rois", p["poc"]))
    # output_order takes the same route; what has no transform keeps refusing one
    out = StreamDecoder(data).output_order(tensor=dict(opts, dtype=torch.uint8), size=(16, 24), to="srgb")
    assert all(a.shape == (3, 16, 24) and a.dtype == np.uint8 for _, a in out) and len(out) == len(ref)
    for bad in (dict(warp=[0.1]), dict(remap=np.zeros((1, 4, 4, 2), np.float32))):
        with pytest.raises(ValueError):
            next(iter(StreamDecoder(data).pictures(tensor=opts, size=(16, 24), to="srgb", **bad)))
    with pytest.raises(ValueError):
        next(iter(StreamDecoder(data).pictures(tensor=opts, size=(16, 24), to="srgb", rois=lambda p: torch.zeros((1, 4), dtype=torch.int32, device="cuda:0"))))
