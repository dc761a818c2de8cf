"""GPU suite for xgpu_pic_output_device_scaled_lin / xgpu_pic_output_device_rois_lin / XgpuDecoder.pic_output_scaled_cm(linear_light=True) /
StreamDecoder.pictures(tensor=, size=, to=, linear_light=True) / tools/xevd_gpu_app.py --linear-light: the picture (or batch of rectangles) resized by filtering
linear light, colour-managed and normalised by the device, against the restatement of INTEGRATION.md section 8n (tests/scaled_lin_ref.py, fed with the library's
own colour and tap tables) and against consequences that do not lean on it.  Every comparison is bit for bit, with the conventions of
test_gpu_output_scaled_cm.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import colour_ref as cr
import golden_io
import scaled_lin_ref as slr
import test_gpu_output_rois as tr
import test_gpu_output_scaled as ts
from test_gpu_output_cm import PQ_TO_SRGB, TRANSFORMS, tables
from test_gpu_output_device import golden_planes, open_picture
from xevd_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32)
MEAN, STD = ts.MEAN, ts.STD
NORM = dict(mean=np.asarray(MEAN, np.float32), inv_std=ts.inv_std(STD))
REDUCED, ENLARGED = (60, 100), (133, 230)      # (H, W); the second: four 64-column strips with a ragged last one, a height that is no multiple of 4
BT709_TO_SRGB = dict(src_primaries=1, src_transfer=1, dst_primaries=1, dst_transfer=13)
CASES = {"pq2020_srgb709_tone": PQ_TO_SRGB, "hlg2020_linear709": TRANSFORMS["hlg2020_linear709"], "bt709_srgb709": BT709_TO_SRGB}
PQ_TO_SRGB_PLAIN = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=False, linear_scale=1.0)


def run(dec, pic, planes, bd, size, colour, tab, code=abi.OUT_U8, channels_last=False, normalise=False, filt="bilinear", lin=None, what="", **kw):
    """one call and its comparison; kw: matrix, full_range, chroma_loc, upsample, crop, dra, bgr; lin: the filtered linear light of (size, filt, those) made before"""
    norm = dict(mean=MEAN, std=STD) if normalise else {}
    t = dec.pic_output_scaled_cm(pic, size, colour, channels_last=channels_last, dtype=ts.torch_dtype(code), filter=filt, linear_light=True, **norm, **kw)
    ref_norm = NORM if normalise else {}
    if lin is None:
        exp = slr.convert(planes, bd, size, tab, filt=ts.FILTERS[filt], dtype=code, lib=dec.lib, **ref_norm, **kw)
    else:
        exp = slr.finish(lin, bd, tab, dtype=code, bgr=kw.get("bgr", False), **ref_norm)
    ts.check(t, exp, code, channels_last, what or (size, code, channels_last, normalise, filt, kw))
    return t


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("case", ["base_p_8b", "base_p_10b", "base_p_12b"])
def test_bit_exact_every_dtype_layout_and_size(case, name):
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    colour = CASES[name]
    try:
        tab = tables(dec, colour, bd)
        codes = slr.rgb_codes(planes, bd, matrix=9)
        for size in (REDUCED, ENLARGED, planes[0].shape):
            lin = slr.filtered_linear(codes, size, tab, lib=dec.lib)
            for code, cl in itertools.product(ALL if size == REDUCED else (abi.OUT_U8, abi.OUT_F32), (False, True)):
                run(dec, pic, planes, bd, size, colour, tab, code, cl, lin=lin, matrix=9, what=(case, name, size, code, cl))
    finally:
        dec.close()


def test_upsample_modes_and_every_chroma_loc():
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    try:
        tab = tables(dec, PQ_TO_SRGB, bd)
        for up, loc in itertools.product(("linear", "nearest"), range(6)):
            run(dec, pic, planes, bd, (40, 52), PQ_TO_SRGB, tab, abi.OUT_U16, upsample=up, chroma_loc=loc, matrix=9)
    finally:
        dec.close()


def test_area_bgr_normalise_and_an_odd_crop():
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    try:
        tab = tables(dec, PQ_TO_SRGB, bd)
        for code, cl, bgr, filt in ((abi.OUT_F32, False, False, "bilinear"), (abi.OUT_F16, True, True, "area"), (abi.OUT_BF16, False, True, "bilinear"),
                                    (abi.OUT_F32, True, True, "area")):
            run(dec, pic, planes, bd, (40, 52), PQ_TO_SRGB, tab, code, cl, normalise=True, filt=filt, bgr=bgr, matrix=9)
        for code, filt in ((abi.OUT_U8, "area"), (abi.OUT_U16, "bilinear")):
            run(dec, pic, planes, bd, (30, 44), PQ_TO_SRGB, tab, code, bgr=True, filt=filt)
        for crop, code, cl, up in (((2, 4, 2, 0), abi.OUT_U8, False, "linear"), ((6, 0, 4, 6), abi.OUT_F32, True, "linear"), ((6, 0, 4, 6), abi.OUT_U16, False, "nearest")):
            run(dec, pic, planes, bd, (33, 70), PQ_TO_SRGB, tab, code, cl, crop=crop, chroma_loc=3, upsample=up, normalise=code == abi.OUT_F32)
    finally:
        dec.close()


def test_dra_picture():
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    h, w = planes[0].shape
    dec, pic = open_picture(planes, 10)
    try:
        tab = tables(dec, PQ_TO_SRGB, 10)
        for name, size, filt, crop, up in (("three_ranges_idx58", (h // 3, w // 3), "bilinear", (0, 0, 0, 0), "linear"),
                                           ("five_ranges_idx40", (h // 2 + 3, w + 10), "area", (2, 4, 0, 2), "nearest")):
            run(dec, pic, planes, 10, size, PQ_TO_SRGB, tab, abi.OUT_U16, dra=d[f"{name}_luts"], crop=crop, filt=filt, upsample=up, matrix=9, what=(name, size))
    finally:
        dec.close()


def test_padded_rows_and_an_odd_element_offset():
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    h, w = 37, 70
    try:
        tab = tables(dec, PQ_TO_SRGB, bd)
        lin = slr.filtered_linear(slr.rgb_codes(planes, bd), (h, w), tab, lib=dec.lib)
        for code, cl in itertools.product((abi.OUT_U8, abi.OUT_U16, abi.OUT_F32), (False, True)):      # a padded row pitch: the padding untouched
            pitch = (3 * w if cl else w) + 7
            buf = torch.full((h, pitch) if cl else (3, h, pitch), 77, dtype=ts.torch_dtype(code), device="cuda:0")
            out = buf[:, :3 * w].unflatten(1, (w, 3)) if cl else buf[:, :, :w]
            dec.pic_output_scaled_cm(pic, (h, w), PQ_TO_SRGB, channels_last=cl, dtype=ts.torch_dtype(code), out=out, linear_light=True)
            ts.check(out, slr.finish(lin, bd, tab, dtype=code), code, cl, ("pitch", code, cl))
            pad = buf[:, 3 * w:] if cl else buf[:, :, w:]
            assert (pad.cpu().numpy() == 77).all(), ("pitch", code, cl)
        for code in (abi.OUT_U8, abi.OUT_F16, abi.OUT_F32):      # a destination one element into an allocation: neither end is overrun
            n = 3 * h * w
            buf = torch.full((n + 2,), 77, dtype=ts.torch_dtype(code), device="cuda:0")
            out = buf[1:1 + n].view(3, h, w)
            dec.pic_output_scaled_cm(pic, (h, w), PQ_TO_SRGB, dtype=ts.torch_dtype(code), out=out, linear_light=True)
            ts.check(out, slr.finish(lin, bd, tab, dtype=code), code, False, ("offset", code))
            ends = buf.cpu()
            assert float(ends[0]) == 77 and float(ends[-1]) == 77, ("offset", code)
    finally:
        dec.close()


@pytest.mark.parametrize("case", ["base_p_8b", "base_p_10b"])
def test_source_size_is_the_full_size_colour_managed_call(case):
    """(a) no restatement: destination size = source size gives pic_output_tensor(colour=, upsample=) for all five dtypes - a single tap of 16384 per axis
    scales by powers of two only, so even the float dtypes are the full-size call's bits"""
    import torch
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    try:
        for dtype, up, name in itertools.product((torch.uint8, torch.int16, torch.float16, torch.bfloat16, torch.float32), ("linear", "nearest"),
                                                 ("pq2020_srgb709_tone", "hlg2020_linear709")):
            for loc in ((0, 3) if dtype != torch.int16 else range(6)):
                full = dec.pic_output_tensor(pic, dtype=dtype, chroma_loc=loc, upsample=up, matrix=9, colour=TRANSFORMS[name])
                same = dec.pic_output_scaled_cm(pic, planes[0].shape, TRANSFORMS[name], dtype=dtype, chroma_loc=loc, upsample=up, matrix=9, linear_light=True)
                assert torch.equal(full.view(torch.uint8), same.view(torch.uint8)), (case, loc, dtype, up, name)
    finally:
        dec.close()


def test_stripes_keep_their_light():
    """(b) no restatement, the point of the feature: one-sample black and white stripes of a 10-bit PQ picture, halved with the area filter.  The linear-light
    result is the encoded mean of the two lights - strictly brighter than the filtered code values' - and equals the value obtained by hand."""
    bd, w, h = 10, 128, 32
    black, white = 64, 940
    y = np.empty((h, w), np.int16)
    y[:, 0::2], y[:, 1::2] = black, white
    planes = [y, np.full((h // 2, w // 2), 512, np.int16), np.full((h // 2, w // 2), 512, np.int16)]
    dec, pic = open_picture(planes, bd)
    try:
        import torch
        tab = tables(dec, PQ_TO_SRGB_PLAIN, bd)
        lin_t = np.asarray(tab["lin"], np.float32)
        for dtype, code in ((torch.float32, abi.OUT_F32), (torch.uint8, abi.OUT_U8)):
            a = dec.pic_output_scaled_cm(pic, (16, 64), PQ_TO_SRGB_PLAIN, dtype=dtype, filter="area", linear_light=True).cpu().numpy()
            b = dec.pic_output_scaled_cm(pic, (16, 64), PQ_TO_SRGB_PLAIN, dtype=dtype, filter="area").cpu().numpy()
            assert (a[:, 1:-1, 1:-1] > b[:, 1:-1, 1:-1]).all(), dtype
            # by hand: the codes of the two stripes, their lights, half their sum (the taps are 8192 + 8192 per axis: powers of two, so the two passes are
            # exactly (Lb + Lw) * 0.5 in float32), then the rest of the transform
            cb, cw = (cr.ycbcr_to_rgb(np.int64(v), np.int64(512), np.int64(512), bd, 1, False, cr.U16).astype(np.int64) for v in (black, white))
            mean = ((lin_t[cb] + lin_t[cw]).astype(np.float32) * np.float32(0.5)).astype(np.float32)
            want = slr.from_linear(mean, tab, code, bd)
            assert (ts.bits(a[:, 1:-1, 1:-1], code) == ts.bits(want, code).reshape(3, 1, 1)).all(), dtype
    finally:
        dec.close()


def _span_bytes(lib, w, wd):
    """the bytes of LDS one destination row of the first 64-column group stages, from xgpu_scale_taps: three float32 channels from the 8-aligned first sample of
    column 0 to the 8-aligned end of column 63"""
    first, count, _ = abi.scale_taps(lib, w, 1, 0, wd)
    return 3 * 4 * (((int(first[63]) + int(count[63]) + 7) & ~7) - (int(first[0]) & ~7))


@pytest.mark.parametrize("w", [4096, 8192])
def test_widest_span_at_the_limit_ratio(w):
    """the limit ratio, 64, both filters.  4096 columns to 64: one row of the only 64-column group stages the whole width, 48 KB of float spans, so a workgroup has
    one row; 65 columns: a second, one-column group; 63: refused.  8192 columns to 128: the bilinear triangle of column 63 reaches into the second group's columns
    and one row passes 48 KB - the edge of the LDS rule, still one plain launch's."""
    bd, h = 10, 16
    wd = w // 64
    planes = ts.random_planes(w, h, bd, seed=913, rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        tab = tables(dec, PQ_TO_SRGB, bd)
        per_row = _span_bytes(dec.lib, w, wd)
        assert (per_row == 48 * 1024) if w == 4096 else (48 * 1024 < per_row <= 64 * 1024), per_row
        codes = slr.rgb_codes(planes, bd)
        for size, filt in (((8, wd), "bilinear"), ((8, wd), "area"), ((8, wd + 1), "bilinear"), ((8, wd + 1), "area")):
            lin = slr.filtered_linear(codes, size, tab, ts.FILTERS[filt], lib=dec.lib)
            for code, cl in ((abi.OUT_U16, False), (abi.OUT_F32, True)):
                run(dec, pic, planes, bd, size, PQ_TO_SRGB, tab, code, cl, filt=filt, lin=lin, normalise=code == abi.OUT_F32)
        with pytest.raises(ValueError):
            dec.pic_output_scaled_cm(pic, (8, wd - 1), PQ_TO_SRGB, linear_light=True)
        rois = [(0, 0, w, h), (2, 2, w - 8, 12)]
        t = dec.pic_output_scaled_cm(pic, (8, wd), PQ_TO_SRGB, rois=rois, dtype=ts.torch_dtype(abi.OUT_U16), linear_light=True)
        tr.check_batch(t, slr.batch(planes, bd, (8, wd), rois, tab, dtype=abi.OUT_U16, lib=dec.lib), abi.OUT_U16, what="rois")
    finally:
        dec.close()


def test_rectangles_stretch_and_letterbox():
    import torch
    planes, bd = golden_planes("base_p_10b")
    h, w = planes[0].shape
    rois = [(0, 0, w, h), (w - 8, h - 6, 8, 6), (20, 10, 100, 40), (20, 10, 100, 40), (60, 0, 20, h), (2, 2, 2, 2)]      # whole, corner, repeated, overlapping, 2 x 2
    size = (12, 16)      # (a 2 x 2 rectangle is enlarged 8 times at the most)
    dec, pic = open_picture(planes, bd)
    try:
        tab = tables(dec, PQ_TO_SRGB, bd)
        for code, cl, fit, pad, norm in ((abi.OUT_U8, False, "stretch", None, False), (abi.OUT_F32, True, "letterbox", (0.25, 0.5, 0.75), True),
                                         (abi.OUT_U16, False, "letterbox", 7, False),
                                         # every dtype in either layout: the batch kernels' instances come from one dispatch
                                         (abi.OUT_U8, True, "letterbox", 200, False), (abi.OUT_U16, True, "letterbox", 3, False),
                                         (abi.OUT_F16, False, "letterbox", 0.447, True), (abi.OUT_F16, True, "letterbox", (0.25, 0.5, 0.75), False),
                                         (abi.OUT_BF16, False, "stretch", None, False), (abi.OUT_BF16, True, "letterbox", 0.447, True),
                                         (abi.OUT_F32, False, "stretch", None, False)):
            kw = dict(mean=MEAN, std=STD) if norm else {}
            common = dict(rois=rois, fit=fit, pad=pad, channels_last=cl, dtype=ts.torch_dtype(code), **kw)
            t = dec.pic_output_scaled_cm(pic, size, PQ_TO_SRGB, linear_light=True, **common)
            assert tuple(t.shape) == ((len(rois), *size, 3) if cl else (len(rois), 3, *size))
            exp = slr.batch(planes, bd, size, rois, tab, slr.LETTERBOX if fit == "letterbox" else slr.STRETCH, 0.0 if pad is None else pad, dtype=code,
                            lib=dec.lib, **(NORM if norm else {}))
            tr.check_batch(t, exp, code, cl, (code, cl, fit, pad))
            if fit == "letterbox":      # every pad element is the plain RoI call's
                plain = dec.pic_output_tensor(pic, size=size, **common)
                for i, r in enumerate(rois):
                    ix, iy, wi, hi = tr.rr.inner(r[2], r[3], size[1], size[0], slr.LETTERBOX)
                    a, b = (x[i].movedim(-1, 0) if cl else x[i] for x in (t, plain))
                    mask = torch.ones(size, dtype=torch.bool, device=a.device)
                    mask[iy:iy + hi, ix:ix + wi] = False
                    assert torch.equal(a[:, mask], b[:, mask]), (code, i, "pad")
            else:                       # each image is the single call on its rectangle
                for i, r in enumerate(rois):
                    one = dec.pic_output_scaled_cm(pic, size, PQ_TO_SRGB, crop=tr.rect_crop(r, w, h), dtype=ts.torch_dtype(code), linear_light=True)
                    assert torch.equal(t[i], one), i
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
        need = 2 * 3 * 64 * 48
        dst = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda:0")
        sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        good = PQ_TO_SRGB
        for fmt, s, colour, rc in ((rgb, sc, dict(good, src_transfer=17), -104), (rgb, sc, dict(good, src_peak=-1.0), -101), (rgb, sc, None, -101),
                                   (yuv, sc, good, -101), (yuv, sc, None, -101), (rgb, tiny, None, -104), (yuv, tiny, good, -104)):
            c = C.byref(abi.make_colour_transform(**colour)) if colour else None
            assert lib.xgpu_pic_output_device_scaled_lin(dec.ctx, pic, None, C.byref(fmt), C.byref(s), c, C.c_void_p(dst.data_ptr()), need, sh) == rc, colour
            assert b"pic_output_device_scaled_lin" in lib.xgpu_last_error(dec.ctx)
            assert lib.xgpu_output_scaled_lin_check(C.byref(fmt), C.byref(s), c, w, h, bd) == rc
            rc_rois = lib.xgpu_pic_output_device_rois_lin(dec.ctx, pic, None, C.byref(fmt), C.byref(s), C.byref(rp), ra, 2, c, C.c_void_p(dst.data_ptr()), need, sh)
            assert rc_rois == (rc if s is sc else -104), colour
            assert b"pic_output_device_rois_lin" in lib.xgpu_last_error(dec.ctx)
        torch.cuda.synchronize()
        dec.sync()
        assert (dst.cpu().numpy() == 0x5A).all()
        with pytest.raises(ValueError):
            dec.pic_output_scaled_cm(pic, (48, 64), good, upsample="nearest")      # upsample belongs to the linear-light form
        run(dec, pic, planes, bd, (48, 64), good, tables(dec, good, bd), abi.OUT_U8)
        ts.check(dec.pic_output_scaled_cm(pic, (48, 64), good), __import__("scaled_cm_ref").convert(planes, bd, (48, 64), tables(dec, good, bd), lib=lib), abi.OUT_U8)
    finally:
        dec.close()


def test_golden_stream_and_the_application():
    """a committed stream through StreamDecoder.pictures(tensor=, size=, to=, linear_light=True), with and without rois=: every picture is the per-picture call's
    result (the restatement of its decoded planes); tools/xevd_gpu_app.py --size --to --linear-light writes the same bytes"""
    import torch
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))["bytes"].tobytes()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]
    opts = dict(dtype=torch.float32, matrix=1, full_range=False, chroma_loc=0, crop=(0, 0, 0, 0), dra=None)
    lib = abi.load()
    fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16)

    def tab_of(p, to):
        t = abi.colour_tables(lib, fmt, abi.make_colour_transform(**StreamDecoder.colour_transform(p["colour"], to)), p["bit_depth"])
        assert isinstance(t, dict), t
        return t
    got = [t for _, t in StreamDecoder(data).pictures(tensor=opts, size=(64, 96), to="srgb", mean=MEAN, std=STD, linear_light=True)]
    assert len(got) == len(ref) > 1
    for t, (p, planes) in zip(got, ref):
        assert tuple(t.shape) == (3, 64, 96)
        ts.check(t, slr.convert(planes, p["bit_depth"], (64, 96), tab_of(p, "srgb"), dtype=cr.F32, lib=lib, **NORM), abi.OUT_F32, what=("stream", p["poc"]))

    def boxes(p):
        k = 2 * (abs(p["poc"]) % 8)
        return [(0, 0, p["width"], p["height"]), (k, k, 64, 40 + k)]
    got = [(p, t) for p, t in StreamDecoder(data).pictures(tensor=opts, size=(64, 96), to="srgb", mean=MEAN, std=STD, rois=boxes, fit="letterbox", pad=0.447,
                                                            linear_light=True)]
    assert len(got) == len(ref)
    for (p, t), (_, planes) in zip(got, ref):
        exp = slr.batch(planes, p["bit_depth"], (64, 96), boxes(p), tab_of(p, "srgb"), slr.LETTERBOX, 0.447, dtype=cr.F32, lib=lib, **NORM)
        tr.check_batch(t, exp, abi.OUT_F32, what=("stream rois", p["poc"]))
    with pytest.raises(ValueError):
        next(iter(StreamDecoder(data).pictures(tensor=opts, size=(16, 24), linear_light=True)))      # no to=: no transform, no linear light
    # the application: interleaved 8-bit frames in output order
    want = StreamDecoder(data).output_order(tensor=dict(layout="rgb", channels_last=True, dtype=torch.uint8), size=(64, 96), to="srgb", linear_light=True)
    plain = StreamDecoder(data).output_order(tensor=dict(layout="rgb", channels_last=True, dtype=torch.uint8), size=(64, 96), to="srgb")
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "s.evc"), os.path.join(td, "s.rgb")
        with open(fin, "wb") as f:
            f.write(data)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "xevd_gpu_app.py"), "-i", fin, "-o", fout, "--size", "96x64", "--to", "srgb", "--linear-light"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        raw = open(fout, "rb").read()
    assert raw == b"".join(np.ascontiguousarray(a).tobytes() for _, a in want)
    assert raw != b"".join(np.ascontiguousarray(a).tobytes() for _, a in plain)
