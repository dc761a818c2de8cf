"""GPU suite for xgpu_pic_output_device_scaled / XgpuDecoder.pic_output_tensor(size=...) / StreamDecoder.pictures(tensor=..., size=...): the resized,
converted and normalised picture written by the device into torch tensors, against the numpy restatement of the contract (tests/scale_ref.py) applied to
the uploaded planes with the library's own tap tables (which the CPU suite pins to the Fraction restatement).  Every comparison is bit for bit: integers
as they are, float32 by its bit pattern, float16 / bfloat16 by the bit pattern of the restatement's float32 rounded to nearest even."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import colour_ref as cr
import golden_io
import scale_ref as sr
from xevd_amd import abi

pytestmark = pytest.mark.gpu

DT_NAMES = {abi.OUT_U8: "uint8", abi.OUT_U16: "int16", abi.OUT_F16: "float16", abi.OUT_BF16: "bfloat16", abi.OUT_F32: "float32"}
FILTERS = {"bilinear": sr.BILINEAR, "area": sr.AREA}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def torch_dtype(code):
    import torch
    return getattr(torch, DT_NAMES[code])


def random_planes(w, h, bd, seed, rails=False):
    """seeded random planes; rails: blocks of 0 and of 2^B - 1 laid over them, so that whole windows sit on either rail"""
    rng = np.random.default_rng(seed)
    planes = [rng.integers(0, 1 << bd, s, dtype=np.int64).astype(np.int16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    if rails:
        top = (1 << bd) - 1
        for p in planes:
            ph, pw = p.shape
            p[:ph // 3, :pw // 2] = 0
            p[:ph // 3, pw // 2:] = top
            p[ph // 3:ph // 2, pw // 4:pw // 2] = top
    return planes


def open_picture(planes, bd):
    from xevd_amd.decoder import XgpuDecoder
    h, w = planes[0].shape
    dec = XgpuDecoder(w, h, bd, device=0, max_pics=4)
    pic = dec.pic_alloc()
    dec.pic_upload(pic, planes)
    return dec, pic


def inv_std(std):
    return np.float32(1) / np.asarray(std, np.float32)


def bits(a, code):
    """the bit patterns an output of dtype `code` must hold for the restatement's array a"""
    if code == abi.OUT_U8:
        return np.asarray(a, np.uint8)
    if code == abi.OUT_U16:
        return np.asarray(a, np.uint16)
    if code == abi.OUT_F32:
        return np.ascontiguousarray(a, np.float32).view(np.uint32)
    return cr.to_f16_bits(a) if code == abi.OUT_F16 else cr.to_bf16_bits(a)


def tensor_bits(t, code):
    import torch
    torch.cuda.synchronize()
    t = t.cpu()
    if code == abi.OUT_U8:
        return t.numpy()
    if code == abi.OUT_F32:
        return t.contiguous().view(torch.int32).numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def check(t, exp, code, channels_last=False, what=""):
    """tensor t (written by the device) against the restatement exp [3][H][W], bit for bit"""
    if channels_last:
        exp = np.moveaxis(exp, 0, -1)
    exp = bits(np.ascontiguousarray(exp), code)
    got = tensor_bits(t, code)
    assert got.shape == exp.shape, what
    bad = int((got != exp).sum())
    assert bad == 0, f"{what}: {bad} of {exp.size} elements differ"


def run(dec, pic, planes, bd, size, layout="rgb", filt="bilinear", code=abi.OUT_U8, channels_last=False, normalise=False, what="", **kw):
    """one scaled output and its comparison; kw: matrix, full_range, chroma_loc, crop, dra, bgr"""
    norm = dict(mean=MEAN, std=STD) if normalise else {}
    t = dec.pic_output_tensor(pic, layout=layout, channels_last=channels_last, dtype=torch_dtype(code), size=size, filter=filt, **norm, **kw)
    ref_norm = dict(mean=np.asarray(MEAN, np.float32), inv_std=inv_std(STD)) if normalise else {}
    exp = sr.convert(planes, bd, size, layout=layout, filt=FILTERS[filt], dtype=code, lib=dec.lib, **ref_norm, **kw)
    check(t, exp, code, channels_last, what or (size, layout, filt, code, channels_last, normalise, kw))
    return t


# source size, destination (H, W): reductions by 2, 3.7 and 34, an enlargement by 1.5, different ratios on the two axes (one axis up, one down)
SIZES = {"2x": ((256, 128), (64, 128)), "3.7x": ((592, 296), (80, 160)), "34x": ((1088, 544), (16, 32)), "up1.5x": ((128, 64), (96, 192)),
         "mixed": ((320, 240), (300, 100))}


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("name", list(SIZES))
def test_sizes_filters_and_depths(name, bd):
    (w, h), size = SIZES[name]
    planes = random_planes(w, h, bd, seed=bd * 100 + len(name), rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        for filt in FILTERS:
            run(dec, pic, planes, bd, size, "yuv444", filt, abi.OUT_U16)      # the filtered samples themselves
            run(dec, pic, planes, bd, size, "rgb", filt, abi.OUT_U8)
            run(dec, pic, planes, bd, size, "rgb", filt, abi.OUT_F32, normalise=True)
    finally:
        dec.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_planes_on_the_rails(bd):
    """whole planes of 0 and of 2^B - 1: both passes stay on the rail (no clip needed, none applied)"""
    top = (1 << bd) - 1
    dec = None
    for vy, vc in ((0, 0), (top, top), (top, 0), (0, top)):
        planes = [np.full((96, 160), vy, np.int16), np.full((48, 80), vc, np.int16), np.full((48, 80), vc, np.int16)]
        dec, pic = open_picture(planes, bd)
        try:
            for filt, size in itertools.product(FILTERS, ((36, 70), (130, 200))):
                t = run(dec, pic, planes, bd, size, "yuv444", filt, abi.OUT_U16)
                got = t.cpu().numpy().view(np.uint16)
                assert (got[0] == vy).all() and (got[1:] == vc).all()
                run(dec, pic, planes, bd, size, "rgb", filt, abi.OUT_U16)
        finally:
            dec.close()


def test_every_chroma_location():
    bd = 10
    planes = random_planes(208, 120, bd, seed=5)
    dec, pic = open_picture(planes, bd)
    try:
        for loc, (size, filt) in itertools.product(range(6), (((45, 77), "bilinear"), ((180, 312), "bilinear"), ((60, 104), "area"))):
            run(dec, pic, planes, bd, size, "yuv444", filt, abi.OUT_U16, chroma_loc=loc)
            run(dec, pic, planes, bd, size, "rgb", filt, abi.OUT_U8, chroma_loc=loc, matrix=9, full_range=bool(loc & 1))
    finally:
        dec.close()


def test_crop_is_the_region_of_interest():
    bd = 10
    planes = random_planes(320, 200, bd, seed=11, rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        for crop in ((2, 0, 0, 0), (40, 120, 30, 50), (0, 6, 2, 4), (158, 2, 98, 2)):
            for size, filt in (((64, 64), "bilinear"), ((50, 90), "area")):
                run(dec, pic, planes, bd, size, "rgb", filt, abi.OUT_U8, crop=crop, chroma_loc=1)
                run(dec, pic, planes, bd, size, "yuv444", filt, abi.OUT_F32, crop=crop, chroma_loc=1)
    finally:
        dec.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_every_layout_and_dtype(bd):
    planes = random_planes(240, 136, bd, seed=17 + bd, rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        for layout, cl, code in itertools.product(("rgb", "yuv444"), (False, True), DT_NAMES):
            run(dec, pic, planes, bd, (56, 100), layout, "bilinear", code, cl)
            if code not in (abi.OUT_U8, abi.OUT_U16):
                run(dec, pic, planes, bd, (56, 100), layout, "bilinear", code, cl, normalise=True)
        for code, cl in itertools.product((abi.OUT_U8, abi.OUT_F32, abi.OUT_BF16), (False, True)):
            run(dec, pic, planes, bd, (56, 100), "rgb", "area", code, cl, bgr=True, normalise=code != abi.OUT_U8, matrix=5)
    finally:
        dec.close()


def test_normalise_follows_the_output_order():
    """mean[k] / inv_std[k] belong to the channel at position k of the output: with bgr, mean[0] is blue's"""
    import torch
    bd = 8
    planes = random_planes(128, 72, bd, seed=23)
    dec, pic = open_picture(planes, bd)
    try:
        plain = dec.pic_output_tensor(pic, dtype=torch.float32, size=(30, 50), bgr=True)
        normed = dec.pic_output_tensor(pic, dtype=torch.float32, size=(30, 50), bgr=True, mean=MEAN, std=STD)
        torch.cuda.synchronize()
        exp = sr.normalise(plain.cpu().numpy(), np.asarray(MEAN, np.float32), inv_std(STD))
        assert np.array_equal(normed.cpu().numpy().view(np.uint32), exp.view(np.uint32))
        # one value for all three channels
        one = dec.pic_output_tensor(pic, dtype=torch.float32, size=(30, 50), mean=0.5, std=0.25)
        three = dec.pic_output_tensor(pic, dtype=torch.float32, size=(30, 50), mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25))
        assert torch.equal(one, three)
    finally:
        dec.close()


def test_padded_rows_and_unaligned_destinations():
    import torch
    bd = 10
    planes = random_planes(256, 144, bd, seed=29)
    dec, pic = open_picture(planes, bd)
    hd, wd = 54, 97
    try:
        # rows padded by the caller's strides (row_pitch): a view into a wider tensor, the padding untouched
        for cl, code in ((False, abi.OUT_U8), (False, abi.OUT_F32), (True, abi.OUT_F16)):
            dt = torch_dtype(code)
            fill = 7 if code == abi.OUT_U8 else 3.0
            big = torch.full((hd, wd + 13, 3) if cl else (3, hd, wd + 13), fill, dtype=dt, device="cuda:0")
            view = big[:, 5:5 + wd, :] if cl else big[:, :, 5:5 + wd]
            out = dec.pic_output_tensor(pic, channels_last=cl, dtype=dt, size=(hd, wd), out=view)
            assert out is view
            check(view, sr.convert(planes, bd, (hd, wd), dtype=code, lib=dec.lib), code, cl, ("pitch", cl, code))
            rest = torch.cat([(big[:, :5, :] if cl else big[:, :, :5]).flatten(), (big[:, 5 + wd:, :] if cl else big[:, :, 5 + wd:]).flatten()])
            assert bool((rest == fill).all())
        # element-aligned, not 16-byte-aligned destinations: slots of a byte buffer at odd offsets, the bytes around them untouched
        n = 3 * hd * wd
        exp = sr.convert(planes, bd, (hd, wd), dtype=abi.OUT_U8, lib=dec.lib)
        offs = [1, n + 4, 2 * n + 23]
        buf = torch.full((offs[-1] + n + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        for o in offs:
            dec.pic_output_tensor(pic, size=(hd, wd), out=buf[o:o + n].view(3, hd, wd))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        mask = np.ones(host.size, bool)
        for o in offs:
            assert np.array_equal(host[o:o + n].reshape(3, hd, wd), exp), o
            mask[o:o + n] = False
        assert (host[mask] == 0xA5).all()
        # a float32 slot at a 4-byte, not 16-byte, offset
        fb = torch.full((n + 8,), -1.0, dtype=torch.float32, device="cuda:0")
        dec.pic_output_tensor(pic, dtype=torch.float32, size=(hd, wd), out=fb[3:3 + n].view(3, hd, wd), mean=MEAN, std=STD)
        check(fb[3:3 + n].view(3, hd, wd), sr.convert(planes, bd, (hd, wd), dtype=abi.OUT_F32, lib=dec.lib, mean=np.asarray(MEAN, np.float32), inv_std=inv_std(STD)),
              abi.OUT_F32, what="f32 slot")
        assert bool((fb[:3] == -1).all()) and bool((fb[3 + n:] == -1).all())
    finally:
        dec.close()


def test_dra_picture():
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    h, w = planes[0].shape
    dec, pic = open_picture(planes, 10)
    try:
        for name in ("three_ranges_idx58", "five_ranges_idx40"):
            luts = d[f"{name}_luts"]
            for size, filt, crop in (((h // 3, w // 3), "bilinear", (0, 0, 0, 0)), ((h // 2 + 3, w + 10), "area", (2, 4, 0, 2))):
                run(dec, pic, planes, 10, size, "yuv444", filt, abi.OUT_U16, dra=luts, crop=crop, what=(name, size, "yuv444"))
                run(dec, pic, planes, 10, size, "rgb", filt, abi.OUT_F32, dra=luts, crop=crop, matrix=9, normalise=True, what=(name, size, "rgb"))
    finally:
        dec.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_same_size_equals_the_unscaled_output(bd):
    """Wd x Hd = Ws x Hs: luma is the identity and the chroma taps are the quarter weights of XGPU_UPSAMPLE_LINEAR, whose one rounding (sum + 8) >> 4 the two
    passes reproduce exactly - so the scaled call equals xgpu_pic_output_device bit for bit, for every chroma_loc, in the samples (the YUV444 layouts, every
    dtype) and in integer R'G'B'.  R'G'B' floats: the scaled kernel rounds every float32 operation of section 8a's matrix on its own, as the restatement does
    (checked bit for bit above); the unscaled kernel leaves the compiler free to fuse them, which is why its own suite allows it 4e-6 against the same
    restatement - that is the bound between the two here."""
    import torch
    planes = random_planes(144, 88, bd, seed=31 + bd, rails=True)
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    try:
        for loc, crop in itertools.product(range(6), ((0, 0, 0, 0), (2, 6, 4, 2))):
            size = (h - crop[2] - crop[3], w - crop[0] - crop[1])
            for layout, code, cl in (("yuv444", abi.OUT_U16, False), ("yuv444", abi.OUT_U8, True), ("yuv444", abi.OUT_F32, False), ("yuv444", abi.OUT_BF16, True),
                                     ("rgb", abi.OUT_U8, False), ("rgb", abi.OUT_U16, True)):
                kw = dict(layout=layout, channels_last=cl, dtype=torch_dtype(code), chroma_loc=loc, crop=crop)
                a = dec.pic_output_tensor(pic, size=size, **kw)
                b = dec.pic_output_tensor(pic, upsample="linear", **kw)
                assert np.array_equal(tensor_bits(a, code), tensor_bits(b, code)), (loc, crop, layout, code)
            kw = dict(layout="rgb", dtype=torch.float32, chroma_loc=loc, crop=crop)
            a, b = dec.pic_output_tensor(pic, size=size, **kw), dec.pic_output_tensor(pic, **kw)
            torch.cuda.synchronize()
            assert float((a.double() - b.double()).abs().max()) <= 4e-6, (loc, crop)
    finally:
        dec.close()


def test_streams_and_table_reuse():
    """a non-default torch stream and the null stream, alternating sizes (the tap tables and the intermediate are the context's: rebuilt and regrown between
    calls), no synchronisation between a call and the reduction that reads its tensor"""
    import torch
    bd = 10
    pa = random_planes(320, 176, bd, seed=41)
    pb = random_planes(320, 176, bd, seed=43, rails=True)
    dec, pic_a = open_picture(pa, bd)
    try:
        pic_b = dec.pic_alloc()
        dec.pic_upload(pic_b, pb)
        sizes = ((40, 72), (150, 300), (40, 72), (11, 20))
        sums = {(k, s): int(sr.convert(p, bd, s, dtype=cr.U16, lib=dec.lib).astype(np.int64).sum()) for k, p in (("a", pa), ("b", pb)) for s in set(sizes)}
        order = [("a", sizes[0]), ("b", sizes[1]), ("a", sizes[2]), ("b", sizes[3]), ("a", sizes[1]), ("b", sizes[0])]
        side = torch.cuda.Stream(device=0)
        for stream in (side, torch.cuda.default_stream(0)):
            got = []
            with torch.cuda.stream(stream):
                for k, s in order:
                    t = dec.pic_output_tensor(pic_a if k == "a" else pic_b, dtype=torch.int16, size=s)
                    got.append(t.to(torch.int64).sum())
                    del t
            stream.synchronize()
            assert [int(g) for g in got] == [sums[o] for o in order]
        # two streams in turn on one context: each call behind the previous one
        other = torch.cuda.Stream(device=0)
        got = []
        for i, (k, s) in enumerate(order):
            with torch.cuda.stream(side if i & 1 else other):
                got.append(dec.pic_output_tensor(pic_a if k == "a" else pic_b, dtype=torch.int16, size=s).to(torch.int64).sum())
        torch.cuda.synchronize()
        assert [int(g) for g in got] == [sums[o] for o in order]
        # the C ABI's stream = NULL: the context's own stream
        fmt, sc = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_scale_params(72, 40)
        t = torch.zeros((3, 40, 72), dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        assert dec.lib.xgpu_pic_output_device_scaled(dec.ctx, pic_a, None, C.byref(fmt), C.byref(sc), C.c_void_p(t.data_ptr()), t.numel() * 2, None) == 0
        dec.sync()
        check(t, sr.convert(pa, bd, (40, 72), dtype=cr.U16, lib=dec.lib), abi.OUT_U16, what="null stream")
    finally:
        dec.close()


def test_refusals_queue_nothing():
    import torch
    bd = 8
    planes = random_planes(256, 128, bd, seed=47)
    dec, pic = open_picture(planes, bd)
    lib = dec.lib
    try:
        fmt, sc = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_scale_params(100, 60)
        need = lib.xgpu_output_scaled_size(C.byref(fmt), C.byref(sc), 256, 128, bd)
        assert need == 3 * 60 * 100 * 2
        t = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        host = np.zeros(need, np.uint8)
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(f, s, p=None, n=need):
            return lib.xgpu_pic_output_device_scaled(dec.ctx, pic, None, C.byref(f), C.byref(s), C.c_void_p(t.data_ptr() if p is None else p), n, stream_h)

        assert call(fmt, sc, host.ctypes.data) == -101              # host memory
        assert call(fmt, sc, n=need - 1) == -101                    # too short
        assert call(fmt, sc, t.data_ptr() + 1) == -101              # not aligned to the 2-byte element
        assert b"pic_output_device_scaled" in lib.xgpu_last_error(dec.ctx)
        for layout, dtype in ((abi.OUT_YUV420P, abi.OUT_U16), (abi.OUT_NV12, abi.OUT_U8), (abi.OUT_P016, abi.OUT_U16)):
            assert call(abi.make_output_format(layout, dtype, out_bit_depth=8 if dtype == abi.OUT_U8 else 0), sc) == -101
        assert call(fmt, abi.make_scale_params(3, 60)) == -104      # below 1 / 64 of 256
        assert call(fmt, abi.make_scale_params(100, 1025)) == -104  # above 8 x 128
        assert call(fmt, abi.make_scale_params(100, 60, mean=MEAN, std=STD)) == -101      # normalise into integers
        f32 = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F16)
        assert call(f32, abi.make_scale_params(100, 60, mean=(0.5, float("nan"), 0.5))) == -101
        assert call(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, crop=(1, 0, 0, 0)), sc) == -101
        assert call(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, matrix=2), sc) == -104
        assert call(fmt, abi.make_scale_params(100, 60, filter=5)) == -101
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all()
        for bad in (dict(size=(60, 100), layout="nv12"), dict(size=(60, 100), mean=MEAN), dict(size=(60, 100), filter="lanczos"), dict(size=(1, 100)),
                    dict(mean=MEAN, dtype=torch.float32), dict(size=(60, 100), colour=dict(dst_transfer=13))):
            with pytest.raises(ValueError):
                dec.pic_output_tensor(pic, **bad)
        assert call(fmt, sc) == 0                                   # and the context still works
        check(t[:need].view(torch.int16).view(3, 60, 100), sr.convert(planes, bd, (60, 100), dtype=cr.U16, lib=lib), abi.OUT_U16, what="after the refusals")
    finally:
        dec.close()


def test_golden_stream_resized_and_normalised():
    """a committed stream through StreamDecoder.pictures(tensor=..., size=..., mean=..., std=...): every picture is the restatement of its decoded planes"""
    import torch
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))["bytes"].tobytes()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]
    opts = dict(dtype=torch.float32, matrix=1, full_range=False, chroma_loc=0, crop=(0, 0, 0, 0), dra=None)
    sd = StreamDecoder(data)
    lib = abi.load()
    got = [t for _, t in sd.pictures(tensor=opts, size=(48, 64), mean=MEAN, std=STD)]
    assert len(got) == len(ref) > 1
    for t, (p, planes) in zip(got, ref):
        assert tuple(t.shape) == (3, 48, 64)
        exp = sr.convert(planes, p["bit_depth"], (48, 64), dtype=cr.F32, lib=lib, mean=np.asarray(MEAN, np.float32), inv_std=inv_std(STD))
        check(t, exp, abi.OUT_F32, what=("stream", p["poc"]))
    # the box filter through the tensor options, integers, channels last
    got = [t for _, t in StreamDecoder(data).pictures(tensor=dict(opts, dtype=torch.uint8, channels_last=True, filter="area"), size=(30, 44))]
    for t, (p, planes) in zip(got, ref):
        check(t, sr.convert(planes, p["bit_depth"], (30, 44), filt=sr.AREA, dtype=cr.U8, lib=lib), abi.OUT_U8, True, ("stream area", p["poc"]))
    with pytest.raises(ValueError):
        next(iter(StreamDecoder(data).pictures(size=(48, 64))))
