"""GPU suite for the 3D LUT output (xgpu_pic_output_device_lut3d / _packed_lut3d / XgpuDecoder.pic_output_lut3d / StreamDecoder lut= / the tool's --lut;
INTEGRATION.md section 8q).  Every element the device writes - the integer dtypes and the bits of the three float dtypes - is held to the numpy restatement
tests/lut3d_ref.py; the packed surfaces are held to the interleaved LUT call (R, G, B) and to section 8p's alpha; the identity LUT is held to pic_output_tensor.
Pictures: test_gpu_output_packed.py's - the committed goldens, and random and rail-to-rail planes at 8x8 cropped to 2x2, 24x16 cropped to 18x10 and 528x16 cropped
to 522x14, at 8, 10 and 12 bit.  Cubes: the identity and seeded random uint16 nodes (any wrong vertex, order or weight shows against those) at n = 2, 17, 33, 65;
shapers: the identity and a seeded random, non-monotone one.  The kernel reads its tables the same way at every n (the shaper in LDS, the cube from global memory),
so there is no size at which it changes path.
Census condition (from the restatement, on the CPU, inside the tests): for every (random picture of at least 18x10, n) all six strict orderings of (f_R, f_G, f_B)
are reached; for every rails picture the top-cell clamp (some f = 65535) and the tie bucket are reached with the identity shaper."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_io
import lut3d_ref as lr
import packed_ref as pr
from xevd_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_NAMES = {abi.OUT_U8: "uint8", abi.OUT_U16: "int16", abi.OUT_F16: "float16", abi.OUT_BF16: "bfloat16", abi.OUT_F32: "float32"}
GOLDENS = ["base_p_8b", "base_p_10b", "base_p_12b"]
SHAPES = [(8, 8, (2, 4, 4, 2)), (24, 16, (2, 4, 2, 4)), (528, 16, (2, 4, 2, 0))]      # (width, height, crop) -> 2x2, 18x10, 522x14
NS = (2, 17, 33, 65)
LUTS = [(n, ck, sk) for n in NS for ck, sk in (("random", "random"), ("random", "identity"), ("identity", "random"))]
# the conversions in front of the LUT: (matrix, full_range, chroma_loc, upsample)
CONVS = [(1, False, 0, "linear"), (9, True, 3, "linear"), (5, False, 0, "nearest"), (9, False, 2, "linear"), (6, True, 5, "linear"), (1, True, 0, "nearest")]


def torch_dtype(code):
    import torch
    return getattr(torch, DT_NAMES[code])


def golden_planes(name):
    d = np.load(os.path.join(golden_io.GOLDEN, f"pic_{name}.npz"))
    w, h, bd = (int(v) for v in d["params"][:3])
    pl, pc = abi.PAD_L, abi.PAD_C
    return [d["out_0"][pl:pl + h, pl:pl + w], d["out_1"][pc:pc + h // 2, pc:pc + w // 2], d["out_2"][pc:pc + h // 2, pc:pc + w // 2]], bd


def small_planes(w, h, bd, kind, seed=5):
    """random samples over the whole range, or a checker of the rails 0 and 2^B - 1 (luma and the two chroma planes out of phase)"""
    top = (1 << bd) - 1
    if kind == "random":
        rng = np.random.default_rng(seed + w + bd)
        return [rng.integers(0, top + 1, s).astype(np.int16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    return [(((yy + xx) & 1) * top).astype(np.int16), ((((cy >> 1) + cx) & 1) * top).astype(np.int16), (((cy + (cx >> 1) + 1) & 1) * top).astype(np.int16)]


def pictures():
    for name in GOLDENS:
        planes, bd = golden_planes(name)
        yield name, planes, bd, ((0, 0, 0, 0), (2, 4, 2, 6))
    for (w, h, crop), bd, kind in itertools.product(SHAPES, (8, 10, 12), ("random", "rails")):
        yield f"{kind}_{w}x{h}_{bd}b", small_planes(w, h, bd, kind), bd, (crop,)


PICTURES = {name: (planes, bd, crops) for name, planes, bd, crops in pictures()}


def open_picture(planes, bd):
    from xevd_amd.decoder import XgpuDecoder
    h, w = planes[0].shape
    dec = XgpuDecoder(w, h, bd, device=0, max_pics=4)
    pic = dec.pic_alloc()
    dec.pic_upload(pic, planes)
    return dec, pic


@functools.lru_cache(maxsize=None)
def cube(kind, n):
    if kind == "identity":
        return lr.identity_cube(n)
    return np.random.default_rng(100 + n).integers(0, 65536, (n ** 3, 3)).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def shaper(kind, bd):
    """None: the call's own identity; else seeded random positions, non-monotone, the rails included"""
    if kind == "identity":
        return None
    s = np.random.default_rng(200 + bd).integers(0, 65536, (3, 1 << bd)).astype(np.uint16)
    s[:, 3], s[:, 5] = 0, 65535
    return s


def bits(t):
    """a device tensor as a numpy array of unsigned integers of its element size"""
    import torch
    torch.cuda.synchronize()
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])


def same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


def conv_kw(conv, crop):
    """(keyword arguments of the restatement, of the decoder's call)"""
    m, fr, loc, mode = conv
    return dict(matrix=m, full_range=fr, chroma_loc=loc, mode=mode, crop=crop), dict(matrix=m, full_range=fr, chroma_loc=loc, upsample=mode, crop=crop)


@functools.lru_cache(maxsize=None)
def reference(name, n, ck, sk, conv, crop):
    """(v [3][H][W] in 0 .. 65535, census) of picture `name` through LUT (n, ck, sk); the census condition of the suite is asserted here, on the CPU"""
    planes, bd, _ = PICTURES[name]
    shp = shaper(sk, bd)
    v, census = lr.interpolate(lr.codes_of(planes, bd, **conv_kw(conv, crop)[0]), lr.identity_shaper(bd) if shp is None else shp, cube(ck, n), n)
    if name.startswith("random") and v.shape[1] * v.shape[2] >= 18 * 10:
        assert all(census[k] > 0 for k in lr.ORDERINGS), (name, n, ck, sk, conv, census)
    if name.startswith("rails") and sk == "identity":
        assert census["clamp"] > 0 and census["tie"] > 0, (name, n, ck, sk, conv, census)
    return v, census


def rgb_cases(name, luts=LUTS):
    """every call of the main test on picture `name`: the LUTs in turn, each with the five dtypes in both layouts; conversion, crop, bgr and out_bit_depth rotate"""
    _, bd, crops = PICTURES[name]
    k = 0
    for n, ck, sk in luts:
        for code, chl in itertools.product(DT_NAMES, (False, True)):
            obd = (0, bd, 16)[k % 3] if code == abi.OUT_U16 else (0, bd)[k % 2]
            yield (n, ck, sk), CONVS[k % len(CONVS)], crops[k % len(crops)], code, chl, bool((k >> 1) & 1), obd
            k += 1


def expected_rgb(name, lut, conv, crop, code, bgr, obd):
    _, bd, _ = PICTURES[name]
    v, _ = reference(name, *lut, conv, crop)
    e = lr.store(v, code, lr.store_depth(code, bd, obd))
    return e[::-1] if bgr else e


def check_rgb_cases(name, luts=LUTS):
    planes, bd, _ = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        handles = {}
        for lut, conv, crop, code, chl, bgr, obd in rgb_cases(name, luts):
            if lut not in handles:
                for h in handles.values():      # one at a time here; test_two_luts_in_one_context keeps several
                    dec.lut3d_destroy(h)
                handles = {lut: dec.lut3d_create(cube(lut[1], lut[0]), shaper(lut[2], bd))}
            t = dec.pic_output_lut3d(pic, handles[lut], channels_last=chl, dtype=torch_dtype(code), out_bit_depth=obd, bgr=bgr, **conv_kw(conv, crop)[1])
            got = bits(t)
            got = np.moveaxis(got, -1, 0) if chl else got
            exp = expected_rgb(name, lut, conv, crop, code, bgr, obd)
            assert got.shape == exp.shape and got.dtype == exp.dtype, (name, lut, code, chl)
            assert np.array_equal(got, exp), (name, lut, conv, crop, code, chl, bgr, obd, int((got != exp).sum()))
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ against tests/lut3d_ref.py
@pytest.mark.parametrize("name", list(PICTURES))
def test_every_dtype_and_layout_equals_the_restatement(name):
    check_rgb_cases(name)


@pytest.mark.parametrize("name", ["base_p_12b", "random_528x16_12b", "rails_24x16_8b"])
def test_identity_cube_behind_identity_shaper_in_every_dtype(name):
    """v = p here, which at 12 bit takes values whose float32 quotient lies exactly between two halves (65519 / 65535 -> 1 - 2^-12): the product is rounded to
    float32 before it is rounded to the dtype"""
    check_rgb_cases(name, [(n, "identity", "identity") for n in (2, 17, 65)])


def fields(words, bgr=False):
    """[H][W] 10:10:10:2 words -> ([3][H][W] R, G, B, [H][W] A)"""
    w = np.asarray(words).astype(np.int64)
    lo, mid, hi = w & 1023, (w >> 10) & 1023, (w >> 20) & 1023
    return np.stack([hi, mid, lo] if bgr else [lo, mid, hi]), w >> 30


@pytest.mark.parametrize("name", GOLDENS + ["random_24x16_8b", "rails_24x16_10b", "random_528x16_10b", "rails_528x16_12b", "rails_8x8_10b"])
def test_packed_surfaces(name):
    """RGBA: R, G, B are the interleaved LUT call's bits, A is section 8p's; 10:10:10:2: the restatement"""
    import torch
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        k = 0
        for n, ck, sk in ((17, "random", "random"), (33, "random", "identity"), (2, "identity", "random")):
            lut = dec.lut3d_create(cube(ck, n), shaper(sk, bd))
            for code, bgr in itertools.product(DT_NAMES, (False, True)):
                conv, crop, alpha = CONVS[k % len(CONVS)], crops[k % len(crops)], (1.0, 0.0, 0.5, 1 / 3)[k % 4]
                k += 1
                rkw, dkw = conv_kw(conv, crop)
                t = dec.pic_output_lut3d(pic, lut, layout="bgra" if bgr else "rgba", dtype=torch_dtype(code), alpha=alpha, **dkw)
                ref = dec.pic_output_lut3d(pic, lut, channels_last=True, bgr=bgr, dtype=torch_dtype(code), **dkw)
                assert t.dtype == torch_dtype(code) and tuple(t.shape) == tuple(ref.shape[:2]) + (4,)
                assert same_bits(t[..., :3], ref), (name, n, code, bgr, conv)
                assert (bits(t[..., 3]) == pr.alpha_element(alpha, code, bd)).all(), (name, code, alpha)
                if code == abi.OUT_U8:      # once per (LUT, order): the 10:10:10:2 word
                    w = dec.pic_output_lut3d(pic, lut, layout="bgr10a2" if bgr else "rgb10a2", alpha=alpha, **dkw)
                    assert w.dtype == torch.int32 and w.dim() == 2
                    shp = shaper(sk, bd)
                    assert np.array_equal(bits(w), lr.rgb10a2(planes, bd, cube(ck, n), n, shp, bgr=bgr, alpha=alpha, **rkw)), (name, n, bgr, conv)
                    rgb, a = fields(bits(w), bgr)
                    assert np.array_equal(rgb, lr.store(reference(name, n, ck, sk, conv, crop)[0], lr.U16, 10)) and (a == pr.alpha_code(alpha, 2)).all()
            dec.lut3d_destroy(lut)
    finally:
        dec.close()


@pytest.mark.parametrize("name", list(PICTURES))
def test_identity_lut_is_the_plain_rgb_tensor(name):
    import torch
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        for k, n in enumerate((2, 3, 17, 32, 33, 64, 65)):
            lut = dec.lut3d_create(cube("identity", n), None if k & 1 else lr.identity_shaper(bd))
            for j, (conv, chl) in enumerate(itertools.product(CONVS, (False, True))):
                dkw = conv_kw(conv, crops[(j + k) % len(crops)])[1]
                a = dec.pic_output_lut3d(pic, lut, channels_last=chl, dtype=torch.int16, bgr=bool(j & 2), **dkw)
                assert same_bits(a, dec.pic_output_tensor(pic, layout="rgb", channels_last=chl, dtype=torch.int16, bgr=bool(j & 2), **dkw)), (name, n, conv, chl)
                if bd == 8:
                    a = dec.pic_output_lut3d(pic, lut, channels_last=chl, dtype=torch.uint8, **dkw)
                    assert same_bits(a, dec.pic_output_tensor(pic, layout="rgb", channels_last=chl, dtype=torch.uint8, **dkw)), (name, n, conv, chl)
            dec.lut3d_destroy(lut)
    finally:
        dec.close()


def test_dra_tables_on_the_10_bit_picture():
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    dec, pic = open_picture(planes, 10)
    try:
        n = 17
        lut = dec.lut3d_create(cube("random", n), shaper("random", 10))
        for (name, crop), mode, code in itertools.product((("three_ranges_idx58", (0, 0, 0, 0)), ("five_ranges_idx40", (2, 4, 2, 0))), ("linear", "nearest"),
                                                          (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16)):
            luts = d[f"{name}_luts"]
            t = dec.pic_output_lut3d(pic, lut, dtype=torch_dtype(code), matrix=9, chroma_loc=1, upsample=mode, crop=crop, dra=luts)
            exp, _ = lr.lut3d(planes, 10, cube("random", n), n, shaper("random", 10), dtype=code, matrix=9, chroma_loc=1, mode=mode, crop=crop, dra=luts)
            assert np.array_equal(bits(t), exp), (name, mode, code)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ handles, destinations, streams
def test_two_luts_in_one_context_used_alternately():
    import torch
    name = "random_24x16_10b"
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        la, lb = (33, "random", "random"), (17, "identity", "random")
        ha, hb = (dec.lut3d_create(cube(l[1], l[0]), shaper(l[2], bd)) for l in (la, lb))
        assert ha != hb
        rkw, dkw = conv_kw(CONVS[0], crops[0])
        ea, eb = (lr.store(reference(name, *l, CONVS[0], crops[0])[0], lr.U16, bd) for l in (la, lb))
        assert not np.array_equal(ea, eb)
        outs = [(h, dec.pic_output_lut3d(pic, h, dtype=torch.int16, **dkw)) for h in (ha, hb, ha, hb, hb, ha)]      # queued back to back, read afterwards
        for h, t in outs:
            assert np.array_equal(bits(t), ea if h == ha else eb), h
        dec.lut3d_destroy(ha)
        with pytest.raises(Exception):
            dec.pic_output_lut3d(pic, ha, dtype=torch.int16, **dkw)      # the handle names nothing now
        assert np.array_equal(bits(dec.pic_output_lut3d(pic, hb, dtype=torch.int16, **dkw)), eb)
        hc = dec.lut3d_create(cube("random", 2))
        assert hc == ha      # the freed handle is handed out again
        more = [dec.lut3d_create(cube("identity", 2)) for _ in range(abi.MAX_LUT3D - 2)]
        assert sorted([hb, hc] + more) == list(range(abi.MAX_LUT3D))
        with pytest.raises(Exception):
            dec.lut3d_create(cube("identity", 2))      # a small fixed number per context
        with pytest.raises(Exception):
            dec.lut3d_destroy(abi.MAX_LUT3D)
    finally:
        dec.close()


def test_padded_destinations_keep_their_padding():
    """views into wider tensors: pitches and offsets that are multiples of 16 bytes (vector stores) and that are not (element stores) - the same elements as
    the tight call's, the padding untouched"""
    import torch
    for name in ("base_p_10b", "random_528x16_10b"):
        planes, bd, crops = PICTURES[name]
        dec, pic = open_picture(planes, bd)
        try:
            lut = dec.lut3d_create(cube("random", 33), shaper("random", bd))
            forms = [("rgb", "uint8", 3), ("rgb", "int16", 3), ("rgb", "float32", 3), ("rgba", "bfloat16", 4), ("bgra", "uint8", 4), ("rgb10a2", "int32", 1)]
            for (layout, dtn, last), mode in itertools.product(forms, ("linear", "nearest")):
                dt = getattr(torch, dtn)
                kw = dict(layout=layout, upsample=mode, crop=crops[-1])
                if layout == "rgb":
                    kw.update(channels_last=True, dtype=dt)
                elif layout != "rgb10a2":
                    kw.update(dtype=dt, alpha=0.5)
                tight = dec.pic_output_lut3d(pic, lut, **kw)
                h, w = tight.shape[:2]
                al = (-w) % 16 + 16
                for pad, off in ((al, 16), (al, 1), (3, 1), (5, 0)):
                    big = torch.full((h, w + pad) + tight.shape[2:], 7, dtype=dt, device="cuda:0")
                    view = big[:, off:off + w]
                    assert dec.pic_output_lut3d(pic, lut, out=view, **kw) is view
                    assert same_bits(view, tight), (name, layout, dtn, mode, pad, off)
                    rest = torch.cat([big[:, :off].flatten(), big[:, off + w:].flatten()])
                    assert bool((rest == 7).all()), (name, layout, dtn, mode, pad, off)
            # the planar layout: rows of a plane a pitch apart
            tight = dec.pic_output_lut3d(pic, lut, dtype=torch.int16, crop=crops[-1])
            _, h, w = tight.shape
            big = torch.full((3, h, w + 5), 7, dtype=torch.int16, device="cuda:0")
            view = big[:, :, 2:2 + w]
            dec.pic_output_lut3d(pic, lut, dtype=torch.int16, crop=crops[-1], out=view)
            assert same_bits(view, tight) and bool((big[:, :, :2] == 7).all()) and bool((big[:, :, 2 + w:] == 7).all())
        finally:
            dec.close()


def test_a_callers_stream():
    """output on a non-default torch stream, then the next picture uploaded into the same slot by the context's stream, with no synchronisation in between:
    every output holds the picture it was asked for"""
    import torch
    pa, bd, _ = PICTURES["base_p_10b"]
    pb = [np.asarray((p.astype(np.int32) * 3 + 101) % (1 << bd), np.int16) for p in pa]
    dec, pic = open_picture(pa, bd)
    try:
        n = 33
        lut = dec.lut3d_create(cube("random", n), shaper("random", bd))
        exp = {k: lr.lut3d(p, bd, cube("random", n), n, shaper("random", bd), dtype=lr.U16)[0] for k, p in (("a", pa), ("b", pb))}
        exp10 = {k: lr.rgb10a2(p, bd, cube("random", n), n, shaper("random", bd)) for k, p in (("a", pa), ("b", pb))}
        assert not np.array_equal(exp["a"], exp["b"])
        default = bits(dec.pic_output_lut3d(pic, lut, dtype=torch.int16))
        assert np.array_equal(default, exp["a"])
        s = torch.cuda.Stream(device=0)
        got = []
        with torch.cuda.stream(s):
            for k in "abab":
                if got:
                    dec.pic_upload(pic, pa if k == "a" else pb)      # into the slot the previous output reads
                got.append((k, dec.pic_output_lut3d(pic, lut, dtype=torch.int16), dec.pic_output_lut3d(pic, lut, layout="rgb10a2")))
        s.synchronize()
        for k, t, t10 in got:
            assert np.array_equal(bits(t), exp[k]) and np.array_equal(bits(t10), exp10[k]), k
    finally:
        dec.close()


def test_refusals_leave_the_destination_untouched():
    import torch
    planes, bd, _ = PICTURES["base_p_10b"]
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    lib = dec.lib
    try:
        lut = dec.lut3d_create(cube("random", 17))
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rgb = abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_U8)
        rgb16 = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, out_bit_depth=16)
        rgba = abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_U8)
        r10 = abi.make_packed_format(abi.PACKED_RGB10A2)
        need = lib.xgpu_output_format_size(C.byref(rgb), w, h, bd)
        need4 = lib.xgpu_output_packed_size(C.byref(rgba), w, h, bd)
        assert need == 3 * w * h and need4 == 4 * w * h
        t = torch.full((need4 + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        hostbuf = np.zeros(need4, np.uint8)
        plain = [(rgb, lut, t.data_ptr(), need - 1, -101),                              # one byte short
                 (rgb, lut, hostbuf.ctypes.data, need, -101),                           # host memory
                 (rgb16, lut, t.data_ptr() + 1, 2 * need, -101),                        # the element is aligned to 2
                 (rgb, -1, t.data_ptr(), need, -101), (rgb, abi.MAX_LUT3D, t.data_ptr(), need, -101), (rgb, lut + 1, t.data_ptr(), need, -101),      # no such LUT
                 (abi.make_output_format(abi.OUT_RGB_PLANAR, matrix=2), lut, t.data_ptr(), need, -104),
                 (abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, out_bit_depth=16), lut, t.data_ptr(), need, -101),
                 (abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F16, out_bit_depth=16), lut, t.data_ptr(), 2 * need, -101),
                 (abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_U8), lut, t.data_ptr(), need, -101),
                 (abi.make_output_format(abi.OUT_NV12, abi.OUT_U16), lut, t.data_ptr(), need, -101)]
        for f, l, p, n, code in plain:
            rc = lib.xgpu_pic_output_device_lut3d(dec.ctx, pic, None, C.byref(f), l, C.c_void_p(p), n, stream_h)
            assert rc == code, (f.layout, f.dtype, l, n, rc)
            assert b"pic_output_device_lut3d" in lib.xgpu_last_error(dec.ctx)
        packed = [(rgba, lut, t.data_ptr(), need4 - 1, -101), (r10, lut, t.data_ptr() + 2, need4, -101), (rgba, 5, t.data_ptr(), need4, -101),
                  (abi.make_packed_format(abi.PACKED_YUYV, abi.OUT_U8, out_bit_depth=8), lut, t.data_ptr(), need4, -101),      # 4:2:2 takes no LUT
                  (abi.make_packed_format(abi.PACKED_UYVY, abi.OUT_U16), lut, t.data_ptr(), need4, -101),
                  (abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_U16, out_bit_depth=16), lut, t.data_ptr(), 2 * need4, -101),
                  (abi.make_packed_format(abi.PACKED_RGBA, alpha=1.5), lut, t.data_ptr(), need4, -101),
                  (abi.make_packed_format(abi.PACKED_RGBA, matrix=2), lut, t.data_ptr(), need4, -104)]
        for f, l, p, n, code in packed:
            rc = lib.xgpu_pic_output_device_packed_lut3d(dec.ctx, pic, None, C.byref(f), l, C.c_void_p(p), n, stream_h)
            assert rc == code, (f.layout, f.dtype, l, n, rc)
            assert b"pic_output_device_packed_lut3d" in lib.xgpu_last_error(dec.ctx)
        hdl = C.c_int(7)
        nodes = cube("random", 2)
        assert lib.xgpu_lut3d_create(dec.ctx, 1, nodes.ctypes.data_as(C.POINTER(C.c_uint16)), None, C.byref(hdl)) == -104 and hdl.value == -1
        assert lib.xgpu_lut3d_create(dec.ctx, 66, nodes.ctypes.data_as(C.POINTER(C.c_uint16)), None, C.byref(hdl)) == -104
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all() and not hostbuf.any()
        assert lib.xgpu_pic_output_device_lut3d(dec.ctx, pic, None, C.byref(rgb), lut, C.c_void_p(t.data_ptr()), need, stream_h) == 0      # exactly `need` bytes
        torch.cuda.synchronize()
        assert (t[need:].cpu().numpy() == 0x5A).all()
        exp, _ = lr.lut3d(planes, bd, cube("random", 17), 17, dtype=lr.U8)
        assert np.array_equal(t[:need].cpu().numpy().reshape(h, w, 3), np.moveaxis(exp, 0, -1))
        # the Python layer's own argument checks
        for kw in (dict(layout="yuyv"), dict(layout="yuv444"), dict(layout="rgb10a2", dtype=torch.int16), dict(layout="rgba", out_bit_depth=16, dtype=torch.int16),
                   dict(dtype=torch.uint8, out_bit_depth=16), dict(dtype=torch.float32, out_bit_depth=16), dict(layout="rgba", channels_last=True),
                   dict(layout="rgba", alpha=-0.5), dict(matrix=2), dict(upsample="cubic"), dict(crop=(1, 0, 0, 0)),
                   dict(out=torch.empty((3, h, w), dtype=torch.uint8, device="cuda:0")[:, :, ::2])):
            with pytest.raises(ValueError):
                dec.pic_output_lut3d(pic, lut, **kw)
        with pytest.raises(ValueError):
            dec.lut3d_create(np.zeros((9, 3), np.uint16))      # no cube
        with pytest.raises(ValueError):
            dec.lut3d_create(cube("random", 2), np.zeros((3, 256), np.uint16))      # a shaper of another depth
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ the .cube file, the stream and the tool
def write_cube(path, n, rng, domain=None):
    """a .cube file of random values in [0, 1] (six decimals) -> the float32 nodes a reader gets from it"""
    vals = np.round(rng.uniform(0, 1, (n ** 3, 3)), 6)
    with open(path, "w") as f:
        f.write(f'TITLE "random {n}"\n# a comment\nLUT_3D_SIZE {n}\n')
        if domain is not None:
            f.write("DOMAIN_MIN {} {} {}\nDOMAIN_MAX {} {} {}\n".format(*domain[0], *domain[1]))
        f.write("\n".join("{:.6f} {:.6f} {:.6f}".format(*v) for v in vals) + "\n")
    return np.array([[float("{:.6f}".format(x)) for x in v] for v in vals], np.float32)


def test_stream_decoder_lut(tmp_path):
    import torch
    from xevd_amd.player import StreamDecoder
    d = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))
    data = d["bytes"].tobytes()
    path = str(tmp_path / "look.cube")
    domain = ((0.0, 0.05, 0.1), (1.0, 0.95, 0.9))
    vals = write_cube(path, 9, np.random.default_rng(31), domain)
    nodes = lr.from_float(vals)
    shp = lr.shaper(10, None, *domain)
    seen = []
    for p, t in StreamDecoder(data).pictures(tensor=dict(dtype=torch.int16, channels_last=True), packed=dict(layout="bgra", alpha=0.5), lut=path):
        seen.append((p, t, p["packed"]))
    assert len(seen) == int(d["n"])
    for k, (p, t, pk) in enumerate(seen):
        planes = [d[f"p{k}_{c}"] for c in range(3)]
        dec, pic = open_picture(planes, 10)
        try:
            lut = dec.lut3d_create(path)
            kw = StreamDecoder.tensor_options(p, {})
            assert same_bits(t, dec.pic_output_lut3d(pic, lut, dtype=torch.int16, channels_last=True, **kw)), k
            assert same_bits(pk, dec.pic_output_lut3d(pic, lut, layout="bgra", alpha=0.5, **kw)), k
            rkw = dict(matrix=kw["matrix"], full_range=kw["full_range"], chroma_loc=kw["chroma_loc"], dra=kw["dra"])
            exp, _ = lr.lut3d(planes, 10, nodes, 9, shp, dtype=lr.U16, **rkw)
            assert np.array_equal(np.moveaxis(bits(t), -1, 0), exp), k
        finally:
            dec.close()
    for kw in (dict(to="srgb"), dict(size=(32, 32)), dict(size=(32, 32), rois=[(0, 0, 16, 16)]), dict(size=(32, 32), warp=[[1, 0, 0, 0, 1, 0]]),
               dict(size=(32, 32), remap=np.zeros((32, 32, 2), np.float32)), dict(surfaces=[(44, 72)])):
        with pytest.raises(ValueError, match="lut"):
            next(StreamDecoder(data).pictures(tensor={}, lut=path, **kw))
    with pytest.raises(ValueError, match="lut"):
        next(StreamDecoder(data).pictures(lut=path))
    with pytest.raises(ValueError, match="lut"):
        next(StreamDecoder(data).pictures(packed=dict(layout="yuyv"), lut=path))
    with pytest.raises(ValueError, match="lut"):
        next(StreamDecoder(data).pictures(tensor=dict(layout="nv12"), lut=path))


@pytest.mark.parametrize("pix_fmt", [None, "x2bgr10le"])
def test_app_writes_lut_files(pix_fmt, tmp_path):
    """tools/xevd_gpu_app.py --lut FILE.cube as a child process: interleaved 8-bit RGB frames, or the packed --pix-fmt, against the restatement on the frames of
    its default yuv420p run"""
    name, bd, n = "ippp_10b_offsets", 10, 5
    d = np.load(os.path.join(golden_io.GOLDEN, f"stream_{name}.npz"))
    h, w = d["p0_0"].shape
    count = int(d["n"])
    src, planar, out, path = tmp_path / "s.evc", tmp_path / "planar.yuv", tmp_path / "lut.raw", str(tmp_path / "look.cube")
    src.write_bytes(d["bytes"].tobytes())
    nodes = lr.from_float(write_cube(path, n, np.random.default_rng(32)))
    app = os.path.join(ROOT, "tools", "xevd_gpu_app.py")
    for args in (["-o", str(planar)], ["-o", str(out), "--lut", path] + (["--pix-fmt", pix_fmt] if pix_fmt else [])):
        r = subprocess.run([sys.executable, app, "-i", str(src)] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-2000:])
    a = np.fromfile(planar, np.dtype("<u2")).astype(np.int16)
    frame = w * h * 3 // 2
    assert a.size == count * frame
    b = np.fromfile(out, np.uint8 if pix_fmt is None else np.dtype("<u4"))
    assert b.size == count * w * h * (3 if pix_fmt is None else 1)
    b = b.reshape(count, h, w, -1)
    for k in range(count):
        f = a[k * frame:(k + 1) * frame]
        planes = [f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)]
        if pix_fmt is None:
            exp = np.moveaxis(lr.lut3d(planes, bd, nodes, n, dtype=lr.U8)[0], 0, -1)
        else:
            exp = lr.rgb10a2(planes, bd, nodes, n)[..., None]
        assert np.array_equal(b[k], exp), (pix_fmt, k)
    r = subprocess.run([sys.executable, app, "-i", str(src), "-o", str(out), "--lut", path, "--pix-fmt", "yuyv422"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--lut" in r.stderr
