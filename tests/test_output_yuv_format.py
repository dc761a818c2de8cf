"""CPU suite for the video-surface layouts of device output (NV12, P016, YUV444 planar / interleaved): xgpu_output_format_size against closed
forms, the formats it refuses, xgpu_output_coeffs staying an RGB function, and self-checks of the numpy restatement tests/yuv_ref.py that the GPU
suite holds the kernels to.  Nothing here needs a GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import colour_ref as cr
import yuv_ref as yr
from xevd_amd import abi

DTYPES = (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32)
ES = {abi.OUT_U8: 1, abi.OUT_U16: 2, abi.OUT_F16: 2, abi.OUT_BF16: 2, abi.OUT_F32: 4}
SEMI = (abi.OUT_NV12, abi.OUT_P016)
YUV444 = (abi.OUT_YUV444_PLANAR, abi.OUT_YUV444_INTERLEAVED)
# (width, height, crop): without crop, with crop, and crops that leave an odd chroma width (W / 2 odd)
SIZES = ((64, 48, (0, 0, 0, 0)), (64, 48, (2, 4, 2, 6)), (64, 48, (0, 2, 0, 0)), (72, 40, (4, 2, 2, 0)), (7680, 4320, (0, 0, 0, 0)))


def size(bd=10, width=64, height=48, **kw):
    return abi.load().xgpu_output_format_size(C.byref(abi.make_output_format(**kw)), width, height, bd)


def semi_formats(bd):
    """(layout, dtype, out_bit_depth) of every valid NV12 / P016 form at coding depth bd"""
    out = [(abi.OUT_NV12, abi.OUT_U8, 8)]
    out += [(abi.OUT_NV12, abi.OUT_U16, d) for d in ((0,) if bd > 8 else ()) + tuple(range(9, 17))]
    out += [(abi.OUT_P016, abi.OUT_U16, d) for d in (0,) + tuple(range(8, 17))]
    return out


def test_constants():
    assert (abi.OUT_NV12, abi.OUT_P016, abi.OUT_YUV444_PLANAR, abi.OUT_YUV444_INTERLEAVED) == (3, 4, 5, 6)
    assert C.sizeof(abi.OutputFormat) == 12 * 4 + C.sizeof(C.c_size_t)      # the struct kept its fields and size


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_size_of_semiplanar_layouts(bd):
    for (wd, ht, crop), (layout, dt, obd) in itertools.product(SIZES, semi_formats(bd)):
        w, h, es = wd - crop[0] - crop[1], ht - crop[2] - crop[3], ES[dt]
        for pitch in (0, w * es, w * es + 2, w * es + 64):
            got = size(bd, wd, ht, layout=layout, dtype=dt, out_bit_depth=obd, crop=crop, row_pitch=pitch)
            assert got == (h + h // 2 - 1) * (pitch or w * es) + w * es, (wd, ht, crop, layout, dt, obd, pitch)
        # fields these layouts do not read are not validated
        assert size(bd, wd, ht, layout=layout, dtype=dt, out_bit_depth=obd, crop=crop, matrix=2, chroma_loc=9, upsample=7) == (h + h // 2) * w * es


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_size_of_yuv444_layouts(bd):
    for (wd, ht, crop), layout, dt in itertools.product(SIZES, YUV444, DTYPES):
        w, h, es = wd - crop[0] - crop[1], ht - crop[2] - crop[3], ES[dt]
        row = w * es * (3 if layout == abi.OUT_YUV444_INTERLEAVED else 1)
        rows = h if layout == abi.OUT_YUV444_INTERLEAVED else 3 * h
        for pitch, obd in itertools.product((0, row, row + 4, row + 64), (0, bd)):
            got = size(bd, wd, ht, layout=layout, dtype=dt, out_bit_depth=obd, crop=crop, row_pitch=pitch, matrix=2)      # no matrix is read
            assert got == (rows - 1) * (pitch or row) + row, (wd, ht, crop, layout, dt, pitch)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_size_of_the_existing_layouts(bd):
    """the closed forms of xgpu_pic_output_size (YUV420P) and of INTEGRATION 8a (RGB), now reachable without a context"""
    for wd, ht, crop in SIZES:
        w, h = wd - crop[0] - crop[1], ht - crop[2] - crop[3]
        samples = w * h + 2 * (w // 2) * (h // 2)
        assert size(bd, wd, ht, layout=abi.OUT_YUV420P, dtype=abi.OUT_U8, out_bit_depth=8, crop=crop) == samples
        for obd in ((0,) if bd > 8 else ()) + tuple(range(9, 17)):
            assert size(bd, wd, ht, layout=abi.OUT_YUV420P, dtype=abi.OUT_U16, out_bit_depth=obd, crop=crop) == 2 * samples
        assert size(bd, wd, ht, layout=abi.OUT_YUV420P, dtype=abi.OUT_U8, out_bit_depth=8, crop=crop, row_pitch=w) == 0      # tight rows only
        for dt in DTYPES:
            es = ES[dt]
            for pitch_extra in (None, 0, 16):
                pp, pi = (0, 0) if pitch_extra is None else (w * es + pitch_extra, 3 * w * es + pitch_extra)
                assert size(bd, wd, ht, layout=abi.OUT_RGB_PLANAR, dtype=dt, crop=crop, row_pitch=pp) == (3 * h - 1) * (pp or w * es) + w * es
                assert size(bd, wd, ht, layout=abi.OUT_RGB_INTERLEAVED, dtype=dt, crop=crop, row_pitch=pi) == (h - 1) * (pi or 3 * w * es) + 3 * w * es
        assert size(bd, wd, ht, layout=abi.OUT_RGB_PLANAR, dtype=abi.OUT_U8, matrix=2) == 0


def test_refused_formats_have_size_zero():
    nv8 = dict(layout=abi.OUT_NV12, dtype=abi.OUT_U8, out_bit_depth=8)
    nv16 = dict(layout=abi.OUT_NV12, dtype=abi.OUT_U16)
    p16 = dict(layout=abi.OUT_P016, dtype=abi.OUT_U16)
    y444 = dict(layout=abi.OUT_YUV444_PLANAR, dtype=abi.OUT_U16)
    for ok in (nv8, nv16, p16, y444):
        assert size(10, **ok) > 0, ok
    bad = [dict(p16, dtype=abi.OUT_U8), dict(p16, dtype=abi.OUT_U8, out_bit_depth=8),                  # P016 with U8
           dict(nv8, out_bit_depth=0), dict(nv8, out_bit_depth=10), dict(nv8, out_bit_depth=9),         # NV12 U8 at another depth than 8
           dict(nv16, out_bit_depth=8),                                                                 # NV12 U16 at depth 8
           dict(nv16, out_bit_depth=17), dict(p16, out_bit_depth=17), dict(p16, out_bit_depth=7), dict(p16, out_bit_depth=-1)]
    bad += [dict(base, dtype=dt) for base in (nv16, p16) for dt in (abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32)]      # float dtypes
    bad += [dict(base, bgr=1) for base in (nv8, nv16, p16, y444, dict(y444, layout=abi.OUT_YUV444_INTERLEAVED))]
    bad += [dict(nv8, row_pitch=63), dict(nv16, row_pitch=126), dict(nv16, row_pitch=129), dict(p16, row_pitch=131), dict(p16, row_pitch=64),
            dict(y444, row_pitch=126), dict(y444, row_pitch=131), dict(y444, layout=abi.OUT_YUV444_INTERLEAVED, row_pitch=3 * 128 - 2),
            dict(y444, dtype=abi.OUT_F32, row_pitch=258)]                                                 # shorter than a row / not a multiple of the element
    bad += [dict(base, crop=c) for base in (nv8, p16, y444) for c in ((1, 0, 0, 0), (0, 0, 3, 0), (-2, 0, 0, 0), (0, 0, 0, -4), (32, 32, 0, 0), (0, 0, 24, 24))]
    bad += [dict(layout=7, dtype=abi.OUT_U8), dict(layout=7, dtype=abi.OUT_U16), dict(layout=-1, dtype=abi.OUT_U8)]
    bad += [dict(y444, out_bit_depth=d) for d in (8, 9, 12, 16)]                                          # YUV444 U16: 0 or the coding depth
    bad += [dict(y444, dtype=5), dict(y444, chroma_loc=6), dict(y444, upsample=2)]
    for b in bad:
        assert size(10, **b) == 0, b
    assert size(8, **nv16) == 0                      # out_bit_depth 0 = the coding depth, which must be above 8 for NV12 U16
    assert size(8, **dict(nv16, out_bit_depth=10)) > 0 and size(8, **p16) > 0
    assert abi.load().xgpu_output_format_size(None, 64, 48, 10) == 0
    for wd, ht, bd in ((0, 48, 10), (64, -8, 10), (64, 48, 7), (64, 48, 13)):
        assert size(bd, wd, ht, **nv8) == 0, (wd, ht, bd)


def test_coeffs_stay_an_rgb_function():
    coef, shift, fcoef = (C.c_int32 * 5)(), C.c_int(), (C.c_float * 5)()
    valid = [dict(layout=abi.OUT_NV12, dtype=abi.OUT_U8, out_bit_depth=8), dict(layout=abi.OUT_NV12, dtype=abi.OUT_U16),
             dict(layout=abi.OUT_P016, dtype=abi.OUT_U16, out_bit_depth=10)]
    valid += [dict(layout=l, dtype=dt) for l in YUV444 for dt in DTYPES]
    for kw in valid:
        assert size(10, **kw) > 0
        rc = abi.load().xgpu_output_coeffs(C.byref(abi.make_output_format(**kw)), 10, coef, C.byref(shift), fcoef)
        assert rc == -101, kw      # XGPU_ERR_INVALID_ARGUMENT
    assert abi.load().xgpu_output_coeffs(C.byref(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8)), 10, coef, C.byref(shift), fcoef) == 0


# ------------------------------------------------------------------------------------------------ the restatement's own checks
def _picture(bd, w=48, h=32, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, (h, w)).astype(np.int16), rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(np.int16),
            rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(np.int16)]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_nv12_is_yuv420p_in_another_place(bd):
    planes = _picture(bd)
    for crop, d in itertools.product(((0, 0, 0, 0), (2, 4, 2, 6)), (8, 9, 10, 12, 16)):
        w, h = 48 - crop[0] - crop[1], 32 - crop[2] - crop[3]
        got = yr.nv12(planes, bd, d, crop)
        assert got.shape == (h * 3 // 2, w) and got.dtype == (np.uint8 if d == 8 else np.uint16)
        assert np.array_equal(got, yr.interleave_420p(yr.yuv420p(planes, bd, d, crop), w, h)), (crop, d)
        p = yr.p016(planes, bd, d, crop)
        assert np.array_equal(p >> (16 - d), got) and not (p & ((1 << (16 - d)) - 1)).any(), (crop, d)
    assert np.array_equal(yr.nv12(planes, bd, bd if bd > 8 else 8)[:32], planes[0])      # the coding depth: a copy


def test_depth_conversion_rules():
    v = np.array([0, 1, 2, 3, 510, 511, 1020, 1021, 1022, 1023])
    assert list(yr.depth_convert(v, 10, 8)) == [0, 0, 1, 1, 128, 128, 255, 255, 255, 255]      # (v + 2) >> 2 clipped to 255
    assert list(yr.depth_convert(v, 10, 9)) == [0, 1, 1, 2, 255, 256, 510, 511, 511, 511]      # (v + 1) >> 1 clipped to 511
    assert list(yr.depth_convert(v, 10, 12)) == list(v << 2) and list(yr.depth_convert(v, 10, 10)) == list(v)
    assert list(yr.depth_convert(np.array([-3, 300]), 8, 8)) == [0, 255]                       # the 8-bit rule clips (DRA can leave the range)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_yuv444_nearest_subsampled_gives_the_chroma_planes_back(bd):
    planes = _picture(bd)
    for crop in ((0, 0, 0, 0), (2, 4, 2, 6), (0, 2, 4, 0)):
        y, u, v = cr.crop_planes(planes, crop)
        got = yr.yuv444(planes, bd, mode="nearest", dtype=yr.U16, crop=crop)
        assert got.dtype == np.uint16 and got.shape == (3,) + y.shape
        assert np.array_equal(got[0], y) and np.array_equal(got[1][0::2, 0::2], u) and np.array_equal(got[2][0::2, 0::2], v)
        assert np.array_equal(got[1][1::2, 1::2], u)
        # co-sited linear keeps the chroma samples at their own positions (type 2: co-sited both ways)
        lin = yr.yuv444(planes, bd, chroma_loc=2, mode="linear", dtype=yr.U16, crop=crop)
        assert np.array_equal(lin[1][0::2, 0::2], u) and np.array_equal(lin[2][0::2, 0::2], v)
        u8 = yr.yuv444(planes, bd, mode="nearest", dtype=yr.U8, crop=crop)
        assert np.array_equal(u8[0], yr.depth_convert(y, bd, 8)) and np.array_equal(u8[2][0::2, 0::2], yr.depth_convert(v, bd, 8))


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_normalised_floats_at_the_ends_of_the_range(bd):
    co = 1 << (bd - 1)
    for full in (False, True):
        yo, yrng, crng = cr.ranges(bd, full)
        yrng, crng = int(yrng), int(crng)
        fy = np.float32(1.0 / yrng)
        e = yr.normalised(np.array([yo, yo + yrng, yo - 5, yo + yrng + 9, 0, (1 << bd) - 1]), np.full(6, co), np.full(6, co), bd, full)
        assert e.dtype == np.float32
        assert e[0][0] == 0 and not np.signbit(e[0][0])
        top = np.float32(yrng) * fy
        assert e[0][1] == top
        # the product of the excursion and its rounded reciprocal: exactly 1 in full range, one ulp below in limited range - kept, not rounded up
        assert float(top) == (1.0 if full else 1.0 - 2.0 ** -24), (bd, full, float(top))
        assert e[0][2] == 0 and e[0][3] == 1 and e[0][4] == 0 and e[0][5] == (1 if not full else top)
        assert (e[1] == 0).all() and (e[2] == 0).all()
        lo, hi = co - crng // 2 - 40, co + crng // 2 + 40      # beyond the nominal chroma range (limited range leaves room for it)
        c = yr.normalised(np.full(4, yo), np.array([lo, hi, 0, (1 << bd) - 1]), np.array([hi, lo, (1 << bd) - 1, 0]), bd, full)
        if not full:
            assert list(c[1][:2]) == [-0.5, 0.5] and list(c[2][:2]) == [0.5, -0.5]
        assert (np.abs(c[1:]) <= 0.5).all()
        one = yr.normalised(np.array([yo]), np.array([co + 1]), np.array([co - 1]), bd, full)
        assert one[1][0] == np.float32(1.0 / crng) and one[2][0] == -np.float32(1.0 / crng)


def test_yuv444_floats_follow_the_range_and_dra():
    planes = _picture(10)
    luts = [np.arange(1024, dtype=np.int32)[::-1].copy(), np.full(1024, 400, np.int32), np.full(1024, 600, np.int32)]
    a = yr.yuv444(planes, 10, False, 1, "linear", yr.F32, (2, 0, 0, 2))
    b = yr.yuv444(planes, 10, True, 1, "linear", yr.F32, (2, 0, 0, 2))
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (3, 30, 46) and not np.array_equal(a, b)
    assert a[0].min() >= 0 and a[0].max() <= 1 and a[1:].min() >= -0.5 and a[1:].max() <= 0.5
    d = yr.yuv444(planes, 10, dtype=yr.U16, dra=luts)
    assert np.array_equal(d[0], 1023 - planes[0].astype(np.int64))      # luma through its table
    dn = yr.nv12(planes, 10, 10, dra=luts)
    assert np.array_equal(dn[:32], d[0]) and np.array_equal(dn[32:, 0::2], cr.dra_apply(planes, luts)[1])
