"""CPU suite for the packed display surfaces (xgpu_packed_format: RGBA, 10:10:10:2, YUYV / UYVY): xgpu_output_packed_size
against closed forms, every refusal of the contract with its code, xgpu_output_packed_coeffs and the alpha codes against the numpy restatement
tests/packed_ref.py, that restatement's own checks, and xgpu_output_format keeping its seven layouts.  Nothing here needs a GPU."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import colour_ref as cr
import packed_ref as pr
import yuv_ref as yr
from xevd_amd import abi

INVALID, UNSUPPORTED = -101, -104
DTYPES = (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32)
ES = {abi.OUT_U8: 1, abi.OUT_U16: 2, abi.OUT_F16: 2, abi.OUT_BF16: 2, abi.OUT_F32: 4}
YUV = (abi.PACKED_YUYV, abi.PACKED_UYVY)
SIZES = ((64, 48, (0, 0, 0, 0)), (64, 48, (2, 4, 2, 6)), (72, 40, (4, 2, 2, 0)), (8, 8, (2, 4, 4, 2)), (7680, 4320, (0, 0, 0, 0)))
PQ_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)


def size(bd=10, width=64, height=48, **kw):
    return abi.load().xgpu_output_packed_size(C.byref(abi.make_packed_format(**kw)), width, height, bd)


def check(bd=10, width=64, height=48, cm=None, **kw):
    cmv = None if cm is None else C.byref(abi.make_colour_transform(**cm))
    return abi.load().xgpu_output_packed_check(C.byref(abi.make_packed_format(**kw)), cmv, width, height, bd)


def forms(bd):
    """(layout, dtype, out_bit_depth, element size, elements per pixel) of every valid form at coding depth bd"""
    out = [(abi.PACKED_RGBA, dt, obd, ES[dt], 4) for dt in DTYPES for obd in (0, bd)]
    out += [(abi.PACKED_RGB10A2, 0, 0, 4, 1)]
    for lay in YUV:
        out += [(lay, abi.OUT_U8, 8, 1, 2)] + [(lay, abi.OUT_U16, d, 2, 2) for d in (0,) + tuple(range(8, 17))]
    return out


def test_constants_and_struct():
    assert (abi.PACKED_RGBA, abi.PACKED_RGB10A2, abi.PACKED_YUYV, abi.PACKED_UYVY) == (0, 1, 2, 3)
    assert C.sizeof(abi.PackedFormat) == 12 * 4 + C.sizeof(C.c_size_t) + 8      # the float and its tail padding (LP64)
    assert abi.PackedFormat.row_pitch.offset == 48 and abi.PackedFormat.alpha.offset == 56
    for name in ("xgpu_output_packed_size", "xgpu_output_packed_check", "xgpu_output_packed_coeffs", "xgpu_pic_output_device_packed"):
        assert name in abi.exported_names(), name


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_size_of_every_layout_dtype_and_pitch(bd):
    for (wd, ht, crop), (lay, dt, obd, es, per) in itertools.product(SIZES, forms(bd)):
        w, h = wd - crop[0] - crop[1], ht - crop[2] - crop[3]
        row = per * w * es
        for pitch in (0, row, row + es, row + 16, row + 64 + es):
            kw = dict(layout=lay, dtype=dt, out_bit_depth=obd, crop=crop, row_pitch=pitch)
            assert size(bd, wd, ht, **kw) == (h - 1) * (pitch or row) + row, (wd, ht, crop, lay, dt, obd, pitch)
            assert check(bd, wd, ht, **kw) == 0
        assert size(bd, wd, ht, layout=lay, dtype=dt, out_bit_depth=obd, crop=crop, row_pitch=row - es) == 0      # shorter than a row


def test_fields_a_layout_does_not_read_are_not_validated():
    for lay in YUV:
        kw = dict(layout=lay, dtype=abi.OUT_U8, out_bit_depth=8, matrix=2, alpha=7.0)
        assert size(10, **kw) == 48 * 64 * 2 and check(10, **kw) == 0
        f = abi.make_packed_format(**kw)
        f.full_range = 5
        f.alpha = float("nan")
        assert abi.load().xgpu_output_packed_size(C.byref(f), 64, 48, 10) == 48 * 64 * 2
        for loc in range(6):      # (the horizontal bit is not read, the value is still a ChromaSampleLocType)
            assert check(10, **dict(kw, chroma_loc=loc)) == 0


def test_refusals_one_per_rule():
    rgba = dict(layout=abi.PACKED_RGBA, dtype=abi.OUT_U8)
    r10 = dict(layout=abi.PACKED_RGB10A2)
    y8 = dict(layout=abi.PACKED_YUYV, dtype=abi.OUT_U8, out_bit_depth=8)
    y16 = dict(layout=abi.PACKED_UYVY, dtype=abi.OUT_U16)
    for ok in (rgba, r10, y8, y16):
        assert size(10, **ok) > 0 and check(10, **ok) == 0, ok
    bad = [dict(rgba, layout=4), dict(rgba, layout=-1), dict(rgba, layout=7)]                                              # layout
    bad += [dict(rgba, dtype=5), dict(rgba, dtype=-1)]                                                                     # RGBA: dtype
    bad += [dict(rgba, out_bit_depth=d) for d in (8, 12, 16)] + [dict(rgba, dtype=abi.OUT_U16, out_bit_depth=8)]           # RGBA: 0 or the coding depth
    bad += [dict(r10, dtype=dt) for dt in DTYPES[1:]] + [dict(r10, out_bit_depth=10)]                                      # RGB10A2: dtype and out_bit_depth 0
    bad += [dict(y8, out_bit_depth=0), dict(y8, out_bit_depth=10)]                                                         # 4:2:2 U8: depth 8 only
    bad += [dict(y16, out_bit_depth=7), dict(y16, out_bit_depth=17), dict(y16, out_bit_depth=-1)]                          # 4:2:2 U16: 0 or 8..16
    bad += [dict(y16, dtype=dt) for dt in (abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32)]                                         # 4:2:2: integers only
    bad += [dict(y8, bgr=1), dict(y16, bgr=1)]                                                                             # 4:2:2: bgr must be 0
    bad += [dict(base, chroma_loc=c) for base in (rgba, r10, y8) for c in (-1, 6)]
    bad += [dict(base, upsample=u) for base in (rgba, r10, y16) for u in (-1, 2)]
    bad += [dict(rgba, row_pitch=4 * 64 - 1), dict(rgba, dtype=abi.OUT_U16, row_pitch=8 * 64 + 1), dict(rgba, dtype=abi.OUT_F32, row_pitch=16 * 64 + 2),
            dict(r10, row_pitch=4 * 64 + 2), dict(r10, row_pitch=4 * 64 - 4), dict(y8, row_pitch=127), dict(y16, row_pitch=4 * 64 + 1),
            dict(y16, row_pitch=4 * 64 - 2)]                                                                               # pitch: element multiple, >= a row
    bad += [dict(base, crop=c) for base in (rgba, r10, y8) for c in ((1, 0, 0, 0), (0, 0, 3, 0), (-2, 0, 0, 0), (0, 0, 0, -4), (32, 32, 0, 0), (0, 0, 24, 24))]
    bad += [dict(base, alpha=a) for base in (rgba, r10) for a in (-0.01, 1.01, float("nan"), float("inf"), -float("inf"))]  # alpha: where it is read
    for b in bad:
        assert size(10, **b) == 0 and check(10, **b) == INVALID, b
    for base in (rgba, r10):                                                                                               # bgr / full_range: 0 | 1
        for field in ("bgr", "full_range"):
            f = abi.make_packed_format(**base)
            setattr(f, field, 2)
            assert abi.load().xgpu_output_packed_size(C.byref(f), 64, 48, 10) == 0
            assert abi.load().xgpu_output_packed_check(C.byref(f), None, 64, 48, 10) == INVALID
    assert size(8, **dict(rgba, out_bit_depth=8)) > 0 and size(8, **y16) > 0
    assert abi.load().xgpu_output_packed_size(None, 64, 48, 10) == 0 and abi.load().xgpu_output_packed_check(None, None, 64, 48, 10) == INVALID
    for wd, ht, bd in ((0, 48, 10), (64, -8, 10), (63, 48, 10), (64, 47, 10), (64, 48, 7), (64, 48, 13)):                   # xgpu_output_format_size's limits
        for base in (rgba, r10, y8):
            assert size(bd, wd, ht, **base) == 0 and check(bd, wd, ht, **base) == INVALID, (wd, ht, bd)


def test_unsupported_matrix_and_transform():
    for base in (dict(layout=abi.PACKED_RGBA, dtype=abi.OUT_F16), dict(layout=abi.PACKED_RGB10A2)):
        for m in (0, 2, 3, 8, 10, 14):
            assert size(10, **dict(base, matrix=m)) == 0 and check(10, **dict(base, matrix=m)) == UNSUPPORTED, m
        for m in (1, 4, 5, 6, 7, 9):
            assert check(10, **dict(base, matrix=m)) == 0, m
        assert check(10, cm=PQ_SRGB, **base) == 0
        assert check(10, cm=dict(PQ_SRGB, src_transfer=17), **base) == UNSUPPORTED
        assert check(10, cm=dict(PQ_SRGB, dst_primaries=22), **base) == UNSUPPORTED
        assert check(10, cm=dict(PQ_SRGB, src_peak=-1.0), **base) == INVALID
        assert check(10, cm=PQ_SRGB, **dict(base, alpha=2.0)) == INVALID      # the format's own refusal comes first
    for lay in YUV:      # 4:2:2 takes no transform
        assert check(10, cm=PQ_SRGB, layout=lay, dtype=abi.OUT_U8, out_bit_depth=8) == INVALID
        assert check(10, layout=lay, dtype=abi.OUT_U8, out_bit_depth=8) == 0


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_coeffs_against_the_restatement(bd):
    lib = abi.load()
    for matrix, full in itertools.product((1, 4, 5, 6, 7, 9), (False, True)):
        coef, shift, fcoef, _ = abi.packed_coeffs(lib, abi.make_packed_format(abi.PACKED_RGB10A2, matrix=matrix, full_range=full), bd)
        want, s = pr.coeffs10(matrix, full, bd)
        assert (coef, shift) == (want, s) and s == 17, (matrix, full, coef, want)
        fwant = cr.coeffs(matrix, full, bd, cr.F32)[2]
        assert [np.float32(v) for v in fcoef] == fwant
        if bd == 10:      # on a 10-bit stream the fields are the U16 output's values: the same coefficients
            assert (coef, shift) == cr.coeffs(matrix, full, 10, cr.U16)[:2]
        # the bound stated next to the code: every sum of the rule stays below 2^31 for samples in 0 .. 2^B - 1
        yo, co, top = cr.ranges(bd, full)[0], 1 << (bd - 1), (1 << bd) - 1
        worst = max(abs(coef[0] * (y - yo)) for y in (0, top)) + (abs(coef[2]) + abs(coef[3])) * max(co, top - co) + (1 << 16)
        worst = max(worst, max(abs(coef[0] * (y - yo)) for y in (0, top)) + max(abs(coef[1]), abs(coef[4])) * max(co, top - co) + (1 << 16))
        assert worst < (1 << 30), (matrix, full, worst)
        for dt, rdt in zip(DTYPES, (cr.U8, cr.U16, cr.F16, cr.BF16, cr.F32)):      # RGBA: xgpu_output_coeffs' of the dtype
            got = abi.packed_coeffs(lib, abi.make_packed_format(abi.PACKED_RGBA, dt, matrix=matrix, full_range=full), bd)
            k, s, f = cr.coeffs(matrix, full, bd, rdt)
            assert (got[0], got[1]) == (k, s) and [np.float32(v) for v in got[2]] == f, (matrix, full, dt)
    for lay in YUV:      # no matrix
        assert abi.packed_coeffs(lib, abi.make_packed_format(lay, abi.OUT_U8, out_bit_depth=8), bd) == INVALID
    assert abi.packed_coeffs(lib, abi.make_packed_format(abi.PACKED_RGBA, matrix=2), bd) == UNSUPPORTED
    assert abi.packed_coeffs(lib, abi.make_packed_format(abi.PACKED_RGBA), 13) == INVALID


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_alpha_codes(bd):
    lib = abi.load()
    third = float(np.float32(1 / 3))
    for alpha, c2, c8 in ((0.0, 0, 0), (1.0, 3, 255), (0.5, 2, 128), (1 / 3, 1, 85)):
        code = lambda **kw: abi.packed_coeffs(lib, abi.make_packed_format(alpha=alpha, **kw), bd)[3]      # noqa: E731
        assert code(layout=abi.PACKED_RGB10A2) == c2 == pr.alpha_code(alpha, 2)
        assert code(layout=abi.PACKED_RGBA, dtype=abi.OUT_U8) == c8 == pr.alpha_code(alpha, 8) == pr.alpha_element(alpha, pr.U8, bd)
        top = (1 << bd) - 1
        a32 = float(np.float32(alpha))
        assert code(layout=abi.PACKED_RGBA, dtype=abi.OUT_U16) == math.floor(a32 * top + 0.5) == pr.alpha_element(alpha, pr.U16, bd)
        for dt in (abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32):      # the float32 bits of alpha; the dtype's rounding is the kernel's
            assert code(layout=abi.PACKED_RGBA, dtype=dt) == int(np.float32(alpha).view(np.uint32))
    assert pr.alpha_element(1.0, pr.F16, bd) == 0x3C00 and pr.alpha_element(1.0, pr.BF16, bd) == 0x3F80 and pr.alpha_element(0.5, pr.F32, bd) == 0x3F000000
    assert pr.alpha_element(1 / 3, pr.F16, bd) == 0x3555 and pr.alpha_element(1 / 3, pr.BF16, bd) == 0x3EAB and third != 1 / 3


def test_output_format_keeps_its_seven_layouts():
    lib = abi.load()
    for layout, dt, obd in itertools.product((7, 8, 9, 10), (abi.OUT_U8, abi.OUT_U16, abi.OUT_F32), (0, 8, 10)):
        f = abi.make_output_format(layout=layout, dtype=dt, out_bit_depth=obd)
        assert lib.xgpu_output_format_size(C.byref(f), 64, 48, 10) == 0, (layout, dt, obd)
    assert C.sizeof(abi.OutputFormat) == 12 * 4 + C.sizeof(C.c_size_t)


# ------------------------------------------------------------------------------------------------ the restatement's own checks
def _picture(bd, w=24, h=16, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, (h, w)).astype(np.int16), rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(np.int16),
            rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(np.int16)]


def test_rgb10a2_on_a_10_bit_picture_is_the_u16_output():
    planes = _picture(10)
    for crop, bgr, mode, full in itertools.product(((0, 0, 0, 0), (2, 4, 2, 4)), (False, True), ("linear", "nearest"), (False, True)):
        w = pr.rgb10a2(planes, 10, matrix=9, full_range=full, chroma_loc=1, mode=mode, crop=crop, bgr=bgr, alpha=1 / 3).astype(np.int64)
        rgb = cr.convert(planes, 10, matrix=9, full_range=full, chroma_loc=1, mode=mode, dtype=cr.U16, crop=crop).astype(np.int64)
        lo, hi = (2, 0) if bgr else (0, 2)
        assert np.array_equal(w & 1023, rgb[lo]) and np.array_equal((w >> 10) & 1023, rgb[1]) and np.array_equal((w >> 20) & 1023, rgb[hi])
        assert ((w >> 30) == 1).all()


@pytest.mark.parametrize("bd", [8, 12])
def test_rgb10a2_at_other_depths_is_within_one_code_of_float64(bd):
    planes = _picture(bd)
    y, u, v = planes
    w = pr.rgb10a2(planes, bd, matrix=1, mode="nearest").astype(np.int64)
    up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)      # noqa: E731
    want = cr.h273_float64(y, up(u), up(v), bd, 1, False, 10)
    for k in range(3):
        assert np.abs(((w >> (10 * k)) & 1023) - want[k]).max() <= 1


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_yuv422_is_nv12_in_another_place(bd):
    planes = _picture(bd)
    for crop, d, uyvy in itertools.product(((0, 0, 0, 0), (2, 4, 2, 4)), (8, 10, 12, 16), (False, True)):
        got = pr.yuv422(planes, bd, d, pr.U8 if d == 8 else pr.U16, uyvy=uyvy, mode="nearest", crop=crop)
        h, w = got.shape[:2]
        nv = (yr.p016(planes, bd, d, crop) if d > 8 else yr.nv12(planes, bd, 8, crop)).astype(np.int64)
        yi, ci = (1, 0) if uyvy else (0, 1)
        assert np.array_equal(got[:, :, yi], nv[:h])
        for r in range(h):
            assert np.array_equal(got[r, :, ci], nv[h + (r >> 1)]), (crop, d, uyvy, r)
    # LINEAR: co-sited top keeps the even rows, the odd rows are the rounded mean; centred weights meet the clamp at both edges
    u = np.array([[100, 200], [300, 400], [500, 700]])
    top = pr.chroma_full_height(u, "linear", 2)
    assert np.array_equal(top[0::2], u) and np.array_equal(top[1], (u[0] + u[1] + 1) >> 1) and np.array_equal(top[5], u[2])
    cen = pr.chroma_full_height(u, "linear", 0)
    assert np.array_equal(cen[0], u[0]) and np.array_equal(cen[5], u[2]) and np.array_equal(cen[1], (3 * u[0] + u[1] + 2) >> 2)
    assert np.array_equal(cen[2], (u[0] + 3 * u[1] + 2) >> 2)
    bot = pr.chroma_full_height(u, "linear", 4)
    assert np.array_equal(bot[1::2], u) and np.array_equal(bot[0], u[0]) and np.array_equal(bot[2], (u[0] + u[1] + 1) >> 1)
    assert np.array_equal(pr.chroma_full_height(u, "linear", 5), bot)      # the horizontal bit is not read
