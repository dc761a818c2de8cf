"""CPU suite of the picture comparison (xgpu_pic_compare): the host-only argument checks and size functions against a Python restatement of their rules, the
layout of xgpu_compare_result, and the numpy restatement of the contract (tests/metrics_ref.py) against itself - hand-computed windows, the constants, the
textbook formula in floats."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import metrics_ref as mr
from xevd_amd import abi

INVALID = -101
ADDR = 0x10000      # d_yuv is not read by the host-only functions: any non-NULL address


# ------------------------------------------------------------------------------------------------ the rules, restated
def rule_ref_size(kind, dtype, pitch, w, h):
    if w <= 0 or h <= 0 or (w | h) & 1 or kind != abi.CMP_REF_YUV420 or dtype not in (abi.OUT_U8, abi.OUT_U16):
        return 0
    es = 1 if dtype == abi.OUT_U8 else 2
    if pitch % (2 * es) or (pitch and pitch < w * es):
        return 0
    pitch = pitch or w * es
    return h * pitch + (h - 1) * (pitch // 2) + (w // 2) * es


def rule_params_ok(crop, ssim, block_map, w, h):
    if w <= 0 or h <= 0 or (w | h) & 1 or any(v < 0 or v & 1 for v in crop):
        return False
    return crop[0] + crop[1] < w and crop[2] + crop[3] < h and ssim in (0, 1) and block_map in (0, 1)


def rule_map_size(crop, ssim, block_map, w, h):
    if not rule_params_ok(crop, ssim, block_map, w, h) or not block_map:
        return 0
    cw, ch = w - crop[0] - crop[1], h - crop[2] - crop[3]
    return 3 * -(-ch // 16) * -(-cw // 16) * 8


def rule_check(ref, par, w, h, bd):
    kind, pic, d_yuv, size, dtype, pitch = ref
    if not rule_params_ok(*par, w, h) or not 8 <= bd <= 12:
        return INVALID
    if kind == abi.CMP_REF_PIC:
        return INVALID if pic < 0 else 0
    need = rule_ref_size(kind, dtype, pitch, w, h)
    if need == 0 or (dtype == abi.OUT_U8 and bd != 8) or not d_yuv or size < need:
        return INVALID
    return 0


def c_ref(kind, pic, d_yuv, size, dtype, pitch):
    r = abi.CompareRef()
    r.kind, r.pic, r.d_yuv, r.size, r.dtype, r.row_pitch = kind, pic, d_yuv, size, dtype, pitch
    return r


def c_par(crop, ssim, block_map):
    p = abi.CompareParams()
    for i in range(4):
        p.crop[i] = crop[i]
    p.ssim, p.block_map = ssim, block_map
    return p


SIZES = [(8, 8), (72, 40), (136, 72), (200, 136), (7680, 4320), (0, 8), (8, -2), (9, 8), (8, 10)]
CROPS = [(0, 0, 0, 0), (2, 6, 4, 2), (1, 0, 0, 0), (0, 0, 0, 3), (-2, 0, 0, 0), (4, 4, 0, 0), (0, 0, 6, 2), (100, 100, 0, 0), (0, 0, 60, 76)]


# ------------------------------------------------------------------------------------------------ the size functions and the check
def test_ref_size_sweep():
    lib = abi.load()
    assert lib.xgpu_compare_ref_size(None, 72, 40) == 0
    seen = set()
    for (w, h), kind, dtype in itertools.product(SIZES, (abi.CMP_REF_PIC, abi.CMP_REF_YUV420, 2, -1), (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16, abi.OUT_F32, -1)):
        for pitch in (0, w, w + 1, 2 * w, 2 * w - 2, 2 * w + 2, 2 * w + 4, 2 * w + 3, 512, 16384):
            if pitch < 0:
                continue
            got = lib.xgpu_compare_ref_size(C.byref(c_ref(kind, 0, ADDR, 0, dtype, pitch)), w, h)
            assert got == rule_ref_size(kind, dtype, pitch, w, h), (w, h, kind, dtype, pitch)
            seen.add(got > 0)
    assert seen == {False, True}
    # spelled out once: tight 8 and 16 bit, a pitch, the 8K picture
    assert lib.xgpu_compare_ref_size(C.byref(abi.make_compare_ref(d_yuv=ADDR, dtype=abi.OUT_U8)), 200, 136) == 200 * 136 * 3 // 2
    assert lib.xgpu_compare_ref_size(C.byref(abi.make_compare_ref(d_yuv=ADDR)), 200, 136) == 200 * 136 * 3
    assert lib.xgpu_compare_ref_size(C.byref(abi.make_compare_ref(d_yuv=ADDR, row_pitch=512)), 200, 136) == 136 * 512 + 135 * 256 + 200
    assert lib.xgpu_compare_ref_size(C.byref(abi.make_compare_ref(d_yuv=ADDR)), 7680, 4320) == 7680 * 4320 * 3


def test_map_size_sweep():
    lib = abi.load()
    assert lib.xgpu_compare_map_size(None, 72, 40) == 0
    seen = set()
    for (w, h), crop, ssim, bm in itertools.product(SIZES, CROPS, (0, 1, 2, -1), (0, 1, 2, -1)):
        got = lib.xgpu_compare_map_size(C.byref(c_par(crop, ssim, bm)), w, h)
        assert got == rule_map_size(crop, ssim, bm, w, h), (w, h, crop, ssim, bm)
        seen.add(got > 0)
    assert seen == {False, True}
    assert lib.xgpu_compare_map_size(C.byref(abi.make_compare_params((2, 6, 4, 2), block_map=True)), 200, 136) == 3 * 9 * 12 * 8      # 192 x 130
    assert lib.xgpu_compare_map_size(C.byref(abi.make_compare_params(block_map=True)), 8, 8) == 24


def test_check_sweep():
    lib = abi.load()
    good_r, good_p = abi.make_compare_ref(pic=0), abi.make_compare_params()
    assert lib.xgpu_compare_check(None, C.byref(good_p), 72, 40, 8) == INVALID
    assert lib.xgpu_compare_check(C.byref(good_r), None, 72, 40, 8) == INVALID
    assert lib.xgpu_compare_check(C.byref(good_r), C.byref(good_p), 72, 40, 8) == 0
    refs = [(abi.CMP_REF_PIC, 0, 0, 0, 0, 0), (abi.CMP_REF_PIC, 3, 0, 0, 7, 5), (abi.CMP_REF_PIC, -1, 0, 0, 0, 0), (2, 0, ADDR, 1 << 40, abi.OUT_U16, 0),
            (-1, 0, ADDR, 1 << 40, abi.OUT_U16, 0)]
    for dtype, pitch, d_yuv in itertools.product((abi.OUT_U8, abi.OUT_U16, abi.OUT_F16), (0, 200, 202, 400, 402, 404, 512, 1024), (ADDR, 0)):
        for size in (0, 200 * 136 * 3 // 2 - 1, 200 * 136 * 3 // 2, 200 * 136 * 3 - 1, 200 * 136 * 3, 1 << 40):
            refs.append((abi.CMP_REF_YUV420, 0, d_yuv, size, dtype, pitch))
    pars = [(crop, 1, 0) for crop in CROPS] + [((0, 0, 0, 0), s, b) for s, b in ((0, 0), (0, 1), (1, 1), (2, 0), (0, 2), (-1, 0))]
    seen = set()
    for ref, par, (w, h), bd in itertools.product(refs, pars, [(200, 136), (72, 40), (0, 8), (9, 8)], (7, 8, 10, 12, 13)):
        got = lib.xgpu_compare_check(C.byref(c_ref(*ref)), C.byref(c_par(*par)), w, h, bd)
        assert got == rule_check(ref, par, w, h, bd), (ref, par, w, h, bd)
        seen.add(got)
    assert seen == {0, INVALID}
    # each refusal of the contract, spelled out once against a call that passes
    ok = dict(d_yuv=ADDR, size=200 * 136 * 3, dtype=abi.OUT_U16)

    def chk(ref_kw, par_kw=None, bd=10, w=200, h=136):
        return lib.xgpu_compare_check(C.byref(abi.make_compare_ref(**ref_kw)), C.byref(abi.make_compare_params(**(par_kw or {}))), w, h, bd)

    assert chk(ok) == 0
    assert chk(dict(pic=-1)) == INVALID                                               # a bad slot
    assert chk(ok, dict(crop=(1, 1, 0, 0))) == INVALID                                # an odd crop
    assert chk(ok, dict(crop=(0, -2, 0, 0))) == INVALID                               # a negative crop
    assert chk(ok, dict(crop=(100, 100, 0, 0))) == INVALID                            # a crop that leaves nothing
    assert chk(dict(ok, dtype=abi.OUT_U8)) == INVALID and chk(dict(ok, dtype=abi.OUT_U8), bd=8) == 0      # U8 at another depth
    assert chk(dict(ok, row_pitch=398)) == INVALID                                    # a pitch shorter than a row
    assert chk(dict(ok, row_pitch=402, size=1 << 30)) == INVALID and chk(dict(ok, row_pitch=404, size=1 << 30)) == 0      # not a multiple of 2 elements
    assert chk(dict(ok, size=200 * 136 * 3 - 1)) == INVALID                           # too small
    assert chk(dict(ok, d_yuv=None)) == INVALID


# ------------------------------------------------------------------------------------------------ the result's layout
def test_result_layout():
    r = abi.CompareResult
    assert C.sizeof(r) == 3 * 8 * 4 + 16 + 3 * 8 * 2 == 160
    assert C.alignment(r) == 8
    offs = {"n": 0, "sse": 24, "n_diff": 48, "first_diff": 72, "max_abs": 96, "reserved": 108, "ssim_windows": 112, "ssim_q30": 136}
    for name, off in offs.items():
        assert getattr(r, name).offset == off, name
    assert r.max_abs.size == 12 and r.reserved.size == 4 and r.ssim_q30.size == 24
    assert C.sizeof(abi.CompareRef) == 40 and abi.CompareRef.d_yuv.offset == 8 and abi.CompareRef.size.offset == 16 and abi.CompareRef.dtype.offset == 24
    assert abi.CompareRef.row_pitch.offset == 32
    assert C.sizeof(abi.CompareParams) == 24 and abi.CompareParams.ssim.offset == 16 and abi.CompareParams.block_map.offset == 20
    # the words of a result as the device writes them -> the dict
    words = np.arange(20, dtype=np.uint64)
    words[17] = np.uint64((1 << 64) - 5)
    d = abi.compare_result_dict(words.view(np.int64))
    assert d["n"] == [0, 1, 2] and d["first_diff"] == [9, 10, 11] and d["max_abs"] == [12, 0, 13] and d["ssim_windows"] == [14, 15, 16] and d["ssim_q30"] == [-5, 18, 19]


def test_psnr_and_ssim_helpers():
    d = {"n": [100, 25, 25], "sse": [0, 25, 25 * 255 * 255], "ssim_windows": [4, 0, 2], "ssim_q30": [4 << 30, 0, 1 << 30]}
    p = abi.psnr(d, 8)
    assert p[0] == math.inf and p[1] == pytest.approx(10 * math.log10(255 * 255)) and p[2] == 0.0
    assert abi.psnr({"n": [4] * 3, "sse": [4] * 3}, 10)[0] == pytest.approx(20 * math.log10(1023))
    s = abi.ssim(d)
    assert s[0] == 1.0 and math.isnan(s[1]) and s[2] == 0.5


# ------------------------------------------------------------------------------------------------ metrics_ref against itself
def test_ssim_constants():
    assert mr.ssim_constants(8) == (416, 235963)
    assert mr.ssim_constants(10) == (6698, 3797644)
    assert mr.ssim_constants(12) == (107322, 60851438)


def rand_planes(seed, w, h, bd):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << bd, (h, w)).astype(np.uint16), rng.integers(0, 1 << bd, (h, w)).astype(np.uint16)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_identical_planes_give_windows_shl_30(bd):
    for w, h in ((8, 8), (72, 40), (50, 22), (7, 40), (40, 7), (4, 4)):
        a, _ = rand_planes(1, w, h, bd)
        n, q = mr.ssim_q30(a, a, bd)
        assert n == max((w >> 2) - 1, 0) * max((h >> 2) - 1, 0)
        assert q == n << 30
    full = np.full((16, 16), 0xFFFF, np.uint16)      # any 16-bit pattern
    assert mr.ssim_q30(full, full, bd) == (9, 9 << 30)


def test_hand_computed_window():
    """one 8x8 window at 8 bit: a = 10 everywhere but a[0, 0] = 74; r = 10 everywhere"""
    a = np.full((8, 8), 10, np.uint16)
    r = a.copy()
    a[0, 0] = 74
    s1, s2, ss, s12 = (int(v[0, 0]) for v in mr.window_sums(a, r))
    assert (s1, s2) == (704, 640)
    assert ss == 63 * 100 + 74 * 74 + 64 * 100 == 18176
    assert s12 == 63 * 100 + 740 == 7040
    vars_, cov = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    assert (vars_, cov) == (258048, 0)
    num, den = (2 * s1 * s2 + 416) * (2 * cov + 235963), (s1 * s1 + s2 * s2 + 416) * (vars_ + 235963)
    assert (num, den) == (901536 * 235963, 905632 * 494011)
    # num and den are below 2^53: both products are exact, and q is the one rounded division, scaled and rounded
    want = math.floor(float(num) / float(den) * 2.0 ** 30 + 0.5)
    assert mr.ssim_q30(a, r, 8) == (1, want)
    assert abs(want / 2.0 ** 30 - num / den) <= 2.0 ** -31 + 1e-15
    c = mr.census(a, r)
    assert c == {"n": 64, "sse": 4096, "n_diff": 1, "max_abs": 64, "first_diff": 0}


def test_census_first_is_raster_first():
    a, _ = rand_planes(2, 40, 24, 10)
    r = a.copy()
    r[7, 3] ^= 1
    r[5, 30] ^= 2
    c = mr.census(a, r)
    assert c["first_diff"] == (5 << 32) | 30 and c["n_diff"] == 2 and c["sse"] == 5 and c["max_abs"] == 2
    assert mr.census(a, a)["first_diff"] == mr.NO_DIFF


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_ssim_agrees_with_the_float_formula(bd):
    """per window |q / 2^30 - f| <= 1e-9: the quantisation is worth at most 2^-31 = 4.7e-10, the float roundings of either side some 1e-15"""
    for seed, (w, h) in enumerate(((24, 16), (30, 22))):
        a, r = rand_planes(10 * bd + seed, w, h, bd)
        r = np.where(np.random.default_rng(seed).random((h, w)) < 0.5, a, r)      # correlated: SSIM away from 0
        q = mr.ssim_q30_windows(a, r, bd).reshape(-1) / 2.0 ** 30
        f = mr.ssim_float(a, r, bd)
        assert q.shape == f.shape and q.size == ((w >> 2) - 1) * ((h >> 2) - 1)
        assert np.abs(q - f).max() <= 1e-9
        assert f.min() < 0.9 and f.max() > 0.1


def test_map_sums_to_sse_and_compare_collects():
    rng = np.random.default_rng(5)
    w, h, bd, crop = 200, 136, 10, (2, 6, 4, 2)
    pic = [rng.integers(0, 1 << bd, (h >> s, w >> s)).astype(np.int16) for s in (0, 1, 1)]
    ref = [rng.integers(0, 1 << bd, (h >> s, w >> s)).astype(np.int16) for s in (0, 1, 1)]
    d = mr.compare(pic, ref, bd, crop=crop, block_map=True)
    assert d["map"].shape == (3, 9, 12) and d["map"].dtype == np.uint64
    assert [int(d["map"][c].sum()) for c in range(3)] == d["sse"]
    assert d["n"] == [192 * 130, 96 * 65, 96 * 65]
    assert d["ssim_windows"] == [47 * 31, 23 * 15, 23 * 15]
    # a block clipped at both edges: the last one holds 192 - 176 = 16 columns and 130 - 128 = 2 rows
    a, r = mr.crop_plane(pic[0], crop, 0).astype(np.int64), mr.crop_plane(ref[0], crop, 0).astype(np.int64)
    assert int(d["map"][0, 8, 11]) == int(((a[128:, 176:] - r[128:, 176:]) ** 2).sum())
    # 16-bit patterns in int16 planes are read as unsigned
    neg = [np.full_like(p, -1) for p in pic]
    zero = [np.zeros_like(p) for p in pic]
    assert mr.compare(neg, zero, bd)["max_abs"] == [0xFFFF] * 3
