"""CPU suite of the picture statistics (xgpu_pic_stats): the layout of xgpu_stats_result, the host-only size function and argument check against a Python
restatement of their rules, xgpu_stats_lin against xgpu_colour_tables, and the numpy restatement of the contract (tests/stats_ref.py) against itself -
hand-computed planes, the percentile rule on both sides of its threshold, the order of light_sum, max(R', G', B') against colour_ref."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import colour_ref
import stats_ref as sr
from xevd_amd import abi

INVALID, UNSUPPORTED = -101, -104
MATRICES = (1, 4, 5, 6, 7, 9)


# ------------------------------------------------------------------------------------------------ the rules, restated
def rule_params(par, bd):
    """0, INVALID or UNSUPPORTED for the parameters alone at depth bd; every INVALID before UNSUPPORTED"""
    crop, hist_bits, pctl, light, matrix, full_range, chroma_loc, upsample, transfer = par
    if not 8 <= bd <= 12 or any(v < 0 or v & 1 for v in crop):
        return INVALID
    if hist_bits != 0 and not 4 <= hist_bits <= bd:
        return INVALID
    if light not in (0, 1):
        return INVALID
    if (hist_bits or light) and any(not 0 <= p <= 10000 for p in pctl):
        return INVALID
    if light:
        if full_range not in (0, 1) or not 0 <= chroma_loc <= 5 or upsample not in (abi.UPSAMPLE_NEAREST, abi.UPSAMPLE_LINEAR):
            return INVALID
        if matrix not in MATRICES or transfer not in abi.STATS_TRANSFERS:
            return UNSUPPORTED
    return 0


def rule_hist_size(par, bd):
    if rule_params(par, bd) != 0:
        return 0
    return (3 * (1 << par[1]) * (par[1] != 0) + (1 << bd) * par[3]) * 4


def rule_check(par, w, h, bd):
    if w <= 0 or h <= 0 or (w | h) & 1 or w * h >= 1 << 31 or not 8 <= bd <= 12:
        return INVALID
    crop = par[0]
    if any(v < 0 or v & 1 for v in crop) or crop[0] + crop[1] >= w or crop[2] + crop[3] >= h:
        return INVALID
    return rule_params(par, bd)


def c_par(crop, hist_bits, pctl, light, matrix, full_range, chroma_loc, upsample, transfer):
    p = abi.StatsParams()
    for i in range(4):
        p.crop[i] = crop[i]
    p.hist_bits, p.light, p.matrix, p.full_range, p.chroma_loc, p.upsample, p.transfer = hist_bits, light, matrix, full_range, chroma_loc, upsample, transfer
    p.pctl_e4[0], p.pctl_e4[1] = pctl
    return p


SIZES = [(8, 8), (72, 40), (200, 136), (7680, 4320), (0, 8), (8, -2), (9, 8), (8, 10), (65536, 32766), (65536, 32768), (46342, 46342)]
CROPS = [(0, 0, 0, 0), (2, 6, 4, 2), (1, 0, 0, 0), (0, 0, 0, 3), (-2, 0, 0, 0), (4, 4, 0, 0), (0, 0, 6, 2), (100, 100, 0, 0), (0, 0, 60, 76)]
GOOD = ((0, 0, 0, 0), 8, (100, 9999), 0, 1, 0, 0, abi.UPSAMPLE_LINEAR, 1)


def variations():
    """the good parameters with one field at a time (and some pairs) walked through good and bad values"""
    out = [GOOD]
    out += [(crop,) + GOOD[1:] for crop in CROPS]
    for hb, light in itertools.product((0, 3, 4, 7, 8, 9, 10, 11, 12, 13, -1, 16), (0, 1, 2, -1)):
        out.append(GOOD[:1] + (hb, GOOD[2], light) + GOOD[4:])
    for pctl, hb, light in itertools.product(((0, 10000), (-1, 5), (5, 10001), (10000, 0), (5000, 1 << 30)), (0, 8), (0, 1)):
        out.append(GOOD[:1] + (hb, pctl, light) + GOOD[4:])
    for light in (0, 1):
        for matrix in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, -1):
            out.append(GOOD[:3] + (light, matrix) + GOOD[5:])
        for fr, loc, up in itertools.product((0, 1, 2, -1), (0, 2, 5, 6, -1), (abi.UPSAMPLE_NEAREST, abi.UPSAMPLE_LINEAR, 2, -1)):
            out.append(GOOD[:3] + (light, 1, fr, loc, up, 16))
        for tc in range(-1, 20):
            out.append(GOOD[:3] + (light,) + GOOD[4:8] + (tc,))
        # an unsupported matrix or transfer next to an invalid field: the invalid argument is reported
        out.append(GOOD[:3] + (light, 2, 0, 9, abi.UPSAMPLE_LINEAR, 1))
        out.append(GOOD[:1] + (8, (0, 20000), light, 1, 0, 0, abi.UPSAMPLE_LINEAR, 3))
    return out


# ------------------------------------------------------------------------------------------------ the layout
def test_result_layout():
    r = abi.StatsResult
    assert C.sizeof(r) == 176 and C.alignment(r) == 8
    offs = {"n": 0, "sum": 24, "sum_sq": 48, "min": 72, "max": 84, "pctl": 96, "light_n": 120, "light_sum": 128, "light_mean": 136, "light_max_code": 144,
            "light_pctl_code": 148, "reserved": 156, "light_max": 160, "light_pctl": 164, "reserved2": 172}
    for name, off in offs.items():
        assert getattr(r, name).offset == off, name
        assert off % (8 if name in ("n", "sum", "sum_sq", "light_n", "light_sum", "light_mean") else 4) == 0
    assert r.pctl.size == 24 and r.min.size == 12 and r.light_pctl.size == 8
    p = abi.StatsParams
    assert C.sizeof(p) == 52 and p.hist_bits.offset == 16 and p.pctl_e4.offset == 20 and p.light.offset == 28 and p.matrix.offset == 32
    assert p.full_range.offset == 36 and p.chroma_loc.offset == 40 and p.upsample.offset == 44 and p.transfer.offset == 48
    # the bytes of a result as the device writes them -> the dict
    raw = np.zeros(176, np.uint8)
    raw[:120].view(np.uint64)[:9] = np.arange(1, 10)
    raw[72:120].view(np.uint32)[:] = np.arange(100, 112)
    raw[120:128].view(np.uint64)[0] = 77
    raw[128:144].view(np.float64)[:] = (1.5, 0.25)
    raw[144:160].view(np.uint32)[:] = (900, 10, 800, 0)
    raw[160:176].view(np.float32)[:] = (0.5, 0.125, 0.25, 0)
    d = abi.stats_result_dict(raw)
    assert d["n"] == [1, 2, 3] and d["sum"] == [4, 5, 6] and d["sum_sq"] == [7, 8, 9] and d["min"] == [100, 101, 102] and d["max"] == [103, 104, 105]
    assert d["pctl"] == [[106, 107], [108, 109], [110, 111]] and d["light_n"] == 77 and (d["light_sum"], d["light_mean"]) == (1.5, 0.25)
    assert (d["light_max_code"], d["light_pctl_code"]) == (900, [10, 800]) and (d["light_max"], d["light_pctl"]) == (0.5, [0.125, 0.25])
    assert d == abi.stats_result_dict(raw.view(np.int64))


def test_moments():
    mean, var = abi.stats_moments({"n": [4, 2, 1], "sum": [10, 3, 7], "sum_sq": [30, 5, 49]})
    assert mean == [Fraction(5, 2), Fraction(3, 2), 7] and var == [Fraction(5, 4), Fraction(1, 4), 0]


# ------------------------------------------------------------------------------------------------ the size function and the check
def test_hist_size_sweep():
    lib = abi.load()
    assert lib.xgpu_stats_hist_size(None, 10) == 0
    seen = set()
    for par, bd in itertools.product(variations(), (7, 8, 10, 12, 13)):
        got = lib.xgpu_stats_hist_size(C.byref(c_par(*par)), bd)
        assert got == rule_hist_size(par, bd), (par, bd)
        seen.add(got > 0)
    assert seen == {False, True}
    # spelled out once
    assert lib.xgpu_stats_hist_size(C.byref(abi.make_stats_params()), 10) == 3 * 256 * 4
    assert lib.xgpu_stats_hist_size(C.byref(abi.make_stats_params(hist_bits=12, light=True, transfer=16)), 12) == 4 * 4096 * 4
    assert lib.xgpu_stats_hist_size(C.byref(abi.make_stats_params(hist_bits=0, light=True)), 8) == 256 * 4
    assert lib.xgpu_stats_hist_size(C.byref(abi.make_stats_params(hist_bits=0)), 8) == 0      # valid, nothing to write


def test_check_sweep():
    lib = abi.load()
    assert lib.xgpu_stats_check(None, 72, 40, 8) == INVALID
    seen = set()
    for par, (w, h), bd in itertools.product(variations(), SIZES, (7, 8, 10, 12, 13)):
        got = lib.xgpu_stats_check(C.byref(c_par(*par)), w, h, bd)
        assert got == rule_check(par, w, h, bd), (par, w, h, bd)
        seen.add(got)
    assert seen == {0, INVALID, UNSUPPORTED}

    # each refusal of the contract, spelled out once against a call that passes
    def chk(bd=10, w=200, h=136, **kw):
        return lib.xgpu_stats_check(C.byref(abi.make_stats_params(**kw)), w, h, bd)

    lit = dict(light=True, transfer=16, matrix=9)
    assert chk() == 0 and chk(**lit) == 0 and chk(hist_bits=0) == 0 and chk(hist_bits=10) == 0
    assert chk(w=0) == INVALID and chk(h=-2) == INVALID and chk(w=201) == INVALID                     # a size that is not positive and even
    assert chk(bd=7) == INVALID and chk(bd=13) == INVALID
    assert chk(w=65536, h=32768) == INVALID and chk(w=65536, h=32766) == 0                            # width * height >= 2^31
    assert chk(crop=(1, 1, 0, 0)) == INVALID and chk(crop=(0, -2, 0, 0)) == INVALID and chk(crop=(100, 100, 0, 0)) == INVALID
    assert chk(hist_bits=3) == INVALID and chk(hist_bits=11) == INVALID and chk(hist_bits=11, bd=12) == 0
    assert chk(pctl_e4=(0, 10001)) == INVALID and chk(pctl_e4=(-1, 0)) == INVALID and chk(pctl_e4=(0, 10000)) == 0
    assert chk(pctl_e4=(0, 10001), hist_bits=0) == 0 and chk(pctl_e4=(0, 10001), hist_bits=0, **lit) == INVALID      # read only with a histogram
    assert chk(light=2) == INVALID
    assert chk(**dict(lit, upsample=2)) == INVALID and chk(**dict(lit, chroma_loc=6)) == INVALID and chk(**dict(lit, full_range=2)) == INVALID
    assert chk(upsample=2, chroma_loc=6, matrix=0, transfer=0) == 0                                  # not read without light
    assert chk(**dict(lit, matrix=2)) == UNSUPPORTED and chk(**dict(lit, transfer=2)) == UNSUPPORTED and chk(**dict(lit, transfer=17)) == UNSUPPORTED


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_lin_is_the_lin_of_colour_tables(bd):
    lib = abi.load()
    fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16)
    seen = 0
    for tc in range(-1, 20):
        got = abi.stats_lin(lib, tc, bd)
        want = abi.colour_tables(lib, fmt, abi.make_colour_transform(src_transfer=tc, dst_transfer=8), bd)
        if tc not in abi.STATS_TRANSFERS:
            assert isinstance(got, int) and got == UNSUPPORTED and want == UNSUPPORTED, tc
            continue
        assert got.dtype == np.float32 and got.shape == (1 << bd,) and np.array_equal(got.view(np.uint32), want["lin"].view(np.uint32)), tc
        assert got[0] == 0 and got[-1] == 1 and np.all(np.diff(got) > 0), tc
        seen += 1
    assert seen == len(abi.STATS_TRANSFERS)
    buf = (C.c_float * 4096)(*([7.0] * 4096))
    assert lib.xgpu_stats_lin(16, bd, buf) == 0 and not any(buf[1 << bd:])      # 0 behind the table
    assert lib.xgpu_stats_lin(16, bd, None) == INVALID and lib.xgpu_stats_lin(16, 7, buf) == INVALID and lib.xgpu_stats_lin(16, 13, buf) == INVALID


# ------------------------------------------------------------------------------------------------ stats_ref against itself
def test_hand_computed_planes():
    """4x4 luma, 2x2 chroma at 8 bit"""
    y = np.array([[0, 1, 2, 3], [16, 17, 18, 19], [128, 128, 128, 128], [255, 255, 240, 15]], np.uint16)
    u = np.array([[128, 128], [128, 128]], np.uint16)
    v = np.array([[0, 255], [16, 31]], np.uint16)
    d = sr.stats([y, u, v], 8, hist_bits=4, pctl_e4=(0, 10000))
    assert d["n"] == [16, 4, 4] and d["sum"] == [6 + 70 + 512 + 765, 512, 302] and d["min"] == [0, 128, 0] and d["max"] == [255, 128, 255]
    assert d["sum_sq"] == [1 + 4 + 9 + 256 + 289 + 324 + 361 + 4 * 16384 + 2 * 65025 + 57600 + 225, 4 * 16384, 65025 + 256 + 961]
    assert d["hist"].dtype == np.uint32 and d["hist"].shape == (3, 16)
    assert d["hist"][0].tolist() == [5, 4, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 3]
    assert d["hist"][1].tolist() == [0] * 8 + [4] + [0] * 7 and d["hist"][2].tolist() == [1, 2] + [0] * 13 + [1]
    assert d["pctl"] == [[0, 240], [128, 128], [0, 240]]      # the lowest and the highest occupied bin, as its lower edge
    assert [int(h.sum()) for h in d["hist"]] == d["n"]
    assert d["light_hist"] is None and d["light_n"] == 0 and d["light_sum"] == 0
    # hist_bits = B: the bin is the sample; a crop; no histogram
    d = sr.stats([y, u, v], 8, crop=(2, 0, 0, 2), hist_bits=8, pctl_e4=(5000, 7500))
    assert d["n"] == [4, 1, 1] and d["sum"] == [2 + 3 + 18 + 19, 128, 255] and d["pctl"] == [[3, 18], [128, 128], [255, 255]]
    d = sr.stats([y, u, v], 8, hist_bits=0)
    assert d["hist"] is None and d["pctl"] == [[0, 0]] * 3 and d["n"] == [16, 4, 4]


def test_patterns_above_the_depth_count_in_the_last_bin():
    s = np.array([[0x3FF, 0x400, 0xFFFF, 0x8000]], np.uint16)
    assert sr.histogram(s, 10, 10)[-1] == 4 and sr.histogram(s, 10, 4)[-1] == 4
    c = sr.census(s)
    assert c == {"n": 4, "sum": 0x3FF + 0x400 + 0xFFFF + 0x8000, "sum_sq": 0x3FF ** 2 + 0x400 ** 2 + 0xFFFF ** 2 + 0x8000 ** 2, "min": 0x3FF, "max": 0xFFFF}
    # int16 planes are read as unsigned patterns
    assert sr.census(sr.crop_plane(np.full((2, 2), -1, np.int16), (0, 0, 0, 0), 0))["max"] == 0xFFFF


def test_percentile_on_both_sides_of_its_threshold():
    """n = 10000: cum * 10000 >= p * n is cum >= p.  2500 samples in bin 3, the rest in bin 9: p = 2500 is reached by bin 3 exactly; with one sample fewer in
    bin 3 it is not"""
    h = np.zeros(16, np.uint32)
    h[3], h[9] = 2500, 7500
    assert sr.percentile_bin(h, 2500) == 3 and sr.percentile_bin(h, 2501) == 9 and sr.percentile_bin(h, 2499) == 3
    h[3], h[9] = 2499, 7501
    assert sr.percentile_bin(h, 2500) == 9 and sr.percentile_bin(h, 2499) == 3
    # p = 0 and p = 10000: the lowest and the highest occupied bin
    assert sr.percentile_bin(h, 0) == 3 and sr.percentile_bin(h, 10000) == 9
    one = np.zeros(16, np.uint32)
    one[15] = 1
    assert sr.percentile_bin(one, 0) == 15 and sr.percentile_bin(one, 10000) == 15 and sr.percentile_bin(one, 1) == 15
    # an n that does not divide: 3 samples, p = 3333 -> 3 * 3333 = 9999 <= 10000 * 1, p = 3334 -> 10002 > 10000
    h3 = np.array([1, 1, 1, 0], np.uint32)
    assert sr.percentile_bin(h3, 3333) == 0 and sr.percentile_bin(h3, 3334) == 1 and sr.percentile_bin(h3, 6667) == 2


def test_histogram_sums_equal_n():
    rng = np.random.default_rng(1)
    planes = [rng.integers(0, 1 << 16, (24 >> s, 40 >> s)).astype(np.uint16) for s in (0, 1, 1)]
    for bd, hb in ((8, 4), (10, 8), (12, 12)):
        d = sr.stats(planes, bd, crop=(2, 4, 0, 2), hist_bits=hb)
        assert [int(h.astype(np.uint64).sum()) for h in d["hist"]] == d["n"] == [34 * 22, 17 * 11, 17 * 11]


def test_light_sum_order():
    lib = abi.load()
    lin = abi.stats_lin(lib, 16, 10)
    # one bin: count * lin[k], rounded once
    h = np.zeros(1024, np.uint32)
    h[700] = 33177600
    assert sr.light_sum(h, lin) == np.float64(33177600) * np.float64(lin[700])
    # two bins of one residue class: added in ascending k; of two classes: the lower class first
    h[700 - 64] = 12345
    a, b = np.float64(12345) * np.float64(lin[636]), np.float64(33177600) * np.float64(lin[700])
    assert sr.light_sum(h, lin) == a + b
    h[5] = 99
    c = np.float64(99) * np.float64(lin[5])
    assert sr.light_sum(h, lin) == c + (a + b)      # part[5] comes before part[60] (636 = 9 * 64 + 60)
    # a full histogram: the same as the definition written with Python floats (binary64, one rounding per operation)
    rng = np.random.default_rng(2)
    h = rng.integers(0, 1 << 16, 1024).astype(np.uint32)
    part = [0.0] * 64
    for k in range(1024):
        part[k % 64] = part[k % 64] + float(int(h[k])) * float(lin[k])
    tot = part[0]
    for l in range(1, 64):
        tot = tot + part[l]
    assert float(sr.light_sum(h, lin)).hex() == tot.hex()


@pytest.mark.parametrize("bd", [8, 10])
def test_max_rgb_is_the_maximum_of_the_rgb_output(bd):
    lib = abi.load()
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 1 << bd, (24 >> s, 40 >> s)).astype(np.uint16) for s in (0, 1, 1)]
    crop = (2, 4, 0, 2)
    for matrix, fr, loc, up in ((1, False, 0, "linear"), (9, True, 2, "nearest"), (5, False, 1, "linear")):
        m = sr.max_rgb(planes, bd, crop=crop, matrix=matrix, full_range=fr, chroma_loc=loc, upsample=up)
        rgb = colour_ref.convert([p.view(np.int16) for p in planes], bd, matrix=matrix, full_range=fr, chroma_loc=loc, mode=up, dtype=colour_ref.U16, crop=crop)
        assert m.shape == (22, 34) and np.array_equal(m, rgb.max(axis=0)) and int(m.max()) <= (1 << bd) - 1
        lin = abi.stats_lin(lib, 16, bd)
        d = sr.stats(planes, bd, crop=crop, hist_bits=0, pctl_e4=(0, 5000), light=dict(matrix=matrix, full_range=fr, chroma_loc=loc, upsample=up), lin=lin)
        assert d["light_n"] == 22 * 34 == int(d["light_hist"].sum()) and d["light_max_code"] == int(m.max()) and d["light_pctl_code"][0] == int(m.min())
        assert d["light_pctl_code"][1] == int(np.sort(m.reshape(-1))[22 * 34 // 2 - 1])      # the smallest code with at least half of the samples at or below it
        assert d["light_max"] == lin[int(m.max())] and d["light_mean"] == d["light_sum"] / np.float64(22 * 34)
        assert abs(float(d["light_mean"]) - float(lin[m].astype(np.float64).mean())) < 1e-12
