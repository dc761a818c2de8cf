"""CPU suite for the surface ladder: xgpu_scale_taps_ex against the fractions.Fraction restatement (tests/ladder_ref.py), the
invariants of a tap row, the two degenerate cases, the sizes and refusals of xgpu_output_ladder_check and the Python plumbing.  No GPU: the functions tested are
the host-only ones."""
import ctypes as C
from fractions import Fraction
import itertools

import numpy as np
import pytest

import ladder_ref as lr
import stub_decoder
from xevd_amd import abi

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -101, -104
PLANES = (2, 9, 37, 148, 296)
# destination luma samples per source luma sample: reductions down to 1 / 64, the same size, enlargements up to 8 times
RATIOS = (Fraction(1, 64), Fraction(1, 33), Fraction(10, 37), Fraction(1, 2), Fraction(1), Fraction(3, 2), Fraction(8))
SUBS = ((1, 1), (2, 2))
FILTERS = (lr.BILINEAR, lr.AREA)


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def _dst(n, ratio):
    N = n * ratio
    return int(N) if N.denominator == 1 else int(N) + 1      # rounded up: never below the 1 / 64 limit


def _grid():
    """(n, s, S, N) of every table of the grid that is inside the limits"""
    for n, ratio, (s, S) in itertools.product(PLANES, RATIOS, SUBS):
        N = _dst(n, ratio)      # s = S: the ratio of the planes is the ratio of the luma grids
        if N >= 1 and N * S >= 2 and n * s <= 64 * N * S and N * S <= 8 * n * s:
            yield n, s, S, N


def _checked_outputs(N):
    """every destination sample of a short axis; of a long one both ends and every 37th"""
    if N <= 2048:
        return list(range(N))
    return sorted(set(range(48)) | set(range(N - 48, N)) | set(range(0, N, 37)))


@pytest.mark.parametrize("n", PLANES)
def test_taps_equal_the_fraction_restatement(lib, n):
    done = 0
    for (n_, s, S, N), d, D, filt in itertools.product(_grid(), (0, 1, 2), (0, 1, 2), FILTERS):
        if n_ != n:
            continue
        first, count, w = abi.scale_taps_ex(lib, n, s, d, N, S, D, filt)
        outs = _checked_outputs(N)
        exp = lr.taps_ex(n, s, d, N, S, D, filt, outs)
        for o, (e_first, e_q) in zip(outs, exp):
            assert (int(first[o]), int(count[o])) == (e_first, len(e_q)), (n, s, d, N, S, D, filt, o)
            assert [int(v) for v in w[o, :count[o]]] == e_q, (n, s, d, N, S, D, filt, o)
            assert not w[o, count[o]:].any()
        done += 1
    assert done >= 2 * 9 * 2 * 3


def test_every_row_sums_to_one_is_positive_and_contiguous(lib):
    widest = 0
    for (n, s, S, N), d, D, filt in itertools.product(_grid(), (0, 1, 2), (0, 1, 2), FILTERS):
        first, count, w = abi.scale_taps_ex(lib, n, s, d, N, S, D, filt)
        what = (n, s, d, N, S, D, filt)
        assert (w.astype(np.int64).sum(1) == 16384).all(), what
        assert (w >= 0).all(), what
        assert (first >= 0).all() and (count >= 1).all() and (first + count <= n).all(), what
        inside = np.arange(w.shape[1])[None, :] < count[:, None]
        # contiguous: the count[o] samples from first[o] (a weight at a window's edge may quantise to 0), zeros behind them
        assert not w[~inside].any() and (w.max(1) > 0).all(), what
        assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all(), what      # rows move right monotonically: what pass 2's staging relies on
        widest = max(widest, int(count.max()))
    assert 100 < widest <= 131


def test_luma_destination_is_xgpu_scale_taps(lib):
    """S = 1, D = 0: xgpu_scale_taps_ex is xgpu_scale_taps array for array, for every source subsampling and siting"""
    for n, ratio, s, d, filt in itertools.product(PLANES, RATIOS, (1, 2), (0, 1, 2), FILTERS):
        N = _dst(n * s, ratio)
        a, b = abi.scale_taps(lib, n, s, d, N, filt), abi.scale_taps_ex(lib, n, s, d, N, 1, 0, filt)
        if isinstance(a, int):
            assert a == b == ERR_UNSUPPORTED, (n, s, d, N, filt)
            continue
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y), (n, s, d, N, filt)


def test_same_size_and_siting_is_the_single_tap(lib):
    for n, (s, S), d, filt in itertools.product(PLANES, SUBS, (0, 1, 2), FILTERS):
        if n * S < 2:
            continue
        first, count, w = abi.scale_taps_ex(lib, n, s, d, n, S, d, filt)
        assert np.array_equal(first, np.arange(n)) and (count == 1).all() and w.shape == (n, 1) and (w == 16384).all(), (n, s, d, filt)


def test_taps_ex_refusals(lib):
    assert abi.scale_taps_ex(lib, 16, 2, 0, 8, 3, 0) == ERR_INVALID_ARGUMENT      # destination subsampling
    assert abi.scale_taps_ex(lib, 16, 2, 0, 8, 2, 3) == ERR_INVALID_ARGUMENT      # destination siting
    assert abi.scale_taps_ex(lib, 16, 2, 3, 8, 2, 0) == ERR_INVALID_ARGUMENT
    assert abi.scale_taps_ex(lib, 16, 2, 0, 8, 2, 0, 7) == ERR_INVALID_ARGUMENT
    assert abi.scale_taps_ex(lib, 128, 2, 0, 1, 2, 0) == ERR_UNSUPPORTED          # 256 luma samples to 2: below 1 / 64
    assert abi.scale_taps_ex(lib, 2, 2, 0, 17, 2, 0) == ERR_UNSUPPORTED           # above 8 times
    assert abi.scale_taps_ex(lib, 2, 1, 0, 1, 1, 0) == ERR_UNSUPPORTED            # one luma sample
    assert not isinstance(abi.scale_taps_ex(lib, 2, 2, 0, 1, 2, 0), int)          # the 1 x 1 chroma plane of a 2 x 2 rung


# ---- sizes and refusals
W, H = 592, 296


def _fmt(layout=abi.OUT_NV12, dtype=abi.OUT_U8, obd=8, **kw):
    return abi.make_output_format(layout, dtype, out_bit_depth=obd, **kw)


def _check(lib, fmt, sizes, lp=None, bd=10, pitch=0, short=0, n=None, width=W, height=H):
    """xgpu_output_ladder_check for rungs of (H, W) `sizes`, each destination `short` bytes below what the rung needs"""
    need = [lib.xgpu_output_ladder_rung_size(C.byref(fmt), w, h, pitch, bd) for h, w in sizes]
    rungs = abi.make_rungs([(w, h, pitch, None, max(nb - short, 0)) for (h, w), nb in zip(sizes, need)])
    lp = lp or abi.make_ladder_params()
    return lib.xgpu_output_ladder_check(C.byref(fmt), C.byref(lp), rungs, len(sizes) if n is None else n, width, height, bd)


ACCEPTED = [(abi.OUT_YUV420P, abi.OUT_U8, 8), (abi.OUT_YUV420P, abi.OUT_U16, 0), (abi.OUT_YUV420P, abi.OUT_U16, 12), (abi.OUT_NV12, abi.OUT_U8, 8),
            (abi.OUT_NV12, abi.OUT_U16, 0), (abi.OUT_NV12, abi.OUT_U16, 16), (abi.OUT_P016, abi.OUT_U16, 0), (abi.OUT_P016, abi.OUT_U16, 8),
            (abi.OUT_P016, abi.OUT_U16, 16)]
REFUSED = [(abi.OUT_YUV420P, abi.OUT_U8, 0), (abi.OUT_YUV420P, abi.OUT_U16, 8), (abi.OUT_YUV420P, abi.OUT_F32, 0), (abi.OUT_NV12, abi.OUT_U8, 0),
           (abi.OUT_NV12, abi.OUT_U8, 10), (abi.OUT_NV12, abi.OUT_U16, 8), (abi.OUT_NV12, abi.OUT_F16, 0), (abi.OUT_P016, abi.OUT_U8, 8),
           (abi.OUT_P016, abi.OUT_U16, 7), (abi.OUT_P016, abi.OUT_U16, 17)]


def test_rung_size_is_the_format_size_at_the_rung(lib):
    for (layout, dtype, obd), (h, w), pitch_extra in itertools.product(ACCEPTED, ((148, 296), (10, 18), (2, 2), (444, 888)), (0, 6)):
        es = 1 if dtype == abi.OUT_U8 else 2
        pitch = 0 if layout == abi.OUT_YUV420P or not pitch_extra else (w + pitch_extra) * es
        # the crop of the call is the source: it has no part in the size of a rung
        got = lib.xgpu_output_ladder_rung_size(C.byref(_fmt(layout, dtype, obd, crop=(2, 4, 6, 8))), w, h, pitch, 10)
        exp = lib.xgpu_output_format_size(C.byref(_fmt(layout, dtype, obd, row_pitch=pitch)), w, h, 10)
        assert got == exp > 0, (layout, dtype, obd, h, w, pitch)
        tight = w * h * 3 // 2 * es
        assert got == (tight if not pitch else (h * 3 // 2 - 1) * pitch + w * es)
    for layout, dtype, obd in REFUSED:
        assert lib.xgpu_output_ladder_rung_size(C.byref(_fmt(layout, dtype, obd)), 296, 148, 0, 10) == 0, (layout, dtype, obd)
    f = _fmt()
    assert lib.xgpu_output_ladder_rung_size(C.byref(f), 297, 148, 0, 10) == 0
    assert lib.xgpu_output_ladder_rung_size(C.byref(f), 296, 148, 200, 10) == 0                                    # shorter than a row
    assert lib.xgpu_output_ladder_rung_size(C.byref(_fmt(abi.OUT_P016, abi.OUT_U16, 0)), 296, 148, 601, 10) == 0  # not a multiple of the element
    assert lib.xgpu_output_ladder_rung_size(C.byref(_fmt(abi.OUT_YUV420P, abi.OUT_U8, 8)), 296, 148, 296, 10) == 0
    assert lib.xgpu_output_ladder_rung_size(C.byref(_fmt(abi.OUT_RGB_PLANAR, abi.OUT_U8, 0)), 296, 148, 0, 10) == 0
    assert lib.xgpu_output_ladder_rung_size(C.byref(_fmt(bgr=True)), 296, 148, 0, 10) == 0


def test_check_accepts_the_ladder(lib):
    sizes = [(148, 296), (80, 160), (10, 18), (296, 592), (444, 888)]
    for (layout, dtype, obd), filt, loc in itertools.product(ACCEPTED, (abi.SCALE_BILINEAR, abi.SCALE_AREA), (None, 0, 5)):
        assert _check(lib, _fmt(layout, dtype, obd), sizes, abi.make_ladder_params(filt, loc)) == 0, (layout, dtype, obd, filt, loc)
    assert _check(lib, _fmt(), [(148, 296)] * 8) == 0
    assert _check(lib, _fmt(crop=(2, 4, 6, 8)), [(148, 296)]) == 0
    assert _check(lib, _fmt(), [(100, 300)], width=320, height=240) == 0
    assert _check(lib, _fmt(), [(2, 2), (64, 64)], width=64, height=64) == 0
    assert _check(lib, _fmt(), [(6, 10), (296 * 8, 592 * 8)]) == 0                     # the limits themselves: 1 / 64 rounded up, 8 times
    assert _check(lib, _fmt(abi.OUT_P016, abi.OUT_U16, 0), [(10, 18)], pitch=(18 + 3) * 2) == 0


def test_check_refusals(lib):
    f, one = _fmt(), [(148, 296)]
    inv, uns = ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED
    assert _check(lib, f, one, n=0) == inv and _check(lib, f, one * 9) == inv and _check(lib, f, one, n=-1) == inv      # n outside 1 .. 8
    assert _check(lib, f, [(148, 297)]) == inv and _check(lib, f, [(147, 296)]) == inv and _check(lib, f, one + [(81, 160)]) == inv      # odd rung sizes
    for crop in ((1, 0, 0, 0), (0, 0, 0, 3), (-2, 0, 0, 0), (300, 292, 0, 0)):
        assert _check(lib, _fmt(crop=crop), one) == inv, crop
    assert _check(lib, f, one, abi.make_ladder_params(filter=2)) == inv and _check(lib, f, one, abi.make_ladder_params(filter=-1)) == inv
    assert _check(lib, f, one, abi.make_ladder_params(dst_chroma_loc=6)) == inv and _check(lib, f, one, abi.make_ladder_params(dst_chroma_loc=-2)) == inv
    assert _check(lib, _fmt(chroma_loc=6), one) == inv
    for layout in (abi.OUT_RGB_PLANAR, abi.OUT_RGB_INTERLEAVED, abi.OUT_YUV444_PLANAR, abi.OUT_YUV444_INTERLEAVED, 7, -1):
        assert _check(lib, _fmt(layout, abi.OUT_U8, 0), one) == inv, layout
    for layout, dtype, obd in REFUSED:
        assert _check(lib, _fmt(layout, dtype, obd), one) == inv, (layout, dtype, obd)
    assert _check(lib, _fmt(abi.OUT_YUV420P, abi.OUT_U8, 8), one, pitch=296) == inv          # a pitch with YUV420P
    assert _check(lib, f, one, pitch=295) == inv                                             # shorter than a row
    assert _check(lib, _fmt(abi.OUT_P016, abi.OUT_U16, 0), one, pitch=2 * 296 + 1) == inv    # not a multiple of the element
    assert _check(lib, _fmt(bgr=True), one) == inv
    assert _check(lib, f, one, short=1) == inv and _check(lib, f, one + [(80, 160)], short=1) == inv      # undersized destinations
    lp = abi.make_ladder_params()
    assert lib.xgpu_output_ladder_check(None, C.byref(lp), abi.make_rungs([]), 1, W, H, 10) == inv
    assert lib.xgpu_output_ladder_check(C.byref(f), None, abi.make_rungs([]), 1, W, H, 10) == inv
    assert lib.xgpu_output_ladder_check(C.byref(f), C.byref(lp), None, 1, W, H, 10) == inv
    assert _check(lib, f, one, width=591) == inv and _check(lib, f, one, bd=13) == inv
    # outside the scaled output's limits: 2 .. 16384, Ws / 64 <= Wd <= 8 Ws per axis
    for size in ((148, 8), (4, 296), (148, 592 * 8 + 2), (296 * 8 + 2, 296), (0, 296), (148, 0), (148, 16386)):
        assert _check(lib, f, [size]) == uns, size
    assert _check(lib, f, one, width=4096, height=2048) == 0 and _check(lib, f, [(2048, 16386)], width=4096, height=2048) == uns
    # the intermediates of all rungs together: 8 rungs of 16384 rows from a 8192-wide source are 8 x 384 MiB
    assert _check(lib, f, [(16384, 8192)], width=8192, height=4096) == 0
    assert _check(lib, f, [(16384, 8192)] * 2, width=8192, height=4096) == uns


# ---- Python plumbing
def test_structs_and_prototypes_load(lib):
    assert C.sizeof(abi.SurfaceRung) == 4 + 4 + 8 + 8 + 8 and C.sizeof(abi.LadderParams) == 8
    assert abi.SurfaceRung.row_pitch.offset == 8 and abi.SurfaceRung.d_dst.offset == 16 and abi.SurfaceRung.dst_size.offset == 24
    assert abi.MAX_RUNGS == 8
    for name in ("xgpu_scale_taps_ex", "xgpu_output_ladder_rung_size", "xgpu_output_ladder_check", "xgpu_pic_output_device_ladder"):
        assert name in abi.exported_names() and getattr(lib, name).argtypes
    lp = abi.make_ladder_params()
    assert (lp.filter, lp.dst_chroma_loc) == (abi.SCALE_BILINEAR, -1)
    lp = abi.make_ladder_params(abi.SCALE_AREA, 3)
    assert (lp.filter, lp.dst_chroma_loc) == (abi.SCALE_AREA, 3)
    r = abi.make_rungs([(296, 148, 300, None, 12345), (18, 10, 0, 4096, 7)])
    assert (r[0].width, r[0].height, r[0].row_pitch, r[0].d_dst, r[0].dst_size) == (296, 148, 300, None, 12345)
    assert (r[1].width, r[1].d_dst, r[1].dst_size) == (18, 4096, 7)


def test_python_refusals_come_before_any_library_call(lib):
    """pic_output_surfaces raises ValueError for what the arguments alone decide - on a decoder object without a context, so no call into a context can have run"""
    import torch
    from xevd_amd.decoder import XgpuDecoder
    dec = stub_decoder.XgpuDecoder(W, H, 10)
    dec.lib, dec.sp, dec.ctx = lib, abi.make_seq_params(W, H, 10), None
    surfaces = XgpuDecoder.pic_output_surfaces
    one = [(148, 296)]
    for bad in (dict(sizes=one, layout="rgb"), dict(sizes=one, layout="yuv444"), dict(sizes=one, filter="lanczos"), dict(sizes=[]), dict(sizes=one * 9),
                dict(sizes=[(148, 297)]), dict(sizes=[(147, 296)]), dict(sizes=[(0, 296)]), dict(sizes=one, dst_chroma_loc=6), dict(sizes=one, chroma_loc=7),
                dict(sizes=one, dtype=torch.float32), dict(sizes=one, layout="p016", dtype=torch.uint8), dict(sizes=one, dtype=torch.uint8, out_bit_depth=10),
                dict(sizes=one, layout="nv12", dtype=torch.int16, out_bit_depth=8), dict(sizes=one, layout="p016", out_bit_depth=17),
                dict(sizes=one, crop=(1, 0, 0, 0)), dict(sizes=[(148, 8)]), dict(sizes=[(296 * 8 + 2, 296)]), dict(sizes=one, out=[]),
                dict(sizes=one, out=[None, None])):
        with pytest.raises(ValueError):
            surfaces(dec, 0, **bad)
