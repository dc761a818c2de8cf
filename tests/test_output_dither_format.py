"""CPU suite for the dithered output (xgpu_pic_output_device_dithered / _packed_dithered): the exported symbols, the refusal codes
of xgpu_output_dither_check in their order, the host constructors xgpu_dither_bayer / _blue / _phase against the numpy restatement tests/dither_ref.py bit for
bit, the blue-noise matrix' spectrum against a random permutation's, and two properties of the rule through the restatement alone.  Nothing here needs a GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import colour_ref as cr
import dither_ref as dr
import packed_ref as pr
import yuv_ref as yr
from xevd_amd import abi

INVALID, UNSUPPORTED = -101, -104
PQ_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)


def check(f=None, pf=None, cm=None, mw=8, mh=8, k=6, width=64, height=48, bd=10):
    cmt = None if cm is None else abi.make_colour_transform(**cm)
    return abi.load().xgpu_output_dither_check(None if f is None else C.byref(f), None if pf is None else C.byref(pf), None if cmt is None else C.byref(cmt),
                                               mw, mh, k, width, height, bd)


def test_exported_symbols():
    for name in ("xgpu_dither_bayer", "xgpu_dither_blue", "xgpu_dither_phase", "xgpu_output_dither_check", "xgpu_dither_create", "xgpu_dither_destroy",
                 "xgpu_pic_output_device_dithered", "xgpu_pic_output_device_packed_dithered"):
        assert name in abi.exported_names(), name
        assert hasattr(abi.load(), name)
    assert abi.MAX_DITHER == 4
    d = abi.make_dither_params(2, (3, 1))
    assert (d.handle, d.phase_x, d.phase_y) == (2, 3, 1)


def test_check_accepts_every_listed_form():
    for bd in (8, 10, 12):
        for lay, dt, cm in itertools.product((abi.OUT_RGB_PLANAR, abi.OUT_RGB_INTERLEAVED), (abi.OUT_U8, abi.OUT_U16), (None, PQ_SRGB)):
            assert check(abi.make_output_format(lay, dt, bgr=True), cm=cm, bd=bd) == 0, (bd, lay, dt, cm)
        assert check(abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8), bd=bd) == 0
        assert check(abi.make_output_format(abi.OUT_NV12, abi.OUT_U16, out_bit_depth=10), bd=bd) == 0
        for d in (0, 8, 10, 12):
            assert check(abi.make_output_format(abi.OUT_P016, abi.OUT_U16, out_bit_depth=d), bd=bd) == 0
        for dt, cm in itertools.product((abi.OUT_U8, abi.OUT_U16), (None, PQ_SRGB)):
            assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, dt, bgr=True, alpha=0.5), cm=cm, bd=bd) == 0
            assert check(pf=abi.make_packed_format(abi.PACKED_RGB10A2, bgr=dt == abi.OUT_U8), cm=cm, bd=bd) == 0
    # every matrix size and k in range; k = 14 <= S = 15 of the 12-bit U16 matrix
    for side, k in itertools.product((1, 2, 4, 128), (1, 14)):
        assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), mw=side, mh=128 // side, k=k, bd=12) == 0
    f = abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_U8, row_pitch=3 * 64 + 16)
    assert check(f) == 0


def test_check_refusals_come_in_their_order():
    rgb = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8)
    nv12 = abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)
    # neither or both formats
    assert check() == INVALID and check(rgb, abi.make_packed_format()) == INVALID
    # 1. the plain call's refusals, with its codes: before the dtype, the layout and the matrix
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, matrix=2), k=0) == UNSUPPORTED
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, crop=(1, 0, 0, 0)), k=0) == INVALID
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, out_bit_depth=12), bd=10, k=0) == INVALID
    assert check(abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_U8, row_pitch=3 * 64 - 1), k=0) == INVALID
    assert check(abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=10), k=0) == INVALID
    assert check(rgb, bd=13) == INVALID and check(rgb, width=0) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_F16, matrix=2), k=0) == UNSUPPORTED
    assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_F16, alpha=1.5), k=0) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_RGB10A2, dtype=abi.OUT_U16), k=0) == INVALID
    # 2. a float dtype: UNSUPPORTED, before the layout (YUV444 has float forms) and the matrix
    for dt in (abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32):
        assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, dt), mw=3) == UNSUPPORTED
        assert check(abi.make_output_format(abi.OUT_YUV444_PLANAR, dt), mw=3) == UNSUPPORTED
        assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, dt), mw=3) == UNSUPPORTED
        assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, dt), cm=PQ_SRGB) == UNSUPPORTED
    # 3. a layout outside the list: INVALID, before the matrix (whose refusal is UNSUPPORTED)
    assert check(abi.make_output_format(abi.OUT_YUV420P, abi.OUT_U8, out_bit_depth=8), k=0) == INVALID
    assert check(abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_U8), k=0) == INVALID
    assert check(abi.make_output_format(abi.OUT_YUV444_INTERLEAVED, abi.OUT_U16), k=0) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_YUYV, abi.OUT_U8, out_bit_depth=8), k=0) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_UYVY, abi.OUT_U16), k=0) == INVALID
    # 4. a transform with NV12 / P016: INVALID, before the matrix; an unsupported transform keeps the plain call's code
    assert check(nv12, cm=PQ_SRGB, k=0) == INVALID
    assert check(abi.make_output_format(abi.OUT_P016, abi.OUT_U16), cm=PQ_SRGB, k=0) == INVALID
    bad = dict(PQ_SRGB, src_transfer=3)
    plain = abi.load().xgpu_colour_tables(C.byref(rgb), C.byref(abi.make_colour_transform(**bad)), 10, C.byref(abi.ColourTables()))
    assert plain < 0 and check(rgb, cm=bad, k=0) == plain
    # 7. sizes or k outside their ranges, or k > S: UNSUPPORTED, last
    for mw, mh, k in ((0, 8, 6), (3, 8, 6), (256, 8, 6), (8, 0, 6), (8, 6, 6), (8, 256, 6), (8, 8, 0), (8, 8, 15), (-8, 8, 6)):
        assert check(rgb, mw=mw, mh=mh, k=k) == UNSUPPORTED, (mw, mh, k)
        assert check(nv12, mw=mw, mh=mh, k=k) == UNSUPPORTED
        assert check(pf=abi.make_packed_format(), mw=mw, mh=mh, k=k) == UNSUPPORTED
    # S = 27 - D >= 15 for every D <= 12, so k <= 14 always passes: the bound exists and every k in range is below it
    for bd, k in itertools.product((8, 10, 12), (1, 14)):
        assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), k=k, bd=bd) == 0


def test_bayer_is_the_reference():
    lib = abi.load()
    for log2n in range(1, 8):
        m = abi.dither_bayer(lib, log2n)
        n = 1 << log2n
        assert m.shape == (n, n) and m.dtype == np.uint16
        assert np.array_equal(m, dr.bayer(log2n)), log2n
        assert np.array_equal(np.sort(m.ravel()), np.arange(n * n)), log2n
    assert abi.dither_bayer(lib, 3)[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42]
    assert abi.dither_bayer(lib, 0) == UNSUPPORTED and abi.dither_bayer(lib, 8) == UNSUPPORTED
    assert lib.xgpu_dither_bayer(3, None) == INVALID


@pytest.mark.parametrize("log2n", (4, 5, 6))
def test_blue_is_the_reference_and_blue(log2n):
    lib = abi.load()
    n = 1 << log2n
    for seed in (1, 2):
        m = abi.dither_blue(lib, log2n, seed)
        assert np.array_equal(m, dr.blue(log2n, seed)), (log2n, seed)
        assert np.array_equal(np.sort(m.ravel()), np.arange(n * n)), (log2n, seed)
        rnd = np.random.default_rng(1000 * log2n + seed).permutation(n * n).reshape(n, n)
        share, share_rnd = dr.low_frequency_share(m), dr.low_frequency_share(rnd)
        print(f"n {n} seed {seed}: low-frequency share {share:.3g}, random permutation {share_rnd:.3g}")
        assert share < share_rnd / 10, (log2n, seed, share, share_rnd)
    assert not np.array_equal(abi.dither_blue(lib, log2n, 1), abi.dither_blue(lib, log2n, 2))


def test_blue_refusals():
    lib = abi.load()
    assert abi.dither_blue(lib, 1) == UNSUPPORTED and abi.dither_blue(lib, 8) == UNSUPPORTED
    assert lib.xgpu_dither_blue(4, 1, None) == INVALID
    m = abi.dither_blue(lib, 2, 7)
    assert np.array_equal(np.sort(m.ravel()), np.arange(16)) and np.array_equal(m, dr.blue(2, 7))      # the Gaussian wraps several times round a 4 x 4 torus


def test_phase_is_the_reference():
    lib = abi.load()
    for mw, mh in ((1, 1), (4, 2), (16, 4), (8, 8), (2, 128), (128, 64)):
        for index in list(range(1001)) + [0x7FFFFFFF, 0xFFFFFFFF]:
            px, py = abi.dither_phase(lib, index, mw, mh)
            assert (px, py) == dr.phase(index, mw, mh), (index, mw, mh)
            assert 0 <= px < mw and 0 <= py < mh
    assert abi.dither_phase(lib, 1, 3, 4) == INVALID and abi.dither_phase(lib, 1, 4, 256) == INVALID
    assert len({abi.dither_phase(lib, i, 64, 64) for i in range(64)}) > 48      # the pictures of a second do not share a phase


def _planes(bd, w, h, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, (h, w)), rng.integers(0, 1 << bd, (h // 2, w // 2)), rng.integers(0, 1 << bd, (h // 2, w // 2))]


def test_threshold_one_half_is_the_plain_rule():
    """through the reference alone: the 1 x 1 matrix with k = 1 and rank 1 gives the plain references' integers"""
    half = np.array([[1]])
    for bd in (8, 10, 12):
        pl = _planes(bd, 24, 16, bd)
        for dt in (cr.U8, cr.U16):
            for kw in (dict(), dict(matrix=9, full_range=True, chroma_loc=1), dict(mode="nearest", crop=(2, 4, 0, 2))):
                assert np.array_equal(dr.rgb(pl, bd, half, 1, dtype=dt, **kw), cr.convert(pl, bd, dtype=dt, **kw))
        assert np.array_equal(dr.rgb10a2(pl, bd, half, 1, bgr=True, alpha=0.4), pr.rgb10a2(pl, bd, bgr=True, alpha=0.4))
        assert np.array_equal(dr.nv12(pl, bd, 8, half, 1), yr.nv12(pl, bd, 8))
        for d in (8, 10, 12):
            assert np.array_equal(dr.p016(pl, bd, d, half, 1), yr.p016(pl, bd, d)), (bd, d)
        if bd > 10:
            assert np.array_equal(dr.nv12(pl, bd, 10, half, 1), yr.nv12(pl, bd, 10))


def test_flat_mean_is_kept():
    """a flat 10-bit plane 4 c + j through Bayer 8 to 8 bit: in every aligned 8 x 8 block 4 * sum(out) == sum(in)"""
    m = dr.bayer(3)
    for v in (0, 1, 2, 3, 64, 65, 66, 67, 509, 510, 511, 1016, 1017, 1018, 1019):
        pl = [np.full((32, 48), v), np.full((16, 24), v), np.full((16, 24), v)]
        out = dr.nv12(pl, 10, 8, m, 6).astype(np.int64)
        luma = out[:32].reshape(4, 8, 6, 8).sum(axis=(1, 3))
        assert np.all(4 * luma == 64 * v), v
        for c in (0, 1):
            chroma = out[32:, c::2].reshape(2, 8, 3, 8).sum(axis=(1, 3))
            assert np.all(4 * chroma == 64 * v), (v, c)
