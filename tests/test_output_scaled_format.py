"""CPU suite for the scaled device output: xgpu_scale_taps against the fractions.Fraction restatement (tests/scale_ref.py),
the invariants of a tap row, the integer contract against torch's antialiased bilinear resize in float64, the destination sizes and the refusals.
No GPU: the functions tested are the host-only ones."""
import ctypes as C
from fractions import Fraction
import itertools

import numpy as np
import pytest

import scale_ref as sr
from xevd_amd import abi

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -101, -104
# destination samples per source LUMA sample
RATIOS = (Fraction(1, 64), Fraction(1, 34), Fraction(10, 37), Fraction(1, 2), Fraction(1), Fraction(3, 2), Fraction(8))
PLANES = (16, 270, 1080, 4320)


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def test_error_codes_are_the_headers():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xevd_hip.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(XGPU_ERR_\w+)\s+\(?(-?\d+)\)?", src)}
    assert vals["XGPU_ERR_INVALID_ARGUMENT"] == ERR_INVALID_ARGUMENT and vals["XGPU_ERR_UNSUPPORTED"] == ERR_UNSUPPORTED
    assert (abi.SCALE_BILINEAR, abi.SCALE_AREA) == (0, 1) == (sr.BILINEAR, sr.AREA)


def _checked_outputs(N):
    """every destination sample of a short axis; of a long one both ends and every 37th"""
    if N <= 2048:
        return list(range(N))
    return sorted(set(range(48)) | set(range(N - 48, N)) | set(range(0, N, 37)))


@pytest.mark.parametrize("n", PLANES)
def test_taps_equal_the_fraction_restatement(lib, n):
    done = 0
    for ratio, filt, s, half in itertools.product(RATIOS, (sr.BILINEAR, sr.AREA), (1, 2), (0, 1, 2)):
        N = n * s * ratio
        N = int(N) if N.denominator == 1 else int(N) + 1      # rounded up: never below the 1 / 64 limit
        got = abi.scale_taps(lib, n, s, half, N, filt)
        if N < 2 or N > 16384:
            assert got == ERR_UNSUPPORTED, (n, s, half, N, filt)
            continue
        first, count, w = got
        outs = _checked_outputs(N)
        exp = sr.taps(n, s, half, N, filt, outs)
        for o, (e_first, e_q) in zip(outs, exp):
            assert (int(first[o]), int(count[o])) == (e_first, len(e_q)), (n, s, half, N, filt, o)
            assert [int(v) for v in w[o, :count[o]]] == e_q, (n, s, half, N, filt, o)
            assert not w[o, count[o]:].any()
        done += 1
    assert done >= 50


@pytest.mark.parametrize("n", PLANES)
def test_tap_invariants(lib, n):
    for ratio, filt, s, half in itertools.product(RATIOS, (sr.BILINEAR, sr.AREA), (1, 2), (0, 1, 2)):
        N = -(-n * s * ratio.numerator // ratio.denominator)
        if N < 2 or N > 16384:
            continue
        first, count, w = abi.scale_taps(lib, n, s, half, N, filt)
        what = (n, s, half, N, filt)
        assert (w.astype(np.int64).sum(1) == 16384).all(), what
        assert (w >= 0).all(), what
        assert (count >= 1).all() and (first >= 0).all() and (first + count <= n).all(), what
        assert w.shape[1] == count.max() and w.shape[1] <= 132, what      # n_src / 64 <= n_dst bounds a row at about 130 entries
        # contiguous: a row is samples first .. first + count - 1, no gaps to encode; and rows move right with the destination sample
        assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all(), what
        # the weights of one row are exactly those of its count[o] entries: what lies behind them is zero
        assert not (w * (np.arange(w.shape[1])[None, :] >= count[:, None])).any(), what


@pytest.mark.parametrize("n", PLANES)
@pytest.mark.parametrize("filt", (sr.BILINEAR, sr.AREA))
def test_same_size_luma_is_the_identity(lib, n, filt):
    first, count, w = abi.scale_taps(lib, n, 1, 0, n, filt)
    assert w.shape == (n, 1) and (w == 16384).all() and (count == 1).all() and (first == np.arange(n)).all()


def test_same_size_chroma_taps_are_the_quarter_weights_of_the_unscaled_output(lib):
    """the LINEAR upsampling of section 8a is the triangle at ratio 1 / 2: weights in quarters, by siting"""
    n = 20
    for half, even, odd in ((0, {0: 4}, {0: 2, 1: 2}), (1, {-1: 1, 0: 3}, {0: 3, 1: 1}), (2, {-1: 2, 0: 2}, {0: 4})):
        first, count, w = abi.scale_taps(lib, n, 2, half, 2 * n, sr.BILINEAR)
        for o in range(2, 2 * n - 2):
            exp = even if o % 2 == 0 else odd
            got = {int(first[o]) + k - o // 2: int(w[o, k]) for k in range(count[o])}
            assert got == {d: q * 4096 for d, q in exp.items()}, (half, o)
        # at the ends the sample outside the plane is dropped and the row renormalised: the edge sample alone - the clamp of the unscaled output
        assert (first[0], count[0], w[0, 0]) == (0, 1, 16384) and (first[-1], count[-1], w[-1, 0]) == (n - 1, 1, 16384)


def test_invalid_tap_arguments(lib):
    f, c = (C.c_int32 * 64)(), (C.c_int32 * 64)()
    w = (C.c_int16 * 64)()
    assert lib.xgpu_scale_taps(0, 1, 0, 16, 0, f, c, None, 0) == ERR_INVALID_ARGUMENT
    assert lib.xgpu_scale_taps(16, 3, 0, 16, 0, f, c, None, 0) == ERR_INVALID_ARGUMENT
    assert lib.xgpu_scale_taps(16, 1, 3, 16, 0, f, c, None, 0) == ERR_INVALID_ARGUMENT
    assert lib.xgpu_scale_taps(16, 1, 0, 16, 2, f, c, None, 0) == ERR_INVALID_ARGUMENT
    assert lib.xgpu_scale_taps(16, 1, 0, 16, 0, None, c, None, 0) == ERR_INVALID_ARGUMENT
    assert lib.xgpu_scale_taps(64, 1, 0, 16, 0, f, c, w, 2) == ERR_INVALID_ARGUMENT      # rows of 8 and more do not fit a stride of 2
    assert lib.xgpu_scale_taps(16, 1, 0, 1, 0, f, c, None, 0) == ERR_UNSUPPORTED
    assert lib.xgpu_scale_taps(130, 1, 0, 2, 0, f, c, None, 0) == ERR_UNSUPPORTED          # below 1 / 64
    assert lib.xgpu_scale_taps(4, 1, 0, 33, 0, f, c, None, 0) == ERR_UNSUPPORTED           # above 8
    assert lib.xgpu_scale_taps(128, 1, 0, 2, 0, f, c, None, 0) > 0 and lib.xgpu_scale_taps(4, 1, 0, 32, 0, f, c, None, 0) > 0


# ---------------------------------------------------------------------------------------------------------------- accuracy
# The yardstick is torch's own antialiased bilinear resize in float64; the integer contract (14-bit taps, two roundings) must stay within one code value of
# it.  Two roundings of at most half a code value each (the first one of 1 / 16: three fraction bits), plus the quantisation of up to ~130 weights of which
# each is off by at most 2^-15 of full scale: 1.0 is a condition on the contract, not a fit to its output.  Measured maxima on these seeded planes: 0.54, 0.71, 0.56, 0.64.
@pytest.mark.parametrize("ws, hs, wd, hd, bd", [(1920, 1080, 224, 224, 10), (960, 544, 958, 540, 12), (480, 270, 700, 400, 8), (3840, 2160, 64, 64, 12)])
def test_restatement_is_within_one_code_value_of_torch(ws, hs, wd, hd, bd):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(ws * 31 + wd)
    plane = rng.integers(0, 1 << bd, (hs, ws), dtype=np.int64)
    got = sr.resize_plane(plane, sr.taps(hs, 1, 0, hd, sr.BILINEAR), sr.taps(ws, 1, 0, wd, sr.BILINEAR))
    ref = torch.nn.functional.interpolate(torch.from_numpy(plane.astype(np.float64))[None, None], size=(hd, wd), mode="bilinear", antialias=True,
                                          align_corners=False)[0, 0].numpy()
    err = np.abs(got - ref).max()
    print(f"{ws}x{hs} -> {wd}x{hd} at {bd} bit: max |integer contract - torch float64| = {err:.3f} code values")
    assert got.min() >= 0 and got.max() <= (1 << bd) - 1
    assert err <= 1.0


def test_rails_stay_on_the_rails():
    """a plane of 0 stays 0 and a plane of 2^B - 1 stays 2^B - 1 through both passes, for either filter: the rows sum to 16384 exactly"""
    for bd, filt in itertools.product((8, 10, 12), (sr.BILINEAR, sr.AREA)):
        ty, tx = sr.taps(54, 1, 0, 20, filt), sr.taps(96, 1, 0, 131, filt)
        for v in (0, (1 << bd) - 1):
            assert (sr.resize_plane(np.full((54, 96), v, np.int64), ty, tx) == v).all(), (bd, filt, v)


# ---------------------------------------------------------------------------------------------------------------- sizes and refusals
def _size(lib, fmt, sc, w=1920, h=1080, bd=10):
    return lib.xgpu_output_scaled_size(C.byref(fmt), C.byref(sc), w, h, bd), lib.xgpu_output_scaled_check(C.byref(fmt), C.byref(sc), w, h, bd)


def test_destination_sizes(lib):
    sc = abi.make_scale_params(224, 200)
    for layout, dtype, es in itertools.product((abi.OUT_RGB_PLANAR, abi.OUT_RGB_INTERLEAVED, abi.OUT_YUV444_PLANAR, abi.OUT_YUV444_INTERLEAVED),
                                               (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32), (None,)):
        es = {abi.OUT_U8: 1, abi.OUT_F32: 4}.get(dtype, 2)
        planar = layout in (abi.OUT_RGB_PLANAR, abi.OUT_YUV444_PLANAR)
        assert _size(lib, abi.make_output_format(layout, dtype), sc) == (3 * 224 * 200 * es, 0)
        row = (224 if planar else 3 * 224) * es
        pitch = row + 64
        rows = 3 * 200 if planar else 200
        assert _size(lib, abi.make_output_format(layout, dtype, row_pitch=pitch), sc) == ((rows - 1) * pitch + row, 0)
        assert _size(lib, abi.make_output_format(layout, dtype, row_pitch=row - es), sc) == (0, ERR_INVALID_ARGUMENT)
    # the crop is the region of interest: it changes the source, not the destination
    assert _size(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, crop=(200, 100, 40, 60)), sc) == (3 * 224 * 200 * 4, 0)
    # normalise with a float dtype
    assert _size(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F16), abi.make_scale_params(224, 224, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))) == (3 * 224 * 224 * 2, 0)


def test_refusals(lib):
    ok = abi.make_scale_params(224, 224)
    rgb = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32)
    assert _size(lib, rgb, ok)[1] == 0
    # a layout outside the four
    for layout, dtype, obd in ((abi.OUT_YUV420P, abi.OUT_U16, 0), (abi.OUT_NV12, abi.OUT_U16, 0), (abi.OUT_P016, abi.OUT_U16, 0)):
        assert _size(lib, abi.make_output_format(layout, dtype, out_bit_depth=obd), ok) == (0, ERR_INVALID_ARGUMENT)
    assert _size(lib, abi.make_output_format(7, abi.OUT_U8), ok) == (0, ERR_INVALID_ARGUMENT)
    # a ratio past the limits, a size outside 2 .. 16384
    for w, h in ((29, 224), (224, 16), (15361, 224), (224, 8641), (1, 224), (224, 16385)):
        assert _size(lib, rgb, abi.make_scale_params(w, h)) == (0, ERR_UNSUPPORTED), (w, h)
    assert _size(lib, rgb, abi.make_scale_params(30, 17))[1] == 0 and _size(lib, rgb, abi.make_scale_params(15360, 8640))[1] == 0
    assert _size(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, crop=(0, 1856, 0, 0)), abi.make_scale_params(513, 224)) == (0, ERR_UNSUPPORTED)      # 64 columns left
    # normalise with an integer dtype
    norm = abi.make_scale_params(224, 224, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25))
    for dtype in (abi.OUT_U8, abi.OUT_U16):
        assert _size(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, dtype), norm) == (0, ERR_INVALID_ARGUMENT)
    # a NaN mean, an infinite inv_std (std = 0)
    assert _size(lib, rgb, abi.make_scale_params(224, 224, mean=(0.5, float("nan"), 0.5))) == (0, ERR_INVALID_ARGUMENT)
    assert _size(lib, rgb, abi.make_scale_params(224, 224, inv_std=(1.0, 1.0, float("inf")))) == (0, ERR_INVALID_ARGUMENT)
    # odd crops, a crop that leaves nothing
    for crop in ((1, 0, 0, 0), (0, 0, 0, 3), (0, -2, 0, 0), (960, 960, 0, 0)):
        assert _size(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, crop=crop), ok) == (0, ERR_INVALID_ARGUMENT), crop
    # an unknown filter, normalize outside 0 / 1, an unsupported matrix (the unscaled path's code), NULL
    assert _size(lib, rgb, abi.make_scale_params(224, 224, filter=2)) == (0, ERR_INVALID_ARGUMENT)
    bad = abi.make_scale_params(224, 224)
    bad.normalize = 2
    assert _size(lib, rgb, bad) == (0, ERR_INVALID_ARGUMENT)
    assert _size(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, matrix=2), ok) == (0, ERR_UNSUPPORTED)
    assert lib.xgpu_output_scaled_size(None, C.byref(ok), 1920, 1080, 10) == 0 and lib.xgpu_output_scaled_size(C.byref(rgb), None, 1920, 1080, 10) == 0


def test_make_scale_params_inverts_std_in_float32():
    p = abi.make_scale_params(10, 10, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    assert p.normalize == 1
    for k, (m, s) in enumerate(zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
        assert np.float32(p.mean[k]) == np.float32(m) and np.float32(p.inv_std[k]) == np.float32(1) / np.float32(s)
    assert abi.make_scale_params(10, 10).normalize == 0
