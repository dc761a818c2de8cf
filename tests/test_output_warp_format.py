"""CPU suite for the warped regions of interest (xgpu_warp_from_matrix, xgpu_warp_from_rotated_box, xgpu_output_warp_check, xgpu_output_warp_size;
INTEGRATION.md section 8j): every refusal with its code and the map it names, the size formula, the two host helpers against their restatement
(tests/warp_ref.py), and the restatement itself anchored to the unscaled contract - all without a device."""
import numpy as np
import pytest

import colour_ref as cr
import warp_ref as wr
from xevd_amd import abi

INVALID, UNSUPPORTED = -101, -104
W, H = 320, 200
SIZE = (48, 64)


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def check(lib, maps=(wr.IDENTITY,), n=None, size=SIZE, bd=10, fmt=None, wp=None, sc=None, device=False):
    """(code, bad_index) of one call's arguments; device: maps in device memory (the host is given none)"""
    fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8) if fmt is None else fmt
    sc = abi.make_scale_params(size[1], size[0]) if sc is None else sc
    wp = abi.make_warp_params() if wp is None else wp
    n = len(maps) if n is None else n
    rc, bad = abi.output_warp_check(lib, fmt, sc, wp, None if device else abi.make_warp_maps(maps), n, W, H, bd)
    if not device or rc == 0:      # the size does not look at the maps
        size_ok = abi.output_warp_size(lib, fmt, sc, wp, n, W, H, bd) != 0
        assert size_ok == (rc == 0 or bad >= 0), (rc, bad)
    return rc, bad


def test_every_refusal_with_its_code_and_map(lib):
    assert check(lib) == (0, -1)
    assert check(lib, device=True) == (0, -1)
    for s in (1, 2, 4):
        assert check(lib, wp=abi.make_warp_params(samples=s)) == (0, -1)
    for s in (0, 3, 8, -1):
        assert check(lib, wp=abi.make_warp_params(samples=s)) == (INVALID, -1), s
    assert check(lib, wp=abi.make_warp_params(border=abi.WARP_PAD)) == (0, -1)
    assert check(lib, wp=abi.make_warp_params(border=2)) == (INVALID, -1)
    assert check(lib, wp=abi.make_warp_params(border=-1)) == (INVALID, -1)
    assert check(lib, sc=abi.make_scale_params(64, 48, filter=abi.SCALE_AREA)) == (INVALID, -1)      # filter 1
    assert check(lib, sc=abi.make_scale_params(64, 48, filter=2)) == (INVALID, -1)
    assert check(lib, fmt=abi.make_output_format(abi.OUT_YUV420P, abi.OUT_U16, out_bit_depth=10)) == (INVALID, -1)
    assert check(lib, fmt=abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)) == (INVALID, -1)
    for layout in (abi.OUT_RGB_PLANAR, abi.OUT_RGB_INTERLEAVED, abi.OUT_YUV444_PLANAR, abi.OUT_YUV444_INTERLEAVED):
        assert check(lib, fmt=abi.make_output_format(layout, abi.OUT_F16)) == (0, -1)
    # a coefficient at each limit passes, one past it is refused and named
    for k in range(6):
        lim = wr.OFF_LIMIT if k in (2, 5) else wr.LIN_LIMIT
        for sign in (1, -1):
            at, past = list(wr.IDENTITY), list(wr.IDENTITY)
            at[k], past[k] = sign * lim, sign * (lim + 1)
            assert check(lib, [wr.IDENTITY, tuple(at), wr.IDENTITY]) == (0, -1), (k, sign)
            assert check(lib, [wr.IDENTITY, wr.IDENTITY, tuple(past)]) == (INVALID, 2), (k, sign)
            assert check(lib, [tuple(past), tuple(past)]) == (INVALID, 0), (k, sign)
    extreme = (-(1 << 63), (1 << 63) - 1, 0, 0, 0, 0)
    assert check(lib, [wr.IDENTITY, extreme]) == (INVALID, 1)
    # n
    assert check(lib, n=0) == (INVALID, -1)
    assert check(lib, [wr.IDENTITY] * (abi.MAX_ROIS + 1)) == (INVALID, -1)
    assert check(lib, [wr.IDENTITY] * abi.MAX_ROIS) == (0, -1)
    assert check(lib, n=0, device=True) == (INVALID, -1) and check(lib, n=abi.MAX_ROIS + 1, device=True) == (INVALID, -1)
    # sizes
    for size in ((1, 64), (48, 1), (16385, 64), (48, 16385)):
        assert check(lib, size=size) == (UNSUPPORTED, -1), size
    assert check(lib, size=(2, 2)) == (0, -1) and check(lib, size=(16384, 16384)) == (0, -1)
    # the normalise into integers
    assert check(lib, sc=abi.make_scale_params(64, 48, mean=(0.5, 0.5, 0.5))) == (INVALID, -1)
    assert check(lib, fmt=abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32), sc=abi.make_scale_params(64, 48, mean=(0.5, 0.5, 0.5))) == (0, -1)
    # a bad pad only where it is read: with XGPU_WARP_PAD, or with maps in device memory
    for pad in (256, 0.5, -1, float("nan")):
        assert check(lib, wp=abi.make_warp_params(pad=pad)) == (0, -1), pad
        assert check(lib, wp=abi.make_warp_params(border=abi.WARP_PAD, pad=pad)) == (INVALID, -1), pad
        assert check(lib, wp=abi.make_warp_params(pad=pad), device=True) == (INVALID, -1), pad
    assert check(lib, wp=abi.make_warp_params(border=abi.WARP_PAD, pad=(0, 255, 17))) == (0, -1)
    assert check(lib, wp=abi.make_warp_params(border=abi.WARP_PAD, pad=1023), fmt=abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16)) == (0, -1)
    assert check(lib, wp=abi.make_warp_params(border=abi.WARP_PAD, pad=1024), fmt=abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16)) == (INVALID, -1)
    f32 = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32)
    assert check(lib, wp=abi.make_warp_params(border=abi.WARP_PAD, pad=-3.25), fmt=f32) == (0, -1)
    assert check(lib, wp=abi.make_warp_params(border=abi.WARP_PAD, pad=float("inf")), fmt=f32) == (INVALID, -1)
    # image_pitch: a multiple of the element, not below one image
    image = 3 * 48 * 64 * 4
    assert check(lib, fmt=f32, wp=abi.make_warp_params(image_pitch=image)) == (0, -1)
    assert check(lib, fmt=f32, wp=abi.make_warp_params(image_pitch=image - 4)) == (INVALID, -1)
    assert check(lib, fmt=f32, wp=abi.make_warp_params(image_pitch=image + 2)) == (INVALID, -1)
    # NULLs
    assert lib.xgpu_output_warp_check(None, None, None, None, 1, W, H, 10, None) == INVALID
    assert lib.xgpu_output_warp_size(None, None, None, 1, W, H, 10) == 0


def test_size_formula(lib):
    for layout, dtype, es in ((abi.OUT_RGB_PLANAR, abi.OUT_U8, 1), (abi.OUT_RGB_INTERLEAVED, abi.OUT_F16, 2), (abi.OUT_YUV444_PLANAR, abi.OUT_F32, 4),
                              (abi.OUT_YUV444_INTERLEAVED, abi.OUT_U16, 2)):
        fmt, sc = abi.make_output_format(layout, dtype), abi.make_scale_params(SIZE[1], SIZE[0])
        image = 3 * 48 * 64 * es
        for n in (1, 3, abi.MAX_ROIS):
            assert abi.output_warp_size(lib, fmt, sc, abi.make_warp_params(), n, W, H, 10) == n * image
            pitch = image + 4 * es
            assert abi.output_warp_size(lib, fmt, sc, abi.make_warp_params(image_pitch=pitch), n, W, H, 10) == (n - 1) * pitch + image
        # padded rows: the tight batch stride is whole rows, one image ends with its last element
        interleaved = layout in (abi.OUT_RGB_INTERLEAVED, abi.OUT_YUV444_INTERLEAVED)
        row, rows = (3 if interleaved else 1) * 64 * es, 48 if interleaved else 3 * 48
        fmt.row_pitch = row + 32
        one = (rows - 1) * (row + 32) + row
        assert abi.output_warp_size(lib, fmt, sc, abi.make_warp_params(), 3, W, H, 10) == 2 * rows * (row + 32) + one
        assert abi.output_warp_size(lib, fmt, sc, abi.make_warp_params(image_pitch=one), 3, W, H, 10) == 3 * one
        # one image is the scaled output's
        assert abi.output_warp_size(lib, fmt, sc, abi.make_warp_params(), 1, W, H, 10) == lib.xgpu_output_scaled_size(fmt, sc, W, H, 10)


def test_from_matrix_equals_the_restatement(lib):
    rng = np.random.default_rng(77)
    thetas = [(1, 0, 0, 0, 1, 0), (-1, 0, 320, 0, -1, 200), (0, 1, 0, -1, 0, 320), (0, 0, 0, 0, 0, 0)]
    # ties: multiples of 2^-17 round half away from zero, on either side of zero
    thetas += [(k / 131072.0, -k / 131072.0, k / 131072.0, -k / 131072.0, k / 131072.0, 0.5 - k / 131072.0) for k in (1, 3, 5, 65537, -1, -3, -65535)]
    thetas += [(0.5 / 65536, 1.5 / 65536, 2.5 / 65536, -0.5 / 65536, -1.5 / 65536, -2.5 / 65536)]
    # the limits, exactly at and just past
    thetas += [(64, -64, 0, 64, -64, 0), (64.00001, 0, 0, 0, 1, 0), (1, 0, 0, 0, -64.00002, 0), (1, 0, float(1 << 20), 0, 1, -float(1 << 20)),
               (1, 0, float(1 << 20) + 1, 0, 1, 0), (1, 0, 0, 0, 1, -float(1 << 20) - 1), (1e300, 0, 0, 0, 1, 0), (1, 0, -1e300, 0, 1, 0)]
    thetas += [(float("nan"), 0, 0, 0, 1, 0), (1, 0, float("inf"), 0, 1, 0), (1, 0, 0, 0, 1, float("-inf"))]
    for _ in range(4000):
        lin = rng.uniform(-66, 66, 4) if rng.integers(8) == 0 else rng.normal(0, 3, 4)
        off = rng.uniform(-9000, 9000, 2)
        thetas.append((lin[0], lin[1], off[0], lin[2], lin[3], off[1]))
    refused = 0
    for t in thetas:
        got, exp = abi.warp_from_matrix(lib, t), wr.from_matrix(t)
        if exp is None:
            assert got == INVALID, t
            refused += 1
        else:
            assert got == exp, t
    assert 8 <= refused < len(thetas) // 2
    assert abi.warp_from_matrix(lib, (1, 0, 0, 0, 1, 0)) == wr.IDENTITY      # the centre of destination pixel 0 is the centre of sample 0
    assert abi.warp_from_matrix(lib, (0.5 / 65536, 0, 0, 0, -0.5 / 65536, 0))[0::4] == (1, -1)
    assert lib.xgpu_warp_from_matrix(None, None) == INVALID


def test_from_rotated_box_within_one_step_of_the_restatement(lib):
    """libm's sine and cosine may differ in the last ulp between two builds: at coordinates below 2^14 - values below 2^30 once scaled by 65536, with 53 bits
    kept - that moves the value before its rounding by about 2^-23, so an entry can differ only where that value lies next to a rounding boundary, and then by
    one step"""
    rng = np.random.default_rng(78)
    boxes = [(160, 100, 320, 200, 0, (200, 320)), (160, 100, 320, 200, 90, (320, 200)), (100, 50, 64, 32, 30, (32, 64)), (0, 0, 2, 2, -45, (224, 224)),
             (8000, 4000, 300, 100, 180, (48, 160)), (50.5, 60.25, 10, 400, 270, (7, 3))]
    for _ in range(3000):
        boxes.append((rng.uniform(-100, 8000), rng.uniform(-100, 4400), rng.uniform(1, 2000), rng.uniform(1, 2000), rng.uniform(-720, 720),
                      (int(rng.integers(2, 600)), int(rng.integers(2, 600)))))
    seen = 0
    for cx, cy, w, h, ang, size in boxes:
        got, exp = abi.warp_from_rotated_box(lib, cx, cy, w, h, ang, size), wr.from_rotated_box(cx, cy, w, h, ang, size)
        if exp is None or not isinstance(got, tuple):      # at a limit the two may fall on either side: both must be within a step of it
            continue
        seen += 1
        assert max(abs(a - b) for a, b in zip(got, exp)) <= 1, (cx, cy, w, h, ang, size, got, exp)
    assert seen > 2500
    assert abi.warp_from_rotated_box(lib, 160, 100, 320, 200, 0, (200, 320)) == wr.IDENTITY      # the whole picture, upright, at its own size
    # a 180 degree turn of the whole picture: the flip of both axes, to within the sine's last bit times the size
    m = abi.warp_from_rotated_box(lib, 160, 100, 320, 200, 180, (200, 320))
    assert all(abs(a - b) <= 1 for a, b in zip(m, (-65536, 0, 319 << 16, 0, -65536, 199 << 16)))
    assert abi.warp_from_rotated_box(lib, float("nan"), 0, 1, 1, 0, (8, 8)) == INVALID
    assert abi.warp_from_rotated_box(lib, 0, 0, 1, 1, 0, (0, 8)) == INVALID
    assert abi.warp_from_rotated_box(lib, 0, 0, 1e9, 1, 0, (8, 8)) == INVALID


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_identity_is_the_plain_output_with_linear_upsampling(bd):
    """the restatement without a GPU: the identity map at S = 1 gives Y = the luma and Cb, Cr = colour_ref.upsample(..., "linear", loc) for every
    ChromaSampleLocType - (4096 q + 2^15) >> 16 = (q + 8) >> 4 for the sixteenth weights q"""
    rng = np.random.default_rng(900 + bd)
    w, h = 64, 48
    planes = [rng.integers(0, 1 << bd, s, dtype=np.int64) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    for loc in range(6):
        (y, cb, crr), outside = wr.warped_ycbcr(planes, bd, (h, w), wr.IDENTITY, 1, loc)
        assert np.array_equal(y, planes[0])
        assert np.array_equal(cb, cr.upsample(planes[1], w, h, "linear", loc)), loc
        assert np.array_equal(crr, cr.upsample(planes[2], w, h, "linear", loc)), loc
        assert not outside.any()
        for dtype in (cr.U8, cr.U16, cr.F32):
            assert np.array_equal(wr.batch(planes, bd, (h, w), [wr.IDENTITY], chroma_loc=loc, dtype=dtype)[0], cr.convert(planes, bd, chroma_loc=loc, dtype=dtype))
    # an integer shift moves the samples as they are
    shift = (65536, 0, 3 << 16, 0, 65536, 2 << 16)
    (y1, _, _), _ = wr.warped_ycbcr(planes, bd, (h - 2, w - 3), shift, 1)
    assert np.array_equal(y1, planes[0][2:, 3:])
    # border: one column left of the picture and one row below it are outside, nothing else
    _, outside = wr.warped_ycbcr(planes, bd, (h + 1, w + 1), (65536, 0, -65536, 0, 65536, 0), 1)
    exp = np.zeros((h + 1, w + 1), bool)
    exp[:, 0] = True
    exp[h, :] = True
    assert np.array_equal(outside, exp)
