"""CPU suite for the remapped output (xgpu_remap_grid_dims, xgpu_remap_grid_size, xgpu_output_remap_check, xgpu_output_remap_size, xgpu_remap_from_warp,
_from_homography, _from_lens): the struct, the grid's dimensions, every refusal that needs no device with its code, the size
formulas, the three host helpers against their restatement (tests/remap_ref.py) bit for bit, and the restatement itself anchored to warp_ref (an affine grid) and
to torch's grid_sample in float64 - all without a device.  (A short grid_size or dst_size is refused by the device call, which compares them with the sizes
checked here; tests/test_gpu_output_remap.py makes those calls.)"""
import ctypes as C

import numpy as np
import pytest

import remap_ref as mr
import warp_ref as wr
from xevd_amd import abi

INVALID, UNSUPPORTED = -101, -104
W, H = 320, 200
SIZE = (48, 64)
Q = 65536


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def check(lib, n=1, size=SIZE, bd=10, fmt=None, rp=None, sc=None):
    """the code of one call's arguments; the size function agrees with it"""
    fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8) if fmt is None else fmt
    sc = abi.make_scale_params(size[1], size[0]) if sc is None else sc
    rp = abi.make_remap_params() if rp is None else rp
    rc = abi.output_remap_check(lib, fmt, sc, rp, n, W, H, bd)
    assert (abi.output_remap_size(lib, fmt, sc, rp, n, W, H, bd) != 0) == (rc == 0), rc
    return rc


def test_struct_layout():
    assert C.sizeof(abi.RemapParams) == 48
    offs = {k: getattr(abi.RemapParams, k).offset for k, _ in abi.RemapParams._fields_}
    assert offs == {"grid_format": 0, "step_log2": 4, "samples": 8, "border": 12, "pad": 16, "grid_pitch": 32, "image_pitch": 40}
    assert C.sizeof(abi.RemapLens) == 13 * 8
    assert (abi.GRID_Q16_I32, abi.GRID_F32, abi.GRID_INVALID) == (0, 1, -(1 << 31))


def test_grid_dims(lib):
    exp = {(2, 0): 2, (2, 1): 2, (2, 4): 2, (2, 6): 2, (64, 0): 64, (64, 1): 33, (64, 4): 5, (64, 6): 2, (65, 0): 65, (65, 1): 34, (65, 4): 6, (65, 6): 3,
           (129, 0): 129, (129, 1): 66, (129, 4): 10, (129, 6): 4}
    for (d, k), g in exp.items():
        assert abi.remap_grid_dims(lib, (d, 2), k) == (g, 2), (d, k)
        assert abi.remap_grid_dims(lib, (2, d), k)[1] == g, (d, k)
        assert mr.grid_dims((d, d), k) == (g, g)
        # the last pixel's cell ends at the last node
        if k:
            assert ((d - 1) >> k) + 1 == g - 1
    for k in (-1, 7):
        assert abi.remap_grid_dims(lib, SIZE, k) == INVALID
    assert abi.remap_grid_dims(lib, (0, 8), 0) == INVALID
    assert lib.xgpu_remap_grid_dims(64, 48, 4, None, None) == 0


def test_every_refusal_with_its_code(lib):
    assert check(lib) == 0
    for k in range(7):
        assert check(lib, rp=abi.make_remap_params(step_log2=k)) == 0, k
    for k in (-1, 7, 64):
        assert check(lib, rp=abi.make_remap_params(step_log2=k)) == INVALID, k
    assert check(lib, rp=abi.make_remap_params(abi.GRID_F32)) == 0
    for fm in (-1, 2):
        assert check(lib, rp=abi.make_remap_params(fm)) == INVALID, fm
    assert check(lib, rp=abi.make_remap_params(border=abi.WARP_PAD)) == 0
    for b in (-1, 2):
        assert check(lib, rp=abi.make_remap_params(border=b)) == INVALID, b
    for s in (1, 2, 4):
        assert check(lib, rp=abi.make_remap_params(samples=s)) == 0
    for s in (0, 3, 8, -1):
        assert check(lib, rp=abi.make_remap_params(samples=s)) == INVALID, s
    assert check(lib, n=0) == INVALID and check(lib, n=1025) == INVALID and check(lib, n=abi.MAX_ROIS + 1) == INVALID
    assert check(lib, n=abi.MAX_ROIS) == 0
    # grid_pitch: 0, or a multiple of 8 not below one grid
    for k, one in ((0, 48 * 64 * 8), (4, 4 * 5 * 8)):
        assert mr.grid_dims(SIZE, k) == ((48, 64) if k == 0 else (4, 5))
        assert check(lib, n=3, rp=abi.make_remap_params(step_log2=k, grid_pitch=one)) == 0
        assert check(lib, n=3, rp=abi.make_remap_params(step_log2=k, grid_pitch=one + 8)) == 0
        assert check(lib, n=3, rp=abi.make_remap_params(step_log2=k, grid_pitch=one + 4)) == INVALID
        assert check(lib, n=3, rp=abi.make_remap_params(step_log2=k, grid_pitch=one - 8)) == INVALID
        assert check(lib, n=3, rp=abi.make_remap_params(step_log2=k, grid_pitch=8)) == INVALID
    # filter, layout
    assert check(lib, sc=abi.make_scale_params(64, 48, filter=abi.SCALE_AREA)) == INVALID
    assert check(lib, sc=abi.make_scale_params(64, 48, filter=2)) == INVALID
    assert check(lib, fmt=abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)) == INVALID
    assert check(lib, fmt=abi.make_output_format(abi.OUT_YUV420P, abi.OUT_U16, out_bit_depth=10)) == INVALID
    for layout in (abi.OUT_RGB_PLANAR, abi.OUT_RGB_INTERLEAVED, abi.OUT_YUV444_PLANAR, abi.OUT_YUV444_INTERLEAVED):
        assert check(lib, fmt=abi.make_output_format(layout, abi.OUT_F16)) == 0
    # the pad is always read: either grid format can carry invalid nodes
    for pad in (256, 0.5, -1, float("nan")):
        for fm in (abi.GRID_Q16_I32, abi.GRID_F32):
            for b in (abi.WARP_CLAMP, abi.WARP_PAD):
                assert check(lib, rp=abi.make_remap_params(fm, border=b, pad=pad)) == INVALID, (pad, fm, b)
    assert check(lib, rp=abi.make_remap_params(pad=(0, 255, 17))) == 0
    u16 = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16)
    assert check(lib, rp=abi.make_remap_params(pad=1023), fmt=u16) == 0 and check(lib, rp=abi.make_remap_params(pad=1024), fmt=u16) == INVALID
    f32 = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32)
    assert check(lib, rp=abi.make_remap_params(pad=-3.25), fmt=f32) == 0
    assert check(lib, rp=abi.make_remap_params(pad=float("inf")), fmt=f32) == INVALID
    # image_pitch: a multiple of the element, not below one image
    image = 3 * 48 * 64 * 4
    assert check(lib, fmt=f32, rp=abi.make_remap_params(image_pitch=image)) == 0
    assert check(lib, fmt=f32, rp=abi.make_remap_params(image_pitch=image - 4)) == INVALID
    assert check(lib, fmt=f32, rp=abi.make_remap_params(image_pitch=image + 2)) == INVALID
    # sizes
    for size in ((1, 64), (48, 1), (16385, 64), (48, 16385)):
        assert check(lib, size=size) == UNSUPPORTED, size
    assert check(lib, size=(2, 2)) == 0 and check(lib, size=(16384, 16384)) == 0
    # the normalise into integers
    assert check(lib, sc=abi.make_scale_params(64, 48, mean=(0.5, 0.5, 0.5))) == INVALID
    assert check(lib, fmt=f32, sc=abi.make_scale_params(64, 48, mean=(0.5, 0.5, 0.5))) == 0
    # NULLs
    assert lib.xgpu_output_remap_check(None, None, None, 1, W, H, 10) == INVALID
    assert lib.xgpu_output_remap_size(None, None, None, 1, W, H, 10) == 0
    assert lib.xgpu_remap_grid_size(None, None, 1) == 0


def test_size_formulas(lib):
    """what the device call compares grid_size and dst_size with"""
    sc = abi.make_scale_params(SIZE[1], SIZE[0])
    for k in (0, 1, 4, 6):
        gh, gw = mr.grid_dims(SIZE, k)
        one = gh * gw * 8
        for n in (1, 3, abi.MAX_ROIS):
            assert abi.remap_grid_size(lib, sc, abi.make_remap_params(step_log2=k), n) == n * one
            assert abi.remap_grid_size(lib, sc, abi.make_remap_params(step_log2=k, grid_pitch=one + 24), n) == (n - 1) * (one + 24) + one
        assert abi.remap_grid_size(lib, sc, abi.make_remap_params(step_log2=k, grid_pitch=one - 8), 2) == 0
        assert abi.remap_grid_size(lib, sc, abi.make_remap_params(step_log2=k), 0) == 0
    assert abi.remap_grid_size(lib, sc, abi.make_remap_params(step_log2=7), 1) == 0
    for layout, dtype, es in ((abi.OUT_RGB_PLANAR, abi.OUT_U8, 1), (abi.OUT_RGB_INTERLEAVED, abi.OUT_F16, 2), (abi.OUT_YUV444_PLANAR, abi.OUT_F32, 4)):
        fmt = abi.make_output_format(layout, dtype)
        image = 3 * 48 * 64 * es
        for n in (1, 3):
            assert abi.output_remap_size(lib, fmt, sc, abi.make_remap_params(), n, W, H, 10) == n * image
            assert abi.output_remap_size(lib, fmt, sc, abi.make_remap_params(image_pitch=image + 4 * es), n, W, H, 10) == (n - 1) * (image + 4 * es) + image
        # one image is the warp's and the scaled output's
        assert abi.output_remap_size(lib, fmt, sc, abi.make_remap_params(), 1, W, H, 10) == abi.output_warp_size(lib, fmt, sc, abi.make_warp_params(), 1, W, H, 10)


LENS = dict(fx=301.5, fy=298.25, cx=161.3, cy=99.1, k1=-0.31, k2=0.12, p1=0.0013, p2=-0.0021, k3=-0.027, nfx=260.0, nfy=255.0, ncx=33.5, ncy=22.25)


def test_helpers_equal_the_restatement(lib):
    rng = np.random.default_rng(91)
    sizes = [((48, 64), 0), ((50, 70), 1), ((2, 2), 0), ((5, 65), 4), ((9, 129), 6), ((33, 31), 3)]
    # from_warp
    maps = [wr.IDENTITY, (Q, 0, 37 * Q, 0, Q, 21 * Q), (-Q, 0, 319 * Q, 0, Q, 0), wr.from_rotated_box(300, 20, 120, 80, 30, SIZE), wr.from_matrix((3.7, 0.9, 5, 0.2, 3.7, 3)),
            (64 << 16, -(64 << 16), 1 << 36, 64 << 16, 64 << 16, -(1 << 36))]      # the last one leaves int32: clamped to +-INT32_MAX
    for m in maps:
        for size, k in sizes:
            got = abi.remap_from_warp(lib, m, size, k)
            assert got.dtype == np.int32 and got.shape == (*mr.grid_dims(size, k), 2)
            assert np.array_equal(got, mr.from_warp(m, size, k)), (m, size, k)
    g = abi.remap_from_warp(lib, maps[-1], (9, 129), 6)
    assert g.max() == (1 << 31) - 1 and g.min() == -((1 << 31) - 1)
    assert abi.remap_from_warp(lib, (Q, 0, 0, 0, (64 << 16) + 1, 0), SIZE, 0) == INVALID
    # from_homography: the identity, a perspective, one whose denominator changes sign inside the image (invalid nodes), random ones
    hs = [(1, 0, 0, 0, 1, 0, 0, 0, 1), (1.1, 0.05, -3, 0.02, 0.9, 4, 0.0004, -0.0003, 1), (1, 0, 0, 0, 1, 0, -1 / 32, 0, 1), (2, 0, 0, 0, 2, 0, 0, -1 / 20, 1),
              (1e6, 0, 0, 0, 1e6, 0, 0, 0, 1), (float("nan"), 0, 0, 0, 1, 0, 0, 0, 1), (1, 0, 0, 0, 1, 0, 0, 0, 0)]
    hs += [tuple(rng.normal(0, 1, 6)) + tuple(rng.normal(0, 0.01, 2)) + (1.0,) for _ in range(20)]
    invalid = 0
    for h in hs:
        for size, k in sizes:
            got, exp = abi.remap_from_homography(lib, h, size, k), mr.from_homography(h, size, k)
            assert np.array_equal(got, exp), (h, size, k)
            bad = (got == mr.INVALID).any(axis=-1)
            assert np.array_equal(bad, (got == mr.INVALID).all(axis=-1))
            invalid += int(bad.any() and not bad.all())
    assert np.array_equal(abi.remap_from_homography(lib, hs[0], SIZE, 0), mr.from_warp(wr.IDENTITY, SIZE, 0))
    g = abi.remap_from_homography(lib, hs[2], SIZE, 0)      # den = 1 - (ox + 0.5) / 32 is positive up to column 31
    assert (g[:, :32] != mr.INVALID).all() and (g[:, 32:] == mr.INVALID).all()
    assert invalid >= 4
    # from_lens: all five coefficients non-zero; an identity lens; extreme coefficients that overflow to non-finite values far from the centre
    lenses = [LENS, dict(fx=100, fy=100, cx=31.5, cy=23.5), dict(LENS, k1=1e308, k2=1e308, k3=1e308, nfx=1.0, nfy=1.0), dict(LENS, k1=2.5, k3=40.0, nfx=20.0, nfy=20.0)]
    for lens in lenses:
        for size, k in sizes:
            got, exp = abi.remap_from_lens(lib, lens, size, k), mr.from_lens(lens, size, k)
            assert np.array_equal(got, exp), (lens, size, k)
    assert np.array_equal(abi.remap_from_lens(lib, lenses[1], SIZE, 0), mr.from_warp(wr.IDENTITY, SIZE, 0))
    assert (abi.remap_from_lens(lib, lenses[2], SIZE, 0) == mr.INVALID).any()
    for name in ("xgpu_remap_from_warp", "xgpu_remap_from_homography", "xgpu_remap_from_lens"):
        assert getattr(lib, name)(None, 64, 48, 0, None) == INVALID
    assert abi.remap_from_lens(lib, LENS, SIZE, 7) == INVALID and abi.remap_from_lens(lib, LENS, (1, 8), 0) == INVALID


def test_float_nodes():
    """the float32 conversion: clamp, exact scaling, round half to even, non-finite = invalid"""
    v = np.array([0.0, -0.0, 1.0, -1.5, 0.5 / 65536, 1.5 / 65536, 2.5 / 65536, -0.5 / 65536, 32767.0, 32768.0, -40000.0, 1e30, -1e30, 1e-40], np.float32)
    exp = [0, 0, Q, -98304, 0, 2, 2, 0, 32767 << 16, 32767 << 16, -(32767 << 16), 32767 << 16, -(32767 << 16), 0]
    q, valid = mr.nodes_q16(np.stack([v, v[::-1]], axis=-1)[None])
    assert valid.all() and q[0, :, 0].tolist() == exp and q[0, :, 1].tolist() == exp[::-1]
    bad = np.array([[np.nan, 0], [0, np.inf], [-np.inf, 1], [1, 2]], np.float32)[None]
    assert mr.nodes_q16(bad)[1].tolist() == [[False, False, False, True]]
    ints = np.array([[mr.INVALID, 0], [0, mr.INVALID], [mr.INVALID + 1, (1 << 31) - 1]], np.int32)[None]
    assert mr.nodes_q16(ints)[1].tolist() == [[False, False, True]]


@pytest.mark.parametrize("k", [0, 1, 3, 6])
def test_an_affine_grid_is_the_warp(k):
    """the restatement against warp_ref: bilinear interpolation of an affine function is exact and the derivatives are the map's linear part, so for maps whose
    nodes stay inside int32 the two restatements agree bit for bit, at every S and under both borders"""
    rng = np.random.default_rng(93)
    bd = 10
    planes = [rng.integers(0, 1 << bd, s, dtype=np.int64) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]
    maps = [wr.IDENTITY, (Q, 0, 10 * Q + Q // 2, 0, Q, 5 * Q + Q // 2), wr.from_rotated_box(300, 20, 120, 80, 30, SIZE), wr.from_matrix((3.7, 0.9, 5, 0.2, 3.7, 3)),
            (Q, 0, -500 * Q, 0, Q, 400 * Q)]
    size = (21, 67)
    for samples in (1, 2, 4):
        for border in (mr.CLAMP, mr.PAD):
            a = mr.batch(planes, bd, size, [mr.from_warp(m, size, k) for m in maps], k, samples, border, 7, dtype=mr.U16, layout="yuv444", chroma_loc=samples & 1)
            b = wr.batch(planes, bd, size, maps, samples, border, 7, dtype=wr.U16, layout="yuv444", chroma_loc=samples & 1)
            assert np.array_equal(a, b), (k, samples, border)


def test_the_restatement_within_one_code_value_of_grid_sample():
    """S = 1, k = 0, positions inside the picture, a ramp whose slope is at most 4 code values per sample: the Q8 fractions err by at most 1 / 512 sample per axis
    (4 * 2 / 512 code values), the final rounding adds 0.5 - within 1 code value of torch's grid_sample (bilinear, align_corners=False) in float64"""
    import torch
    rng = np.random.default_rng(95)
    bd, w, h = 10, 96, 64
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    y = (3 * xx + 4 * yy + 40).astype(np.int64)
    assert y.max() < 1 << bd
    c = np.full((h // 2, w // 2), 512, np.int64)
    size = (40, 56)
    pos = np.stack([rng.uniform(0, w - 1, size), rng.uniform(0, h - 1, size)], axis=-1).astype(np.float32)
    (got, _, _), outside, invalid = mr.remapped_ycbcr([y, c, c], bd, size, pos, 0, 1)
    assert not outside.any() and not invalid.any()
    p64 = pos.astype(np.float64)
    norm = np.stack([(2 * p64[..., 0] + 1) / w - 1, (2 * p64[..., 1] + 1) / h - 1], axis=-1)      # align_corners=False: sample i's centre at (2 i + 1) / n - 1
    ref = torch.nn.functional.grid_sample(torch.from_numpy(y.astype(np.float64))[None, None], torch.from_numpy(norm)[None], mode="bilinear", padding_mode="border",
                                          align_corners=False)[0, 0].numpy()
    err = np.abs(got - ref).max()
    print("max |remap_ref - grid_sample| =", err)
    assert err <= 1.0
    # the same grid in Q16 gives the same image
    q, _ = mr.nodes_q16(pos)
    (again, _, _), _, _ = mr.remapped_ycbcr([y, c, c], bd, size, q.astype(np.int32), 0, 1)
    assert np.array_equal(got, again)
