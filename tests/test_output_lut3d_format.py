"""CPU suite for the 3D LUT output (xgpu_pic_output_device_lut3d / _packed_lut3d): the exported symbols, the refusal codes of
xgpu_output_lut3d_check in their order, the host helpers xgpu_lut3d_from_float / _identity / _shaper against the numpy restatement tests/lut3d_ref.py bit for
bit, the identity property through the restatement, the .cube reader, and the distance of a baked LUT from the analytic colour transform it replaces.  Nothing
here needs a GPU."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import colour_cm_ref as cmr
import golden_io
import lut3d_ref as lr
from xevd_amd import abi, lut3d

INVALID, UNSUPPORTED = -101, -104
DTYPES = (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32)
PQ_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)


def check(f=None, pf=None, n=17, width=64, height=48, bd=10):
    return abi.load().xgpu_output_lut3d_check(None if f is None else C.byref(f), None if pf is None else C.byref(pf), n, width, height, bd)


def test_exported_symbols():
    for name in ("xgpu_lut3d_from_float", "xgpu_lut3d_identity", "xgpu_lut3d_shaper", "xgpu_output_lut3d_check", "xgpu_lut3d_create", "xgpu_lut3d_destroy",
                 "xgpu_pic_output_device_lut3d", "xgpu_pic_output_device_packed_lut3d"):
        assert name in abi.exported_names(), name
        assert hasattr(abi.load(), name)
    assert abi.MAX_LUT3D == 8


def test_check_accepts_every_form():
    for bd, lay, dt, n in itertools.product((8, 10, 12), (abi.OUT_RGB_PLANAR, abi.OUT_RGB_INTERLEAVED), DTYPES, (2, 17, 65)):
        for obd in (0, bd) + ((16,) if dt == abi.OUT_U16 else ()):
            assert check(abi.make_output_format(lay, dt, out_bit_depth=obd), n=n, bd=bd) == 0, (bd, lay, dt, obd)
    for bd, dt in itertools.product((8, 10, 12), DTYPES):
        assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, dt, bgr=True, alpha=0.5), bd=bd) == 0
    assert check(pf=abi.make_packed_format(abi.PACKED_RGB10A2)) == 0
    f = abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_U16, out_bit_depth=16, row_pitch=3 * 64 * 2 + 32)
    assert check(f) == 0


def test_check_refusals_come_in_their_order():
    rgb = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8)
    # neither or both formats
    assert check() == INVALID and check(rgb, abi.make_packed_format()) == INVALID
    # the plain call's refusals, with its codes: they come before the layout and before n
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, matrix=2), n=1) == UNSUPPORTED
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, crop=(1, 0, 0, 0)), n=1) == INVALID
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, out_bit_depth=16)) == INVALID      # the 16-bit store is U16's
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, out_bit_depth=16)) == INVALID
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, out_bit_depth=12), bd=10) == INVALID
    assert check(abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_U16, row_pitch=3 * 64 * 2 - 2)) == INVALID
    assert check(rgb, bd=13) == INVALID and check(rgb, width=0) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, matrix=2), n=1) == UNSUPPORTED
    assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, alpha=1.5), n=1) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_U16, out_bit_depth=16)) == INVALID      # only the RGB call takes 16
    assert check(pf=abi.make_packed_format(abi.PACKED_RGB10A2, dtype=abi.OUT_U16)) == INVALID
    # then the layout: before n
    for lay in (abi.OUT_YUV420P, abi.OUT_NV12, abi.OUT_YUV444_PLANAR):
        dt = abi.OUT_U16 if lay != abi.OUT_YUV444_PLANAR else abi.OUT_U8
        assert check(abi.make_output_format(lay, dt), n=1) == INVALID, lay
    assert check(abi.make_output_format(abi.OUT_YUV444_INTERLEAVED, abi.OUT_U16, out_bit_depth=16)) == INVALID      # 16 is not let through for other layouts
    assert check(pf=abi.make_packed_format(abi.PACKED_YUYV, abi.OUT_U8, out_bit_depth=8), n=66) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_UYVY, abi.OUT_U16), n=1) == INVALID
    # then n
    for n in (-1, 0, 1, 66, 129):
        assert check(rgb, n=n) == UNSUPPORTED and check(pf=abi.make_packed_format(), n=n) == UNSUPPORTED, n
    for n in (2, 65):
        assert check(rgb, n=n) == 0


def test_existing_calls_keep_their_out_bit_depth_rule():
    lib = abi.load()
    f = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, out_bit_depth=16)
    assert lib.xgpu_output_format_size(C.byref(f), 64, 48, 10) == 0


# ------------------------------------------------------------------------------------------------ the helpers against the restatement
def test_from_float_equals_the_restatement():
    lib = abi.load()
    rng = np.random.default_rng(11)
    for n in (2, 3, 17):
        v = rng.uniform(-0.25, 1.25, (n ** 3, 3)).astype(np.float32)
        v.ravel()[:12] = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.0000001, 0.5, 0.5 / 65535, 1.5 / 65535, 65534.5 / 65535]
        got = abi.lut3d_from_float(lib, v)
        assert got.dtype == np.uint16 and np.array_equal(got, lr.from_float(v)), n
        assert list(got.ravel()[:8]) == [0, 0, 65535, 0, 0, 0, 65535, 65535]
    assert abi.lut3d_from_float(lib, np.zeros((1, 3), np.float32)) == UNSUPPORTED
    assert abi.lut3d_from_float(lib, np.zeros((66 ** 3, 3), np.float32)) == UNSUPPORTED
    assert lib.xgpu_lut3d_from_float(None, 2, None) == INVALID


@pytest.mark.parametrize("n", [2, 3, 5, 17, 32, 33, 64, 65])
def test_identity_cube_equals_the_closed_formula(n):
    got = abi.lut3d_identity(abi.load(), n)
    assert np.array_equal(got, lr.identity_cube(n))
    e = [(2 * 65535 * i + n - 1) // (2 * (n - 1)) for i in range(n)]
    assert e[0] == 0 and e[-1] == 65535
    for r, g, b in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (n - 1, n - 2, 1)):
        assert list(got[r + n * (g + n * b)]) == [e[r], e[g], e[b]]
    assert abi.lut3d_identity(abi.load(), 1) == UNSUPPORTED and abi.lut3d_identity(abi.load(), 66) == UNSUPPORTED


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_identity_shaper_equals_the_closed_formula(bd):
    lib = abi.load()
    m = (1 << bd) - 1
    closed = np.array([(2 * 65535 * c + m) // (2 * m) for c in range(m + 1)], np.uint16)
    for kw in (dict(), dict(in_min=(0, 0, 0), in_max=(1, 1, 1))):
        got = abi.lut3d_shaper(lib, bd, **kw)
        assert got.shape == (3, m + 1) and all(np.array_equal(got[k], closed) for k in range(3))
    assert np.array_equal(lr.identity_shaper(bd)[1], closed) and np.array_equal(lr.shaper(bd), lr.identity_shaper(bd))


def test_shaper_equals_the_restatement():
    lib = abi.load()
    rng = np.random.default_rng(12)
    curves = {"ramp": np.linspace(0, 1, 5, dtype=np.float32)[:, None].repeat(3, 1),
              "non_monotone": rng.uniform(-0.2, 1.2, (33, 3)).astype(np.float32),
              "two_points": np.array([[1, 0, 0.25], [0, 1, 0.75]], np.float32),
              "nan": np.array([[0, 0, 0], [np.nan, 0.5, 2], [1, 1, 1]], np.float32),
              "long": rng.uniform(0, 1, (4096, 3)).astype(np.float32)}
    bounds = [((0, 0, 0), (1, 1, 1)), ((0.0625, 0.1, -0.5), (0.9, 0.5, 1.5)), ((-1e-3, 0.25, 0.999), (1e3, 0.26, 1.0))]
    for bd, (name, cv), (lo, hi) in itertools.product((8, 10, 12), [("none", None)] + list(curves.items()), bounds):
        got = abi.lut3d_shaper(lib, bd, curve=cv, in_min=lo, in_max=hi)
        exp = lr.shaper(bd, cv, lo, hi)
        assert np.array_equal(got, exp), (bd, name, lo, hi, int((got != exp).sum()))
    assert abi.lut3d_shaper(lib, 10, in_min=(0.5, 0, 0), in_max=(0.5, 1, 1)) == INVALID      # an empty range
    assert abi.lut3d_shaper(lib, 10, in_min=(0, 0, 0), in_max=(1, np.nan, 1)) == INVALID
    assert abi.lut3d_shaper(lib, 10, in_max=(np.inf, 1, 1)) == INVALID
    assert abi.lut3d_shaper(lib, 10, curve=np.zeros((1, 3), np.float32)) == INVALID
    assert abi.lut3d_shaper(lib, 7) == INVALID and abi.lut3d_shaper(lib, 13) == INVALID


def test_the_kernels_division_is_the_floor_division():
    rng = np.random.default_rng(13)
    top = 65535 * 65535 + 32767
    x = np.concatenate([np.arange(0, 1 << 20), np.arange(top - (1 << 20), top + 1), rng.integers(0, top + 1, 2_000_000)]).astype(np.uint64)
    assert np.array_equal(lr.div65535_shift(x), x // np.uint64(65535))
    assert int(x.max() + (x.max() >> np.uint64(16)) + np.uint64(1)) < 1 << 32


# ------------------------------------------------------------------------------------------------ the identity property
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("n", [2, 3, 5, 17, 32, 33, 64, 65])
def test_identity_lut_returns_the_shaper_position(bd, n):
    m = (1 << bd) - 1
    rng = np.random.default_rng(14 + n)
    every = np.arange(m + 1)
    codes = np.stack([np.concatenate([every, rng.integers(0, m + 1, 20000)]), np.concatenate([every[::-1], rng.integers(0, m + 1, 20000)]),
                      np.concatenate([(every * 7) % (m + 1), rng.integers(0, m + 1, 20000)])])
    shp = lr.identity_shaper(bd)
    v, census = lr.interpolate(codes, shp, lr.identity_cube(n), n)
    assert np.array_equal(v, shp.astype(np.int64)[0][codes])      # v = p, channel by channel
    assert all(census[k] > 0 for k in lr.ORDERINGS) and census["clamp"] > 0
    assert np.array_equal(lr.store(v, lr.U16, bd), codes)        # the U16 output is the code itself ...
    if bd == 8:
        assert np.array_equal(lr.store(v, lr.U8, 8), codes)     # ... and so is U8 at 8 bit
    assert np.array_equal(lr.store(v, lr.U16, 16), shp[0][codes])


def test_census_buckets():
    n, bd = 5, 8
    shp = lr.identity_shaper(bd)
    nodes = lr.identity_cube(n)
    _, c = lr.interpolate(np.array([[0], [0], [0]]), shp, nodes, n)
    assert c["node"] == 1 and c["tie"] == 1 and c["clamp"] == 0 and sum(c[k] for k in lr.ORDERINGS) == 0
    _, c = lr.interpolate(np.array([[255], [255], [0]]), shp, nodes, n)
    assert c["node"] == 1 and c["clamp"] == 1 and c["tie"] == 1
    _, c = lr.interpolate(np.array([[30, 10, 20], [20, 30, 10], [10, 20, 30]]), shp, nodes, n)
    assert (c["RGB"], c["GBR"], c["BRG"], c["tie"], c["node"]) == (1, 1, 1, 0, 0)
    # a random cube: the four vertices and their weights against a direct evaluation of one pixel
    rng = np.random.default_rng(15)
    nodes = rng.integers(0, 65536, (n ** 3, 3)).astype(np.uint16)
    code = np.array([[50], [70], [100]])      # cells of 63.75 codes: fractions 0.78, 0.10, 0.57
    v, c = lr.interpolate(code, shp, nodes, n)
    p = [int(shp[k][code[k, 0]]) for k in range(3)]
    i = [min(p[k] * (n - 1) // 65535, n - 2) for k in range(3)]
    f = [p[k] * (n - 1) - 65535 * i[k] for k in range(3)]
    assert f[0] > f[2] > f[1] and c["RBG"] == 1
    at = lambda r, g, b: nodes[r + n * (g + n * b)].astype(np.int64)      # noqa: E731
    s = ((65535 - f[0]) * at(*i) + (f[0] - f[2]) * at(i[0] + 1, i[1], i[2]) + (f[2] - f[1]) * at(i[0] + 1, i[1], i[2] + 1)
         + f[1] * at(i[0] + 1, i[1] + 1, i[2] + 1))
    assert list(v[:, 0]) == list((s + 32767) // 65535)


# ------------------------------------------------------------------------------------------------ the .cube reader
def write(path, text):
    path.write_text(text)
    return str(path)


def test_cube_reader(tmp_path):
    rows2 = "\n".join(f"{r} {g} {b}" for b in (0, 1) for g in (0, 1) for r in (0, 1))
    c = lut3d.load_cube(write(tmp_path / "a.cube", f'# a comment\nTITLE "two nodes"\n\nLUT_3D_SIZE 2\nDOMAIN_MIN 0.0 0.1 0.2\nDOMAIN_MAX 1.0 0.9 0.8\n{rows2}\n'))
    assert c["title"] == "two nodes" and c["n"] == 2 and c["curve"] is None
    assert c["nodes"].dtype == np.float32 and c["nodes"].shape == (8, 3)
    assert list(c["nodes"][1]) == [1, 0, 0] and list(c["nodes"][2]) == [0, 1, 0] and list(c["nodes"][4]) == [0, 0, 1]      # red fastest
    assert c["in_min"] == [0.0, 0.1, 0.2] and c["in_max"] == [1.0, 0.9, 0.8]
    assert c["shaper"]["curve"] is None and c["shaper"]["in_min"] == c["in_min"]
    got = abi.lut3d_shaper(abi.load(), 10, **c["shaper"])
    assert np.array_equal(got, lr.shaper(10, None, c["in_min"], c["in_max"]))
    # no domain: the identity shaper
    assert lut3d.load_cube(write(tmp_path / "b.cube", f"LUT_3D_SIZE 2\n{rows2}\n"))["shaper"] is None
    # 1D + 3D
    one_d = "\n".join(f"{v} {v * v} {1 - v}" for v in (0.0, 0.25, 0.5, 1.0))
    c = lut3d.load_cube(write(tmp_path / "c.cube", f"LUT_1D_SIZE 4\nLUT_1D_INPUT_RANGE 0.0 2.0\nLUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0.0 1.0\n{one_d}\n{rows2}  # tail\n"))
    assert c["n"] == 2 and c["curve"].shape == (4, 3) and list(c["curve"][1]) == [0.25, 0.0625, 0.75]
    assert c["in_min"] == [0.0] * 3 and c["in_max"] == [2.0] * 3 and c["nodes"].shape == (8, 3) and list(c["nodes"][1]) == [1, 0, 0]
    assert np.array_equal(abi.lut3d_shaper(abi.load(), 8, **c["shaper"]), lr.shaper(8, c["curve"], c["in_min"], c["in_max"]))
    c = lut3d.load_cube(write(tmp_path / "d.cube", f"LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0.0 4.0\n{rows2}\n"))
    assert c["in_max"] == [4.0] * 3 and c["curve"] is None


@pytest.mark.parametrize("text", [
    "LUT_3D_SIZE 2\n" + "0 0 0\n" * 7,                     # a row short
    "LUT_3D_SIZE 2\n" + "0 0 0\n" * 9,                     # a row too many
    "LUT_3D_SIZE 1\n0 0 0\n",                              # n = 1
    "LUT_3D_SIZE 66\n",                                    # n = 66
    "0 0 0\n" * 8,                                         # no size
    "LUT_3D_SIZE 2\n" + "0 0\n" * 8,                       # two values in a row
    "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0\n" + "0 0 0\n" * 8,     # two values in a domain
    "LUT_3D_SIZE 2\nDOMAIN_MIN 1 1 1\n" + "0 0 0\n" * 8,   # an empty domain
    "LUT_3D_SIZE 2\nSOMETHING 3\n" + "0 0 0\n" * 8,        # an unknown keyword
    "LUT_3D_SIZE two\n" + "0 0 0\n" * 8,
    "LUT_1D_SIZE 4\nLUT_3D_SIZE 2\n" + "0 0 0\n" * 8,      # the 1D block is missing
])
def test_cube_reader_refuses_malformed_files(text, tmp_path):
    with pytest.raises(ValueError):
        lut3d.load_cube(write(tmp_path / "bad.cube", text))


# ------------------------------------------------------------------------------------------------ a baked LUT against the analytic transform
def small_random(w, h, bd, crop, seed=5):
    rng = np.random.default_rng(seed + w + bd)      # test_gpu_output_packed.py's random planes
    planes = [rng.integers(0, 1 << bd, s).astype(np.int16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    return planes, crop


def golden_10b():
    d = np.load(os.path.join(golden_io.GOLDEN, "pic_base_p_10b.npz"))
    w, h = (int(v) for v in d["params"][:2])
    pl, pc = abi.PAD_L, abi.PAD_C
    return [d["out_0"][pl:pl + h, pl:pl + w], d["out_1"][pc:pc + h // 2, pc:pc + w // 2], d["out_2"][pc:pc + h // 2, pc:pc + w // 2]], (0, 0, 0, 0)


def bake(n, bd, cm):
    """the transform at the nodes: node i of an axis sits at code (2^bd - 1) * i / (n - 1), evaluated in float64 from the formulae"""
    m = float((1 << bd) - 1)
    ax = np.arange(n, dtype=np.float64) * m / float(n - 1)
    b, g, r = np.meshgrid(ax, ax, ax, indexing="ij")
    out = cmr.exact64(np.stack([r.ravel(), g.ravel(), b.ravel()]), cm, bd)
    return abi.lut3d_from_float(abi.load(), out.T.astype(np.float32))


# The largest difference, in code values of the output, between the LUT output and the colour-managed output (PQ / BT.2020 -> sRGB with the tone curve, B = 10,
# identity shaper) over the three pictures, measured once on the CPU - both sides are numpy, so the figures are exact on these inputs - and asserted rounded up
# to the next whole code value.  INTEGRATION.md section 8q records them.  Measured: 51 / 206 at n = 33 and 38 / 154 at n = 65 (U8 / U16 codes; the means are 0.41 /
# 1.65 and 0.14 / 0.56), all on the steep foot of the PQ curve, where a uniform grid behind the identity shaper is coarsest - what a PQ-spaced shaper is for.
BAKED_BOUNDS = {(33, lr.U8): 51, (33, lr.U16): 206, (65, lr.U8): 38, (65, lr.U16): 154}


@pytest.mark.parametrize("n", [33, 65])
def test_baked_lut_against_the_colour_managed_output(n):
    bd = 10
    lib = abi.load()
    tab = abi.colour_tables(lib, abi.make_output_format(abi.OUT_RGB_INTERLEAVED), abi.make_colour_transform(**PQ_SRGB), bd)
    nodes = bake(n, bd, PQ_SRGB)
    pictures = [small_random(24, 16, bd, (2, 4, 2, 4)), small_random(528, 16, bd, (2, 4, 2, 0)), golden_10b()]
    for dt in (lr.U8, lr.U16):
        worst = 0
        for planes, crop in pictures:
            got, _ = lr.lut3d(planes, bd, nodes, n, dtype=dt, matrix=9, crop=crop)
            exp = cmr.convert(planes, bd, tab, matrix=9, dtype=dt, crop=crop)
            worst = max(worst, int(np.abs(got.astype(np.int64) - exp.astype(np.int64)).max()))
        print(f"baked LUT n={n} dtype={'u8' if dt == lr.U8 else 'u16'}: largest difference {worst} code values")
        assert worst <= BAKED_BOUNDS[(n, dt)], (n, dt, worst)
