"""CPU suite for the device-output feature: the conversion contract (xgpu_output_coeffs against tests/colour_ref.py, the fixed-point
restatement against float64, fixed points, invalid formats), the VUI the writer and parser carry, and the defaults the stream player
derives from it.  Nothing here needs a GPU."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

import colour_ref as cr
from xevd_amd import abi, stream, synth

MATRICES = (1, 4, 5, 6, 7, 9)
DTYPES = (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32)


def lib_coeffs(fmt, bd):
    coef, shift, fcoef = (C.c_int32 * 5)(), C.c_int(), (C.c_float * 5)()
    rc = abi.load().xgpu_output_coeffs(C.byref(fmt), bd, coef, C.byref(shift), fcoef)
    return rc, list(coef), shift.value, [np.float32(v) for v in fcoef]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_coeffs_equal_the_restatement(bd):
    for m, fr, dt in itertools.product(MATRICES, (0, 1), DTYPES):
        fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, dt, matrix=m, full_range=fr)
        rc, coef, shift, fcoef = lib_coeffs(fmt, bd)
        k, s, f = cr.coeffs(m, fr, bd, dt)
        assert rc == 0 and coef == k and shift == s and fcoef == f, (m, fr, dt, coef, k)
        if dt in (abi.OUT_U8, abi.OUT_U16):
            assert s == 27 - (8 if dt == abi.OUT_U8 else bd) and coef[2] < 0 and coef[3] < 0


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("matrix", MATRICES)
def test_fixed_point_within_one_lsb_of_float64(bd, matrix):
    g = np.unique(np.linspace(0, (1 << bd) - 1, 41).round().astype(np.int64))
    y, cb, crr = (a.ravel() for a in np.meshgrid(g, g, g, indexing="ij"))
    for fr, dt in itertools.product((0, 1), (abi.OUT_U8, abi.OUT_U16)):
        got = cr.ycbcr_to_rgb(y, cb, crr, bd, matrix, fr, dt).astype(np.int64)
        ref = cr.h273_float64(y, cb, crr, bd, matrix, fr, cr.out_depth(dt, bd))
        assert np.abs(got - ref).max() <= 1, (fr, dt)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_fixed_points(bd):
    co = 1 << (bd - 1)
    for m, dt in itertools.product(MATRICES, DTYPES):
        mx = 1.0 if dt not in (abi.OUT_U8, abi.OUT_U16) else (1 << cr.out_depth(dt, bd)) - 1
        # limited range black / white, full range 0 / 2^B - 1, neutral chroma
        for fr, lo, hi in ((0, 16 << (bd - 8), 235 << (bd - 8)), (1, 0, (1 << bd) - 1)):
            rgb = cr.ycbcr_to_rgb(np.array([lo, hi]), np.array([co, co]), np.array([co, co]), bd, m, fr, dt)
            tol = 0 if dt in (abi.OUT_U8, abi.OUT_U16) else 4e-7      # float32 coefficients: white may land an ulp below 1
            assert (rgb[:, 0] == 0).all() and (np.abs(rgb[:, 1].astype(np.float64) - mx) <= tol).all(), (m, dt, fr, rgb)
        grey = cr.ycbcr_to_rgb(np.arange(0, 1 << bd, 7), np.full(((1 << bd) + 6) // 7, co), np.full(((1 << bd) + 6) // 7, co), bd, m, 0, dt)
        assert (grey[0] == grey[1]).all() and (grey[1] == grey[2]).all()


def test_invalid_formats_are_refused():
    ok = dict(layout=abi.OUT_RGB_PLANAR, dtype=abi.OUT_U8)
    assert lib_coeffs(abi.make_output_format(**ok), 10)[0] == 0
    for m in (0, 2, 3, 8, 10, 11, 14):
        assert lib_coeffs(abi.make_output_format(matrix=m, **ok), 10)[0] == -104, m       # XGPU_ERR_UNSUPPORTED
    bad = [dict(chroma_loc=6), dict(chroma_loc=-1), dict(crop=(1, 0, 0, 0)), dict(crop=(0, 0, 0, 3)), dict(crop=(-2, 0, 0, 0)), dict(upsample=2),
           dict(layout=3), dict(dtype=5), dict(row_pitch=3, dtype=abi.OUT_U16)]
    for b in bad:
        assert lib_coeffs(abi.make_output_format(**{**ok, **b}), 10)[0] < 0, b
    for obd in (8, 12, 16):      # an RGB u16 format: out_bit_depth 0 or the coding depth
        assert lib_coeffs(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, out_bit_depth=obd), 10)[0] < 0, obd
    assert lib_coeffs(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, out_bit_depth=10), 10)[0] == 0
    lib = abi.load()
    assert lib.xgpu_pic_output_device_size(None, C.byref(abi.make_output_format(**ok))) == 0
    assert lib.xgpu_pic_output_device(None, 0, None, C.byref(abi.make_output_format(**ok)), None, 0, None) < 0


def _one_picture_stream(vui, bd=10, seed=1, w=64, h=64):
    rng = np.random.default_rng(seed)
    wr = stream.StreamWriter(w, h, bd, vui=vui)
    try:
        wr.add_picture(synth.gen_frame(rng, w, h, bd, inter_frac=0.0, n_refs=(1, 0)), stream.SLICE_I, 30, idr=True)
        return wr.bytes()
    finally:
        wr.close()


def _vui_cases():
    out = []
    for fr, colour, loc, extra in itertools.product((None, 0, 1), (None, (1, 1, 1), (9, 16, 9), (6, 6, 5)), (None, (0, 0), (3, 2), (5, 4)), (False, True)):
        vui = {}
        if fr is not None:
            vui["full_range"] = fr
        if colour is not None:
            vui["colour"] = colour
        if loc is not None:
            vui["chroma_loc"] = loc
        if extra:
            vui["extra"] = True
        out.append(vui)
    return out


def test_vui_round_trip():
    """every combination of the writer's VUI fields parses back to the same colour description; the VUI's other syntax (SAR, timing, HRD with two
    CPB specifications, bitstream restriction) is stepped over without running out of bits - the picture after it is the same as without a VUI"""
    plain = stream.parse_stream(_one_picture_stream(None))
    assert plain[0]["colour"] == {"vui_present": False, "full_range": 0, "colour_primaries": 2, "transfer_characteristics": 2,
                                  "matrix_coefficients": 2, "chroma_sample_loc_type": 0}
    for vui in _vui_cases():
        data = _one_picture_stream(vui or {"extra": False})
        pics = stream.parse_stream(data)
        col = pics[0]["colour"]
        signalled = bool(vui)
        assert col["vui_present"] == signalled, vui
        colour = vui.get("colour", (2, 2, 2))
        assert (col["colour_primaries"], col["transfer_characteristics"], col["matrix_coefficients"]) == tuple(colour), vui
        assert col["full_range"] == int(bool(vui.get("full_range", 0))), vui
        assert col["chroma_sample_loc_type"] == (vui.get("chroma_loc") or (0, 0))[0], vui
        assert len(pics) == 1 and np.array_equal(pics[0]["batch"]["coef"], plain[0]["batch"]["coef"]), vui


def test_truncated_vui_is_refused():
    data = _one_picture_stream({"extra": True, "colour": (1, 1, 1)})
    n = int.from_bytes(data[:4], "big")               # the SPS is the first NAL unit: cut it inside its VUI
    cut = n - 6
    bad = (cut).to_bytes(4, "big") + data[4:4 + cut] + data[4 + n:]
    with pytest.raises(RuntimeError, match="SPS"):
        stream.parse_stream(bad)


def test_writer_default_bytes_unchanged():
    """with every VUI field zero the writer writes the bytes it wrote before the VUI fields existed (hashes taken from that tree)"""
    import stream_util as su
    a = su.make_stream(128, 64, 3, seed=5)
    b = su.make_stream(192, 128, 3, seed=7, main=True, iqt=True, addb=True, alf=True, admvp=True, crop=(2, 4, 0, 2))
    assert (len(a), hashlib.sha256(a).hexdigest()) == (363, "b19e41fae3e4e341b0d75a531dc5489e3490934ef389e7aa01b7bf577b9693ef")
    assert (len(b), hashlib.sha256(b).hexdigest()) == (1364, "4dac145e31020b22b32a486bcc0b962069b78feb13e04193c9dead2d6410f4ab")


def test_player_tensor_defaults_follow_the_vui():
    from xevd_amd.player import StreamDecoder

    def opts(vui, **over):
        p = stream.parse_stream(_one_picture_stream(vui))[0]
        kw = StreamDecoder.tensor_options(p, over)
        return kw["matrix"], kw["full_range"], kw["chroma_loc"]
    assert opts(None) == (1, False, 0)
    assert opts({"colour": (2, 2, 2)}) == (1, False, 0)            # unspecified -> BT.709
    assert opts({"colour": (6, 6, 5), "full_range": 1, "chroma_loc": (2, 2)}) == (5, True, 2)
    assert opts({"colour": (9, 16, 9), "chroma_loc": (1, 1)}) == (9, False, 1)
    assert opts({"colour": (6, 6, 5)}, matrix=1, full_range=True) == (1, True, 0)      # explicit arguments win


@pytest.mark.parametrize("loc", range(6))
def test_linear_upsampling_weights(loc):
    """LINEAR keeps a constant plane constant and a ramp along the siting; NEAREST repeats samples"""
    c = np.full((5, 7), 300)
    assert (cr.upsample(c, 14, 10, "linear", loc) == 300).all()
    ramp = np.tile(np.arange(7) * 16, (5, 1))
    up = cr.upsample(ramp, 14, 10, "linear", loc)
    exp = np.arange(14) * 8 - (4 if loc % 2 else 0)       # co-sited: sample j at x = 2j; centred: at x = 2j + 1/2
    assert (up[:, 1:13] == exp[1:13]).all(), up[0]
    assert (cr.upsample(ramp, 14, 10, "nearest", loc) == np.repeat(np.repeat(ramp, 2, 0), 2, 1)).all()


@pytest.mark.ref
@pytest.mark.parametrize("main", [False, True])
def test_reference_decoder_reads_the_written_vui(main):
    """the reference decoder (xevd_eco_vui) steps over the VUI the writer puts in the SPS: the same pictures as from the stream without one"""
    import stream_util as su

    def make(vui):
        rng = np.random.default_rng(2)
        wr = stream.StreamWriter(64, 64, 10, vui=vui, main=main)
        try:
            for k in range(2):
                wr.add_picture(synth.gen_frame(rng, 64, 64, 10, inter_frac=0.0, n_refs=(1, 0)), stream.SLICE_I, 30 + k, idr=True)
            return wr.bytes()
        finally:
            wr.close()
    plain = su.decode_reference(make(None), 64, 64, main=main)
    assert len(plain) == 2
    for vui in ({"extra": True, "colour": (9, 16, 9), "full_range": 1, "chroma_loc": (1, 1)}, {"chroma_loc": (4, 5)}):
        got = su.decode_reference(make(vui), 64, 64, main=main)
        assert len(got) == 2 and all(np.array_equal(a, b) for p, q in zip(got, plain) for a, b in zip(p, q)), vui
