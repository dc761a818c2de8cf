"""CPU suite for the scaled output filtered in linear light: the exported symbols, the check functions' codes in their order, the 512 MiB
rule of the float32 intermediate with bad_index, the Python argument mapping that needs no context, and the float32 contract (tests/scaled_lin_ref.py) against a
float64 evaluation of the same pipeline with exact taps.  No GPU: host-only functions."""
import ctypes as C
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import colour_cm_ref as cmr
import colour_ref as cr
import scale_ref as sr
import scaled_cm_ref as scm
import scaled_lin_ref as slr
import stub_decoder
from test_gpu_output_device import golden_planes
from xevd_amd import abi

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -101, -104
W, H, BD = 320, 200, 10
PQ_TO_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
PQ_TO_SRGB_PLAIN = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=False, linear_scale=1.0)
HLG_TO_LINEAR = dict(src_primaries=9, src_transfer=18, dst_primaries=1, dst_transfer=8)
BT709_TO_SRGB = dict(src_primaries=1, src_transfer=1, dst_primaries=1, dst_transfer=13)


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def test_library_exports_the_symbols():
    raw = C.CDLL(abi.LIB_PATH)
    for name in ("xgpu_pic_output_device_scaled_lin", "xgpu_pic_output_device_rois_lin", "xgpu_output_scaled_lin_check", "xgpu_output_rois_lin_check"):
        assert hasattr(raw, name), name
        assert name in abi.exported_names(), name


def _check(lib, fmt, sc, cm, w=W, h=H, bd=BD):
    return lib.xgpu_output_scaled_lin_check(C.byref(fmt), C.byref(sc), C.byref(cm) if cm is not None else None, w, h, bd)


def test_check_codes_and_their_order(lib):
    rgb = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32)
    sc = abi.make_scale_params(224, 224, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25))
    good = abi.make_colour_transform(**PQ_TO_SRGB)
    for bd, up in itertools.product((8, 10, 12), (abi.UPSAMPLE_NEAREST, abi.UPSAMPLE_LINEAR)):
        assert _check(lib, abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_F32, upsample=up), sc, good, bd=bd) == 0
    assert _check(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, upsample=7), sc, good) == ERR_INVALID_ARGUMENT      # upsample is read here
    # the transform's own refusals
    bad_cm = abi.make_colour_transform(**dict(PQ_TO_SRGB, src_transfer=17))
    assert _check(lib, rgb, sc, bad_cm) == ERR_UNSUPPORTED
    assert _check(lib, rgb, sc, abi.make_colour_transform(**dict(PQ_TO_SRGB, src_peak=-1.0))) == ERR_INVALID_ARGUMENT
    # no transform: no linear light - for an RGB layout and for one a transform would refuse
    yuv = abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_F32)
    assert _check(lib, rgb, sc, None) == ERR_INVALID_ARGUMENT
    assert _check(lib, yuv, sc, None) == ERR_INVALID_ARGUMENT
    assert _check(lib, yuv, sc, good) == ERR_INVALID_ARGUMENT
    # the order: the plain call's refusal first, then the intermediate, the missing transform, the layout, the transform
    tiny = abi.make_scale_params(2, 224)      # below 1 / 64 of the width: the plain call says UNSUPPORTED
    assert _check(lib, yuv, tiny, None, w=640) == ERR_UNSUPPORTED
    assert _check(lib, rgb, tiny, abi.make_colour_transform(**dict(PQ_TO_SRGB, src_peak=-1.0)), w=640) == ERR_UNSUPPORTED
    int_norm = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8)
    assert _check(lib, int_norm, sc, bad_cm) == ERR_INVALID_ARGUMENT      # the normalise with an integer dtype, not the transfer's UNSUPPORTED
    assert _check(lib, yuv, sc, bad_cm) == ERR_INVALID_ARGUMENT           # the layout, not the transfer
    # the plain and the colour-managed checks say the same wherever this one says 0
    for fmt, s in itertools.product((rgb, abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_U8, crop=(2, 0, 0, 4))), (abi.make_scale_params(64, 48), abi.make_scale_params(640, 400))):
        assert _check(lib, fmt, s, good) == 0 == lib.xgpu_output_scaled_cm_check(C.byref(fmt), C.byref(s), C.byref(good), W, H, BD)


def test_the_512_mib_rule_counts_the_float_intermediate(lib):
    """3 x Hd x align8(Ws) x 4 bytes: a 16384-wide source may have 2730 destination rows and not 2731, where the 16-bit intermediate of the other scaled outputs is
    far from its limit; the rule comes behind the plain call's refusals and before the missing transform"""
    rgb = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8)
    good = abi.make_colour_transform(**PQ_TO_SRGB)
    w, h = 16384, 4096
    assert 3 * 2730 * w * 4 <= 512 << 20 < 3 * 2731 * w * 4
    assert _check(lib, rgb, abi.make_scale_params(256, 2730), good, w=w, h=h) == 0
    assert _check(lib, rgb, abi.make_scale_params(256, 2731), good, w=w, h=h) == ERR_UNSUPPORTED
    assert _check(lib, rgb, abi.make_scale_params(256, 2731), None, w=w, h=h) == ERR_UNSUPPORTED             # before the missing transform
    assert lib.xgpu_output_scaled_cm_check(C.byref(rgb), C.byref(abi.make_scale_params(256, 2731)), C.byref(good), w, h, BD) == 0
    narrow = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, crop=(0, 8192, 0, 0))      # the source is the picture minus the crop
    assert _check(lib, narrow, abi.make_scale_params(256, 2731), good, w=w, h=h) == 0
    # the batch: the sum over the rectangles of 3 x Hi x align8(Wi) x 4, bad_index = the rectangle that passes the limit
    sc, rp = abi.make_scale_params(256, 1024), abi.make_roi_params()
    one = 3 * 1024 * w * 4
    assert 2 * one <= 512 << 20 < 3 * one
    bad = C.c_int(-7)

    def rois_check(n, cm=good, fmt=rgb, rects=None):
        ra = abi.make_rois(rects or [(0, 2 * i, w, 2048) for i in range(n)])
        return lib.xgpu_output_rois_lin_check(C.byref(fmt), C.byref(sc), C.byref(rp), ra, n, C.byref(cm) if cm is not None else None, w, h, BD, C.byref(bad))
    assert rois_check(2) == 0 and bad.value == -1
    assert rois_check(3) == ERR_UNSUPPORTED and bad.value == 2
    assert rois_check(5, cm=None) == ERR_UNSUPPORTED and bad.value == 2
    ra = abi.make_rois([(0, 2 * i, w, 2048) for i in range(3)])
    assert lib.xgpu_output_rois_check(C.byref(rgb), C.byref(sc), C.byref(rp), ra, 3, w, h, BD, C.byref(bad)) == 0      # the 16-bit intermediate fits
    # the batch's own refusals with their index first, then the missing transform, the layout and the transform
    assert rois_check(2, rects=[(0, 0, w, 2048), (1, 0, 64, 64)]) == ERR_INVALID_ARGUMENT and bad.value == 1
    assert rois_check(2, cm=abi.make_colour_transform(**dict(PQ_TO_SRGB, src_transfer=17)), rects=[(0, 0, w, 2048), (1, 0, 64, 64)]) == ERR_INVALID_ARGUMENT and bad.value == 1
    assert rois_check(2, cm=None) == ERR_INVALID_ARGUMENT and bad.value == -1
    assert rois_check(2, fmt=abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_U8)) == ERR_INVALID_ARGUMENT and bad.value == -1
    assert rois_check(2, cm=abi.make_colour_transform(**dict(PQ_TO_SRGB, src_transfer=17))) == ERR_UNSUPPORTED and bad.value == -1


def test_python_argument_mapping(lib):
    """pic_output_scaled_cm(linear_light=True, upsample=) on a decoder object without a context: what the arguments alone decide raises ValueError, and what reaches
    the library is the _lin entry with f->upsample set; linear_light=False keeps the _cm entry"""
    import torch
    from xevd_amd.decoder import XgpuDecoder
    dec = stub_decoder.XgpuDecoder(W, H, BD)
    dec.lib, dec.sp, dec.ctx = lib, abi.make_seq_params(W, H, BD), None
    for name in ("_scaled_setup", "_pic_output_tensor_scaled", "_pic_output_tensor_rois", "_cm_check"):
        setattr(dec, name, getattr(XgpuDecoder, name).__get__(dec))
    dec._rois_fit = XgpuDecoder._rois_fit
    call = XgpuDecoder.pic_output_scaled_cm
    size = (48, 64)
    for bad in (dict(colour=PQ_TO_SRGB, upsample="cubic"), dict(colour=PQ_TO_SRGB, upsample="nearest", linear_light=False), dict(colour=None),
                dict(colour=PQ_TO_SRGB, layout="yuv444"), dict(colour=dict(PQ_TO_SRGB, src_transfer=17)), dict(colour=PQ_TO_SRGB, rois=[(1, 0, 64, 64)]),
                dict(colour=dict(PQ_TO_SRGB, src_transfer=17), rois=[(0, 0, 64, 64)]), dict(colour=PQ_TO_SRGB, crop=(1, 0, 0, 0)),
                dict(colour=PQ_TO_SRGB, rois=torch.zeros((1, 4), dtype=torch.int32))):
        with pytest.raises(ValueError):
            call(dec, 0, size, linear_light=bad.pop("linear_light", True), **bad)
    with pytest.raises(ValueError):
        call(dec, 0, (1, 64), PQ_TO_SRGB, linear_light=True)
    big = stub_decoder.XgpuDecoder(16384, 4096, BD)      # the 512 MiB rule, before a tensor is made
    big.lib, big.sp, big.ctx = lib, abi.make_seq_params(16384, 4096, BD), None
    for name in ("_scaled_setup", "_pic_output_tensor_scaled", "_pic_output_tensor_rois", "_cm_check"):
        setattr(big, name, getattr(XgpuDecoder, name).__get__(big))
    big._rois_fit = XgpuDecoder._rois_fit
    with pytest.raises(ValueError):
        call(big, 0, (2731, 256), PQ_TO_SRGB, linear_light=True)
    with pytest.raises(ValueError):
        call(big, 0, (1024, 256), PQ_TO_SRGB, linear_light=True, rois=[(0, 2 * i, 16384, 2048) for i in range(3)])
    # what reaches the library
    seen = []
    dec._device_call = lambda name, out, *args: seen.append((name, args))
    out = torch.empty((3, *size), dtype=torch.uint8)
    outs = torch.empty((2, 3, *size), dtype=torch.uint8)
    import xevd_amd.decoder as decmod
    real = decmod._out_tensor
    decmod._out_tensor = lambda o, shape, dtype, dev: o
    try:
        call(dec, 0, size, PQ_TO_SRGB, out=out, linear_light=True, upsample="nearest", chroma_loc=3)
        call(dec, 0, size, PQ_TO_SRGB, out=out, linear_light=True)
        call(dec, 0, size, PQ_TO_SRGB, out=out)
        call(dec, 0, size, PQ_TO_SRGB, out=outs, rois=[(0, 0, 64, 64), (2, 2, 32, 32)], linear_light=True)
        call(dec, 0, size, PQ_TO_SRGB, out=outs, rois=[(0, 0, 64, 64), (2, 2, 32, 32)])
    finally:
        decmod._out_tensor = real
    assert [n for n, _ in seen] == ["xgpu_pic_output_device_scaled_lin", "xgpu_pic_output_device_scaled_lin", "xgpu_pic_output_device_scaled_cm",
                                    "xgpu_pic_output_device_rois_lin", "xgpu_pic_output_device_rois_cm"]
    fmts = [args[2]._obj for _, args in seen]
    assert [f.upsample for f in fmts] == [abi.UPSAMPLE_NEAREST] + [abi.UPSAMPLE_LINEAR] * 4
    assert fmts[0].chroma_loc == 3 and fmts[0].layout == abi.OUT_RGB_PLANAR


def _tables(lib, colour, bd):
    t = abi.colour_tables(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_colour_transform(**colour), bd)
    assert isinstance(t, dict), t
    return t


def _planes(w, h, bd, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, s, dtype=np.int64).astype(np.int16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_at_the_source_size_is_the_full_size_restatement(lib, bd):
    """destination size = source size: one tap of 16384 per axis scales by powers of two only, so scaled_lin_ref equals colour_cm_ref.convert for both upsampling
    modes, every chroma_loc and every dtype, float32 bits included"""
    w, h = 48, 36
    planes = _planes(w, h, bd, 60 + bd)
    tab = _tables(lib, PQ_TO_SRGB, bd)
    for loc, up, dtype in itertools.product(range(6), ("linear", "nearest"), (cr.U8, cr.U16, cr.F32)):
        got = slr.convert(planes, bd, (h, w), tab, matrix=9, chroma_loc=loc, upsample=up, dtype=dtype, lib=lib)
        exp = cmr.convert(planes, bd, tab, matrix=9, chroma_loc=loc, mode=up, dtype=dtype)
        assert got.dtype == exp.dtype and np.array_equal(got.view(np.uint32) if dtype == cr.F32 else got, exp.view(np.uint32) if dtype == cr.F32 else exp), (loc, up, dtype)


def test_restatement_of_a_flat_picture_and_of_stripes(lib):
    """a flat picture keeps the full-size value (the taps sum to 16384: powers of two again, as long as every partial sum is exact - a flat value times an integer
    below 2^14 is); stripes halved by the area filter give the mean of the two lights, brighter than the filtered code values'"""
    bd = 10
    tab = _tables(lib, PQ_TO_SRGB_PLAIN, bd)
    planes = [np.full(s, 512, np.int16) for s in ((32, 128), (16, 64), (16, 64))]
    planes[0][:, 0::2], planes[0][:, 1::2] = 64, 940
    lin = slr.convert(planes, bd, (16, 64), tab, filt=sr.AREA, dtype=cr.F32, lib=lib)
    enc = scm.convert(planes, bd, (16, 64), tab, filt=sr.AREA, dtype=cr.F32, lib=lib)
    assert (lin > enc).all()
    lt = np.asarray(tab["lin"], np.float32)
    cb, cw = (cr.ycbcr_to_rgb(np.int64(v), np.int64(512), np.int64(512), bd, 1, False, cr.U16).astype(np.int64) for v in (64, 940))
    want = slr.from_linear(((lt[cb] + lt[cw]).astype(np.float32) * np.float32(0.5)).astype(np.float32), tab, cr.F32, bd)
    assert (lin.view(np.uint32) == want.view(np.uint32).reshape(3, 1, 1)).all()
    img = slr.batch(planes, bd, (16, 16), [(0, 0, 128, 16)], tab, fit=slr.LETTERBOX, pad=(0.25, 0.5, 0.75), dtype=cr.F32, lib=lib)[0]
    assert (img[:, 0, :] == np.asarray((0.25, 0.5, 0.75), np.float32).reshape(3, 1)).all()      # the pad value, untransformed


# ---------------------------------------------------------------------------------------------- the float32 contract against float64 with exact taps
def exact_weights(n, N, filt):
    """the luma axis (subsampling 1, siting 0) without the 14-bit quantisation: [N][n] float64 from exact fractions, rows summing to 1"""
    r = Fraction(n, N)
    f = max(Fraction(1), r)
    m = np.zeros((N, n))
    for o in range(N):
        c = (o + Fraction(1, 2)) * r - Fraction(1, 2)
        reach = f if filt == sr.BILINEAR else (f + 1) / 2
        ws = {}
        for i in range(max(math.floor(c - reach) - 1, 0), min(math.ceil(c + reach) + 1, n - 1) + 1):
            w = 1 - abs(i - c) / f if filt == sr.BILINEAR else min(i + Fraction(1, 2), c + f / 2) - max(i - Fraction(1, 2), c - f / 2)
            if w > 0:
                ws[i] = w
        if not ws:
            ws = {min(max(math.floor(c + Fraction(1, 2)), 0), n - 1): Fraction(1)}
        total = sum(ws.values())
        for i, w in ws.items():
            m[o, i] = float(w / total)
    return m


def curve64(t, v):
    """a curve table as the piecewise-linear function it samples, in float64"""
    x = np.concatenate([[0.0], cmr.curve_x().astype(np.float64)])
    return np.interp(v, x, np.asarray(t, np.float64)[:len(x)])


def pipeline64(codes, size, tab, filt, dtype, bd):
    """section 8n in float64 with exact taps and the library's tables: -> [3][Hd][Wd], for the integer dtypes q * (2^D - 1) without the rounding"""
    hs, ws = codes.shape[1:]
    wy, wx = exact_weights(hs, size[0], filt), exact_weights(ws, size[1], filt)
    lin = np.asarray(tab["lin"], np.float64)
    e = [wy @ lin[codes[c]] @ wx.T for c in range(3)]
    mat = np.asarray(tab["matrix"], np.float64)
    p = [mat[r][0] * e[0] + mat[r][1] * e[1] + mat[r][2] * e[2] for r in range(3)] if tab["use_matrix"] else e
    if tab["tone"] is not None:
        lu = np.asarray(tab["luma"], np.float64)
        yl = np.clip(lu[0] * e[0] + lu[1] * e[1] + lu[2] * e[2], 0.0, 1.0)
        s = np.where(yl > 0, curve64(tab["tone"], yl) / np.where(yl > 0, yl, 1.0), 0.0)
    else:
        s = float(tab["scale"])
    q = [np.clip(c * s, 0.0, 1.0) for c in p]
    if tab["encode"] is not None:
        q = [curve64(tab["encode"], c) for c in q]
    m = float((1 << cr.out_depth(dtype, bd)) - 1) if dtype in (cr.U8, cr.U16) else 1.0
    return np.stack(q) * m


# The maxima this test measures on the pictures below, per output dtype and coding depth: |float32 contract - float64 with exact taps|, in code values for the
# integer dtypes (INTEGRATION.md section 8n quotes them).  They are the 14-bit quantisation of the taps far more than float32's rounding: linear light spans four
# decades, so a tap that is off by 2^-15 beside a highlight moves a dark neighbour, and the tone curve's gain and the encode curve's slope near black multiply it -
# every maximum is the PQ -> sRGB transform with the tone curve.  Integers: the bound is the maximum rounded up to a whole code value; F32: twice the maximum.
MEASURED = {(cr.U8, 8): 0.765, (cr.U8, 10): 0.615, (cr.U8, 12): 0.626, (cr.U16, 8): 0.765, (cr.U16, 10): 0.929, (cr.U16, 12): 5.886,
            (cr.F32, 8): 2.25e-3, (cr.F32, 10): 6.86e-4, (cr.F32, 12): 1.36e-3}
BOUND = {k: (2 * v if k[0] == cr.F32 else float(math.ceil(v))) for k, v in MEASURED.items()}


def _stripes():
    planes = [np.full(s, 512, np.int16) for s in ((32, 128), (16, 64), (16, 64))]
    planes[0][:, 0::2], planes[0][:, 1::2] = 64, 940
    return planes, 10


def test_float32_contract_against_float64_with_exact_taps(lib, capsys):
    worst = {k: 0.0 for k in MEASURED}
    pictures = [golden_planes(c) for c in ("base_p_8b", "base_p_10b", "base_p_12b")] + [_stripes()]
    for (planes, bd), (name, colour) in itertools.product(pictures, (("pq_srgb_tone", PQ_TO_SRGB), ("pq_srgb", PQ_TO_SRGB_PLAIN), ("hlg_linear", HLG_TO_LINEAR),
                                                                      ("bt709_srgb", BT709_TO_SRGB))):
        tab = _tables(lib, colour, bd)
        codes = slr.rgb_codes(planes, bd, matrix=9)
        h, w = planes[0].shape
        for size, filt in (((h // 2, w // 2), sr.AREA), ((h // 3 + 1, w // 3 + 2), sr.BILINEAR), ((h + 9, w + 14), sr.BILINEAR)):
            v = slr.filtered_linear(codes, size, tab, filt, lib)
            for dtype in (cr.U8, cr.U16, cr.F32):
                d = float(np.abs(slr.finish(v, bd, tab, dtype).astype(np.float64) - pipeline64(codes, size, tab, filt, dtype, bd)).max())
                worst[dtype, bd] = max(worst[dtype, bd], d)
    with capsys.disabled():
        print("\nscaled_lin: float32 contract against float64 with exact taps, max |diff| per (dtype, depth): " +
              ", ".join(f"{k}: {v:.4g}" for k, v in sorted(worst.items())))
    for k, v in worst.items():
        assert v <= BOUND[k], (k, v, BOUND[k])
