"""CPU suite for the colour-managed scaled output: the three exported symbols, xgpu_output_scaled_cm_check's codes in their order, the
Python refusals that need no context, and the restatement (tests/scaled_cm_ref.py) against the restatements it is made of.  No GPU: host-only functions."""
import ctypes as C
import itertools

import numpy as np
import pytest

import colour_cm_ref as cmr
import colour_ref as cr
import scale_ref as sr
import scaled_cm_ref as scm
import stub_decoder
from xevd_amd import abi

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -101, -104
W, H, BD = 320, 200, 10
PQ_TO_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
BT709_TO_LINEAR = dict(src_primaries=1, src_transfer=1, dst_primaries=1, dst_transfer=8)


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def test_library_exports_the_three_symbols():
    raw = C.CDLL(abi.LIB_PATH)
    for name in ("xgpu_pic_output_device_scaled_cm", "xgpu_pic_output_device_rois_cm", "xgpu_output_scaled_cm_check"):
        assert hasattr(raw, name), name
        assert name in abi.exported_names(), name


def _check(lib, fmt, sc, cm, w=W, h=H, bd=BD):
    return lib.xgpu_output_scaled_cm_check(C.byref(fmt), C.byref(sc), C.byref(cm) if cm is not None else None, w, h, bd)


def test_check_codes_and_their_order(lib):
    rgb = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32)
    sc = abi.make_scale_params(224, 224, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25))
    good = abi.make_colour_transform(**PQ_TO_SRGB)
    assert _check(lib, rgb, sc, good) == 0
    for bd in (8, 10, 12):
        assert _check(lib, rgb, sc, good, bd=bd) == 0
    # the transform's own refusals: a transfer or primaries outside the lists, a negative peak or scale
    assert _check(lib, rgb, sc, abi.make_colour_transform(**dict(PQ_TO_SRGB, src_transfer=17))) == ERR_UNSUPPORTED
    assert _check(lib, rgb, sc, abi.make_colour_transform(**dict(PQ_TO_SRGB, dst_primaries=22))) == ERR_UNSUPPORTED
    assert _check(lib, rgb, sc, abi.make_colour_transform(**dict(PQ_TO_SRGB, src_peak=-1.0))) == ERR_INVALID_ARGUMENT
    assert _check(lib, rgb, sc, abi.make_colour_transform(**dict(BT709_TO_LINEAR, linear_scale=-2.0))) == ERR_INVALID_ARGUMENT
    # a layout that is not RGB, with a transform
    yuv = abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_F32)
    assert _check(lib, yuv, sc, good) == ERR_INVALID_ARGUMENT
    assert _check(lib, yuv, sc, None) == 0
    # the order: the plain call's refusal wins over the layout's and the transform's; the layout's over the transform's
    bad_cm = abi.make_colour_transform(**dict(PQ_TO_SRGB, src_transfer=17))
    tiny = abi.make_scale_params(2, 224)      # below 1 / 64 of the width: the plain call says UNSUPPORTED
    assert _check(lib, yuv, tiny, good, w=640) == ERR_UNSUPPORTED
    int_norm = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8)
    assert _check(lib, int_norm, sc, bad_cm) == ERR_INVALID_ARGUMENT      # the normalise with an integer dtype, not the transfer's UNSUPPORTED
    assert _check(lib, rgb, abi.make_scale_params(1, 224), good) == ERR_UNSUPPORTED
    assert _check(lib, rgb, tiny, abi.make_colour_transform(**dict(PQ_TO_SRGB, src_peak=-1.0)), w=640) == ERR_UNSUPPORTED
    assert _check(lib, yuv, sc, bad_cm) == ERR_INVALID_ARGUMENT           # the layout, not the transfer
    bad_matrix = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, matrix=2)
    assert _check(lib, bad_matrix, sc, abi.make_colour_transform(**dict(PQ_TO_SRGB, src_peak=-1.0))) == ERR_UNSUPPORTED      # the plain call's code for the matrix


def test_null_transform_is_the_plain_check(lib):
    formats = [abi.make_output_format(l, d, matrix=m, crop=c) for l, d, m, c in itertools.product(
        (abi.OUT_RGB_PLANAR, abi.OUT_YUV444_INTERLEAVED, abi.OUT_NV12), (abi.OUT_U8, abi.OUT_F16), (1, 2), ((0, 0, 0, 0), (2, 0, 0, 4), (1, 0, 0, 0)))]
    scales = [abi.make_scale_params(64, 48), abi.make_scale_params(2, 48), abi.make_scale_params(64, 48, mean=(0, 0, 0)), abi.make_scale_params(64, 48, filter=7),
              abi.make_scale_params(W * 8 + 2, 48)]
    seen = set()
    for fmt, sc in itertools.product(formats, scales):
        plain = lib.xgpu_output_scaled_check(C.byref(fmt), C.byref(sc), W, H, BD)
        assert _check(lib, fmt, sc, None) == plain
        seen.add(plain)
    assert seen == {0, ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED}


def test_python_refusals_come_before_any_library_call(lib):
    """pic_output_scaled_cm raises ValueError for what the arguments alone decide - on a decoder object without a context, so no call into a context can have run"""
    import torch
    from xevd_amd.decoder import XgpuDecoder
    dec = stub_decoder.XgpuDecoder(W, H, BD)
    dec.lib, dec.sp, dec.ctx = lib, abi.make_seq_params(W, H, BD), None
    for name in ("_scaled_setup", "_pic_output_tensor_scaled", "_pic_output_tensor_rois", "_cm_check"):      # the real checks in front of the stub's do-nothing surface
        setattr(dec, name, getattr(XgpuDecoder, name).__get__(dec))
    dec._rois_fit = XgpuDecoder._rois_fit
    call = XgpuDecoder.pic_output_scaled_cm
    size = (48, 64)
    for bad in (dict(colour=PQ_TO_SRGB, layout="yuv444"), dict(colour=PQ_TO_SRGB, dtype=torch.uint8, mean=(0.5, 0.5, 0.5)),
                dict(colour=PQ_TO_SRGB, dtype=torch.int16, std=(0.5, 0.5, 0.5)), dict(colour=None), dict(colour=PQ_TO_SRGB, filter="lanczos"),
                dict(colour=PQ_TO_SRGB, fit="letterbox"), dict(colour=PQ_TO_SRGB, pad=0.5), dict(colour=PQ_TO_SRGB, rois=[(0, 0, 64, 64)], fit="pad"),
                dict(colour=dict(PQ_TO_SRGB, src_transfer=17)), dict(colour=dict(PQ_TO_SRGB, dst_peak=-5.0)),
                dict(colour=dict(PQ_TO_SRGB, src_transfer=17), rois=[(0, 0, 64, 64)]), dict(colour=PQ_TO_SRGB, rois=[(1, 0, 64, 64)]),
                dict(colour=PQ_TO_SRGB, crop=(1, 0, 0, 0))):
        with pytest.raises(ValueError):
            call(dec, 0, size, **bad)
    with pytest.raises(ValueError):
        call(dec, 0, (1, 64), PQ_TO_SRGB)


def _planes(w, h, bd, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, s, dtype=np.int64).astype(np.int16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]


def _tables(lib, colour, bd):
    t = abi.colour_tables(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_colour_transform(**colour), bd)
    assert isinstance(t, dict), t
    return t


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_at_the_source_size_is_the_full_size_restatement(lib, bd):
    """destination size = source size: the taps are the linear upsampling's, so scaled_cm_ref equals colour_cm_ref.convert(mode="linear") for every chroma_loc
    and the dtypes that are exact in integers (U8, U16) or one table value (F32)"""
    w, h = 48, 36
    planes = _planes(w, h, bd, 40 + bd)
    tab = _tables(lib, PQ_TO_SRGB, bd)
    for loc, dtype in itertools.product(range(6), (cr.U8, cr.U16, cr.F32)):
        got = scm.convert(planes, bd, (h, w), tab, matrix=9, chroma_loc=loc, dtype=dtype, lib=lib)
        exp = cmr.convert(planes, bd, tab, matrix=9, chroma_loc=loc, mode="linear", dtype=dtype)
        assert got.dtype == exp.dtype and np.array_equal(got.view(np.uint32) if dtype == cr.F32 else got, exp.view(np.uint32) if dtype == cr.F32 else exp), (loc, dtype)


def test_restatement_of_a_flat_picture_is_one_flat_value(lib):
    bd = 10
    tab = _tables(lib, PQ_TO_SRGB, bd)
    for code in (0, 1 << (bd - 1), (1 << bd) - 1):
        planes = [np.full(s, code, np.int16) for s in ((40, 64), (20, 32), (20, 32))]
        one = cmr.convert(planes, bd, tab, dtype=cr.F32)[:, 0, 0]
        for size, filt in (((7, 9), sr.BILINEAR), ((60, 100), sr.BILINEAR), ((5, 8), sr.AREA)):
            got = scm.convert(planes, bd, size, tab, filt=filt, dtype=cr.F32, lib=lib)
            assert got.shape == (3, *size) and (got == one.reshape(3, 1, 1)).all(), (code, size)
        img = scm.batch(planes, bd, (16, 16), [(0, 0, 64, 16)], tab, fit=scm.LETTERBOX, pad=(0.25, 0.5, 0.75), dtype=cr.F32, lib=lib)[0]
        assert (img[:, 0, :] == np.asarray((0.25, 0.5, 0.75), np.float32).reshape(3, 1)).all()      # the pad value, untransformed
        assert (img[:, 8, :] == one.reshape(3, 1)).all()
