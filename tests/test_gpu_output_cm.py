"""GPU suite for the colour-managed RGB output (xgpu_pic_output_device_cm / pic_output_tensor(colour=...) / StreamDecoder.pictures(to=...)): the bytes
the device writes against tests/colour_cm_ref.py fed with the library's own tables (xgpu_colour_tables).  Every dtype is compared bit for bit: the
contract is built from table lookups and float32 operations rounded one by one, so there is one answer."""
import ctypes as C
import itertools

import numpy as np
import pytest

import colour_cm_ref as cm
import colour_ref as cr
from test_gpu_output_device import DT_NAMES, _intra_stream, golden_planes, open_picture, torch_dtype
from xevd_amd import abi

pytestmark = pytest.mark.gpu

PQ_TO_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
HLG_TO_LINEAR = dict(src_primaries=9, src_transfer=18, dst_primaries=1, dst_transfer=8)
BT709_TO_LINEAR = dict(src_primaries=1, src_transfer=1, dst_primaries=1, dst_transfer=8)
SRGB_TO_PQ = dict(src_primaries=1, src_transfer=13, dst_primaries=9, dst_transfer=16, linear_scale=0.01)
TRANSFORMS = {"pq2020_srgb709_tone": PQ_TO_SRGB, "hlg2020_linear709": HLG_TO_LINEAR, "bt709_linear709": BT709_TO_LINEAR, "srgb709_pq2020": SRGB_TO_PQ}


def tables(dec, colour, bd):
    fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16)
    t = abi.colour_tables(dec.lib, fmt, abi.make_colour_transform(**colour), bd)
    assert isinstance(t, dict), t
    return t


def check_bits(t, exp, code, channels_last=False, bgr=False, what=""):
    """tensor t against the restatement exp [3][H][W] (float32 before f16 / bf16 rounding): equal bit patterns"""
    import torch
    torch.cuda.synchronize()
    if bgr:
        exp = exp[::-1]
    if channels_last:
        exp = np.moveaxis(exp, 0, -1)
    exp = np.ascontiguousarray(exp)
    got = t.cpu()
    assert tuple(got.shape) == exp.shape, what
    if code == abi.OUT_U8:
        ok = np.array_equal(got.numpy(), exp)
    elif code == abi.OUT_U16:
        ok = np.array_equal(got.numpy().view(np.uint16), exp)
    elif code == abi.OUT_F32:
        ok = np.array_equal(got.numpy().view(np.uint32), exp.view(np.uint32))
    else:
        ref = cr.to_f16_bits(exp) if code == abi.OUT_F16 else cr.to_bf16_bits(exp)
        ok = np.array_equal(got.view(torch.int16).numpy().view(np.uint16), ref)
    assert ok, what


@pytest.mark.parametrize("name", sorted(TRANSFORMS))
@pytest.mark.parametrize("case", ["base_p_10b", "base_p_12b", "base_p_8b"])
def test_bit_exact_every_dtype_layout_and_mode(case, name):
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    colour = TRANSFORMS[name]
    try:
        tab = tables(dec, colour, bd)
        for code, mode, cl in itertools.product(DT_NAMES, ("linear", "nearest"), (False, True)):
            exp = cm.convert(planes, bd, tab, matrix=9, mode=mode, dtype=code)
            t = dec.pic_output_tensor(pic, channels_last=cl, dtype=torch_dtype(code), upsample=mode, matrix=9, colour=colour)
            check_bits(t, exp, code, cl, what=(case, name, code, mode, cl))
    finally:
        dec.close()


def test_crop_tail_columns_row_pitch_and_bgr():
    """a cropped width that is not a multiple of 8 (the element-store tail), rows padded by the caller's strides, B, G, R order"""
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    try:
        tab = tables(dec, PQ_TO_SRGB, bd)
        for crop in ((2, 4, 2, 0), (6, 0, 4, 6)):
            assert (w - crop[0] - crop[1]) % 8
            for code, cl, mode in itertools.product((abi.OUT_U8, abi.OUT_F16, abi.OUT_F32), (False, True), ("linear", "nearest")):
                t = dec.pic_output_tensor(pic, channels_last=cl, dtype=torch_dtype(code), upsample=mode, chroma_loc=3, crop=crop, bgr=cl, colour=PQ_TO_SRGB)
                check_bits(t, cm.convert(planes, bd, tab, chroma_loc=3, mode=mode, dtype=code, crop=crop), code, cl, bgr=cl, what=(crop, code, cl, mode))
        for code, cl in itertools.product((abi.OUT_U8, abi.OUT_U16), (False, True)):      # an odd row pitch: no vector stores, the padding untouched
            pitch = (3 * w if cl else w) + 7
            buf = torch.full((h, pitch) if cl else (3, h, pitch), 77, dtype=torch_dtype(code), device="cuda:0")
            out = buf[:, :3 * w].unflatten(1, (w, 3)) if cl else buf[:, :, :w]
            dec.pic_output_tensor(pic, channels_last=cl, dtype=torch_dtype(code), out=out, colour=PQ_TO_SRGB)
            check_bits(out, cm.convert(planes, bd, tab, dtype=code), code, cl, what=("pitch", code, cl))
            pad = buf[:, 3 * w:] if cl else buf[:, :, w:]
            assert (pad.cpu().numpy() == 77).all()
    finally:
        dec.close()


def test_dra_picture():
    import os

    import golden_io
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    dec, pic = open_picture(planes, 10)
    try:
        tab = tables(dec, PQ_TO_SRGB, 10)
        luts = d["three_ranges_idx58_luts"]
        for code, crop in ((abi.OUT_U8, (0, 0, 0, 0)), (abi.OUT_U16, (2, 0, 0, 2)), (abi.OUT_F32, (0, 6, 2, 0))):
            t = dec.pic_output_tensor(pic, dtype=torch_dtype(code), crop=crop, dra=luts, matrix=9, colour=PQ_TO_SRGB)
            check_bits(t, cm.convert(planes, 10, tab, matrix=9, dtype=code, crop=crop, dra=luts), code, what=(code, crop))
    finally:
        dec.close()


def test_null_transform_is_the_plain_call():
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    try:
        for layout, code in ((abi.OUT_RGB_PLANAR, abi.OUT_U8), (abi.OUT_RGB_INTERLEAVED, abi.OUT_F16), (abi.OUT_NV12, abi.OUT_U16), (abi.OUT_YUV444_PLANAR, abi.OUT_F32)):
            fmt = abi.make_output_format(layout, code)
            need = dec.lib.xgpu_pic_output_device_size(dec.ctx, C.byref(fmt))
            a = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda:0")
            b = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda:0")
            sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert dec.lib.xgpu_pic_output_device(dec.ctx, pic, None, C.byref(fmt), C.c_void_p(a.data_ptr()), need, sh) == 0
            assert dec.lib.xgpu_pic_output_device_cm(dec.ctx, pic, None, C.byref(fmt), None, C.c_void_p(b.data_ptr()), need, sh) == 0
            torch.cuda.synchronize()
            dec.sync()
            assert torch.equal(a, b), (layout, code)
        # and the plain call still is what colour_ref says
        t = dec.pic_output_tensor(pic, dtype=torch.int16)
        assert np.array_equal(t.cpu().numpy().view(np.uint16), cr.convert(planes, bd, dtype=cr.U16))
    finally:
        dec.close()


def test_refusals_launch_nothing():
    import torch
    planes, bd = golden_planes("base_p_8b")
    dec, pic = open_picture(planes, bd)
    lib = dec.lib
    try:
        rgb = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8)
        nv12 = abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)
        need = max(lib.xgpu_pic_output_device_size(dec.ctx, C.byref(rgb)), lib.xgpu_pic_output_device_size(dec.ctx, C.byref(nv12)))
        t = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda:0")
        sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for fmt, colour, rc in ((rgb, dict(PQ_TO_SRGB, src_transfer=17), -104), (rgb, dict(PQ_TO_SRGB, dst_transfer=2), -104),
                                (rgb, dict(PQ_TO_SRGB, src_primaries=11), -104), (rgb, dict(PQ_TO_SRGB, dst_primaries=11), -104),
                                (rgb, dict(PQ_TO_SRGB, dst_transfer=18), -104),                # the tone curve into an HLG destination
                                (rgb, dict(PQ_TO_SRGB, src_peak=-1.0), -101), (rgb, dict(PQ_TO_SRGB, dst_peak=float("inf")), -101),
                                (rgb, dict(HLG_TO_LINEAR, linear_scale=float("nan")), -101),
                                (nv12, PQ_TO_SRGB, -101)):
            c = abi.make_colour_transform(**colour)
            assert lib.xgpu_pic_output_device_cm(dec.ctx, pic, None, C.byref(fmt), C.byref(c), C.c_void_p(t.data_ptr()), need, sh) == rc, colour
            assert b"pic_output_device_cm" in lib.xgpu_last_error(dec.ctx)
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all()
        with pytest.raises(ValueError):
            dec.pic_output_tensor(pic, layout="nv12", colour=PQ_TO_SRGB)
    finally:
        dec.close()


def test_a_refused_call_leaves_no_tables_behind():
    """a call that is refused after its tables were made (DRA tables with a missing plane; DRA on a 12-bit context) must not leave the table cache naming
    that transform: the same transform right after it, and after another transform was in use, is bit-exact"""
    import torch
    for case in ("base_p_10b", "base_p_12b"):
        planes, bd = golden_planes(case)
        dec, pic = open_picture(planes, bd)
        try:
            fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16)
            need = dec.lib.xgpu_pic_output_device_size(dec.ctx, C.byref(fmt))
            dst = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda:0")
            sh = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            luts = np.zeros((3, 1024), np.int32)
            bad = abi.DraLuts()
            bad.luma_inv_scale_lut = luts[0].ctypes.data
            bad.chroma_inv_scale_lut[0] = luts[1].ctypes.data      # [1] stays NULL; at 12 bit DRA is refused whatever the tables
            for first in (None, "hlg2020_linear709"):               # the cache empty / holding another transform's tables
                if first:
                    dec.pic_output_tensor(pic, dtype=torch.int16, colour=TRANSFORMS[first])
                for name in ("pq2020_srgb709_tone", "srgb709_pq2020"):
                    c = abi.make_colour_transform(**TRANSFORMS[name])
                    rc = dec.lib.xgpu_pic_output_device_cm(dec.ctx, pic, C.byref(bad), C.byref(fmt), C.byref(c), C.c_void_p(dst.data_ptr()), need, sh)
                    assert rc == -101, (case, name)
                    torch.cuda.synchronize()
                    dec.sync()
                    assert (dst.cpu().numpy() == 0x5A).all()
                    t = dec.pic_output_tensor(pic, dtype=torch.int16, colour=TRANSFORMS[name])
                    check_bits(t, cm.convert(planes, bd, tables(dec, TRANSFORMS[name], bd), dtype=cr.U16), abi.OUT_U16, what=(case, first, name))
                    if first:      # and the transform that was in use before the refusal still gets its own tables
                        t = dec.pic_output_tensor(pic, dtype=torch.int16, colour=TRANSFORMS[first])
                        check_bits(t, cm.convert(planes, bd, tables(dec, TRANSFORMS[first], bd), dtype=cr.U16), abi.OUT_U16, what=(case, first, "again"))
        finally:
            dec.close()


def test_side_stream_and_two_transforms_back_to_back():
    """queued on a torch side stream without synchronisation in between; the second transform must not be served the first one's tables, nor the first
    one's kernel the second one's"""
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    try:
        order = ["pq2020_srgb709_tone", "hlg2020_linear709", "pq2020_srgb709_tone", "pq2020_srgb709_tone", "srgb709_pq2020", "bt709_linear709"]
        exp = {n: cm.convert(planes, bd, tables(dec, TRANSFORMS[n], bd), dtype=cr.U16) for n in set(order)}
        s = torch.cuda.Stream(device=0)
        got = []
        with torch.cuda.stream(s):
            for n in order:
                got.append(dec.pic_output_tensor(pic, dtype=torch.int16, colour=TRANSFORMS[n]))
        s.synchronize()
        for n, t in zip(order, got):
            assert np.array_equal(t.cpu().numpy().view(np.uint16), exp[n]), n
    finally:
        dec.close()


def test_stream_decoder_to_srgb():
    """a written 10-bit stream whose VUI says BT.2020 / PQ / BT.2020 NCL: pictures(tensor=..., to="srgb") is the direct call with that source"""
    from xevd_amd.decoder import XgpuDecoder
    from xevd_amd.player import StreamDecoder
    data = _intra_stream(128, 96, 10, 2, {"colour": (9, 16, 9)})
    ref = [planes for _, planes in StreamDecoder(data).pictures()]
    got = list(StreamDecoder(data).pictures(tensor={}, to="srgb"))
    assert len(got) == len(ref) == 2
    with XgpuDecoder(128, 96, 10, device=0, max_pics=2) as dec:
        tab = tables(dec, PQ_TO_SRGB, 10)
        pic = dec.pic_alloc()
        for (p, t), planes in zip(got, ref):
            assert (p["colour"]["colour_primaries"], p["colour"]["transfer_characteristics"], p["colour"]["matrix_coefficients"]) == (9, 16, 9)
            dec.pic_upload(pic, planes)
            direct = dec.pic_output_tensor(pic, matrix=9, colour=PQ_TO_SRGB)
            assert np.array_equal(t.cpu().numpy(), direct.cpu().numpy())
            check_bits(t, cm.convert(planes, 10, tab, matrix=9), abi.OUT_U8)
