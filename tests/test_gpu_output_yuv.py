"""GPU suite for the video-surface layouts of xgpu_pic_output_device / XgpuDecoder.pic_output_tensor / StreamDecoder: NV12, P016 (P010, P012) and
Y'CbCr 4:4:4 written by the device into torch tensors.  NV12 against the host output path (whose bytes the reference-made goldens pin) re-interleaved;
P016 and YUV444 against the numpy restatement tests/yuv_ref.py applied to the downloaded planes.  Integers and f32 bit-exact; f16 / bf16 within one
unit in the last place of the restatement's f32 rounded."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_ref as cr
import golden_io
import yuv_ref as yr
from xevd_amd import abi, stream, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_NAMES = {abi.OUT_U8: "uint8", abi.OUT_U16: "int16", abi.OUT_F16: "float16", abi.OUT_BF16: "bfloat16", abi.OUT_F32: "float32"}
CASES = ["base_p_8b", "base_p_10b", "base_p_12b"]


def torch_dtype(code):
    import torch
    return getattr(torch, DT_NAMES[code])


def golden_planes(name):
    """the decoded picture of a committed golden case: [Y, U, V] of the active area, bit depth"""
    d = np.load(os.path.join(golden_io.GOLDEN, f"pic_{name}.npz"))
    w, h, bd = (int(v) for v in d["params"][:3])
    pl, pc = abi.PAD_L, abi.PAD_C
    return [d["out_0"][pl:pl + h, pl:pl + w], d["out_1"][pc:pc + h // 2, pc:pc + w // 2], d["out_2"][pc:pc + h // 2, pc:pc + w // 2]], bd


def open_picture(planes, bd):
    from xevd_amd.decoder import XgpuDecoder
    h, w = planes[0].shape
    dec = XgpuDecoder(w, h, bd, device=0, max_pics=4)
    pic = dec.pic_alloc()
    dec.pic_upload(pic, planes)
    assert all(np.array_equal(a, b) for a, b in zip(dec.pic_download(pic), planes))
    return dec, pic


def host(t):
    """an integer tensor written by the device as a numpy array of unsigned elements"""
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def check444(t, exp, code, channels_last=False, what=""):
    """tensor t against the restatement exp [3][H][W] (float32 before rounding for the float dtypes)"""
    import torch
    torch.cuda.synchronize()
    if channels_last:
        exp = np.moveaxis(exp, 0, -1)
    exp = np.ascontiguousarray(exp)
    got = t.cpu()
    assert tuple(got.shape) == exp.shape, what
    if code == abi.OUT_U8:
        assert np.array_equal(got.numpy(), exp), what
    elif code == abi.OUT_U16:
        assert np.array_equal(got.numpy().view(np.uint16), exp), what
    elif code == abi.OUT_F32:
        g = got.numpy()
        diff = g.view(np.uint32) != exp.view(np.uint32)
        print(f"f32 {what}: {int(diff.sum())} of {diff.size} elements differ, max |d| = {float(np.abs(g.astype(np.float64) - exp).max()):.3g}")
        assert not diff.any(), what      # one correctly rounded float32 multiplication: the same bits
    else:
        bits = got.view(torch.int16).numpy().view(np.uint16).astype(np.int64)
        ref = (cr.to_f16_bits(exp) if code == abi.OUT_F16 else cr.to_bf16_bits(exp)).astype(np.int64)
        # sign-magnitude bit patterns: compare on a line where neighbouring values are one apart on both sides of zero
        d = np.abs(np.where(bits & 0x8000, -(bits & 0x7FFF), bits & 0x7FFF) - np.where(ref & 0x8000, -(ref & 0x7FFF), ref & 0x7FFF)).max()
        print(f"{DT_NAMES[code]} {what}: max distance {int(d)} units in the last place")
        assert d <= 1, what


@pytest.mark.parametrize("case", CASES)
def test_nv12_equals_the_host_output_reinterleaved(case):
    import torch
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    hh, ww = planes[0].shape
    try:
        for crop in ((0, 0, 0, 0), (2, 4, 2, 6)):
            w, h = ww - crop[0] - crop[1], hh - crop[2] - crop[3]
            for dt, d in ((torch.uint8, 8),) + (((torch.int16, bd),) if bd > 8 else ()):
                flat = dec.pic_output(pic, d, crop)
                exp = yr.interleave_420p(flat if d == 8 else flat.view("<u2"), w, h)
                assert np.array_equal(exp, yr.nv12(planes, bd, d, crop))      # the restatement agrees with the host path
                t = dec.pic_output_tensor(pic, layout="nv12", dtype=dt, crop=crop)
                assert tuple(t.shape) == (h * 3 // 2, w) and t.dtype == dt
                assert np.array_equal(host(t), exp), (case, crop, d, "tight")
                if d > 8:      # out_bit_depth spelled out is the same format
                    assert np.array_equal(host(dec.pic_output_tensor(pic, layout="nv12", dtype=dt, crop=crop, out_bit_depth=d)), exp)
                # padded rows: a view into a wider tensor (16-byte aligned pitch or not), the padding untouched
                for pad, off in ((24, 8), (16, 16), (3, 1)):
                    big = torch.full((h * 3 // 2, w + pad), 7, dtype=dt, device="cuda:0")
                    view = big[:, off:off + w]
                    assert dec.pic_output_tensor(pic, layout="nv12", dtype=dt, crop=crop, out=view) is view
                    b = host(big)
                    assert np.array_equal(b[:, off:off + w], exp), (case, crop, d, pad, off)
                    assert (b[:, :off] == 7).all() and (b[:, off + w:] == 7).all()
    finally:
        dec.close()


def test_nv12_converts_to_other_depths():
    """NV12 U16 at depths below and above the coding depth: the samples of YUV420P at that depth"""
    import torch
    for case in CASES:
        planes, bd = golden_planes(case)
        dec, pic = open_picture(planes, bd)
        h, w = planes[0].shape
        try:
            for d in (9, 10, 12, 16):
                t = dec.pic_output_tensor(pic, layout="nv12", dtype=torch.int16, out_bit_depth=d)
                assert np.array_equal(host(t), yr.interleave_420p(dec.pic_output(pic, d).view("<u2"), w, h)), (case, d)
        finally:
            dec.close()


def test_nv12_of_the_dra_goldens():
    """the bytes the reference application wrote for the DRA pictures (8-bit output), re-interleaved"""
    import torch
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    h, w = planes[0].shape
    dec, pic = open_picture(planes, 10)
    try:
        for name in ("one_range_idx30", "three_ranges_idx58", "five_ranges_idx40"):
            luts = d[f"{name}_luts"]
            t = dec.pic_output_tensor(pic, layout="nv12", dra=luts)
            assert np.array_equal(host(t), yr.interleave_420p(d[f"{name}_out8"], w, h)), name
            t = dec.pic_output_tensor(pic, layout="nv12", dtype=torch.int16, dra=luts)
            assert np.array_equal(host(t), yr.interleave_420p(d[f"{name}_out10"].view("<u2"), w, h)), name
            t = dec.pic_output_tensor(pic, layout="p016", dra=luts, crop=(2, 0, 0, 2))
            assert np.array_equal(host(t), yr.p016(planes, 10, 10, (2, 0, 0, 2), dra=luts)), name
    finally:
        dec.close()


def test_p016():
    import torch
    for case, depths in (("base_p_8b", (0, 8, 10, 16)), ("base_p_10b", (0, 10, 12)), ("base_p_12b", (0, 12, 10, 8))):
        planes, bd = golden_planes(case)
        dec, pic = open_picture(planes, bd)
        hh, ww = planes[0].shape
        try:
            for obd, crop in itertools.product(depths, ((0, 0, 0, 0), (2, 4, 2, 6))):
                d = obd or bd
                w, h = ww - crop[0] - crop[1], hh - crop[2] - crop[3]
                exp = yr.p016(planes, bd, d, crop)
                t = dec.pic_output_tensor(pic, layout="p016", out_bit_depth=obd, crop=crop)
                assert t.dtype == torch.int16 and tuple(t.shape) == (h * 3 // 2, w)
                got = host(t)
                assert np.array_equal(got, exp), (case, obd, crop)
                assert not (got & ((1 << (16 - d)) - 1)).any()      # the low 16 - D bits are zero
                flat = dec.pic_output(pic, d, crop)
                assert np.array_equal(got >> (16 - d), yr.interleave_420p(flat if d == 8 else flat.view("<u2"), w, h))
                big = torch.full((h * 3 // 2, w + 5), 7, dtype=torch.int16, device="cuda:0")
                dec.pic_output_tensor(pic, layout="p016", out_bit_depth=obd, crop=crop, out=big[:, 2:2 + w])
                b = host(big)
                assert np.array_equal(b[:, 2:2 + w], exp) and (b[:, :2] == 7).all() and (b[:, 2 + w:] == 7).all()
        finally:
            dec.close()


@pytest.mark.parametrize("case", CASES)
def test_yuv444_every_dtype_layout_and_mode(case):
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    try:
        for code, mode, cl in itertools.product(DT_NAMES, ("linear", "nearest"), (False, True)):
            exp = yr.yuv444(planes, bd, False, 0, mode, code)
            t = dec.pic_output_tensor(pic, layout="yuv444", channels_last=cl, dtype=torch_dtype(code), upsample=mode)
            check444(t, exp, code, cl, what=(case, code, mode, cl))
        t = dec.pic_output_tensor(pic, layout="yuv444", dtype=torch_dtype(abi.OUT_U16), out_bit_depth=bd, matrix=2)      # no matrix is read
        check444(t, yr.yuv444(planes, bd, dtype=abi.OUT_U16), abi.OUT_U16)
    finally:
        dec.close()


@pytest.mark.parametrize("case", CASES)
def test_yuv444_chroma_locations_and_ranges(case):
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    try:
        for loc, fr in itertools.product(range(6), (False, True)):
            for code in (abi.OUT_U8, abi.OUT_U16, abi.OUT_F32, abi.OUT_F16):
                t = dec.pic_output_tensor(pic, layout="yuv444", dtype=torch_dtype(code), full_range=fr, chroma_loc=loc)
                check444(t, yr.yuv444(planes, bd, fr, loc, "linear", code), code, what=(loc, fr, code))
    finally:
        dec.close()


def test_yuv444_floats_clip_at_the_bounds():
    """samples outside the nominal range (limited range leaves room for them): E'Y clipped to [0, 1], E'Cb / E'Cr to [-0.5, 0.5], bit-exact"""
    import torch
    bd, w, h = 10, 64, 16
    y = np.tile(np.array([0, 3, 63, 64, 65, 939, 940, 941, 1023, 512, 300, 700, 64, 940, 1, 1022], np.int16), (h, w // 16))
    u = np.tile(np.array([0, 63, 64, 65, 511, 512, 513, 959, 960, 961, 1023, 1, 2, 1000, 20, 40], np.int16), (h // 2, w // 32))
    v = u[:, ::-1].copy()
    dec, pic = open_picture([y, u, v], bd)
    try:
        for fr, mode in itertools.product((False, True), ("nearest", "linear")):
            exp = yr.yuv444([y, u, v], bd, fr, 0, mode, abi.OUT_F32)
            if not fr:
                assert exp[0].min() == 0 and exp[0].max() == 1 and exp[1].min() == -0.5 and exp[1].max() == 0.5
            check444(dec.pic_output_tensor(pic, layout="yuv444", dtype=torch.float32, full_range=fr, upsample=mode), exp, abi.OUT_F32, what=(fr, mode))
            check444(dec.pic_output_tensor(pic, layout="yuv444", dtype=torch.bfloat16, full_range=fr, upsample=mode), exp, abi.OUT_BF16, what=(fr, mode))
    finally:
        dec.close()


def test_yuv444_crop_with_odd_chroma_widths_and_padded_rows():
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    try:
        for crop in ((2, 4, 2, 0), (0, 2, 0, 2), (6, 0, 4, 6), (2, 2, 2, 2)):
            for code, cl, mode in itertools.product((abi.OUT_U8, abi.OUT_U16, abi.OUT_F32), (False, True), ("linear", "nearest")):
                t = dec.pic_output_tensor(pic, layout="yuv444", channels_last=cl, dtype=torch_dtype(code), upsample=mode, chroma_loc=3, crop=crop)
                check444(t, yr.yuv444(planes, bd, False, 3, mode, code, crop), code, cl, what=(crop, code, cl, mode))
        hh, ww = h - 2, w - 6      # (W / 2 odd) rows padded by the caller's strides, the padding untouched
        exp = yr.yuv444(planes, bd, crop=(2, 4, 0, 2))
        big = torch.full((3, hh, ww + 40), 7, dtype=torch.uint8, device="cuda:0")
        view = big[:, :, 8:8 + ww]
        dec.pic_output_tensor(pic, layout="yuv444", crop=(2, 4, 0, 2), out=view)
        check444(view, exp, abi.OUT_U8)
        assert (torch.cat([big[:, :, :8].flatten(), big[:, :, 8 + ww:].flatten()]).cpu().numpy() == 7).all()
        bigc = torch.full((hh, ww + 16, 3), 7, dtype=torch.uint8, device="cuda:0")
        viewc = bigc[:, :ww, :]
        dec.pic_output_tensor(pic, layout="yuv444", channels_last=True, crop=(2, 4, 0, 2), out=viewc)
        check444(viewc, exp, abi.OUT_U8, True)
        assert (bigc[:, ww:, :].cpu().numpy() == 7).all()
    finally:
        dec.close()


def test_yuv444_dra_picture():
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    dec, pic = open_picture(planes, 10)
    try:
        for name in ("three_ranges_idx58", "five_ranges_idx40"):
            luts = d[f"{name}_luts"]
            for code, crop, mode in ((abi.OUT_U8, (0, 0, 0, 0), "nearest"), (abi.OUT_U16, (2, 0, 0, 2), "linear"), (abi.OUT_F32, (0, 6, 2, 0), "linear")):
                t = dec.pic_output_tensor(pic, layout="yuv444", dtype=torch_dtype(code), crop=crop, dra=luts, upsample=mode, chroma_loc=1)
                check444(t, yr.yuv444(planes, 10, False, 1, mode, code, crop, dra=luts), code, what=(name, code, crop))
            # nearest at 8 bit, sub-sampled again, is the reference application's 8-bit output
            t = dec.pic_output_tensor(pic, layout="yuv444", dra=luts, upsample="nearest")
            g = host(t)
            assert np.array_equal(np.concatenate([g[0].ravel(), g[1][0::2, 0::2].ravel(), g[2][0::2, 0::2].ravel()]), d[f"{name}_out8"])
    finally:
        dec.close()


def test_batch_slots_at_any_offset():
    """frame k of a [N, H * 3 // 2, W] and of a [N, 3, H, W] batch, and frames at offsets that are not 16-byte aligned (element stores): the same
    bytes as the aligned result, the bytes around them untouched"""
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    try:
        for layout, shape, exp in (("nv12", (h * 3 // 2, w), yr.nv12(planes, bd, 8)), ("yuv444", (3, h, w), yr.yuv444(planes, bd))):
            n = int(np.prod(shape))
            aligned = dec.pic_output_tensor(pic, layout=layout)
            assert aligned.data_ptr() % 16 == 0 and np.array_equal(host(aligned), exp)
            batch = torch.empty((4,) + shape, dtype=torch.uint8, device="cuda:0")
            for k in range(4):
                dec.pic_output_tensor(pic, layout=layout, out=batch[k])
            assert all(np.array_equal(host(batch[k]), exp) for k in range(4))
            offs = [1, n + 3, 2 * n + 21, 3 * n + 30]
            buf = torch.full((offs[-1] + n + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
            for o in offs:
                dec.pic_output_tensor(pic, layout=layout, out=buf[o:o + n].view(shape))
            hb = host(buf)
            mask = np.ones(hb.size, bool)
            for o in offs:
                assert np.array_equal(hb[o:o + n].reshape(shape), exp), (layout, o)
                mask[o:o + n] = False
            assert (hb[mask] == 0xA5).all()
        # 16-bit words at a 2-byte aligned offset
        exp = yr.p016(planes, bd, 10)
        n = exp.size
        buf = torch.full((n + 9,), 0x5A5A, dtype=torch.int16, device="cuda:0")
        dec.pic_output_tensor(pic, layout="p016", out=buf[3:3 + n].view(h * 3 // 2, w))
        hb = host(buf)
        assert np.array_equal(hb[3:3 + n].reshape(exp.shape), exp) and (hb[:3] == 0x5A5A).all() and (hb[3 + n:] == 0x5A5A).all()
    finally:
        dec.close()


def test_ordering_on_a_side_stream():
    """NV12 output on a non-default torch stream, then the next picture uploaded into the same slot by the context's stream, with no
    synchronisation in between: the first output holds the first picture"""
    import torch
    pa, bd = golden_planes("base_p_10b")
    pb = [np.asarray((p.astype(np.int32) * 3 + 101) % (1 << bd), np.int16) for p in pa]
    dec, pic = open_picture(pa, bd)
    try:
        exp = {"a": yr.nv12(pa, bd, 8), "b": yr.nv12(pb, bd, 8)}
        assert not np.array_equal(exp["a"], exp["b"])
        s = torch.cuda.Stream(device=0)
        got = []
        with torch.cuda.stream(s):
            for k in "abab":
                if got:
                    dec.pic_upload(pic, pa if k == "a" else pb)      # into the slot the previous output reads
                got.append((k, dec.pic_output_tensor(pic, layout="nv12")))
        s.synchronize()
        for k, t in got:
            assert np.array_equal(host(t), exp[k]), k
    finally:
        dec.close()


def test_bad_destinations_launch_nothing():
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    lib = dec.lib
    try:
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        fmt = abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)
        need = lib.xgpu_pic_output_device_size(dec.ctx, C.byref(fmt))
        assert need == h * w * 3 // 2 == lib.xgpu_output_format_size(C.byref(fmt), w, h, bd)
        f16 = abi.make_output_format(abi.OUT_P016, abi.OUT_U16, out_bit_depth=10)
        need16 = lib.xgpu_pic_output_device_size(dec.ctx, C.byref(f16))
        assert need16 == 2 * need
        t = torch.full((need16 + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        hostbuf = np.zeros(need16, np.uint8)
        calls = [(fmt, t.data_ptr(), h * w, str(need)),                 # an H x W buffer: no room for the chroma plane
                 (fmt, hostbuf.ctypes.data, need, str(need)),           # host memory
                 (f16, t.data_ptr() + 1, need16, str(need16)),          # not aligned to the 16-bit word
                 (f16, t.data_ptr(), need16 - 2, str(need16))]          # one word short
        for f, p, n, size_text in calls:
            rc = lib.xgpu_pic_output_device(dec.ctx, pic, None, C.byref(f), C.c_void_p(p), n, stream_h)
            assert rc == -101, (p, n)
            msg = lib.xgpu_last_error(dec.ctx)
            assert b"pic_output_device" in msg and size_text.encode() in msg, msg
        bad = abi.make_output_format(abi.OUT_NV12, abi.OUT_U16, out_bit_depth=8)
        assert lib.xgpu_pic_output_device(dec.ctx, pic, None, C.byref(bad), C.c_void_p(t.data_ptr()), need16, stream_h) == -101
        assert b"NV12" in lib.xgpu_last_error(dec.ctx)
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all() and not hostbuf.any()
        # the Python layer's own argument checks
        for kw in (dict(layout="p016", dtype=torch.uint8), dict(layout="nv12", dtype=torch.float16), dict(layout="nv12", out_bit_depth=10),
                   dict(layout="nv12", dtype=torch.int16, out_bit_depth=8), dict(layout="p016", out_bit_depth=17), dict(layout="yuv444", out_bit_depth=8),
                   dict(layout="rgb", out_bit_depth=8), dict(layout="yuv444", bgr=True), dict(layout="nv21"),
                   dict(layout="nv12", out=torch.empty((h * 3 // 2, w), dtype=torch.uint8, device="cuda:0").t()),
                   dict(layout="nv12", out=torch.empty((h, w), dtype=torch.uint8, device="cuda:0"))):
            with pytest.raises(ValueError):
                dec.pic_output_tensor(pic, **kw)
        assert dec.pic_output_tensor(pic, layout="rgb", out_bit_depth=bd).shape == (3, h, w)      # 0 or the coding depth
    finally:
        dec.close()


def _intra_stream(w, h, bd, n, vui, seed=3):
    rng = np.random.default_rng(seed)
    wr = stream.StreamWriter(w, h, bd, vui=vui)
    try:
        for k in range(n):
            wr.add_picture(synth.gen_frame(rng, w, h, bd, inter_frac=0.0, n_refs=(1, 0)), stream.SLICE_I, 28 + k, idr=True)
        return wr.bytes()
    finally:
        wr.close()


def test_stream_decoder_surfaces():
    import torch
    from xevd_amd.player import StreamDecoder
    d = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))
    data = d["bytes"].tobytes()
    w, h = d["p0_0"].shape[1], d["p0_0"].shape[0]
    ref = [frame for _, frame in StreamDecoder(data).pictures(output_bit_depth=8)]
    got = [t for _, t in StreamDecoder(data).pictures(tensor=dict(layout="nv12"))]
    assert len(got) == len(ref) == int(d["n"])
    for k, (t, frame) in enumerate(zip(got, ref)):
        assert np.array_equal(host(t), yr.interleave_420p(frame, w, h)), k
        assert np.array_equal(host(t), yr.nv12([d[f"p{k}_{c}"] for c in range(3)], 10, 8)), k      # the reference decoder's pictures
    got = [t for _, t in StreamDecoder(data).pictures(tensor=dict(layout="p016"))]
    for k, t in enumerate(got):
        assert np.array_equal(host(t), yr.p016([d[f"p{k}_{c}"] for c in range(3)], 10, 10)), k
    # yuv444 takes range and chroma siting from the stream's VUI
    vui = {"colour": (6, 6, 5), "full_range": 1, "chroma_loc": (2, 2)}
    data = _intra_stream(128, 96, 10, 3, vui)
    planes = [p for _, p in StreamDecoder(data).pictures()]
    got = [t for _, t in StreamDecoder(data).pictures(tensor=dict(layout="yuv444", dtype=torch.float32))]
    assert len(got) == len(planes) == 3
    for t, pl in zip(got, planes):
        check444(t, yr.yuv444(pl, 10, True, 2, "linear", abi.OUT_F32), abi.OUT_F32, what="vui")
        assert not np.array_equal(t.cpu().numpy(), yr.yuv444(pl, 10, False, 0, "linear", abi.OUT_F32))
    got = [t for _, t in StreamDecoder(data).pictures(tensor=dict(layout="yuv444", full_range=False, chroma_loc=0, channels_last=True))]      # overridden
    for t, pl in zip(got, planes):
        check444(t, yr.yuv444(pl, 10), abi.OUT_U8, True)


@pytest.mark.parametrize("name,pix_fmt,depth", [("hier_b_gop4", "nv12", 8), ("hier_b_gop4", "p010", 10), ("ippp_10b_offsets", "nv12", 8),
                                                ("ippp_10b_offsets", "p010", 10)])
def test_app_writes_semiplanar_files(name, pix_fmt, depth, tmp_path):
    """tools/xevd_gpu_app.py --pix-fmt nv12 / p010 against its default yuv420p run at the same output depth, re-interleaved frame by frame
    (a B-picture stream: output order; p010 on 8-bit pictures converts up, nv12 on 10-bit pictures converts down)"""
    d = np.load(os.path.join(golden_io.GOLDEN, f"stream_{name}.npz"))
    h, w = d["p0_0"].shape
    n = int(d["n"])
    src, planar, semi = tmp_path / "s.evc", tmp_path / "planar.yuv", tmp_path / "semi.yuv"
    src.write_bytes(d["bytes"].tobytes())
    app = os.path.join(ROOT, "tools", "xevd_gpu_app.py")
    for args in (["-o", str(planar), "--output-bit-depth", str(depth)], ["-o", str(semi), "--pix-fmt", pix_fmt]):
        r = subprocess.run([sys.executable, app, "-i", str(src)] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-2000:])
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    a, b = np.fromfile(planar, dt), np.fromfile(semi, dt)
    frame = w * h * 3 // 2
    assert a.size == b.size == n * frame
    for k in range(n):
        exp = yr.interleave_420p(a[k * frame:(k + 1) * frame], w, h)
        if pix_fmt == "p010":
            exp = exp << 6
        assert np.array_equal(b[k * frame:(k + 1) * frame].reshape(h * 3 // 2, w), exp), k
