"""GPU suite for xgpu_pic_output_device / XgpuDecoder.pic_output_tensor / StreamDecoder.pictures(tensor=...): R'G'B' and YUV420P written by the
device into torch tensors, against the numpy restatement of the contract (tests/colour_ref.py) applied to the downloaded planes.  Integer outputs
bit-exact, f32 within 4e-6, f16 / bf16 within one ulp of the restatement's f32 rounded."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_ref as cr
import golden_io
from xevd_amd import abi, stream, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_NAMES = {abi.OUT_U8: "uint8", abi.OUT_U16: "int16", abi.OUT_F16: "float16", abi.OUT_BF16: "bfloat16", abi.OUT_F32: "float32"}


def torch_dtype(code):
    import torch
    return getattr(torch, DT_NAMES[code])


def golden_planes(name):
    """the decoded picture of a committed golden case: [Y, U, V] of the active area, bit depth"""
    import numpy as np
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


def check(t, exp, code, channels_last=False, bgr=False, what=""):
    """tensor t (written by the device) against the restatement exp [3][H][W] (float32 before rounding for float dtypes)"""
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
        assert np.array_equal(got.numpy(), exp), what
    elif code == abi.OUT_U16:
        assert np.array_equal(got.numpy().view(np.uint16), exp), what
    elif code == abi.OUT_F32:
        assert np.abs(got.numpy().astype(np.float64) - exp).max() <= 4e-6, what
    else:
        bits = got.view(torch.int16).numpy().view(np.uint16).astype(np.int64)
        ref = (cr.to_f16_bits(exp) if code == abi.OUT_F16 else cr.to_bf16_bits(exp)).astype(np.int64)
        assert np.abs(bits - ref).max() <= 1, what


@pytest.mark.parametrize("case", ["base_p_8b", "base_p_10b", "base_p_12b"])
def test_every_layout_dtype_and_mode(case):
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    try:
        for code, mode, cl in itertools.product(DT_NAMES, ("linear", "nearest"), (False, True)):
            exp = cr.convert(planes, bd, 1, False, 0, mode, code)
            t = dec.pic_output_tensor(pic, channels_last=cl, dtype=torch_dtype(code), upsample=mode)
            check(t, exp, code, cl, what=(case, code, mode, cl))
        t = dec.pic_output_tensor(pic, bgr=True, channels_last=True)
        check(t, cr.convert(planes, bd), abi.OUT_U8, True, True, "bgr")
    finally:
        dec.close()


@pytest.mark.parametrize("case", ["base_p_8b", "base_p_10b", "base_p_12b"])
def test_chroma_locations_matrices_and_ranges(case):
    planes, bd = golden_planes(case)
    dec, pic = open_picture(planes, bd)
    try:
        for loc in range(6):
            for m, fr in ((1, False), (5, True), (9, False), (7, True), (4, False), (6, False)):
                for code in (abi.OUT_U8, abi.OUT_U16, abi.OUT_F32):
                    t = dec.pic_output_tensor(pic, dtype=torch_dtype(code), matrix=m, full_range=fr, chroma_loc=loc)
                    check(t, cr.convert(planes, bd, m, fr, loc, "linear", code), code, what=(loc, m, fr, code))
    finally:
        dec.close()


def test_crop_with_odd_chroma_widths_and_padded_rows():
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    try:
        for crop in ((2, 4, 2, 0), (0, 2, 0, 2), (6, 0, 4, 6), (2, 2, 2, 2)):
            cw = (w - crop[0] - crop[1]) // 2
            for code, cl, mode in itertools.product((abi.OUT_U8, abi.OUT_F16), (False, True), ("linear", "nearest")):
                t = dec.pic_output_tensor(pic, channels_last=cl, dtype=torch_dtype(code), upsample=mode, chroma_loc=3, crop=crop)
                check(t, cr.convert(planes, bd, 1, False, 3, mode, code, crop), code, cl, what=(crop, cw, code, cl, mode))
        # rows padded by the caller's strides (row_pitch): a view into a wider tensor, the padding untouched
        hh, ww = h - 2, w - 4
        big = torch.full((3, hh, ww + 40), 7, dtype=torch.uint8, device="cuda:0")
        view = big[:, :, 8:8 + ww]
        dec.pic_output_tensor(pic, crop=(2, 2, 0, 2), out=view)
        check(view, cr.convert(planes, bd, crop=(2, 2, 0, 2)), abi.OUT_U8)
        rest = torch.cat([big[:, :, :8].flatten(), big[:, :, 8 + ww:].flatten()]).cpu().numpy()
        assert (rest == 7).all()
    finally:
        dec.close()


def test_dra_picture():
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    dec, pic = open_picture(planes, 10)
    try:
        for name in ("three_ranges_idx58", "five_ranges_idx40"):
            luts = d[f"{name}_luts"]
            for code, crop in ((abi.OUT_U8, (0, 0, 0, 0)), (abi.OUT_U16, (2, 0, 0, 2)), (abi.OUT_F32, (0, 6, 2, 0))):
                t = dec.pic_output_tensor(pic, dtype=torch_dtype(code), crop=crop, dra=luts, matrix=9)
                check(t, cr.convert(planes, 10, 9, False, 0, "linear", code, crop, dra=luts), code, what=(name, code, crop))
            yuv = dec.pic_output_tensor(pic, layout="yuv420p", dra=luts)
            torch_bytes = yuv.cpu().numpy()
            assert np.array_equal(torch_bytes, dec.pic_output(pic, 8, dra=luts)) and np.array_equal(torch_bytes, d[f"{name}_out8"])
    finally:
        dec.close()


def test_yuv420p_equals_host_output():
    import torch
    for case in ("base_p_8b", "base_p_10b", "base_p_12b"):
        planes, bd = golden_planes(case)
        dec, pic = open_picture(planes, bd)
        try:
            for crop in ((0, 0, 0, 0), (2, 4, 2, 6)):
                for dt, obd in ((torch.uint8, 8),) + (((torch.int16, bd),) if bd > 8 else ()):
                    t = dec.pic_output_tensor(pic, layout="yuv420p", dtype=dt, crop=crop)
                    host = dec.pic_output(pic, obd, crop)
                    assert np.array_equal(t.cpu().numpy().view(np.uint8), host), (case, crop, obd)
        finally:
            dec.close()


def test_batch_slots_at_any_offset():
    """frames of a [N, 3, H, W] u8 batch at element-aligned offsets (16-byte aligned or not): each slot written, the bytes around it untouched"""
    import torch
    planes, bd = golden_planes("base_p_10b")
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    n = 3 * h * w
    try:
        exp = cr.convert(planes, bd)
        batch = torch.empty((4, 3, h, w), dtype=torch.uint8, device="cuda:0")
        for k in range(4):
            dec.pic_output_tensor(pic, out=batch[k])
        for k in range(4):
            check(batch[k], exp, abi.OUT_U8)
        offs = [1, n + 3, 2 * n + 21, 3 * n + 30]      # gaps of 2, 18 and 9 bytes between slots
        buf = torch.full((offs[-1] + n + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        for o in offs:
            dec.pic_output_tensor(pic, out=buf[o:o + n].view(3, h, w))
        host = buf.cpu().numpy()
        mask = np.ones(host.size, bool)
        for o in offs:
            assert np.array_equal(host[o:o + n].reshape(3, h, w), exp), o
            mask[o:o + n] = False
        assert (host[mask] == 0xA5).all()
    finally:
        dec.close()


def test_ordering_on_a_side_stream():
    """output on a non-default torch stream, then a reduction on that stream without any synchronisation in between; the tensor freed and
    reallocated between pictures (the caching allocator hands the same memory back on that stream)"""
    import torch
    pa, bd = golden_planes("base_p_10b")
    pb = [np.asarray((p.astype(np.int32) * 3 + 101) % (1 << bd), np.int16) for p in pa]
    dec, pic_a = open_picture(pa, bd)
    try:
        pic_b = dec.pic_alloc()
        dec.pic_upload(pic_b, pb)
        sums = {k: int(cr.convert(p, bd, dtype=cr.U16).astype(np.int64).sum()) for k, p in (("a", pa), ("b", pb))}
        s = torch.cuda.Stream(device=0)
        got = []
        with torch.cuda.stream(s):
            for k in "abab":
                t = dec.pic_output_tensor(pic_a if k == "a" else pic_b, dtype=torch.int16)
                got.append(t.to(torch.int64).sum())
                del t
        s.synchronize()
        assert [int(g) for g in got] == [sums[k] for k in "abab"]
    finally:
        dec.close()


def test_bad_destinations_launch_nothing():
    import torch
    planes, bd = golden_planes("base_p_8b")
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    lib = dec.lib
    try:
        fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16)
        need = lib.xgpu_pic_output_device_size(dec.ctx, C.byref(fmt))
        assert need == 3 * h * w * 2
        t = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        host = np.zeros(need, np.uint8)
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        calls = [(host.ctypes.data, need),              # host memory
                 (t.data_ptr(), need - 1),              # too short
                 (t.data_ptr() + 1, need)]              # not aligned to the 2-byte element
        for p, n in calls:
            rc = lib.xgpu_pic_output_device(dec.ctx, pic, None, C.byref(fmt), C.c_void_p(p), n, stream_h)
            assert rc == -101, (p, n)
            assert b"pic_output_device" in lib.xgpu_last_error(dec.ctx)
        bad = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, matrix=2)
        assert lib.xgpu_pic_output_device(dec.ctx, pic, None, C.byref(bad), C.c_void_p(t.data_ptr()), need, stream_h) == -104
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all()
        with pytest.raises(ValueError):
            dec.pic_output_tensor(pic, matrix=0)
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


def test_stream_decoder_tensors():
    import torch
    from xevd_amd.player import StreamDecoder
    for vui, bd in ((None, 8), ({"colour": (6, 6, 5), "full_range": 1, "chroma_loc": (2, 2)}, 10)):
        data = _intra_stream(128, 96, bd, 3, vui)
        ref = [planes for _, planes in StreamDecoder(data).pictures()]
        got = [(p["colour"], t) for p, t in StreamDecoder(data).pictures(tensor={})]
        assert len(got) == len(ref) == 3
        m, fr, loc = (5, True, 2) if vui else (1, False, 0)
        for (col, t), planes in zip(got, ref):
            assert col["matrix_coefficients"] == (5 if vui else 2)
            check(t, cr.convert(planes, bd, m, fr, loc), abi.OUT_U8)
            if vui:      # BT.601 is what it was converted with, not BT.709
                assert not np.array_equal(t.cpu().numpy(), cr.convert(planes, bd, 1, fr, loc))
        # explicit arguments override the VUI
        got = [t for _, t in StreamDecoder(data).pictures(tensor={"matrix": 9, "dtype": torch.float32, "channels_last": True})]
        for t, planes in zip(got, ref):
            check(t, cr.convert(planes, bd, 9, fr, loc, "linear", abi.OUT_F32), abi.OUT_F32, True)


CHILD = r"""
import sys, numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
order = sys.argv[1]
if order == "lib_first":
    from xevd_amd import abi
    abi.load()
    import torch
else:
    import torch
    torch.zeros(1, device="cuda:0")
    from xevd_amd import abi
    abi.load()
import colour_ref as cr
from xevd_amd.decoder import XgpuDecoder
rng = np.random.default_rng(5)
planes = [rng.integers(0, 1024, (64, 96)).astype(np.int16), rng.integers(0, 1024, (32, 48)).astype(np.int16), rng.integers(0, 1024, (32, 48)).astype(np.int16)]
with XgpuDecoder(96, 64, 10) as dec:
    pic = dec.pic_alloc()
    dec.pic_upload(pic, planes)
    t = dec.pic_output_tensor(pic, matrix=9)
    torch.cuda.synchronize()
    ok = np.array_equal(t.cpu().numpy(), cr.convert(planes, 10, 9))
maps = open("/proc/self/maps").read()
print("CHILD", order, ok, "libxevd_hip.so" in maps)
sys.exit(0 if ok else 1)
"""


@pytest.mark.parametrize("order", ["lib_first", "torch_first"])
def test_one_hip_runtime_in_either_import_order(order):
    code = CHILD.format(root=ROOT, tests=os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, order], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"CHILD {order} True True" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
