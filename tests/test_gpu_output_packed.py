"""GPU suite for the packed display surfaces (xgpu_pic_output_device_packed / XgpuDecoder.pic_output_packed / StreamDecoder packed= / the tool's --pix-fmt;
INTEGRATION.md section 8p): RGBA, 10:10:10:2 and packed 4:2:2 written by the device into torch tensors.  Where an existing device path writes the same
elements - the interleaved RGB tensor, its colour-managed form, NV12 / P016 - the packed surface is held to it bit for bit in every dtype; what no existing
path writes (10-bit codes at other coding depths, the colour-managed 10:10:10:2 store, chroma at full height) is held to the numpy restatement
tests/packed_ref.py, integers bit-exact.
Pictures: the committed goldens, and random and rail-to-rail planes at the smallest shapes that reach each branch of the kernels - 8x8 cropped to 2x2 (one
lane of n = 2, one chroma row: LINEAR clamps both neighbours), 24x16 cropped to 18x10 (a full lane and a tail lane; five chroma rows: a second, partly
filled row of workgroups), 528x16 cropped to 522x14 (a second workgroup in x)."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_ref as cr
import golden_io
import packed_ref as pr
from xevd_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_NAMES = {abi.OUT_U8: "uint8", abi.OUT_U16: "int16", abi.OUT_F16: "float16", abi.OUT_BF16: "bfloat16", abi.OUT_F32: "float32"}
GOLDENS = ["base_p_8b", "base_p_10b", "base_p_12b"]
SHAPES = [(8, 8, (2, 4, 4, 2)), (24, 16, (2, 4, 2, 4)), (528, 16, (2, 4, 2, 0))]      # (width, height, crop) -> 2x2, 18x10, 522x14
PQ_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
HLG_LINEAR = dict(src_primaries=9, src_transfer=18, dst_primaries=1, dst_transfer=8)


def torch_dtype(code):
    import torch
    return getattr(torch, DT_NAMES[code])


def golden_planes(name):
    d = np.load(os.path.join(golden_io.GOLDEN, f"pic_{name}.npz"))
    w, h, bd = (int(v) for v in d["params"][:3])
    pl, pc = abi.PAD_L, abi.PAD_C
    return [d["out_0"][pl:pl + h, pl:pl + w], d["out_1"][pc:pc + h // 2, pc:pc + w // 2], d["out_2"][pc:pc + h // 2, pc:pc + w // 2]], bd


def small_planes(w, h, bd, kind, seed=5):
    """random samples over the whole range, or a checker of the rails 0 and 2^B - 1 (luma and the two chroma planes out of phase): every clip is reached"""
    top = (1 << bd) - 1
    if kind == "random":
        rng = np.random.default_rng(seed + w + bd)
        return [rng.integers(0, top + 1, s).astype(np.int16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    return [(((yy + xx) & 1) * top).astype(np.int16), ((((cy >> 1) + cx) & 1) * top).astype(np.int16), (((cy + (cx >> 1) + 1) & 1) * top).astype(np.int16)]


def open_picture(planes, bd):
    from xevd_amd.decoder import XgpuDecoder
    h, w = planes[0].shape
    dec = XgpuDecoder(w, h, bd, device=0, max_pics=4)
    pic = dec.pic_alloc()
    dec.pic_upload(pic, planes)
    return dec, pic


def pictures(bd_small=(10,)):
    """(name, planes, bit depth, crops) of every picture of the suite"""
    for name in GOLDENS:
        planes, bd = golden_planes(name)
        yield name, planes, bd, ((0, 0, 0, 0), (2, 4, 2, 6))
    for (w, h, crop), bd, kind in itertools.product(SHAPES, bd_small, ("random", "rails")):
        yield f"{kind}_{w}x{h}_{bd}b", small_planes(w, h, bd, kind), bd, (crop,)


PICTURES = {name: (planes, bd, crops) for name, planes, bd, crops in pictures((8, 10, 12))}
TEN_BIT = [n for n, (_, bd, _) in PICTURES.items() if bd == 10]
SMALL = [n for n in PICTURES if n not in GOLDENS]


def host(t):
    """an integer tensor written by the device as a numpy array of unsigned elements"""
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def same_bits(a, b):
    """two device tensors of one shape and element size hold the same bits"""
    import torch
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return tuple(a.shape) == tuple(b.shape) and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def alpha_is(t, alpha, code, bd):
    """the A element of every pixel of RGBA tensor t holds the bits of the contract"""
    import torch
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    a = t[..., 3].contiguous().view(it).cpu().numpy()
    a = a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])
    return bool((a == pr.alpha_element(alpha, code, bd)).all())


# ------------------------------------------------------------------------------------------------ against the existing device paths, bit for bit
@pytest.mark.parametrize("name", [n for n in PICTURES if n in GOLDENS or "_10b" in n])
def test_rgba_is_the_interleaved_rgb_tensor_and_alpha(name):
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        n = 0
        for crop, code, bgr, mode in itertools.product(crops, DT_NAMES, (False, True), ("linear", "nearest")):
            dt = torch_dtype(code)
            for loc, fr in itertools.product(range(6), (False, True)):
                if mode == "nearest" and loc:      # NEAREST reads no chroma_loc: once per range
                    continue
                kw = dict(dtype=dt, matrix=(1, 9, 5)[n % 3], full_range=fr, chroma_loc=loc, upsample=mode, crop=crop)
                alpha = (1.0, 0.0, 0.5, 1 / 3)[n % 4]
                n += 1
                t = dec.pic_output_packed(pic, "bgra" if bgr else "rgba", alpha=alpha, **kw)
                ref = dec.pic_output_tensor(pic, layout="rgb", channels_last=True, bgr=bgr, **kw)
                assert t.dtype == dt and tuple(t.shape) == tuple(ref.shape[:2]) + (4,)
                assert same_bits(t[..., :3], ref), (name, kw, bgr)
                assert alpha_is(t, alpha, code, bd), (name, kw, alpha)
        t = dec.pic_output_packed(pic, "rgba", dtype=torch_dtype(abi.OUT_U16), out_bit_depth=bd)      # 0 or the coding depth
        assert same_bits(t[..., :3], dec.pic_output_tensor(pic, layout="rgb", channels_last=True, dtype=torch_dtype(abi.OUT_U16)))
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["base_p_10b", "base_p_12b", "random_24x16_10b", "rails_528x16_10b"])
def test_rgba_with_a_colour_transform_is_the_colour_managed_tensor(name):
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        for colour in (PQ_SRGB, HLG_LINEAR):      # (grouped: the context keeps one set of tables)
            for crop, code, mode, bgr in itertools.product(crops, DT_NAMES, ("linear", "nearest"), (False, True)):
                kw = dict(dtype=torch_dtype(code), matrix=9, chroma_loc=2, upsample=mode, crop=crop, colour=colour)
                t = dec.pic_output_packed(pic, "bgra" if bgr else "rgba", alpha=0.5, **kw)
                ref = dec.pic_output_tensor(pic, layout="rgb", channels_last=True, bgr=bgr, **kw)
                assert same_bits(t[..., :3], ref), (name, colour, crop, code, mode, bgr)
                assert alpha_is(t, 0.5, code, bd)
    finally:
        dec.close()


def fields(words, bgr=False):
    """[H][W] 10:10:10:2 words -> ([3][H][W] R, G, B, [H][W] A)"""
    w = np.asarray(words).astype(np.int64)
    lo, mid, hi = w & 1023, (w >> 10) & 1023, (w >> 20) & 1023
    return np.stack([hi, mid, lo] if bgr else [lo, mid, hi]), w >> 30


@pytest.mark.parametrize("name", TEN_BIT)
def test_rgb10a2_on_10_bit_pictures_is_the_u16_rgb_tensor(name):
    import torch
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        for crop, mode, bgr, fr, (loc, matrix) in itertools.product(crops, ("linear", "nearest"), (False, True), (False, True), ((0, 1), (3, 9), (5, 6))):
            kw = dict(matrix=matrix, full_range=fr, chroma_loc=loc, upsample=mode, crop=crop)
            t = dec.pic_output_packed(pic, "bgr10a2" if bgr else "rgb10a2", alpha=1 / 3, **kw)
            assert t.dtype == torch.int32 and t.dim() == 2
            rgb, a = fields(host(t), bgr)
            ref = host(dec.pic_output_tensor(pic, layout="rgb", dtype=torch.int16, **kw))
            assert np.array_equal(rgb, ref), (name, kw, bgr)
            assert (a == 1).all()
            assert np.array_equal(host(t), pr.rgb10a2(planes, bd, bgr=bgr, alpha=1 / 3, mode=mode, **{k: v for k, v in kw.items() if k != "upsample"}))
    finally:
        dec.close()


@pytest.mark.parametrize("name", list(PICTURES))
def test_422_luma_is_nv12_and_nearest_chroma_is_its_rows(name):
    import torch
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        for crop, layout, d in itertools.product(crops, ("yuyv", "uyvy"), (8, 0, 10, 16)):
            yi, ci = (1, 0) if layout == "uyvy" else (0, 1)
            if d == 8:
                t = dec.pic_output_packed(pic, layout, upsample="nearest", crop=crop)
                nv = host(dec.pic_output_tensor(pic, layout="nv12", crop=crop))
                assert t.dtype == torch.uint8
            else:
                t = dec.pic_output_packed(pic, layout, dtype=torch.int16, out_bit_depth=d, upsample="nearest", crop=crop)
                nv = host(dec.pic_output_tensor(pic, layout="p016", out_bit_depth=d, crop=crop))
            g = host(t)
            h, w = g.shape[:2]
            assert g.shape == (h, w, 2) and nv.shape == (h * 3 // 2, w)
            assert np.array_equal(g[:, :, yi], nv[:h]), (name, crop, layout, d)
            assert np.array_equal(g[:, :, ci], nv[h + (np.arange(h) >> 1)]), (name, crop, layout, d)
            lin = host(dec.pic_output_packed(pic, layout, dtype=t.dtype, out_bit_depth=d, upsample="linear", chroma_loc=2, crop=crop))
            assert np.array_equal(lin[:, :, yi], nv[:h])      # luma does not depend on the mode
            assert np.array_equal(lin[0::2, :, ci], nv[h:])   # co-sited top: the even rows are the chroma rows themselves
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ against tests/packed_ref.py
@pytest.mark.parametrize("name", [n for n in PICTURES if "_8b" in n or "_12b" in n])
def test_rgb10a2_at_8_and_12_bit_plain_and_colour_managed(name):
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    rgbf = abi.make_output_format(abi.OUT_RGB_INTERLEAVED)
    try:
        for colour in (None, PQ_SRGB, HLG_LINEAR):
            tab = None if colour is None else abi.colour_tables(dec.lib, rgbf, abi.make_colour_transform(**colour), bd)
            for crop, mode, bgr, fr, (loc, matrix) in itertools.product(crops, ("linear", "nearest"), (False, True), (False, True), ((0, 1), (3, 9))):
                if colour is not None and (fr or (bgr and mode == "nearest")):
                    continue
                t = dec.pic_output_packed(pic, "bgr10a2" if bgr else "rgb10a2", alpha=0.5, matrix=matrix, full_range=fr, chroma_loc=loc, upsample=mode, crop=crop,
                                          colour=colour)
                exp = pr.rgb10a2(planes, bd, matrix, fr, loc, mode, crop, bgr=bgr, alpha=0.5, tab=tab)
                got = host(t)
                diff = int((got != exp).sum())
                print(f"{name} cm={colour is not None} {mode} bgr={bgr} fr={fr} loc={loc}: {diff} of {exp.size} words differ")
                assert diff == 0, (name, colour, crop, mode, bgr, fr, loc)
    finally:
        dec.close()


@pytest.mark.parametrize("name", list(PICTURES))
def test_422_linear_sitings_and_depths(name):
    import torch
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        for crop, loc, d, uyvy in itertools.product(crops, (0, 3, 4), (8, 10, 12, 16), (False, True)):      # centred, top, bottom; the horizontal bit either way
            code = pr.U8 if d == 8 else pr.U16
            t = dec.pic_output_packed(pic, "uyvy" if uyvy else "yuyv", dtype=torch.uint8 if d == 8 else torch.int16, out_bit_depth=d, chroma_loc=loc, crop=crop)
            exp = pr.yuv422(planes, bd, d, code, uyvy, loc, "linear", crop)
            assert np.array_equal(host(t), exp), (name, crop, loc, d, uyvy)
        t = dec.pic_output_packed(pic, "yuyv", dtype=torch.int16, crop=crops[0])      # out_bit_depth 0: the coding depth
        assert np.array_equal(host(t), pr.yuv422(planes, bd, bd, pr.U16, crop=crops[0]))
    finally:
        dec.close()


def test_dra_tables_on_the_10_bit_picture():
    import torch
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    dec, pic = open_picture(planes, 10)
    try:
        for name, crop in (("three_ranges_idx58", (0, 0, 0, 0)), ("five_ranges_idx40", (2, 4, 2, 0))):
            luts = d[f"{name}_luts"]
            for loc, mode, uyvy in ((0, "linear", False), (2, "linear", True), (4, "linear", False), (0, "nearest", True)):
                t = dec.pic_output_packed(pic, "uyvy" if uyvy else "yuyv", chroma_loc=loc, upsample=mode, crop=crop, dra=luts)
                assert np.array_equal(host(t), pr.yuv422(planes, 10, 8, pr.U8, uyvy, loc, mode, crop, dra=luts)), (name, loc, mode)
                t = dec.pic_output_packed(pic, "uyvy" if uyvy else "yuyv", dtype=torch.int16, out_bit_depth=10, chroma_loc=loc, upsample=mode, crop=crop, dra=luts)
                assert np.array_equal(host(t), pr.yuv422(planes, 10, 10, pr.U16, uyvy, loc, mode, crop, dra=luts)), (name, loc, mode)
            for mode in ("linear", "nearest"):
                kw = dict(matrix=9, chroma_loc=1, upsample=mode, crop=crop, dra=luts)
                t = dec.pic_output_packed(pic, "rgb10a2", **kw)
                assert np.array_equal(host(t), pr.rgb10a2(planes, 10, 9, False, 1, mode, crop, dra=luts))
                for code in DT_NAMES:
                    t = dec.pic_output_packed(pic, "rgba", dtype=torch_dtype(code), **kw)
                    assert same_bits(t[..., :3], dec.pic_output_tensor(pic, layout="rgb", channels_last=True, dtype=torch_dtype(code), **kw)), (name, mode, code)
        # the yuyv frame at 8 bit with NEAREST, sub-sampled again, is the reference application's 8-bit output
        luts = d["three_ranges_idx58_luts"]
        g = host(dec.pic_output_packed(pic, "yuyv", upsample="nearest", dra=luts))
        assert np.array_equal(np.concatenate([g[:, :, 0].ravel(), g[0::2, 0::2, 1].ravel(), g[0::2, 1::2, 1].ravel()]), d["three_ranges_idx58_out8"])
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ destination handling
FORMS = [("rgba", "uint8", 4), ("bgra", "int16", 4), ("rgba", "float16", 4), ("rgba", "float32", 4), ("rgb10a2", "int32", 1), ("yuyv", "uint8", 2),
         ("uyvy", "int16", 2)]


@pytest.mark.parametrize("name", ["base_p_10b", "random_24x16_10b", "rails_528x16_10b"])
def test_padded_destinations_keep_their_padding(name):
    """views into wider tensors: pitches and offsets that are multiples of 16 bytes (vector stores) and that are not (element stores) - the same elements as
    the tight call's, the padding untouched"""
    import torch
    planes, bd, crops = PICTURES[name]
    dec, pic = open_picture(planes, bd)
    try:
        for (layout, dtn, last), mode in itertools.product(FORMS, ("linear", "nearest")):
            dt = getattr(torch, dtn)
            kw = dict(upsample=mode, crop=crops[-1], alpha=0.5)
            if layout != "rgb10a2":
                kw["dtype"] = dt
            tight = dec.pic_output_packed(pic, layout, **kw)
            h, w = tight.shape[:2]
            al = (-w) % 16 + 16      # pixels that make the pitch a multiple of 16 pixels, so of 16 bytes for every element
            for pad, off in ((al, 16), (al, 0), (al, 1), (3, 1), (5, 0)):      # in pixels: aligned pitch and offset (twice), aligned pitch alone, neither
                big = torch.full((h, w + pad) + tight.shape[2:], 7, dtype=dt, device="cuda:0")
                view = big[:, off:off + w]
                assert dec.pic_output_packed(pic, layout, out=view, **kw) is view
                assert same_bits(view, tight), (name, layout, dtn, mode, pad, off)
                rest = torch.cat([big[:, :off].flatten(), big[:, off + w:].flatten()])
                assert bool((rest == 7).all()), (name, layout, dtn, mode, pad, off)
    finally:
        dec.close()


def test_a_callers_stream():
    """output on a non-default torch stream, then the next picture uploaded into the same slot by the context's stream, with no synchronisation in between:
    every output holds the picture it was asked for"""
    import torch
    pa, bd, _ = PICTURES["base_p_10b"]
    pb = [np.asarray((p.astype(np.int32) * 3 + 101) % (1 << bd), np.int16) for p in pa]
    dec, pic = open_picture(pa, bd)
    try:
        exp = {"a": pr.yuv422(pa, bd, 8), "b": pr.yuv422(pb, bd, 8)}
        exp10 = {"a": pr.rgb10a2(pa, bd), "b": pr.rgb10a2(pb, bd)}
        assert not np.array_equal(exp["a"], exp["b"])
        s = torch.cuda.Stream(device=0)
        got = []
        with torch.cuda.stream(s):
            for k in "abab":
                if got:
                    dec.pic_upload(pic, pa if k == "a" else pb)      # into the slot the previous output reads
                got.append((k, dec.pic_output_packed(pic, "yuyv"), dec.pic_output_packed(pic, "rgb10a2")))
        s.synchronize()
        for k, t, t10 in got:
            assert np.array_equal(host(t), exp[k]) and np.array_equal(host(t10), exp10[k]), k
    finally:
        dec.close()


def test_bad_destinations_and_formats_launch_nothing():
    import torch
    planes, bd, _ = PICTURES["base_p_10b"]
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    lib = dec.lib
    try:
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rgba = abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_U8)
        r10 = abi.make_packed_format(abi.PACKED_RGB10A2)
        y16 = abi.make_packed_format(abi.PACKED_YUYV, abi.OUT_U16)
        need = lib.xgpu_output_packed_size(C.byref(rgba), w, h, bd)
        assert need == 4 * w * h == lib.xgpu_output_packed_size(C.byref(r10), w, h, bd) == lib.xgpu_output_packed_size(C.byref(y16), w, h, bd)
        t = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        hostbuf = np.zeros(need, np.uint8)
        cm = abi.make_colour_transform(**PQ_SRGB)
        calls = [(rgba, None, t.data_ptr(), need - 1, -101),             # one byte short
                 (rgba, None, hostbuf.ctypes.data, need, -101),          # host memory
                 (r10, None, t.data_ptr() + 2, need, -101),              # the word is aligned to 4
                 (y16, None, t.data_ptr() + 1, need, -101),              # the element is aligned to 2
                 (y16, cm, t.data_ptr(), need, -101),                    # 4:2:2 takes no transform
                 (abi.make_packed_format(abi.PACKED_RGBA, matrix=2), None, t.data_ptr(), need, -104),
                 (rgba, abi.make_colour_transform(**dict(PQ_SRGB, src_transfer=17)), t.data_ptr(), need, -104),
                 (abi.make_packed_format(abi.PACKED_RGBA, alpha=1.5), None, t.data_ptr(), need, -101),
                 (abi.make_packed_format(abi.PACKED_RGB10A2, dtype=abi.OUT_U16), None, t.data_ptr(), need, -101)]
        for f, c, p, n, code in calls:
            rc = lib.xgpu_pic_output_device_packed(dec.ctx, pic, None, C.byref(f), None if c is None else C.byref(c), C.c_void_p(p), n, stream_h)
            assert rc == code, (f.layout, p, n, rc)
            assert b"pic_output_device_packed" in lib.xgpu_last_error(dec.ctx)
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all() and not hostbuf.any()
        assert lib.xgpu_pic_output_device_packed(dec.ctx, pic, None, C.byref(rgba), None, C.c_void_p(t.data_ptr()), need, stream_h) == 0      # exactly `need` bytes
        torch.cuda.synchronize()
        assert (t[need:].cpu().numpy() == 0x5A).all() and (t[3:need:4].cpu().numpy() == 255).all()
        # the Python layer's own argument checks
        for kw in (dict(layout="rgb"), dict(layout="rgb10a2", dtype=torch.int16), dict(layout="rgb10a2", out_bit_depth=10), dict(layout="yuyv", dtype=torch.float16),
                   dict(layout="yuyv", out_bit_depth=10), dict(layout="uyvy", colour=PQ_SRGB), dict(layout="rgba", out_bit_depth=8), dict(layout="rgba", alpha=-0.5),
                   dict(layout="rgba", matrix=2), dict(layout="rgba", upsample="cubic"), dict(layout="rgba", crop=(1, 0, 0, 0)),
                   dict(layout="rgba", out=torch.empty((h, w, 4), dtype=torch.uint8, device="cuda:0").transpose(0, 1)),
                   dict(layout="rgb10a2", out=torch.empty((h, w), dtype=torch.int32, device="cuda:0")[:, ::2]),
                   dict(layout="rgba", out=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0"))):
            with pytest.raises(ValueError):
                dec.pic_output_packed(pic, **kw)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ stream and tool
def test_stream_decoder_packed():
    import torch
    from xevd_amd.player import StreamDecoder
    d = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))
    data = d["bytes"].tobytes()
    seen = []
    for p, planes in StreamDecoder(data).pictures(packed=dict(layout="rgb10a2", alpha=0.5), to="srgb"):
        seen.append((p, planes, p["packed"]))
    assert len(seen) == int(d["n"])
    y210 = [p["packed"] for p, _ in StreamDecoder(data).output_order(packed=dict(layout="yuyv", dtype=torch.int16, out_bit_depth=10))]
    assert all(isinstance(a, np.ndarray) for a in y210)
    for k, (p, planes, t) in enumerate(seen):
        assert all(np.array_equal(planes[c], d[f"p{k}_{c}"]) for c in range(3))
        dec, pic = open_picture(planes, 10)
        try:
            kw = StreamDecoder.tensor_options(p, {})
            colour = StreamDecoder.colour_transform(p["colour"], "srgb")
            assert same_bits(t, dec.pic_output_packed(pic, "rgb10a2", alpha=0.5, colour=colour, **kw)), k
            assert not same_bits(t, dec.pic_output_packed(pic, "rgb10a2", alpha=0.5, **kw))
            assert np.array_equal(y210[k].view(np.uint16), host(dec.pic_output_packed(pic, "yuyv", dtype=torch.int16, out_bit_depth=10, **kw))), k
        finally:
            dec.close()


@pytest.mark.parametrize("name,pix_fmt", [("ippp_10b_offsets", "rgba"), ("hier_b_gop4", "y210le")])
def test_app_writes_packed_files(name, pix_fmt, tmp_path):
    """tools/xevd_gpu_app.py --pix-fmt rgba / y210le against its default yuv420p run at the stream's depth, repacked in numpy frame by frame (y210le on the
    8-bit B-picture stream: output order, converted up)"""
    d = np.load(os.path.join(golden_io.GOLDEN, f"stream_{name}.npz"))
    h, w = d["p0_0"].shape
    n = int(d["n"])
    bd = 10 if "10b" in name else 8
    src, planar, packed = tmp_path / "s.evc", tmp_path / "planar.yuv", tmp_path / "packed.raw"
    src.write_bytes(d["bytes"].tobytes())
    app = os.path.join(ROOT, "tools", "xevd_gpu_app.py")
    for args in (["-o", str(planar)], ["-o", str(packed), "--pix-fmt", pix_fmt]):
        r = subprocess.run([sys.executable, app, "-i", str(src)] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-2000:])
    a = np.fromfile(planar, np.uint8 if bd == 8 else np.dtype("<u2")).astype(np.int16)
    frame = w * h * 3 // 2
    assert a.size == n * frame
    b = np.fromfile(packed, np.uint8 if pix_fmt == "rgba" else np.dtype("<u2"))
    assert b.size == n * w * h * (4 if pix_fmt == "rgba" else 2)
    b = b.reshape(n, h, w, -1)
    for k in range(n):
        f = a[k * frame:(k + 1) * frame]
        planes = [f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)]
        if pix_fmt == "rgba":
            exp = np.concatenate([np.moveaxis(cr.convert(planes, bd), 0, -1), np.full((h, w, 1), 255, np.uint8)], axis=-1)
        else:
            exp = pr.yuv422(planes, bd, 10, pr.U16)
        assert np.array_equal(b[k], exp), (name, pix_fmt, k)
