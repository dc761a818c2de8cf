"""GPU suite for the dithered output (xgpu_pic_output_device_dithered / _packed_dithered): the threshold-one-half matrix against the
plain calls bit for bit, every form and matrix against the numpy restatement tests/dither_ref.py, the phase, the flat-mean property, refusals that launch nothing,
the handles, the stream player and the command-line tool."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import dither_ref as dr
import golden_io
from xevd_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, OOM, UNSUPPORTED = -101, -102, -104
GOLDENS = ["base_p_8b", "base_p_10b", "base_p_12b"]
# (width, height, crop): the three-channel family at 8 pixels per lane -> 2x2, 18x10, 522x14 (a tail lane, a second row of workgroups, a second workgroup in x);
# the semi-planar family at 16 columns per lane -> 2x2, 34x10, 1034x14
SHAPES_RGB = [(8, 8, (2, 4, 4, 2)), (24, 16, (2, 4, 2, 4)), (528, 16, (2, 4, 2, 0))]
SHAPES_SEMI = [(16, 8, (2, 12, 4, 2)), (40, 16, (2, 4, 2, 4)), (1040, 16, (2, 4, 2, 0))]
PQ_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
HLG_LINEAR = dict(src_primaries=9, src_transfer=18, dst_primaries=1, dst_transfer=8)
HALF = ("half", np.array([[1]], np.uint16), 1, (0, 0))


def matrices():
    """(name, ranks [mh, mw], k, phase): 1 x 1; 4 x 2 at (3, 1) - a wrap inside a lane's run; 16 x 4 at (5, 3) - not square; Bayer 8; blue 64 at (63, 63);
    128 x 128 at k = 14"""
    rng = np.random.default_rng(11)
    lib = abi.load()
    return [("1x1", np.array([[1]], np.uint16), 2, (0, 0)),
            ("4x2", rng.permutation(8).reshape(2, 4).astype(np.uint16), 3, (3, 1)),
            ("16x4", rng.integers(0, 64, (4, 16)).astype(np.uint16), 6, (5, 3)),
            ("bayer8", abi.dither_bayer(lib, 3), 6, (0, 0)),
            ("blue64", abi.dither_blue(lib, 6, 1), 12, (63, 63)),
            ("rand128", rng.integers(0, 1 << 14, (128, 128)).astype(np.uint16), 14, (17, 101))]


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


def pictures(shapes):
    """name -> (planes, bit depth, crops)"""
    out = {}
    for name in GOLDENS:
        planes, bd = golden_planes(name)
        out[name] = (planes, bd, ((0, 0, 0, 0), (2, 4, 2, 6)))
    for (w, h, crop), bd, kind in itertools.product(shapes, (8, 10, 12), ("random", "rails")):
        out[f"{kind}_{w}x{h}_{bd}b"] = (small_planes(w, h, bd, kind), bd, (crop,))
    return out


PICS_RGB, PICS_SEMI = pictures(SHAPES_RGB), pictures(SHAPES_SEMI)


def open_picture(planes, bd):
    from xevd_amd.decoder import XgpuDecoder
    h, w = planes[0].shape
    dec = XgpuDecoder(w, h, bd, device=0, max_pics=4)
    pic = dec.pic_alloc()
    dec.pic_upload(pic, planes)
    return dec, pic


def host(t):
    """an integer tensor written by the device as a numpy array of unsigned elements"""
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


class Matrix:
    """a matrix of the list above as a handle of `dec`, destroyed on the way out (a context has four handles)"""

    def __init__(self, dec, m):
        self.dec, (self.name, self.m, self.k, self.ph) = dec, m

    def __enter__(self):
        self.h = self.dec.dither_create(self.m, levels=1 << self.k)
        return self

    def __exit__(self, *exc):
        self.dec.dither_destroy(self.h)


# ------------------------------------------------------------------------------------------------ 1. the threshold-one-half matrix is the plain call
@pytest.mark.parametrize("name", list(PICS_RGB))
def test_half_threshold_is_the_plain_rgb_and_packed_call(name):
    import torch
    planes, bd, crops = PICS_RGB[name]
    dec, pic = open_picture(planes, bd)
    try:
        with Matrix(dec, HALF) as mx:
            n = 0
            for crop, dt, cl, bgr, mode in itertools.product(crops, (torch.uint8, torch.int16), (False, True), (False, True), ("linear", "nearest")):
                kw = dict(dtype=dt, matrix=(1, 9, 5)[n % 3], full_range=bool(n & 1), chroma_loc=n % 6, upsample=mode, crop=crop)
                n += 1
                got = dec.pic_output_dithered(pic, mx.h, "rgb", channels_last=cl, bgr=bgr, **kw)
                assert torch.equal(got, dec.pic_output_tensor(pic, layout="rgb", channels_last=cl, bgr=bgr, **kw)), (name, cl, bgr, kw)
                if not cl:
                    lay = "bgra" if bgr else "rgba"
                    assert torch.equal(dec.pic_output_dithered(pic, mx.h, lay, alpha=0.4, **kw), dec.pic_output_packed(pic, lay, alpha=0.4, **kw)), (name, lay, kw)
                    if dt == torch.uint8:
                        del kw["dtype"]
                        lay = "bgr10a2" if bgr else "rgb10a2"
                        assert torch.equal(dec.pic_output_dithered(pic, mx.h, lay, alpha=0.4, **kw), dec.pic_output_packed(pic, lay, alpha=0.4, **kw)), (name, lay, kw)
    finally:
        dec.close()


def semi_forms(bd):
    """(layout, keyword arguments, depth D) of the surfaces at coding depth bd"""
    import torch
    forms = [("nv12", dict(dtype=torch.uint8), 8)]
    forms += [("nv12", dict(dtype=torch.int16, out_bit_depth=d), d) for d in (9, 10, 12) if bd > 8 or d == 10]
    forms += [("p016", dict(out_bit_depth=d), d) for d in (8, 10, 12)]
    return forms


@pytest.mark.parametrize("name", list(PICS_SEMI))
def test_half_threshold_is_the_plain_surface_and_no_depth_lost_is_too(name):
    """cases 1 and 2: NV12 U8 from 10 and 12 bit, NV12 U16 at depth 10 from 12 bit, P016 D = 10 from 12 bit with the one-half threshold; where D >= B any
    matrix gives the plain call's bytes"""
    import torch
    planes, bd, crops = PICS_SEMI[name]
    dec, pic = open_picture(planes, bd)
    try:
        lossy = 0
        for m in (HALF, matrices()[2], matrices()[5]):
            with Matrix(dec, m) as mx:
                for crop, (layout, kw, d) in itertools.product(crops, semi_forms(bd)):
                    if m is not HALF and d < bd:
                        continue
                    lossy += d < bd
                    got = dec.pic_output_dithered(pic, mx.h, layout, phase=mx.ph, crop=crop, **kw)
                    assert torch.equal(got, dec.pic_output_tensor(pic, layout=layout, crop=crop, **kw)), (name, mx.name, layout, d, crop)
        assert lossy or bd == 8
    finally:
        dec.close()


def test_half_threshold_with_dra_tables_and_padded_destinations():
    import torch
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    luts = d["five_ranges_idx40_luts"]
    dec, pic = open_picture(planes, 10)
    try:
        with Matrix(dec, HALF) as mx, Matrix(dec, matrices()[2]) as m16:
            crop = (2, 4, 2, 0)
            for layout, kw in (("rgb", dict(channels_last=True)), ("rgb", dict(dtype=torch.int16)), ("rgba", {}), ("rgb10a2", {}), ("nv12", {}), ("p016", dict(out_bit_depth=8))):
                plain = dec.pic_output_tensor if layout in ("rgb", "nv12", "p016") else dec.pic_output_packed
                tight = plain(pic, layout=layout, crop=crop, dra=luts, **kw)
                assert torch.equal(dec.pic_output_dithered(pic, mx.h, layout, crop=crop, dra=luts, **kw), tight), layout
                # views into wider tensors: pitches and offsets that allow vector stores and that do not; the padding stays
                if layout == "rgb" and not kw.get("channels_last"):
                    continue
                h, w = tight.shape[:2]
                al = (-w) % 16 + 16
                for pad, off in ((al, 16), (al, 1), (3, 1), (5, 0)):
                    big = torch.full((h, w + pad) + tight.shape[2:], 7, dtype=tight.dtype, device="cuda:0")
                    view = big[:, off:off + w]
                    assert dec.pic_output_dithered(pic, mx.h, layout, crop=crop, dra=luts, out=view, **kw) is view
                    assert torch.equal(view, tight), (layout, pad, off)
                    assert bool((torch.cat([big[:, :off].flatten(), big[:, off + w:].flatten()]) == 7).all()), (layout, pad, off)
                    # ... and a real matrix lands in the same place
                    ref = dec.pic_output_dithered(pic, m16.h, layout, phase=m16.ph, crop=crop, dra=luts, **kw)
                    dec.pic_output_dithered(pic, m16.h, layout, phase=m16.ph, crop=crop, dra=luts, out=view, **kw)
                    assert torch.equal(view, ref), (layout, pad, off)
            got = host(dec.pic_output_dithered(pic, m16.h, "nv12", phase=m16.ph, crop=crop, dra=luts))
            assert np.array_equal(got, dr.nv12(planes, 10, 8, m16.m, m16.k, m16.ph, crop, dra=luts))
            got = host(dec.pic_output_dithered(pic, m16.h, "rgb", phase=m16.ph, crop=crop, dra=luts, matrix=9))
            assert np.array_equal(got, dr.rgb(planes, 10, m16.m, m16.k, m16.ph, crop=crop, dra=luts, matrix=9))
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ 3. against tests/dither_ref.py
@pytest.mark.parametrize("name", list(PICS_RGB))
def test_matrix_path_is_the_reference(name):
    import torch
    planes, bd, crops = PICS_RGB[name]
    dec, pic = open_picture(planes, bd)
    try:
        n = 0
        for m in matrices():
            with Matrix(dec, m) as mx:
                for crop, mode in itertools.product(crops, ("linear", "nearest")):
                    ref = dict(matrix=(1, 9, 6)[n % 3], full_range=bool(n & 1), chroma_loc=n % 6, crop=crop)
                    kw = dict(ref, upsample=mode)
                    u16, bgr, cl = bool(n & 2), bool(n & 4), bool(n % 3)
                    n += 1
                    got = host(dec.pic_output_dithered(pic, mx.h, "rgb", phase=mx.ph, dtype=torch.int16 if u16 else torch.uint8, bgr=bgr, channels_last=cl, **kw))
                    exp = dr.rgb(planes, bd, mx.m, mx.k, mx.ph, dtype=dr.U16 if u16 else dr.U8, bgr=bgr, channels_last=cl, mode=mode, **ref)
                    assert np.array_equal(got, exp), (name, mx.name, kw, u16, bgr, cl)
                    got = host(dec.pic_output_dithered(pic, mx.h, "bgra" if bgr else "rgba", phase=mx.ph, dtype=torch.uint8 if u16 else torch.int16, alpha=0.5, **kw))
                    exp = dr.rgba(planes, bd, mx.m, mx.k, mx.ph, dtype=dr.U8 if u16 else dr.U16, bgr=bgr, alpha=0.5, mode=mode, **ref)
                    assert np.array_equal(got, exp), (name, mx.name, kw, u16, bgr)
                    got = host(dec.pic_output_dithered(pic, mx.h, "bgr10a2" if bgr else "rgb10a2", phase=mx.ph, alpha=1 / 3, **kw))
                    assert np.array_equal(got, dr.rgb10a2(planes, bd, mx.m, mx.k, mx.ph, bgr=bgr, alpha=1 / 3, mode=mode, **ref)), (name, mx.name, kw, bgr)
    finally:
        dec.close()


@pytest.mark.parametrize("name", list(PICS_SEMI))
def test_depth_conversion_is_the_reference(name):
    planes, bd, crops = PICS_SEMI[name]
    dec, pic = open_picture(planes, bd)
    try:
        for m in matrices():
            with Matrix(dec, m) as mx:
                for crop, (layout, kw, d) in itertools.product(crops, semi_forms(bd)):
                    got = host(dec.pic_output_dithered(pic, mx.h, layout, phase=mx.ph, crop=crop, **kw))
                    exp = (dr.nv12 if layout == "nv12" else dr.p016)(planes, bd, d, mx.m, mx.k, mx.ph, crop)
                    assert np.array_equal(got, exp), (name, mx.name, layout, d, crop)
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["base_p_10b", "base_p_12b", "random_8x8_10b", "random_24x16_10b", "rails_24x16_12b", "random_528x16_10b", "rails_528x16_10b"])
def test_colour_managed_path_is_the_reference(name):
    planes, bd, crops = PICS_RGB[name]
    dec, pic = open_picture(planes, bd)
    rgbf = abi.make_output_format(abi.OUT_RGB_INTERLEAVED)
    try:
        for colour in (PQ_SRGB, HLG_LINEAR):      # (grouped: the context keeps one set of tables)
            tab = abi.colour_tables(dec.lib, rgbf, abi.make_colour_transform(**colour), bd)
            for i, m in enumerate(matrices()):
                with Matrix(dec, m) as mx:
                    crop, mode, bgr = crops[-1], ("linear", "nearest")[i & 1], bool(i & 2)
                    ref = dict(matrix=9, chroma_loc=2, crop=crop, tab=tab, mode=mode)
                    kw = dict(matrix=9, chroma_loc=2, crop=crop, colour=colour, upsample=mode, phase=mx.ph)
                    for what, got, exp in (
                            ("rgb u8", dec.pic_output_dithered(pic, mx.h, "rgb", bgr=bgr, **kw), dr.rgb(planes, bd, mx.m, mx.k, mx.ph, bgr=bgr, **ref)),
                            ("rgba u8", dec.pic_output_dithered(pic, mx.h, "bgra" if bgr else "rgba", **kw), dr.rgba(planes, bd, mx.m, mx.k, mx.ph, bgr=bgr, **ref)),
                            ("rgb10a2", dec.pic_output_dithered(pic, mx.h, "bgr10a2" if bgr else "rgb10a2", **kw), dr.rgb10a2(planes, bd, mx.m, mx.k, mx.ph, bgr=bgr, **ref))):
                        got = host(got)
                        diff = int((got != exp).sum())
                        print(f"{name} {colour['src_transfer']} {mx.name} {what}: {diff} of {exp.size} elements differ")
                        assert diff == 0, (name, colour, mx.name, what)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ 4. phase, 5. flat mean
@pytest.mark.parametrize("name", ["base_p_10b", "random_24x16_12b", "random_40x16_12b"])
def test_phase_is_a_roll_of_the_matrix(name):
    import torch
    planes, bd, crops = (PICS_RGB if name in PICS_RGB else PICS_SEMI)[name]
    dec, pic = open_picture(planes, bd)
    try:
        for _, m, k, ph in matrices()[1:5]:
            ph = ph if ph != (0, 0) else (3, 5)
            with Matrix(dec, ("at", m, k, ph)) as at, Matrix(dec, ("rolled", np.roll(m, (-ph[1], -ph[0]), axis=(0, 1)), k, (0, 0))) as rolled:
                for layout in ("rgb", "rgba", "rgb10a2", "nv12", "p016"):
                    kw = dict(out_bit_depth=8) if layout == "p016" else {}
                    a = dec.pic_output_dithered(pic, at.h, layout, phase=ph, crop=crops[-1], **kw)
                    b = dec.pic_output_dithered(pic, rolled.h, layout, crop=crops[-1], **kw)
                    assert torch.equal(a, b), (name, m.shape, layout)
                    assert not torch.equal(a, dec.pic_output_dithered(pic, at.h, layout, crop=crops[-1], **kw)) or name != "base_p_10b", (m.shape, layout)
    finally:
        dec.close()


def test_flat_mean_is_kept_on_the_device():
    """a permutation matrix with k >= shift and a flat input: the mean over one matrix period is the input, exactly - NV12 U8 from 10 bit, luma and chroma"""
    w, h = 80, 32
    for v in (1, 66, 511, 1018):
        planes = [np.full((h, w), v, np.int16), np.full((h // 2, w // 2), v + 1, np.int16), np.full((h // 2, w // 2), v - 1, np.int16)]
        dec, pic = open_picture(planes, 10)
        try:
            for m in (matrices()[3], matrices()[1]):
                with Matrix(dec, m) as mx:
                    mh, mw = mx.m.shape
                    out = host(dec.pic_output_dithered(pic, mx.h, "nv12", phase=mx.ph)).astype(np.int64)
                    for plane, val in ((out[:h], v), (out[h:, 0::2], v + 1), (out[h:, 1::2], v - 1)):
                        ph, pw = plane.shape[0] // mh * mh, plane.shape[1] // mw * mw
                        blocks = plane[:ph, :pw].reshape(ph // mh, mh, pw // mw, mw).sum(axis=(1, 3))
                        assert np.all(4 * blocks == mh * mw * val), (v, mx.name, val)
        finally:
            dec.close()


# ------------------------------------------------------------------------------------------------ 6. refusals, 7. handles
def test_refused_calls_launch_nothing():
    import torch
    planes, bd, _ = PICS_RGB["base_p_10b"]
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    lib = dec.lib
    try:
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        hd = dec.dither_create("bayer", 8)
        gone = dec.dither_create("bayer", 4)
        dec.dither_destroy(gone)
        rgb = abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_U8)
        nv12 = abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)
        rgba = abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_U8)
        need = lib.xgpu_output_packed_size(C.byref(rgba), w, h, bd)
        t = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        hostbuf = np.zeros(need, np.uint8)
        cm = abi.make_colour_transform(**PQ_SRGB)
        ok = abi.make_dither_params(hd)
        calls = [(rgb, None, ok, t.data_ptr(), 3 * w * h - 1, INVALID),                                   # one byte short
                 (rgb, None, ok, hostbuf.ctypes.data, need, INVALID),                                     # host memory
                 (abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), None, ok, t.data_ptr() + 1, need, INVALID),      # the element is aligned to 2
                 (abi.make_output_format(abi.OUT_RGB_PLANAR, matrix=2), None, ok, t.data_ptr(), need, UNSUPPORTED),      # the plain call's refusal and code
                 (abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F16), None, ok, t.data_ptr(), need, UNSUPPORTED),      # a float dtype
                 (abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_U8), None, ok, t.data_ptr(), need, INVALID),       # a layout outside the list
                 (abi.make_output_format(abi.OUT_YUV420P, abi.OUT_U8, out_bit_depth=8), None, ok, t.data_ptr(), need, INVALID),
                 (nv12, cm, ok, t.data_ptr(), need, INVALID),                                             # a transform on a video surface
                 (rgb, abi.make_colour_transform(**dict(PQ_SRGB, src_transfer=17)), ok, t.data_ptr(), need, UNSUPPORTED),
                 (rgb, None, abi.make_dither_params(gone), t.data_ptr(), need, INVALID),                  # a destroyed handle
                 (rgb, None, abi.make_dither_params(3), t.data_ptr(), need, INVALID),                     # a handle never made
                 (rgb, None, abi.make_dither_params(-1), t.data_ptr(), need, INVALID),
                 (rgb, None, abi.make_dither_params(abi.MAX_DITHER), t.data_ptr(), need, INVALID),
                 (nv12, None, abi.make_dither_params(hd, (8, 0)), t.data_ptr(), need, INVALID),           # a phase outside the matrix
                 (rgb, None, abi.make_dither_params(hd, (0, -1)), t.data_ptr(), need, INVALID),
                 (rgba, None, abi.make_dither_params(hd, (0, 8)), t.data_ptr(), need, INVALID),
                 (abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_F32), None, ok, t.data_ptr(), 4 * need, UNSUPPORTED),
                 (abi.make_packed_format(abi.PACKED_YUYV, abi.OUT_U8, out_bit_depth=8), None, ok, t.data_ptr(), need, INVALID),
                 (abi.make_packed_format(abi.PACKED_RGBA, alpha=1.5), None, ok, t.data_ptr(), need, INVALID),
                 (abi.make_packed_format(abi.PACKED_RGB10A2), None, ok, t.data_ptr() + 2, need, INVALID)]       # the word is aligned to 4
        for f, c, dp, p, n, code in calls:
            fn = lib.xgpu_pic_output_device_dithered if isinstance(f, abi.OutputFormat) else lib.xgpu_pic_output_device_packed_dithered
            rc = fn(dec.ctx, pic, None, C.byref(f), None if c is None else C.byref(c), C.byref(dp), C.c_void_p(p), n, stream_h)
            assert rc == code, (f.layout, f.dtype, dp.handle, dp.phase_x, dp.phase_y, p, n, rc)
            assert b"dithered" in lib.xgpu_last_error(dec.ctx)
        assert lib.xgpu_pic_output_device_dithered(dec.ctx, pic, None, C.byref(rgb), None, None, C.c_void_p(t.data_ptr()), need, stream_h) == INVALID
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all() and not hostbuf.any()
        assert lib.xgpu_pic_output_device_packed_dithered(dec.ctx, pic, None, C.byref(rgba), None, C.byref(ok), C.c_void_p(t.data_ptr()), need, stream_h) == 0
        torch.cuda.synchronize()
        assert (t[need:].cpu().numpy() == 0x5A).all() and (t[3:need:4].cpu().numpy() == 255).all()      # exactly `need` bytes
        # the Python layer's own argument checks
        for kw in (dict(layout="yuv444"), dict(layout="yuyv"), dict(layout="rgb", dtype=torch.float16), dict(layout="rgba", dtype=torch.float32),
                   dict(layout="nv12", colour=PQ_SRGB), dict(layout="rgb10a2", dtype=torch.int16), dict(layout="rgb", matrix=2), dict(layout="rgb", crop=(1, 0, 0, 0)),
                   dict(layout="nv12", out_bit_depth=10), dict(layout="rgba", out=torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:0"))):
            with pytest.raises(ValueError):
                dec.pic_output_dithered(pic, hd, **kw)
    finally:
        dec.close()


def test_handles():
    from xevd_amd.decoder import XgpuError
    planes, bd, _ = PICS_RGB["random_24x16_10b"]
    dec, pic = open_picture(planes, bd)
    lib = dec.lib
    try:
        hs = [dec.dither_create("bayer", 2 << i) for i in range(abi.MAX_DITHER)]
        assert sorted(hs) == list(range(abi.MAX_DITHER))
        h = C.c_int(7)
        one = np.zeros((1, 1), np.uint16)
        ptr = one.ctypes.data_as(C.POINTER(C.c_uint16))
        assert lib.xgpu_dither_create(dec.ctx, 1, 1, 1, ptr, C.byref(h)) == OOM and h.value == -1      # a fifth
        dec.dither_destroy(hs[1])
        with pytest.raises(XgpuError):
            dec.dither_destroy(hs[1])
        with pytest.raises(XgpuError):
            dec.pic_output_dithered(pic, hs[1])      # a destroyed handle is refused
        bad = np.array([[0, 1], [2, 4]], np.uint16)
        assert lib.xgpu_dither_create(dec.ctx, 2, 2, 2, bad.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(h)) == INVALID and h.value == -1      # a rank >= L
        for mw, mh, k in ((3, 1, 1), (1, 256, 1), (0, 1, 1), (1, 1, 0), (1, 1, 15)):
            assert lib.xgpu_dither_create(dec.ctx, mw, mh, k, ptr, C.byref(h)) == UNSUPPORTED, (mw, mh, k)
        again = dec.dither_create(bad.clip(0, 3), levels=4)
        assert again == hs[1] and dec.dither_shape(again) == (2, 2, 2)      # the freed handle is used again
        got = host(dec.pic_output_dithered(pic, again, "rgb"))
        assert np.array_equal(got, dr.rgb(planes, bd, bad.clip(0, 3), 2))
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ 8. stream and tool
def test_stream_decoder_dithers_with_the_phase_of_the_poc():
    import torch
    from xevd_amd.decoder import XgpuError
    from xevd_amd.player import StreamDecoder
    d = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))
    data = d["bytes"].tobytes()
    seen = [(p, planes, p["packed"]) for p, planes in StreamDecoder(data).pictures(tensor=dict(layout="rgb"), packed=dict(layout="rgb10a2"),
                                                                                   dither=dict(kind="blue", size=16, temporal=True))]
    assert len(seen) == int(d["n"])
    still = [t for _, t in StreamDecoder(data).pictures(tensor=dict(layout="nv12"), dither="bayer")]
    blue = abi.dither_blue(abi.load(), 4, 1)
    phases = set()
    for k, (p, t, t10) in enumerate(seen):
        planes = [d[f"p{k}_{c}"] for c in range(3)]
        dec, pic = open_picture(planes, 10)
        try:
            kw = StreamDecoder.tensor_options(p, {})
            ph = abi.dither_phase(dec.lib, p["poc"] & 0xFFFFFFFF, 16, 16)
            phases.add(ph)
            hb, hy = dec.dither_create("blue", 16), dec.dither_create("bayer", 64)
            assert torch.equal(t, dec.pic_output_dithered(pic, hb, "rgb", phase=ph, **kw)), k
            assert torch.equal(t10, dec.pic_output_dithered(pic, hb, "rgb10a2", phase=ph, **kw)), k
            ref = {a: b for a, b in kw.items() if a != "dra"}
            assert np.array_equal(host(t), dr.rgb(planes, 10, blue, 8, ph, dra=kw["dra"], **ref)), k
            assert torch.equal(still[k], dec.pic_output_dithered(pic, hy, "nv12", dra=kw["dra"])), k
        finally:
            dec.close()
    assert len(phases) > 1
    # an option without a dithered form: before decoding starts
    for kw in (dict(tensor=dict(layout="rgb"), size=(32, 32)), dict(tensor=dict(layout="yuv444")), dict(tensor=dict(layout="rgb", dtype=torch.float16)),
               dict(packed=dict(layout="yuyv")), dict(tensor=dict(layout="rgb"), lut=0), dict(), dict(tensor=dict(layout="nv12"), to="srgb"),
               dict(tensor=dict(layout="rgb"), surfaces=[(32, 32)])):
        sd = StreamDecoder(data)
        with pytest.raises(XgpuError):
            next(sd.pictures(dither="blue", **kw))
    with pytest.raises(XgpuError):
        next(StreamDecoder(data).pictures(tensor={}, dither="white"))


def test_app_writes_dithered_nv12(tmp_path):
    """tools/xevd_gpu_app.py --pix-fmt nv12 --dither bayer against its default yuv420p run at the stream's depth, dithered in numpy frame by frame"""
    d = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))
    h, w = d["p0_0"].shape
    n = int(d["n"])
    src, planar, out = tmp_path / "s.evc", tmp_path / "planar.yuv", tmp_path / "nv12.yuv"
    src.write_bytes(d["bytes"].tobytes())
    app = os.path.join(ROOT, "tools", "xevd_gpu_app.py")
    for args in (["-o", str(planar)], ["-o", str(out), "--pix-fmt", "nv12", "--dither", "bayer"]):
        r = subprocess.run([sys.executable, app, "-i", str(src)] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-2000:])
    a = np.fromfile(planar, np.dtype("<u2")).astype(np.int16)
    frame = w * h * 3 // 2
    assert a.size == n * frame
    b = np.fromfile(out, np.uint8)
    assert b.size == n * frame
    b = b.reshape(n, h * 3 // 2, w)
    plain = 0
    for k in range(n):
        f = a[k * frame:(k + 1) * frame]
        planes = [f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)]
        assert np.array_equal(b[k], dr.nv12(planes, 10, 8, dr.bayer(3), 6)), k
        plain += int(np.array_equal(b[k], dr.nv12(planes, 10, 8, np.array([[1]]), 1)))
    assert plain < n      # it is not the rounded surface
