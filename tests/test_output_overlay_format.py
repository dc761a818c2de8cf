"""CPU suite for the overlaid output (xgpu_pic_output_device_overlaid / _packed_overlaid): the exported symbols, the refusal codes of
xgpu_output_overlay_check in their order, the host-only xgpu_overlay_coeffs and xgpu_overlay_box_snap against the numpy restatement tests/overlay_ref.py, and the
restatement's own identities.  Nothing here needs a GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import overlay_ref as ov
from xevd_amd import abi

INVALID, UNSUPPORTED = -101, -104
PQ_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
PTR = 0x1000      # the check does not look at the memory behind a pointer


def check(f=None, pf=None, cm=None, layers=(), boxes=None, n=None, width=64, height=48, bd=10):
    cmt = None if cm is None else abi.make_colour_transform(**cm)
    arr = (abi.OverlayLayer * max(len(layers), 1))(*layers)
    return abi.load().xgpu_output_overlay_check(None if f is None else C.byref(f), None if pf is None else C.byref(pf), None if cmt is None else C.byref(cmt),
                                                arr if layers else None, len(layers) if n is None else n, None if boxes is None else C.byref(boxes),
                                                width, height, bd)


def bitmap(kind=abi.OVL_RGBA8, x=0, y=0, w=4, h=4, **kw):
    return abi.make_overlay_layer(kind, x, y, w, h, d_pixels=kw.pop("d_pixels", PTR), **kw)


def box(x=0, y=0, w=4, h=4, **kw):
    return abi.make_overlay_layer(abi.OVL_BOX, x, y, w, h, **kw)


RGB = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8)
NV12 = abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)


def test_exported_symbols():
    for name in ("xgpu_overlay_coeffs", "xgpu_overlay_box_snap", "xgpu_output_overlay_check", "xgpu_pic_output_device_overlaid",
                 "xgpu_pic_output_device_packed_overlaid"):
        assert name in abi.exported_names(), name
        assert hasattr(abi.load(), name)
    assert (abi.MAX_OVERLAY_LAYERS, abi.MAX_OVERLAY_BOXES) == (16, 256)
    assert C.sizeof(abi.OverlayLayer) == 56 and C.sizeof(abi.OverlayBoxes) == 120      # the C structs on an LP64 host


def test_check_accepts_every_listed_form():
    layers = [bitmap(), bitmap(abi.OVL_BGRA8, -5, 70, 16384, 16384, pitch=4 * 16384 + 4), bitmap(abi.OVL_A8, 1 << 20, -(1 << 20), 3, 3, d_pixels=PTR + 1, pitch=5),
              box(thickness=1), box(-4, -4, 100, 100, thickness=1000, opacity=0)]
    boxes = abi.make_overlay_boxes(abi.BOX_XYXY_F32, PTR, 256, PTR, PTR, palette=[(1, 2, 3, 4)] * 16, thickness=1, fill_alpha=255)
    for bd in (8, 10, 12):
        for lay, dt, cm in itertools.product((abi.OUT_RGB_PLANAR, abi.OUT_RGB_INTERLEAVED), (abi.OUT_U8, abi.OUT_U16), (None, PQ_SRGB)):
            assert check(abi.make_output_format(lay, dt, bgr=True), cm=cm, layers=layers, boxes=boxes, bd=bd) == 0, (bd, lay, dt, cm)
        assert check(abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8), layers=layers, boxes=boxes, bd=bd) == 0
        assert check(abi.make_output_format(abi.OUT_NV12, abi.OUT_U16, out_bit_depth=10, matrix=9, full_range=True), layers=layers, bd=bd) == 0
        for d in (0, 8, 10, 12, 16):
            assert check(abi.make_output_format(abi.OUT_P016, abi.OUT_U16, out_bit_depth=d), layers=layers, bd=bd) == 0
        for dt, cm in itertools.product((abi.OUT_U8, abi.OUT_U16), (None, PQ_SRGB)):
            assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, dt, bgr=True, alpha=0.5), cm=cm, layers=layers, boxes=boxes, bd=bd) == 0
            assert check(pf=abi.make_packed_format(abi.PACKED_RGB10A2, bgr=dt == abi.OUT_U8), cm=cm, layers=layers, bd=bd) == 0
    assert check(RGB) == 0 and check(RGB, layers=[box()] * 16) == 0      # no layer at all; sixteen
    assert check(RGB, boxes=abi.make_overlay_boxes(abi.BOX_XYWH_I32, PTR, 1)) == 0


def test_check_refusals_come_in_their_order():
    bad_layer = [bitmap(kind=7)]
    # neither or both formats
    assert check() == INVALID and check(RGB, abi.make_packed_format()) == INVALID
    # 1. the plain call's refusals, with its codes: before the dtype, the layout, the transform and the layers
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, matrix=2), layers=bad_layer) == UNSUPPORTED
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, crop=(1, 0, 0, 0)), layers=bad_layer) == INVALID
    assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16, out_bit_depth=12), bd=10) == INVALID
    assert check(abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_U8, row_pitch=3 * 64 - 1)) == INVALID
    assert check(abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=10)) == INVALID
    assert check(RGB, bd=13) == INVALID and check(RGB, width=0) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_F16, matrix=2)) == UNSUPPORTED
    assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_F16, alpha=1.5)) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_RGB10A2, dtype=abi.OUT_U16)) == INVALID
    # 2. a float dtype: UNSUPPORTED, before the layout (YUV444 has float forms), the transform and the layers
    for dt in (abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32):
        assert check(abi.make_output_format(abi.OUT_RGB_PLANAR, dt), layers=bad_layer) == UNSUPPORTED
        assert check(abi.make_output_format(abi.OUT_YUV444_PLANAR, dt), layers=bad_layer) == UNSUPPORTED
        assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, dt), layers=bad_layer) == UNSUPPORTED
        assert check(pf=abi.make_packed_format(abi.PACKED_RGBA, dt), cm=PQ_SRGB) == UNSUPPORTED
    # 3. a layout outside the list: INVALID, before a transform that would be UNSUPPORTED
    bad_cm = dict(PQ_SRGB, src_transfer=17)
    assert check(abi.make_output_format(abi.OUT_YUV420P, abi.OUT_U8, out_bit_depth=8), cm=bad_cm) == INVALID
    assert check(abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_U8), cm=bad_cm) == INVALID
    assert check(abi.make_output_format(abi.OUT_YUV444_INTERLEAVED, abi.OUT_U16)) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_YUYV, abi.OUT_U8, out_bit_depth=8), cm=bad_cm) == INVALID
    assert check(pf=abi.make_packed_format(abi.PACKED_UYVY, abi.OUT_U16)) == INVALID
    # 4. a transform with NV12 / P016: INVALID whatever the transform; then the surface's own matrix and range
    assert check(NV12, cm=bad_cm) == INVALID and check(NV12, cm=PQ_SRGB) == INVALID
    assert check(abi.make_output_format(abi.OUT_P016, abi.OUT_U16), cm=PQ_SRGB) == INVALID
    assert check(abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8, matrix=2), layers=bad_layer) == UNSUPPORTED
    # ... the transform's own refusal (UNSUPPORTED) before the layers' (INVALID)
    assert check(RGB, cm=bad_cm, layers=bad_layer) == UNSUPPORTED
    assert check(pf=abi.make_packed_format(abi.PACKED_RGBA), cm=bad_cm, layers=bad_layer) == UNSUPPORTED
    # 5. the layers
    assert check(RGB, layers=[box()] * 17) == INVALID and check(RGB, n=-1) == INVALID and check(RGB, n=1) == INVALID      # too many, negative, a NULL list
    for l in (bitmap(kind=4), bitmap(kind=-1), bitmap(w=0), bitmap(h=0), bitmap(w=16385), bitmap(h=16385), bitmap(x=(1 << 20) + 1), bitmap(y=-(1 << 20) - 1),
              bitmap(opacity=-1), bitmap(opacity=256), box(thickness=0), box(thickness=-3), bitmap(d_pixels=0), bitmap(d_pixels=PTR + 2),
              bitmap(abi.OVL_BGRA8, d_pixels=PTR + 1), bitmap(pitch=15), bitmap(pitch=18), bitmap(abi.OVL_A8, pitch=3), bitmap(abi.OVL_BGRA8, w=5, pitch=16)):
        assert check(RGB, layers=[box(), l]) == INVALID, (l.kind, l.x, l.y, l.width, l.height, l.opacity, l.thickness, l.d_pixels, l.pitch)
        assert check(NV12, layers=[l]) == INVALID and check(pf=abi.make_packed_format(abi.PACKED_RGB10A2), layers=[l]) == INVALID
    assert check(RGB, layers=[box(thickness=0, d_pixels=0), bitmap(abi.OVL_A8, d_pixels=PTR + 3, pitch=4)][1:]) == 0      # A8 has no alignment
    mk = abi.make_overlay_boxes
    for b in (mk(2, PTR, 4), mk(-1, PTR, 4), mk(0, PTR, 0), mk(0, PTR, 257), mk(1, 0, 4), mk(1, PTR + 2, 4), mk(1, PTR, 4, d_count=PTR + 1), mk(1, PTR, 4, d_labels=PTR + 2),
              mk(0, PTR, 4, n_palette=0), mk(0, PTR, 4, n_palette=17), mk(0, PTR, 4, thickness=0), mk(0, PTR, 4, fill_alpha=-1), mk(0, PTR, 4, fill_alpha=256)):
        assert check(RGB, boxes=b) == INVALID, (b.box_format, b.d_boxes, b.capacity, b.n_palette, b.thickness, b.fill_alpha)


@pytest.mark.parametrize("matrix", [1, 5, 7, 9])
def test_coeffs_are_the_reference_table(matrix):
    lib = abi.load()
    for full, d in itertools.product((False, True), (8, 10, 12, 16)):
        f = abi.make_output_format(abi.OUT_P016, abi.OUT_U16, out_bit_depth=d, matrix=matrix, full_range=full)
        m, off, s = abi.overlay_coeffs(lib, f, 10)
        rm, roff, rs = ov.forward_matrix(matrix, full, d)
        assert (m, off, s) == ([int(v) for v in rm.flatten()], roff, rs) and s == 28 - d, (matrix, full, d)
        # every product fits int32; greys are exactly neutral; chroma of a saturated colour reaches the clip
        assert np.abs(rm).max() * 255 * 3 < 1 << 31
        grey = ov.to_ycc(np.stack([np.arange(256)] * 3, axis=-1), matrix, full, d)
        assert np.all(grey[:, 1:] == 1 << (d - 1)), (matrix, full, d)
        top = (1 << d) - 1
        assert grey[0, 0] == (0 if full else 16 << (d - 8)) and grey[255, 0] == (top if full else 235 << (d - 8))
        sat = ov.to_ycc(np.array([[0, 0, 255], [255, 0, 0]]), matrix, full, d)
        assert sat[0, 1] == (top if full else 240 << (d - 8)) and sat[1, 2] == sat[0, 1]
    nv = abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8, matrix=matrix)
    assert abi.overlay_coeffs(lib, nv, 10)[2] == 20 and abi.overlay_coeffs(lib, abi.make_output_format(abi.OUT_P016, abi.OUT_U16, matrix=matrix), 12)[2] == 16
    assert abi.overlay_coeffs(lib, abi.make_output_format(abi.OUT_RGB_PLANAR, matrix=matrix), 10) == INVALID
    assert abi.overlay_coeffs(lib, abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8, matrix=2), 10) == UNSUPPORTED
    assert abi.overlay_coeffs(lib, nv, 13) == INVALID


def test_box_snap_is_the_reference():
    lib = abi.load()
    big = float(1 << 20)
    nan, inf = float("nan"), float("inf")
    f32 = [(1.5, 2.5, 3.2, 7.0), (0.0, 0.0, 0.0, 5.0), (3.0, 3.0, 3.0, 3.0), (3.0, 1.0, 2.0, 9.0), (-4.25, -0.5, -1.75, 0.5), (nan, 0, 4, 4), (0, 0, 4, nan),
           (0, inf, 4, 4), (-inf, 0, 4, 4), (0, 0, inf, 4), (-big - 1, -big + 1, big + 1, big - 1), (big + 1, 0, big + 9, 4), (-big - 9, 0, -big - 1, 4),
           (1e30, -1e30, 2e30, 1e30), (0.999, 0.001, 1.001, 1.999), (7.0, 7.0, 8.0, 8.0), (-0.0, -0.0, 0.5, 0.5)]
    for b in f32:
        got = abi.overlay_box_snap(lib, np.array(b, np.float32))
        assert got == ov.box_snap(np.array(b, np.float32), True), b
    top = 1 << 20
    i32 = [(1, 2, 3, 4), (0, 0, 0, 5), (0, 0, 5, 0), (0, 0, -1, 5), (-9, -9, 4, 4), (-9, -9, 20, 20), (top + 1, 0, 5, 5), (top - 1, top - 1, 5, 5), (-top - 9, 0, 5, 5),
           (-top - 1, -top + 1, 3, 3), (2147483647, 2147483647, 2147483647, 2147483647), (-2147483648, -2147483648, 2147483647, 1), (top, 0, 1, 1), (top - 1, 0, 1, 1)]
    for b in i32:
        got = abi.overlay_box_snap(lib, np.array(b, np.int32))
        assert got == ov.box_snap(b, False), b
    assert abi.overlay_box_snap(lib, np.array(f32[0], np.float32)) == (1, 2, 4, 7) and abi.overlay_box_snap(lib, np.array(f32[5], np.float32)) is None
    assert abi.overlay_box_snap(lib, np.array(i32[10], np.int32)) is None and abi.overlay_box_snap(lib, np.array(i32[5], np.int32)) == (-9, -9, 11, 11)
    r = (C.c_int * 4)()
    assert lib.xgpu_overlay_box_snap(2, np.zeros(4, np.int32).ctypes.data_as(C.c_void_p), r) == INVALID and lib.xgpu_overlay_box_snap(0, None, r) == INVALID


def test_reference_identities():
    rng = np.random.default_rng(3)
    h, w = 8, 12
    for maxv in (255, 1023, 4095):
        v = rng.integers(0, maxv + 1, (h, w, 3))
        px = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        # a == 0 leaves v: alpha 0, opacity 0, and alpha 1 with opacity 1 ((1 * 1 + 127) // 255 == 0)
        for alpha, opacity in ((0, 255), (255, 0), (1, 1), (127, 1)):
            px[..., 3] = alpha
            assert np.array_equal(ov.blend_rgb(v, maxv, [dict(kind="rgba", pixels=px, opacity=opacity)]), v), (maxv, alpha, opacity)
        # a == 255 gives cD
        px[..., 3] = 255
        cd = (px[..., :3].astype(np.int64) * maxv + 127) // 255
        assert np.array_equal(ov.blend_rgb(v, maxv, [dict(kind="rgba", pixels=px)]), cd)
        assert np.array_equal(ov.blend_rgb(v, maxv, [dict(kind="bgra", pixels=px)]), cd[..., ::-1])
        assert np.array_equal(ov.blend_rgb(v, maxv, [dict(kind="box", box=(-3, -3, 99, 99), thickness=1, colour=(9, 9, 9, 9), fill=(255, 0, 128, 255))]),
                              np.broadcast_to((np.array([255, 0, 128]) * maxv + 127) // 255, v.shape))
        # the numerator stays below 2^24 at the 16-bit maximum
        assert 65535 * 255 + 127 < 1 << 24
    # the chroma rule: A == 0 leaves the sample, A == 1020 of one colour gives its converted chroma, and luma alike
    for d, lsh in ((8, 0), (10, 0), (10, 6), (12, 4), (16, 0)):
        top = (1 << d) - 1
        surf = (rng.integers(0, top + 1, (h * 3 // 2, w)) << lsh).astype(np.uint8 if d == 8 else np.uint16)
        assert np.array_equal(ov.semiplanar(surf, d, [dict(kind="a8", pixels=np.zeros((h, w), np.uint8))], lsh=lsh), surf)
        assert np.array_equal(ov.semiplanar(surf, d, [dict(kind="box", box=(0, 0, w, h), colour=(1, 2, 3, 0))], lsh=lsh), surf)
        for col in ((255, 255, 255), (0, 0, 0), (200, 30, 90), (0, 0, 255)):
            out = ov.semiplanar(surf, d, [dict(kind="box", box=(0, 0, w, h), thickness=99, colour=col + (255,))], matrix=9, lsh=lsh).astype(np.int64) >> lsh
            ycc = ov.to_ycc(np.array(col), 9, False, d)
            assert np.all(out[:h] == ycc[0]) and np.all(out[h:, 0::2] == ycc[1]) and np.all(out[h:, 1::2] == ycc[2]), (d, col)
        # one covered pixel of four: a quarter of the way, rounded
        one = ov.semiplanar(np.zeros_like(surf), d, [dict(kind="box", box=(2, 2, 1, 1), colour=(0, 0, 255, 255))], full_range=True, lsh=lsh).astype(np.int64) >> lsh
        assert one[h + 1, 2] == (255 * top + 510) // 1020 and one[h + 1, 3] == (255 * ov.to_ycc(np.array((0, 0, 255)), 1, True, d)[2] + 510) // 1020
        assert 4 * 255 * 65535 < 1 << 26
    # a frame is measured on the unclipped rectangle: a box hanging over the edge draws no line along the image edge
    flat = np.zeros((h, w, 3), np.int64)
    out = ov.blend_rgb(flat, 255, [dict(kind="box", box=(-5, 2, 9, 4), thickness=1, colour=(255, 255, 255, 255))])
    assert out[3, 0, 0] == 0 and out[2, 0, 0] == 255 and out[5, 0, 0] == 255 and out[3, 3, 0] == 255
    # order matters
    a, b = dict(kind="box", box=(0, 0, 4, 4), thickness=9, colour=(255, 0, 0, 128)), dict(kind="box", box=(2, 2, 4, 4), thickness=9, colour=(0, 0, 255, 128))
    assert not np.array_equal(ov.blend_rgb(flat, 255, [a, b]), ov.blend_rgb(flat, 255, [b, a]))
    # device boxes: the live count, labels of either sign, skipped boxes
    arr = np.array([[0, 0, 4, 4], [1, 1, 0, 3], [2, 2, 3, 3], [5, 5, 2, 2]], np.int32)
    pal = [(255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255)]
    ls = ov.box_layers(dict(array=arr, count=9, labels=np.array([-1, 0, 4, 3], np.int32), palette=pal, thickness=1, fill_alpha=7))
    assert [l["colour"] for l in ls] == [pal[2], pal[1], pal[0]] and ls[0]["fill"] == (0, 0, 255, 7)
    assert len(ov.box_layers(dict(array=arr, count=-2))) == 0 and len(ov.box_layers(dict(array=arr, count=1))) == 1 and len(ov.box_layers(dict(array=arr))) == 3
