"""GPU suite for xgpu_pic_output_device_warp / XgpuDecoder.pic_output_warped / StreamDecoder.pictures(warp=): N affine maps of one picture as a batch of images
from one launch, against the restatement of the contract (tests/warp_ref.py), against the plain output where the two must agree, and against numpy's own flips
and rotation.  Every comparison is bit for bit, with the conventions of test_gpu_output_scaled.py (integers as they are, float32 by its bit pattern, float16 /
bfloat16 by the bit pattern of the restatement's float32 rounded to nearest even)."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_io
import test_gpu_output_scaled as ts
import warp_ref as wr
from test_gpu_output_rois import check_batch
from xevd_amd import abi

pytestmark = pytest.mark.gpu

W, H = 320, 200
SIZE = (48, 64)
MEAN, STD = ts.MEAN, ts.STD
NORM = dict(mean=np.asarray(MEAN, np.float32), inv_std=ts.inv_std(STD))
Q = 65536
IDENTITY = wr.IDENTITY
HFLIP, VFLIP = (-Q, 0, (W - 1) * Q, 0, Q, 0), (Q, 0, 0, 0, -Q, (H - 1) * Q)
ROT90 = (0, -Q, (W - 1) * Q, Q, 0, 0)      # numpy.rot90 of the picture: out[i, j] = Y[j, W - 1 - i]
MAPS = [
    IDENTITY,
    (Q, 0, 37 * Q, 0, Q, 21 * Q),                                       # an integer shift
    (Q, 0, 10 * Q + Q // 2, 0, Q, 5 * Q + Q // 2),                      # a half-sample shift
    HFLIP, VFLIP,
    (0, -Q, 150 * Q, Q, 0, 20 * Q),                                     # a 90-degree rotation
    wr.from_rotated_box(300, 20, 120, 80, 30, SIZE),                    # a 30-degree box that leaves the picture at the top and on the right
    wr.from_matrix((3.7, 0.9, 5, 0.2, 3.7, 3)),                         # a sheared 3.7x reduction
    wr.from_matrix((0.125, 0, 312, 0, 0.125, 194)),                     # an 8x enlargement in the bottom-right corner
    (0, 0, 100 * Q, 0, 0, 50 * Q + 12345),                              # an all-zero linear part: one position for the whole image
    (Q, 0, -500 * Q, 0, Q, 400 * Q),                                    # entirely outside the picture
    IDENTITY,                                                           # a duplicate
]
TRIPLES = (("rgb", abi.OUT_U8, False), ("yuv444", abi.OUT_U16, False), ("rgb", abi.OUT_F32, True))


def maps_array(maps=MAPS):
    return np.asarray(maps, np.int64).reshape(-1, 6)


def run(dec, pic, planes, bd, maps=MAPS, size=SIZE, layout="rgb", code=abi.OUT_U8, channels_last=False, normalise=False, samples=1, border="clamp", pad=None, what="",
        **kw):
    """one batch and its comparison with the restatement; kw: matrix, full_range, chroma_loc, crop, dra, bgr"""
    if pad is None:
        pad = (17, 0, 200) if code in (abi.OUT_U8, abi.OUT_U16) else (0.25, -0.5, 0.447)
    norm = dict(mean=MEAN, std=STD) if normalise else {}
    t = dec.pic_output_warped(pic, maps_array(maps), size, layout=layout, channels_last=channels_last, dtype=ts.torch_dtype(code), samples=samples, border=border,
                              pad=pad, **norm, **kw)
    assert tuple(t.shape) == ((len(maps), *size, 3) if channels_last else (len(maps), 3, *size))
    exp = wr.batch(planes, bd, size, maps, samples, wr.PAD if border == "pad" else wr.CLAMP, pad, layout=layout, dtype=code, **(NORM if normalise else {}), **kw)
    check_batch(t, exp, code, channels_last, what or (size, layout, code, channels_last, normalise, samples, border, kw))
    return t


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_restatement(bd):
    planes = ts.random_planes(W, H, bd, seed=700 + bd, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        for samples in (1, 2, 4):
            for border in ("clamp", "pad"):
                for layout, code, normalise in TRIPLES:
                    run(dec, pic, planes, bd, layout=layout, code=code, normalise=normalise, samples=samples, border=border)
        # a width that crosses the 64-column tile with a height that is no multiple of 4, and the smallest image
        for size in ((50, 70), (2, 2)):
            for samples, border, (layout, code, normalise) in ((1, "pad", TRIPLES[0]), (2, "clamp", TRIPLES[1]), (4, "pad", TRIPLES[2])):
                run(dec, pic, planes, bd, size=size, layout=layout, code=code, normalise=normalise, samples=samples, border=border)
    finally:
        dec.close()


def test_layouts_dtypes_sitings_and_dra():
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=711, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        run(dec, pic, planes, bd, layout="rgb", code=abi.OUT_F16, channels_last=True, normalise=True, samples=2, border="pad", bgr=True)
        run(dec, pic, planes, bd, layout="yuv444", code=abi.OUT_BF16, channels_last=False, samples=1, border="pad", full_range=True)
        run(dec, pic, planes, bd, layout="yuv444", code=abi.OUT_U8, channels_last=True, samples=4)
        run(dec, pic, planes, bd, layout="rgb", code=abi.OUT_U16, channels_last=True, samples=1, border="pad", matrix=9, full_range=True, pad=(0, 1023, 512))
        for loc in range(6):
            run(dec, pic, planes, bd, layout="yuv444", code=abi.OUT_U16, samples=1 + (loc & 1), chroma_loc=loc, crop=(2 * loc, 4, 6, 2 * loc))
    finally:
        dec.close()
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    h, w = planes[0].shape
    maps = [IDENTITY, wr.from_rotated_box(w / 2, h / 2, w * 0.8, h * 0.6, -20, SIZE), wr.from_matrix((2.5, 0, -10, 0, 2.5, -10)), (-Q, 0, (w - 1) * Q, 0, -Q, (h - 1) * Q)]
    dec, pic = ts.open_picture(planes, 10)
    try:
        luts = d["three_ranges_idx58_luts"]
        run(dec, pic, planes, 10, maps, layout="yuv444", code=abi.OUT_U16, samples=2, dra=luts, what="dra yuv444")
        run(dec, pic, planes, 10, maps, code=abi.OUT_F32, normalise=True, samples=1, border="pad", dra=luts, matrix=9, crop=(2, 4, 0, 2), what="dra rgb")
    finally:
        dec.close()


def test_identity_translation_and_geometry_against_the_plain_output():
    import torch
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=713, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    try:
        # the identity at the picture's size is the plain output with linear upsampling, for every siting
        for loc in range(6):
            for layout, code in (("yuv444", abi.OUT_U16), ("rgb", abi.OUT_U8)):
                t = dec.pic_output_warped(pic, maps_array([IDENTITY]), (H, W), layout=layout, dtype=ts.torch_dtype(code), chroma_loc=loc)
                plain = dec.pic_output_tensor(pic, layout=layout, dtype=ts.torch_dtype(code), upsample="linear", chroma_loc=loc)
                torch.cuda.synchronize()
                assert torch.equal(t[0], plain), (layout, code, loc)
        # An integer translation is the plain output of that crop.  The crop of the plain output is a wall - its chroma upsampling clamps at the crop's edge -
        # while the translated image still sees the picture beyond it, so: where the crop's cut sides have no chroma neighbour beyond them (type 2 - co-sited,
        # top - reads only to the right and below; the crop reaches the picture's right and bottom edge) the two are equal everywhere; for every siting and a
        # crop inside the picture, Y is equal everywhere and all three channels two pixels inside the frame.
        x0, y0 = 38, 22
        shift = (Q, 0, x0 * Q, 0, Q, y0 * Q)
        for layout, code in (("yuv444", abi.OUT_U16), ("rgb", abi.OUT_U8)):
            t = dec.pic_output_warped(pic, maps_array([shift]), (H - y0, W - x0), layout=layout, dtype=ts.torch_dtype(code), chroma_loc=2)
            plain = dec.pic_output_tensor(pic, layout=layout, dtype=ts.torch_dtype(code), upsample="linear", chroma_loc=2, crop=(x0, 0, y0, 0))
            torch.cuda.synchronize()
            assert torch.equal(t[0], plain), (layout, code)
        hh, ww = 90, 150
        for loc in range(6):
            t = dec.pic_output_warped(pic, maps_array([shift]), (hh, ww), layout="yuv444", dtype=torch.int16, chroma_loc=loc)
            plain = dec.pic_output_tensor(pic, layout="yuv444", dtype=torch.int16, upsample="linear", chroma_loc=loc, crop=(x0, W - x0 - ww, y0, H - y0 - hh))
            r = dec.pic_output_warped(pic, maps_array([shift]), (hh, ww), dtype=torch.uint8, chroma_loc=loc)
            rplain = dec.pic_output_tensor(pic, dtype=torch.uint8, upsample="linear", chroma_loc=loc, crop=(x0, W - x0 - ww, y0, H - y0 - hh))
            torch.cuda.synchronize()
            assert torch.equal(t[0, 0], plain[0]), loc
            assert torch.equal(t[0, :, 2:-2, 2:-2], plain[:, 2:-2, 2:-2]) and torch.equal(r[0, :, 2:-2, 2:-2], rplain[:, 2:-2, 2:-2]), loc
        # geometry without the restatement: the Y plane of the flips and of the quarter turn is numpy's
        y = dec.pic_output_tensor(pic, layout="yuv444", dtype=torch.int16, upsample="linear")[0].cpu().numpy()
        flips = dec.pic_output_warped(pic, maps_array([HFLIP, VFLIP]), (H, W), layout="yuv444", dtype=torch.int16).cpu().numpy()
        assert np.array_equal(flips[0, 0], np.flip(y, 1)) and np.array_equal(flips[1, 0], np.flip(y, 0))
        rot = dec.pic_output_warped(pic, maps_array([ROT90]), (W, H), layout="yuv444", dtype=torch.int16).cpu().numpy()
        assert np.array_equal(rot[0, 0], np.rot90(y))
    finally:
        dec.close()


def test_the_crop_is_a_wall():
    bd = 10
    crop = (16, 24, 8, 12)
    a = ts.random_planes(W, H, bd, seed=717, rails=True)
    b = ts.random_planes(W, H, bd, seed=718)
    for pa, pb, s in zip(a, b, (1, 2, 2)):      # the same samples inside the crop, others everywhere else
        hh, ww = pa.shape
        pb[crop[2] // s:hh - crop[3] // s, crop[0] // s:ww - crop[1] // s] = pa[crop[2] // s:hh - crop[3] // s, crop[0] // s:ww - crop[1] // s]
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    ws, hs = W - crop[0] - crop[1], H - crop[2] - crop[3]
    maps = [IDENTITY, (Q, 0, -20 * Q, 0, Q, -9 * Q - 1000), (-Q, 0, (ws + 10) * Q, 0, -Q, (hs + 10) * Q), wr.from_rotated_box(ws, hs, 200, 150, 40, SIZE),
            wr.from_matrix((6.0, 0.5, -30, -0.5, 5.0, -20))]
    got = []
    for planes in (a, b):
        dec, pic = ts.open_picture(planes, bd)
        try:
            for samples, (layout, code) in ((1, ("yuv444", abi.OUT_U16)), (4, ("rgb", abi.OUT_U8))):
                t = run(dec, pic, planes, bd, maps, layout=layout, code=code, samples=samples, border="clamp", crop=crop, chroma_loc=1)
                got.append(t.cpu().numpy())
        finally:
            dec.close()
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])


def test_maps_in_device_memory():
    """the same maps as an int64 tensor give the host call's bytes; a map past a limit and one made of INT64_MIN / INT64_MAX are data like any other for the
    kernel - every position is clamped before it addresses memory - and give status 1 and an image that is all pad, their neighbours unchanged"""
    import torch
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=719, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    lo, hi = -(1 << 63), (1 << 63) - 1
    past = list(MAPS[7])
    past[0] = wr.LIN_LIMIT + 1
    bad = [tuple(past), (lo, hi, lo, hi, lo, hi), (Q, 0, wr.OFF_LIMIT + 1, 0, Q, 0), (hi, hi, hi, hi, hi, hi)]
    maps = MAPS[:3] + bad[:1] + MAPS[3:8] + bad[1:3] + MAPS[8:] + bad[3:]
    status = [0 if wr.map_ok(m) else 1 for m in maps]
    assert sum(status) == 4
    try:
        for (layout, code, normalise), samples, border in zip(TRIPLES, (1, 4, 2), ("clamp", "pad", "clamp")):
            pad = (17, 0, 200) if not normalise else (0.25, -0.5, 0.447)
            norm = dict(mean=MEAN, std=STD) if normalise else {}
            d_maps = torch.from_numpy(maps_array(maps)).to("cuda:0")
            t, st = dec.pic_output_warped(pic, d_maps, SIZE, layout=layout, dtype=ts.torch_dtype(code), samples=samples, border=border, pad=pad, status=True, **norm)
            assert st.dtype == torch.int32 and st.cpu().tolist() == status
            exp = wr.batch(planes, bd, SIZE, maps, samples, wr.PAD if border == "pad" else wr.CLAMP, pad, layout=layout, dtype=code, **(NORM if normalise else {}))
            check_batch(t, exp, code, what=("device maps", layout, code))
            good = [i for i, s in enumerate(status) if not s]
            host = dec.pic_output_warped(pic, maps_array([maps[i] for i in good]), SIZE, layout=layout, dtype=ts.torch_dtype(code), samples=samples, border=border,
                                         pad=pad, **norm)
            assert np.array_equal(ts.tensor_bits(t[good], code), ts.tensor_bits(host, code))
            # without the status tensor
            t2 = dec.pic_output_warped(pic, d_maps, SIZE, layout=layout, dtype=ts.torch_dtype(code), samples=samples, border=border, pad=pad, **norm)
            assert np.array_equal(ts.tensor_bits(t2, code), ts.tensor_bits(t, code))
        for wrong in (d_maps.to(torch.int32), d_maps.cpu(), d_maps.t(), d_maps[:, :4]):
            with pytest.raises(ValueError):
                dec.pic_output_warped(pic, wrong, SIZE)
        with pytest.raises(ValueError):      # the pad is read for device maps, whatever the border
            dec.pic_output_warped(pic, d_maps, SIZE, pad=0.5)
        with pytest.raises(ValueError):
            dec.pic_output_warped(pic, maps_array(), SIZE, status=True)
    finally:
        dec.close()


def test_out_with_batch_stride_and_padded_rows():
    import torch
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=723)
    dec, pic = ts.open_picture(planes, bd)
    maps = MAPS[5:10]
    n, (hd, wd) = len(maps), SIZE
    try:
        for cl, code, off in ((False, abi.OUT_U8, 7), (False, abi.OUT_F32, 3), (True, abi.OUT_F16, 5)):
            dt = ts.torch_dtype(code)
            fill = 0xA5 if code == abi.OUT_U8 else -3.0
            pad = 9 if code == abi.OUT_U8 else 0.5
            pitch = (3 * wd if cl else wd) + 13                       # elements between rows
            image = (hd if cl else 3 * hd) * pitch
            stride = image + 37                                       # elements between images
            buf = torch.full((off + n * stride + 11,), fill, dtype=dt, device="cuda:0")
            view = torch.as_strided(buf, (n, hd, wd, 3) if cl else (n, 3, hd, wd), (stride, pitch, 3, 1) if cl else (stride, hd * pitch, pitch, 1), off)
            out = dec.pic_output_warped(pic, maps_array(maps), SIZE, channels_last=cl, dtype=dt, samples=2, border="pad", pad=pad, out=view)
            assert out is view
            check_batch(view, wr.batch(planes, bd, SIZE, maps, 2, wr.PAD, pad, dtype=code), code, cl, ("out", cl, code))
            untouched = torch.ones(buf.numel(), dtype=torch.bool, device="cuda:0")
            torch.as_strided(untouched, view.shape, view.stride(), off).fill_(False)
            assert int(untouched.sum()) == buf.numel() - view.numel()
            assert bool((buf[untouched] == fill).all()), (cl, code)      # every gap between rows and images, and the tail behind the last image
        t = torch.empty((n, 3, hd, wd), dtype=torch.uint8, device="cuda:0")
        assert dec.pic_output_warped(pic, maps_array(maps), SIZE, out=t) is t
        check_batch(t, wr.batch(planes, bd, SIZE, maps), abi.OUT_U8, what="contiguous out")
        for wrong in (t[:3], t.to(torch.int16), torch.as_strided(t, t.shape, (hd * wd, hd * wd, wd, 1)), t.permute(0, 1, 3, 2)):
            with pytest.raises(ValueError):
                dec.pic_output_warped(pic, maps_array(maps), SIZE, out=wrong)
    finally:
        dec.close()


def test_refusals_queue_nothing_and_thetas():
    import torch
    bd = 8
    planes = ts.random_planes(W, H, bd, seed=727)
    dec, pic = ts.open_picture(planes, bd)
    lib = dec.lib
    try:
        fmt, sc, wp = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), abi.make_scale_params(SIZE[1], SIZE[0]), abi.make_warp_params()
        image = 3 * SIZE[0] * SIZE[1] * 2
        need = abi.output_warp_size(lib, fmt, sc, wp, len(MAPS), W, H, bd)
        assert need == len(MAPS) * image
        t = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        host = np.zeros(need, np.uint8)
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call(maps=MAPS, f=fmt, s=sc, w=wp, p=None, n=need, count=None, on_device=0, raw=None):
            return lib.xgpu_pic_output_device_warp(dec.ctx, pic, None, C.byref(f), C.byref(s), C.byref(w), abi.make_warp_maps(maps) if raw is None else raw, on_device,
                                                   len(maps) if count is None else count, None, C.c_void_p(t.data_ptr() if p is None else p), n, stream_h)

        assert call(p=host.ctypes.data) == -101                     # host memory
        assert call(n=need - 1) == -101                             # too short for the batch
        assert call(p=t.data_ptr() + 1) == -101                     # not aligned to the 2-byte element
        assert "pic_output_device_warp" in lib.xgpu_last_error(dec.ctx).decode()
        assert call(count=0) == -101 and call(count=abi.MAX_ROIS + 1) == -101
        assert call(MAPS[:3] + [(Q, 0, 0, 0, wr.LIN_LIMIT + 1, 0)]) == -101 and "map 3" in lib.xgpu_last_error(dec.ctx).decode()
        assert call(w=abi.make_warp_params(samples=3)) == -101 and call(w=abi.make_warp_params(border=2)) == -101
        assert call(w=abi.make_warp_params(border=abi.WARP_PAD, pad=0.5)) == -101
        assert call(w=abi.make_warp_params(image_pitch=image + 2)) == -101      # the batch no longer fits the destination
        assert call(s=abi.make_scale_params(SIZE[1], SIZE[0], filter=abi.SCALE_AREA)) == -101
        assert call(s=abi.make_scale_params(SIZE[1], 1)) == -104
        assert call(f=abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)) == -101
        assert call(on_device=1) == -101                            # "device maps" that are host memory
        assert call(on_device=2) == -101 and call(raw=C.c_void_p(0)) == -101
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all()
        for wrong in (dict(border="wrap"), dict(samples=3), dict(layout="nv12"), dict(border="pad", pad=0.5), dict(dtype=torch.uint8, mean=MEAN)):
            with pytest.raises(ValueError):
                dec.pic_output_warped(pic, maps_array(), SIZE, **wrong)
        with pytest.raises(ValueError, match="theta 1 "):
            dec.pic_output_warped(pic, [(1, 0, 0, 0, 1, 0), (65, 0, 0, 0, 1, 0)], SIZE)
        with pytest.raises(ValueError, match="map 1 "):
            dec.pic_output_warped(pic, maps_array([IDENTITY, (Q, 0, 0, 0, wr.LIN_LIMIT + 1, 0)]), SIZE)
        with pytest.raises(ValueError):
            dec.pic_output_warped(pic, [], SIZE)
        assert call() == 0                                          # and the context still works
        check_batch(t[:need].view(torch.int16).view(len(MAPS), 3, *SIZE), wr.batch(planes, bd, SIZE, MAPS, dtype=abi.OUT_U16), abi.OUT_U16, what="after the refusals")
        # thetas: converted by the library, and the rotated box of the library within its one step of the restatement's is an image of its own restated map
        thetas = [(1, 0, 0, 0, 1, 0), (2.5, -0.25, 3.5, 0.25, 2.5, -1.25), wr.box_theta(160, 100, 100, 60, 30, SIZE[1], SIZE[0])]
        a = dec.pic_output_warped(pic, thetas, SIZE, samples=2)
        check_batch(a, wr.batch(planes, bd, SIZE, [abi.warp_from_matrix(lib, th) for th in thetas], 2), abi.OUT_U8, what="thetas")
        assert [abi.warp_from_matrix(lib, th) for th in thetas] == [wr.from_matrix(th) for th in thetas]
    finally:
        dec.close()


def test_golden_stream_and_a_side_stream():
    """StreamDecoder.pictures(tensor=, size=, warp=) equals pic_output_warped on the same picture; a call on a non-default torch stream, read on that stream
    without any synchronisation in between, sees the finished images"""
    import torch
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))["bytes"].tobytes()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]
    opts = dict(dtype=torch.float32, matrix=1, full_range=False, chroma_loc=0, crop=(0, 0, 0, 0), dra=None, samples=2, border="pad", pad=0.447)
    size = (24, 32)

    def maps(p):      # a box that turns with the picture, and a flip
        w, h = p["width"], p["height"]
        return maps_array([wr.from_rotated_box(w / 2, h / 2, w / 2, h / 2, 15 * (abs(p["poc"]) % 8), size), (-Q, 0, (w - 1) * Q, 0, Q, 0)])

    got = [(p, t) for p, t in StreamDecoder(data).pictures(tensor=opts, size=size, mean=MEAN, std=STD, warp=maps)]
    assert len(got) == len(ref) > 1
    for (p, t), (_, planes) in zip(got, ref):
        assert tuple(t.shape) == (2, 3, *size)
        dec, pic = ts.open_picture(planes, p["bit_depth"])
        try:
            one = dec.pic_output_warped(pic, maps(p), size, dtype=torch.float32, samples=2, border="pad", pad=0.447, mean=MEAN, std=STD)
            assert np.array_equal(ts.tensor_bits(t, abi.OUT_F32), ts.tensor_bits(one, abi.OUT_F32)), p["poc"]
        finally:
            dec.close()
        check_batch(t, wr.batch(planes, p["bit_depth"], size, maps(p), 2, wr.PAD, 0.447, dtype=abi.OUT_F32, **NORM), abi.OUT_F32, what=("stream", p["poc"]))
    # a fixed list of thetas through output_order, which delivers numpy arrays; without warp= the generator is what it was
    out = StreamDecoder(data).output_order(tensor=dict(dtype=torch.uint8, channels_last=True), size=(16, 16), warp=[(2, 0, 0, 0, 2, 0)])
    by_poc = {p["poc"]: planes for p, planes in ref}
    for p, a in out:
        exp = np.moveaxis(wr.batch(by_poc[p["poc"]], p["bit_depth"], (16, 16), [wr.from_matrix((2, 0, 0, 0, 2, 0))]), 1, -1)
        assert np.array_equal(a, exp), p["poc"]
    for wrong in (dict(warp=[IDENTITY]), dict(tensor={}, warp=[IDENTITY]), dict(tensor={}, size=size, warp=[IDENTITY], rois=[(0, 0, 16, 16)])):
        with pytest.raises(ValueError):
            next(iter(StreamDecoder(data).pictures(**wrong)))
    # a side stream and the null stream, batches of changing size, the ROI call (which shares the context's block) between them
    bd = 10
    planes = ts.random_planes(W, H, bd, seed=731, rails=True)
    dec, pic = ts.open_picture(planes, bd)
    plan = [(MAPS[:1], (40, 72)), (MAPS, SIZE), (MAPS[4:6], (100, 30)), (MAPS[:1], (40, 72))]
    try:
        sums = [[int(v) for v in wr.batch(planes, bd, s, m, 2, dtype=abi.OUT_U16).astype(np.int64).sum(axis=(1, 2, 3))] for m, s in plan]
        side = torch.cuda.Stream(device=0)
        for stream in (side, torch.cuda.default_stream(0)):
            res, rois = [], []
            with torch.cuda.stream(stream):
                for m, s in plan:
                    t = dec.pic_output_warped(pic, maps_array(m), s, dtype=torch.int16, samples=2)
                    res.append(t.to(torch.int64).sum(dim=(1, 2, 3)))
                    del t
                    rois.append(dec.pic_output_tensor(pic, dtype=torch.int16, size=SIZE, rois=[(0, 0, 64, 48), (8, 8, 128, 96)]).to(torch.int64).sum())
            stream.synchronize()
            assert [[int(v) for v in g] for g in res] == sums
            assert len({int(v) for v in rois}) == 1
    finally:
        dec.close()
