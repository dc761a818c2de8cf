"""GPU suite for xgpu_pic_output_device_ladder / XgpuDecoder.pic_output_surfaces / StreamDecoder.pictures(surfaces=...): the renditions of one picture as
scaled NV12 / P016 / YUV420P surfaces written by the device into torch tensors, against the numpy restatement of the contract (tests/ladder_ref.py) applied to
the uploaded planes with the library's own tap tables (which the CPU suite pins to the Fraction restatement).  Every comparison is bit for bit."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import colour_ref as cr
import golden_io
import ladder_ref as lr
import scale_ref as sr
from test_gpu_output_scaled import open_picture, random_planes
from xevd_amd import abi

pytestmark = pytest.mark.gpu

FILTERS = {"bilinear": lr.BILINEAR, "area": lr.AREA}
# (H, W) of the rungs of a 592 x 296 source: the exact half, a reduction by 3.7, one by about 33 (chroma 9 x 5: odd, and rows shorter than a lane's group and
# than the vertical pass' 8 columns), the same size, an enlargement by 1.5
SRC = (592, 296)
RUNGS = [(148, 296), (80, 160), (10, 18), (296, 592), (444, 888)]


def host(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def ref_name(layout, dtype):
    import torch
    return "nv12_u16" if layout == "nv12" and dtype not in (None, torch.uint8) else layout


def depth_of(layout, dtype, obd, bd):
    import torch
    return 8 if dtype is torch.uint8 or (dtype is None and layout != "p016") else (obd or bd)


def check_ladder(dec, pic, planes, bd, sizes, layout, dtype=None, obd=0, filt="bilinear", what="", **kw):
    """one call and the comparison of every rung; kw: chroma_loc, dst_chroma_loc, crop, dra"""
    out = dec.pic_output_surfaces(pic, sizes, layout=layout, dtype=dtype, out_bit_depth=obd, filter=filt, **kw)
    assert len(out) == len(sizes)
    for t, size in zip(out, sizes):
        exp = lr.rung(planes, bd, size, ref_name(layout, dtype), depth_of(layout, dtype, obd, bd), FILTERS[filt], lib=dec.lib, **kw)
        got = host(t)
        assert got.shape == exp.shape and got.dtype == exp.dtype, (what, size, got.shape, exp.shape)
        bad = int((got != exp).sum())
        assert bad == 0, f"{what} {layout} {dtype} D={obd} {filt} {size} {kw}: {bad} of {exp.size} elements differ"
    return out


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_sizes_filters_and_depths(bd):
    import torch
    planes = random_planes(*SRC, bd, seed=300 + bd, rails=True)
    dec, pic = open_picture(planes, bd)
    src = lr.source_planes(planes, bd)
    combos = [("p016", torch.int16, 10), ("p016", torch.int16, 12), ("p016", torch.int16, 16), ("nv12", torch.uint8, 8), ("nv12", torch.int16, 0 if bd > 8 else 10),
              ("yuv420p", torch.uint8, 8), ("yuv420p", torch.int16, 0 if bd > 8 else 10)]
    try:
        for filt in FILTERS:
            # the filtered planes of every rung once, packed per layout and depth
            ycc = [lr.resize_planes(src, s, lr.make_tables(SRC[0], SRC[1], s[1], s[0], FILTERS[filt], lib=dec.lib)) for s in RUNGS]
            for layout, dtype, obd in combos:
                out = dec.pic_output_surfaces(pic, RUNGS, layout=layout, dtype=dtype, out_bit_depth=obd, filter=filt)
                for t, size, p in zip(out, RUNGS, ycc):
                    exp = lr.pack(p, bd, ref_name(layout, dtype), depth_of(layout, dtype, obd, bd))
                    got = host(t)
                    assert got.shape == exp.shape and got.dtype == exp.dtype
                    bad = int((got != exp).sum())
                    assert bad == 0, f"{bd} bit {filt} {layout} {dtype} D={obd} {size}: {bad} of {exp.size} elements differ"
    finally:
        dec.close()


def test_mixed_ratios():
    """320 x 240 to 100 x 300: one axis down, one up"""
    import torch
    bd = 10
    planes = random_planes(320, 240, bd, seed=311, rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        for filt, (layout, dtype) in itertools.product(FILTERS, (("nv12", torch.int16), ("p016", None), ("yuv420p", torch.uint8))):
            check_ladder(dec, pic, planes, bd, [(300, 100)], layout, dtype, filt=filt)
    finally:
        dec.close()


def test_smallest_rung():
    """64 x 64 to 2 x 2 (chroma 1 x 1), next to a rung of the source's size"""
    import torch
    bd = 8
    planes = random_planes(64, 64, bd, seed=313, rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        for filt, (layout, dtype, obd) in itertools.product(FILTERS, (("nv12", torch.uint8, 8), ("p016", torch.int16, 0), ("yuv420p", torch.uint8, 8))):
            check_ladder(dec, pic, planes, bd, [(2, 2), (64, 64)], layout, dtype, obd, filt)
    finally:
        dec.close()


def test_every_siting_pair():
    """all 36 (chroma_loc, dst_chroma_loc) pairs, to another size and - re-siting alone - to the same size"""
    import torch
    bd = 10
    planes = random_planes(64, 48, bd, seed=317)
    dec, pic = open_picture(planes, bd)
    try:
        for loc, dloc in itertools.product(range(6), range(6)):
            check_ladder(dec, pic, planes, bd, [(36, 40), (48, 64)], "nv12", torch.int16, chroma_loc=loc, dst_chroma_loc=dloc)
        check_ladder(dec, pic, planes, bd, [(36, 40), (48, 64)], "yuv420p", torch.int16, filt="area", chroma_loc=2, dst_chroma_loc=5)
    finally:
        dec.close()


def test_crop_is_the_source():
    import torch
    bd = 10
    planes = random_planes(320, 200, bd, seed=319, rails=True)
    dec, pic = open_picture(planes, bd)
    sizes = [(64, 64), (50, 90)]
    try:
        for crop in ((2, 0, 0, 0), (40, 120, 30, 50), (158, 2, 98, 6)):
            a = check_ladder(dec, pic, planes, bd, sizes, "nv12", torch.int16, crop=crop, chroma_loc=1)
            check_ladder(dec, pic, planes, bd, sizes, "yuv420p", torch.uint8, 8, "area", crop=crop)
            if (320 - crop[0] - crop[1]) % 8 or (200 - crop[2] - crop[3]) % 8:
                continue      # (a context takes pictures of whole 8 x 8 blocks)
            # ... and it equals the call on the cropped planes: a picture of that size in a context of its own
            cut = [np.ascontiguousarray(p) for p in cr.crop_planes([np.asarray(p) for p in planes], crop)]
            dec2, pic2 = open_picture(cut, bd)
            try:
                b = dec2.pic_output_surfaces(pic2, sizes, layout="nv12", dtype=torch.int16, chroma_loc=1)
                for x, y in zip(a, b):
                    assert np.array_equal(host(x), host(y)), crop
            finally:
                dec2.close()
    finally:
        dec.close()


def test_dra_picture():
    import torch
    d = np.load(os.path.join(golden_io.GOLDEN, "dra.npz"))
    planes = [d[f"in_{c}"] for c in range(3)]
    h, w = planes[0].shape
    dec, pic = open_picture(planes, 10)
    even = lambda v: max(int(v) & ~1, 2)
    try:
        for name in ("three_ranges_idx58", "five_ranges_idx40"):
            luts = d[f"{name}_luts"]
            sizes = [(even(h / 3), even(w / 3)), (even(h / 2 + 3), even(w + 10)), (h, w)]
            check_ladder(dec, pic, planes, 10, sizes, "p016", torch.int16, dra=luts, what=name)
            check_ladder(dec, pic, planes, 10, sizes[:2], "nv12", torch.uint8, 8, "area", dra=luts, crop=(2, 4, 0, 2), what=name)
    finally:
        dec.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_same_size_and_siting_equals_the_unscaled_surface(bd):
    """consequence (a): every row is the single tap 16384, so the rung is xgpu_pic_output_device's surface of the layout, for every depth both accept"""
    import torch
    planes = random_planes(144, 88, bd, seed=331 + bd, rails=True)
    dec, pic = open_picture(planes, bd)
    h, w = planes[0].shape
    cases = [("nv12", torch.uint8, 0), ("nv12", torch.uint8, 8), ("yuv420p", torch.uint8, 0)] + [("yuv420p", torch.int16, 0)] * (bd > 8)
    cases += [("nv12", torch.int16, d) for d in (0, 9, 10, 12, 16) if d or bd > 8] + [("p016", torch.int16, d) for d in (0, 8, 10, 12, 16)]
    try:
        for (layout, dtype, obd), (loc, crop) in itertools.product(cases, ((0, (0, 0, 0, 0)), (3, (2, 6, 4, 2)))):
            size = (h - crop[2] - crop[3], w - crop[0] - crop[1])
            for filt in FILTERS:
                a = dec.pic_output_surfaces(pic, [size], layout=layout, dtype=dtype, out_bit_depth=obd, filter=filt, chroma_loc=loc, crop=crop)[0]
                b = dec.pic_output_tensor(pic, layout=layout, dtype=dtype, out_bit_depth=obd, crop=crop)
                assert a.shape == b.shape and a.dtype == b.dtype
                assert np.array_equal(host(a), host(b)), (layout, dtype, obd, loc, crop, filt)
    finally:
        dec.close()


def test_centre_siting_is_a_plain_plane_resize():
    """consequence (b): chroma_loc 1 on both sides - the chroma tables are xgpu_scale_taps(n, 1, 0, N), those of a luma plane of that size"""
    import torch
    bd = 10
    planes = random_planes(*SRC, bd, seed=337, rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        for filt, sizes in itertools.product(FILTERS, (RUNGS[:3], RUNGS[3:])):
            out = dec.pic_output_surfaces(pic, sizes, layout="nv12", dtype=torch.int16, filter=filt, chroma_loc=1)
            for t, (hd, wd) in zip(out, sizes):
                plain = lambda n, N: sr.table_rows(*abi.scale_taps(dec.lib, n, 1, 0, N, FILTERS[filt]))
                tables = [plain(SRC[1], hd), plain(SRC[1] // 2, hd // 2), plain(SRC[0], wd), plain(SRC[0] // 2, wd // 2)]
                exp = lr.rung(planes, bd, (hd, wd), "nv12_u16", bd, tables=tables)
                assert np.array_equal(host(t), exp), (filt, hd, wd)
    finally:
        dec.close()


def test_luma_is_the_scaled_output_and_rungs_are_independent():
    """consequences (c) and (d): the luma rows of a rung are channel 0 of the existing scaled yuv444 output at that size; rung i of a call is the one-rung call"""
    import torch
    bd = 10
    planes = random_planes(*SRC, bd, seed=341, rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        for filt in FILTERS:
            for layout, dtype in (("nv12", torch.int16), ("yuv420p", torch.int16), ("p016", torch.int16)):
                many = dec.pic_output_surfaces(pic, RUNGS, layout=layout, dtype=dtype, filter=filt, chroma_loc=2, dst_chroma_loc=0)
                for t, size in zip(many, RUNGS):
                    one = dec.pic_output_surfaces(pic, [size], layout=layout, dtype=dtype, filter=filt, chroma_loc=2, dst_chroma_loc=0)[0]
                    assert torch.equal(t, one), (filt, layout, size)
                    if layout == "p016":
                        continue
                    y444 = dec.pic_output_tensor(pic, layout="yuv444", size=size, dtype=torch.int16, filter=filt)[0]
                    luma = t[:size[0]] if layout == "nv12" else t[:size[0] * size[1]].view(size)
                    assert torch.equal(luma, y444), (filt, layout, size)
    finally:
        dec.close()


def test_unaligned_destinations_and_padded_rows():
    """the vector / element split of the horizontal pass: rows whose starts the pitch or the pointer leaves unaligned, row tails, guard elements untouched"""
    import torch
    bd = 10
    planes = random_planes(*SRC, bd, seed=347, rails=True)
    dec, pic = open_picture(planes, bd)
    try:
        hd, wd = 10, 18
        rows = hd * 3 // 2
        exp8 = lr.rung(planes, bd, (hd, wd), "nv12", 8, lib=dec.lib)
        # NV12 u8, 18-byte rows: tight (a pitch that is no multiple of 4), from a 16-byte-aligned start and from one element into the buffer
        for start in (16, 1, 2, 3):
            buf = torch.full((start + rows * wd + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
            view = buf[start:start + rows * wd].view(rows, wd)
            out = dec.pic_output_surfaces(pic, [(hd, wd)], layout="nv12", dtype=torch.uint8, out=[view])
            assert out[0] is view
            got = host(buf)
            assert np.array_equal(got[start:start + rows * wd].reshape(rows, wd), exp8), start
            assert (got[:start] == 0xA5).all() and (got[start + rows * wd:] == 0xA5).all(), start
        # ... and a view one element into a larger buffer with a pitch of 23 elements
        buf = torch.full((1 + rows * 23 + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        view = torch.as_strided(buf, (rows, wd), (23, 1), 1)
        dec.pic_output_surfaces(pic, [(hd, wd)], layout="nv12", dtype=torch.uint8, out=[view])
        got = host(buf)
        grid = got[1:1 + rows * 23].reshape(rows, 23)
        assert np.array_equal(grid[:, :wd], exp8)
        assert (grid[:-1, wd:] == 0xA5).all() and got[0] == 0xA5 and (got[1 + (rows - 1) * 23 + wd:] == 0xA5).all()
        # P016 at a pitch of W + 3 elements, two rungs in one call, every start of a row pair at another alignment
        sizes = [(10, 18), (148, 296)]
        for layout, off in itertools.product(("p016", "nv12"), (0, 1, 3)):
            bufs, views = [], []
            for h, w in sizes:
                r = h * 3 // 2
                b = torch.full((off + r * (w + 3) + 8,), 0x5A5A, dtype=torch.int16, device="cuda:0")
                bufs.append(b)
                views.append(torch.as_strided(b, (r, w), (w + 3, 1), off))
            dec.pic_output_surfaces(pic, sizes, layout=layout, dtype=torch.int16, out=views)
            for b, (h, w) in zip(bufs, sizes):
                r = h * 3 // 2
                exp = lr.rung(planes, bd, (h, w), "nv12_u16" if layout == "nv12" else layout, bd, lib=dec.lib)
                got = host(b)
                grid = got[off:off + r * (w + 3)].reshape(r, w + 3)
                assert np.array_equal(grid[:, :w], exp), (layout, off, h, w)
                assert (grid[:-1, w:] == 0x5A5A).all() and (got[:off] == 0x5A5A).all() and (got[off + (r - 1) * (w + 3) + w:] == 0x5A5A).all(), (layout, off, h, w)
        # YUV420P u8: tight planes of 18- and 9-byte rows at an odd start
        n = hd * wd * 3 // 2
        buf = torch.full((3 + n + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        dec.pic_output_surfaces(pic, [(hd, wd)], layout="yuv420p", dtype=torch.uint8, out=[buf[3:3 + n]])
        got = host(buf)
        assert np.array_equal(got[3:3 + n], lr.rung(planes, bd, (hd, wd), "yuv420p", 8, lib=dec.lib))
        assert (got[:3] == 0xA5).all() and (got[3 + n:] == 0xA5).all()
    finally:
        dec.close()


def test_streams_and_table_reuse():
    """two calls with the same key, a changed rung list, a side stream and the null stream, no synchronisation between a call and the reduction that reads its
    tensors: identical to what a fresh context gives"""
    import torch
    bd = 10
    pa = random_planes(320, 176, bd, seed=351)
    pb = random_planes(320, 176, bd, seed=353, rails=True)
    lists = ([(88, 160), (40, 72)], [(150, 300), (40, 72), (12, 20)], [(88, 160), (40, 72)], [(40, 72)])
    order = [("a", 0), ("b", 0), ("a", 1), ("b", 2), ("a", 3), ("b", 1), ("a", 0)]

    def sums(ts):
        return [(t.to(torch.int64) & 0xFFFF).sum() for t in ts]      # the 16-bit words as unsigned

    fresh = {}
    for k, planes in (("a", pa), ("b", pb)):
        for i in sorted({i for kk, i in order if kk == k}):
            dec, pic = open_picture(planes, bd)      # a fresh context per call
            try:
                fresh[k, i] = [int(v) for v in sums(dec.pic_output_surfaces(pic, lists[i], layout="p016"))]
                ref = [int(lr.rung(planes, bd, s, "p016", bd, lib=dec.lib).astype(np.int64).sum()) for s in lists[i]]
                assert fresh[k, i] == ref
            finally:
                dec.close()
    dec, pic_a = open_picture(pa, bd)
    try:
        pic_b = dec.pic_alloc()
        dec.pic_upload(pic_b, pb)
        side, other = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
        for streams in ((side,), (torch.cuda.default_stream(0),), (side, other)):
            got = []
            for n, (k, i) in enumerate(order):
                with torch.cuda.stream(streams[n % len(streams)]):
                    got.append(sums(dec.pic_output_surfaces(pic_a if k == "a" else pic_b, lists[i], layout="p016")))
            torch.cuda.synchronize()
            assert [[int(v) for v in g] for g in got] == [fresh[o] for o in order]
        # the same rungs into the same tensors again, from either picture: the call finds its records on the device and uploads nothing
        outs = dec.pic_output_surfaces(pic_a, lists[0], layout="p016")
        for k in ("b", "a", "a", "b"):
            again = dec.pic_output_surfaces(pic_a if k == "a" else pic_b, lists[0], layout="p016", out=outs)
            assert all(x is y for x, y in zip(again, outs))
            assert [int(v) for v in sums(again)] == fresh[k, 0], k
        # the C ABI's stream = NULL: the context's own stream
        fmt, lp = abi.make_output_format(abi.OUT_P016, abi.OUT_U16), abi.make_ladder_params()
        t = torch.zeros((60, 72), dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        rungs = abi.make_rungs([(72, 40, 0, t.data_ptr(), t.numel() * 2)])
        assert dec.lib.xgpu_pic_output_device_ladder(dec.ctx, pic_a, None, C.byref(fmt), C.byref(lp), rungs, 1, None) == 0
        dec.sync()
        assert np.array_equal(host(t), lr.rung(pa, bd, (40, 72), "p016", bd, lib=dec.lib))
    finally:
        dec.close()


def test_refusals_queue_nothing():
    import torch
    bd = 8
    planes = random_planes(256, 128, bd, seed=359)
    dec, pic = open_picture(planes, bd)
    lib = dec.lib
    try:
        fmt, lp = abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8), abi.make_ladder_params()
        sizes = [(60, 100), (30, 50)]
        need = [lib.xgpu_output_ladder_rung_size(C.byref(fmt), w, h, 0, bd) for h, w in sizes]
        assert need == [90 * 100, 45 * 50]
        t = torch.full((sum(need) + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        host_mem = np.zeros(need[0], np.uint8)
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p0, p1 = t.data_ptr(), t.data_ptr() + need[0] + 16

        def call(spec, f=fmt, n=None):
            return lib.xgpu_pic_output_device_ladder(dec.ctx, pic, None, C.byref(f), C.byref(lp), abi.make_rungs(spec), len(spec) if n is None else n, stream_h)

        good = [(100, 60, 0, p0, need[0]), (50, 30, 0, p1, need[1])]
        assert call([good[0], (50, 30, 0, p0 + need[0] - 1, need[1])]) == -101      # overlapping rungs
        assert call([good[0], (50, 30, 0, p0, need[1])]) == -101                    # one inside the other
        assert b"pic_output_device_ladder" in lib.xgpu_last_error(dec.ctx)
        assert call([good[0], (50, 30, 0, p1, need[1] - 1)]) == -101                # an undersized dst_size
        assert call([(100, 60, 0, host_mem.ctypes.data, need[0]), good[1]]) == -101  # host memory
        assert call([good[0], (50, 30, 0, None, need[1])]) == -101                  # a NULL destination
        assert call([good[0]] * 9) == -101 and call(good, n=0) == -101              # 9 rungs, none
        assert call([good[0], (51, 30, 0, p1, need[1])]) == -101                    # an odd size
        assert call([good[0], (2, 30, 0, p1, need[1])]) == -104                     # below 1 / 64 of 256
        assert call([good[0], (50, 1026, 0, p1, need[1])]) == -104                  # above 8 x 128
        assert call(good, abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_U8)) == -101
        assert call(good, abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8, crop=(1, 0, 0, 0))) == -101
        u16 = abi.make_output_format(abi.OUT_P016, abi.OUT_U16)
        assert call([(100, 60, 0, p0 + 1, 2 * need[0])], u16) == -101               # not aligned to the 2-byte element
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all()
        for bad in (dict(sizes=[(60, 101)]), dict(sizes=sizes, layout="rgb"), dict(sizes=sizes, filter="lanczos"), dict(sizes=[(60, 2)])):
            with pytest.raises(ValueError):
                dec.pic_output_surfaces(pic, **bad)
        from xevd_amd.decoder import XgpuError
        with pytest.raises(XgpuError):                                              # overlapping tensors
            dec.pic_output_surfaces(pic, sizes, out=[t[:need[0]].view(90, 100), t[need[0] - 1:need[0] - 1 + need[1]].view(45, 50)])
        with pytest.raises(ValueError):
            dec.pic_output_tensor(pic, layout="nv12", size=(60, 100))               # the single-tensor call keeps refusing the surfaces
        torch.cuda.synchronize()
        assert (t.cpu().numpy() == 0x5A).all()
        assert call(good) == 0                                                      # and the context still works
        got = host(t)
        for (h, w), p, nb in zip(sizes, (0, need[0] + 16), need):
            assert np.array_equal(got[p:p + nb].reshape(h * 3 // 2, w), lr.rung(planes, bd, (h, w), "nv12", 8, lib=lib))
        assert (got[need[0]:need[0] + 16] == 0x5A).all() and (got[need[0] + 16 + need[1]:] == 0x5A).all()
    finally:
        dec.close()


def test_golden_stream_as_a_ladder():
    """a committed stream through StreamDecoder.pictures(surfaces=[...], surface_layout="nv12"), in decoding and in output order: every rung of every picture is
    the restatement of its decoded planes"""
    import torch
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))["bytes"].tobytes()
    lib = abi.load()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]      # in decoding order
    sizes = [(48, 64), (30, 44)]
    opts = dict(chroma_loc=0, crop=(0, 0, 0, 0), dra=None)
    got = [(p, [host(t) for t in p["surfaces"]], planes) for p, planes in StreamDecoder(data).pictures(surfaces=sizes, surface_layout="nv12", surface_options=opts)]
    assert len(got) == len(ref) > 1
    for (p, surf, planes), (pr, ref_planes) in zip(got, ref):
        assert p["poc"] == pr["poc"] and np.array_equal(planes[0], ref_planes[0])      # the planes are still yielded next to the surfaces
        for a, s in zip(surf, sizes):
            e = lr.rung(ref_planes, pr["bit_depth"], s, "nv12", 8, lib=lib)
            assert a.shape == e.shape and np.array_equal(a, e), ("decoding order", p["poc"], s)
    out = StreamDecoder(data).output_order(surfaces=sizes, surface_layout="p016", surface_options=dict(opts, filter="area", dtype=torch.int16))
    assert len(out) == len(ref)
    for p, _ in out:
        pr, ref_planes = ref[p["decode_index"]]
        assert p["poc"] == pr["poc"]
        for a, s in zip(p["surfaces"], sizes):
            e = lr.rung(ref_planes, pr["bit_depth"], s, "p016", pr["bit_depth"], lr.AREA, lib=lib)
            assert np.array_equal(a.view(np.uint16), e), ("output order", p["poc"], s)
    with pytest.raises(ValueError):
        next(iter(StreamDecoder(data).pictures(surface_options=dict(filter="area"))))
