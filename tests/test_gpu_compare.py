"""GPU suite of the picture comparison (xgpu_pic_compare / XgpuDecoder.pic_compare / StreamDecoder(compare=) / tools/xevd_gpu_app.py --ref): pictures are
uploaded with pic_upload and every expectation is tests/metrics_ref.py on the uploaded arrays - never GPU output -, bit for bit.

Sizes are the smallest at which the kernel can go wrong: 8x8 (one luma window, chroma planes of 4x4 without one), 72x40 (a 64x32 tile and an 8-sample remainder
both ways), 136x72 (more than one tile both ways, the halo crossing tile borders), 200x136 minus (2, 6, 4, 2) = 192x130 (h % 4 == 2: trailing rows in no window,
map blocks clipped at the bottom, a left crop that takes the 16-byte loads away from the slot's luma plane) and minus (2, 4, 4, 2) = 194x130 (w % 4 == 2 as well:
trailing columns in no window, map blocks clipped at both edges).  One case of 4096x1088 has more tiles than the launch has workgroups: there a workgroup walks
several tiles and changes planes on the way."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import metrics_ref as mr
from xevd_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -101
NO_CROP = (0, 0, 0, 0)
SIZES = [(8, 8, NO_CROP), (72, 40, NO_CROP), (136, 72, NO_CROP), (200, 136, (2, 6, 4, 2)), (200, 136, (2, 4, 4, 2))]
INT_KEYS = ("n", "sse", "n_diff", "first_diff", "max_abs", "ssim_windows", "ssim_q30")


def rand_pic(seed, w, h, bd):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, (h >> s, w >> s)).astype(np.uint16) for s in (0, 1, 1)]


def const_pic(w, h, v):
    return [np.full((h >> s, w >> s), v, np.uint16) for s in (0, 1, 1)]


def open_pics(bd, *pics):
    """a decoder and one slot per picture ([Y, U, V] of unsigned 16-bit patterns)"""
    from xevd_amd.decoder import XgpuDecoder
    h, w = pics[0][0].shape
    dec = XgpuDecoder(w, h, bd, device=0, max_pics=4)
    slots = []
    for p in pics:
        slots.append(dec.pic_alloc())
        dec.pic_upload(slots[-1], [np.ascontiguousarray(pl).view(np.int16) for pl in p])
    return dec, slots


def same(got, want, what=""):
    """pic_compare's dict against metrics_ref.compare's"""
    for k in INT_KEYS:
        g = got[k]
        if k == "first_diff":
            g = [mr.NO_DIFF if f is None else (f[0] << 32) | f[1] for f in g]
        assert g == want[k], (what, k, g, want[k])
    if want["map"] is None:
        assert got["map"] is None, what
    else:
        m = got["map"].cpu().numpy()
        assert m.shape == want["map"].shape and np.array_equal(m.view(np.uint64), want["map"]), (what, "map")
        assert [int(m[c].sum()) for c in range(3)] == want["sse"], (what, "map sums")


def yuv_tensor(pic, dtype=np.uint16, pitch=None, offset=0):
    """the planes in pic_output's order as a tensor on the device: flat and tight, or [H * 3 // 2, pitch] rows (elements; the chroma planes at pitch / 2);
    offset: the tensor starts that many elements into its allocation"""
    import torch
    h, w = pic[0].shape
    if pitch is None:
        flat = np.concatenate([p.reshape(-1) for p in pic]).astype(dtype)
    else:
        flat = np.full(h * 3 // 2 * pitch, 0x5A, dtype)
        for y in range(h):
            flat[y * pitch:y * pitch + w] = pic[0][y]
        for c in (1, 2):
            base = h * pitch + (c - 1) * (h // 2) * (pitch // 2)
            for y in range(h // 2):
                flat[base + y * (pitch // 2):base + y * (pitch // 2) + w // 2] = pic[c][y]
    host = np.zeros(flat.size + offset, dtype)
    host[offset:] = flat
    if dtype == np.uint16:
        host = host.view(np.int16)
    t = torch.from_numpy(host).cuda()[offset:]
    return t if pitch is None else t.view(h * 3 // 2, pitch)


# ------------------------------------------------------------------------------------------------ the census, the SSIM and the map
@pytest.mark.parametrize("w,h,crop", SIZES)
def test_same_slot_against_itself(w, h, crop):
    bd = 10
    a = rand_pic(1, w, h, bd)
    dec, (pa,) = open_pics(bd, a)
    with dec:
        got = dec.pic_compare(pa, pa, crop=crop, block_map=True)
        same(got, mr.compare(a, a, bd, crop=crop, block_map=True))
        assert got["n_diff"] == [0, 0, 0] and got["first_diff"] == [None] * 3 and got["psnr"] == [float("inf")] * 3
        assert got["ssim_q30"] == [n << 30 for n in got["ssim_windows"]]
        cw, ch = w - crop[0] - crop[1], h - crop[2] - crop[3]
        assert got["ssim_windows"][0] == max((cw >> 2) - 1, 0) * max((ch >> 2) - 1, 0)
        assert not got["map"].any().item()


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("w,h,crop", SIZES)
def test_random_planes(w, h, crop, bd):
    a, r = rand_pic(2, w, h, bd), rand_pic(3, w, h, bd)
    dec, (pa, pr) = open_pics(bd, a, r)
    with dec:
        same(dec.pic_compare(pa, pr, crop=crop, block_map=True), mr.compare(a, r, bd, crop=crop, block_map=True))
        same(dec.pic_compare(pa, pr, crop=crop, ssim=False), mr.compare(a, r, bd, crop=crop, ssim=False), "ssim off")
        same(dec.pic_compare(pa, pr, crop=crop, ssim=False, block_map=True), mr.compare(a, r, bd, crop=crop, ssim=False, block_map=True), "ssim off, map")
        got = dec.pic_compare(pa, pr, crop=crop)
        want = mr.compare(a, r, bd, crop=crop)
        assert got["psnr"] == abi.psnr(want, bd) and all(p < 20 for p in got["psnr"])
        if want["ssim_windows"][0]:
            assert got["ssim"][0] == want["ssim_q30"][0] / (want["ssim_windows"][0] * 2.0 ** 30)


def single_sample_positions(cw, ch):
    """(component, y, x) in the cropped planes: every corner, each side of the tile borders (64 columns, 32 rows) that the plane has"""
    out = []
    for c, (pw, ph) in enumerate(((cw, ch), (cw >> 1, ch >> 1), (cw >> 1, ch >> 1))):
        pos = {(0, 0), (0, pw - 1), (ph - 1, 0), (ph - 1, pw - 1)}
        if pw > 64:
            pos |= {(min(5, ph - 1), 63), (min(5, ph - 1), 64)}
        if ph > 32:
            pos |= {(31, min(7, pw - 1)), (32, min(7, pw - 1))}
        if pw > 64 and ph > 32:
            pos |= {(31, 63), (32, 64)}
        out += [(c, y, x) for y, x in sorted(pos)]
    return out


@pytest.mark.parametrize("w,h,crop", SIZES[1:])
def test_one_differing_sample(w, h, crop):
    """one sample differs by 3: at each corner and on each side of every tile border.  One picture holds the reference; the other is uploaded again per case."""
    bd = 10
    r = rand_pic(4, w, h, bd)
    dec, (pa, pr) = open_pics(bd, r, r)
    cw, ch = w - crop[0] - crop[1], h - crop[2] - crop[3]
    with dec:
        for c, y, x in single_sample_positions(cw, ch):
            a = [p.copy() for p in r]
            a[c][y + (crop[2] >> (c > 0)), x + (crop[0] >> (c > 0))] ^= 3
            dec.pic_upload(pa, [p.view(np.int16) for p in a])
            got = dec.pic_compare(pa, pr, crop=crop, block_map=True)
            want = mr.compare(a, r, bd, crop=crop, block_map=True)
            same(got, want, (c, y, x))
            assert got["n_diff"][c] == 1 and got["first_diff"][c] == (y, x) and sum(got["n_diff"]) == 1
            assert int(got["map"][c, y >> (4 - (c > 0)), x >> (4 - (c > 0))]) == got["sse"][c] > 0


def test_sample_outside_every_window():
    """a difference in the last uncovered column (194 % 4 == 2) or row (130 % 4 == 2) moves sse and first_diff but not ssim_q30"""
    bd, w, h = 10, 200, 136
    r = rand_pic(5, w, h, bd)
    dec, (pa, pr) = open_pics(bd, r, r)
    with dec:
        for crop, (y, x) in (((2, 4, 4, 2), (60, 193)), ((2, 4, 4, 2), (60, 192)), ((2, 6, 4, 2), (129, 100)), ((2, 4, 4, 2), (129, 193))):
            a = [p.copy() for p in r]
            a[0][y + crop[2], x + crop[0]] ^= 0x155
            dec.pic_upload(pa, [p.view(np.int16) for p in a])
            got = dec.pic_compare(pa, pr, crop=crop, block_map=True)
            same(got, mr.compare(a, r, bd, crop=crop, block_map=True), (crop, y, x))
            assert got["sse"][0] > 0 and got["first_diff"][0] == (y, x)
            assert got["ssim_q30"][0] == got["ssim_windows"][0] << 30


def test_two_differing_samples_first_is_raster_first():
    """the raster-first difference lies in a tile that comes later in the kernel's tile order than the other one's"""
    bd, w, h = 8, 136, 72
    r = rand_pic(6, w, h, bd)
    a = [p.copy() for p in r]
    a[0][33, 100] ^= 1      # tile (1, 1)
    a[0][34, 3] ^= 7        # tile (1, 0)
    a[2][35, 1] ^= 1        # chroma: tile (1, 0) ...
    a[2][3, 66] ^= 2        # ... and tile (0, 1), raster-first
    dec, (pa, pr) = open_pics(bd, a, r)
    with dec:
        got = dec.pic_compare(pa, pr)
        same(got, mr.compare(a, r, bd))
        assert got["first_diff"] == [(33, 100), None, (3, 66)] and got["n_diff"] == [2, 0, 2]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_extremes_of_the_range(bd):
    w, h = 136, 72
    zero, top = const_pic(w, h, 0), const_pic(w, h, (1 << bd) - 1)
    dec, (p0, p1) = open_pics(bd, zero, top)
    with dec:
        for x, y, px, py in ((zero, top, p0, p1), (top, zero, p1, p0)):
            got = dec.pic_compare(px, py, block_map=True)
            same(got, mr.compare(x, y, bd, block_map=True))
            assert got["max_abs"] == [(1 << bd) - 1] * 3 and got["psnr"] == [0.0] * 3


def test_any_16_bit_pattern():
    """a 16-bit reference full of 0xFFFF against random 12-bit samples, and 0xFFFF in the slot too: ss and s12 of a window pass 2^32"""
    bd, w, h = 12, 72, 40
    a, full = rand_pic(7, w, h, bd), const_pic(w, h, 0xFFFF)
    dec, (pa, pf) = open_pics(bd, a, full)
    with dec:
        want = mr.compare(a, full, bd, block_map=True)
        assert want["sse"][0] > 1 << 32
        same(dec.pic_compare(pa, yuv_tensor(full), block_map=True), want, "tensor of 0xFFFF")
        same(dec.pic_compare(pa, pf, block_map=True), want, "slot of 0xFFFF")
        same(dec.pic_compare(pf, pf), mr.compare(full, full, bd), "0xFFFF against itself")
        same(dec.pic_compare(pf, yuv_tensor(a)), mr.compare(full, a, bd), "0xFFFF in the slot")


@pytest.mark.parametrize("w,h,crop", SIZES)
def test_reference_in_device_memory(w, h, crop):
    """the reference as a slot and the same planes as a tensor - tight, at a pitch, one element into its allocation (the element loads), bytes at 8 bit -
    give the same result"""
    for bd in (8, 10):
        a, r = rand_pic(8, w, h, bd), rand_pic(9, w, h, bd)
        dec, (pa, pr) = open_pics(bd, a, r)
        with dec:
            want = mr.compare(a, r, bd, crop=crop, block_map=True)
            refs = {"slot": pr, "tight": yuv_tensor(r), "pitch": yuv_tensor(r, pitch=w + 56), "pitch, not 16 bytes": yuv_tensor(r, pitch=w + 2),
                    "offset": yuv_tensor(r, offset=1), "pitch and offset": yuv_tensor(r, pitch=w + 56, offset=1)}
            if bd == 8:
                refs.update({"u8": yuv_tensor(r, np.uint8), "u8 pitch": yuv_tensor(r, np.uint8, pitch=w + 24), "u8 offset": yuv_tensor(r, np.uint8, offset=1),
                             "u8 pitch, not 8 bytes": yuv_tensor(r, np.uint8, pitch=w + 2)})
            for name, ref in refs.items():
                same(dec.pic_compare(pa, ref, crop=crop, block_map=True), want, (bd, name))
            # the flat tensor the decoder itself makes of the reference slot
            import torch
            own = dec.pic_output_tensor(pr, layout="yuv420p", dtype=torch.uint8 if bd == 8 else torch.int16)
            same(dec.pic_compare(pa, own, crop=crop, block_map=True), want, (bd, "pic_output_tensor"))


def test_more_tiles_than_workgroups():
    """4096x1088: 2176 luma tiles and 1088 chroma tiles, walked by 2048 workgroups"""
    bd, w, h = 10, 4096, 1088
    a = rand_pic(10, w, h, bd)
    r = [p.copy() for p in a]
    rng = np.random.default_rng(11)
    for c in range(3):
        ys, xs = rng.integers(0, r[c].shape[0], 5000), rng.integers(0, r[c].shape[1], 5000)
        r[c][ys, xs] ^= rng.integers(1, 1 << bd, 5000).astype(np.uint16)
    r[0][1087, 4095] ^= 1
    dec, (pa, pr) = open_pics(bd, a, r)
    with dec:
        same(dec.pic_compare(pa, pr, block_map=True), mr.compare(a, r, bd, block_map=True))
        same(dec.pic_compare(pa, yuv_tensor(r), crop=(2, 0, 0, 2)), mr.compare(a, r, bd, crop=(2, 0, 0, 2)), "cropped, element loads of the slot")


# ------------------------------------------------------------------------------------------------ the call
def raw_call(dec, pic, ref, par, res, bmap=None, stream=None):
    import torch      # noqa: F401
    return dec.lib.xgpu_pic_compare(dec.ctx, pic, C.byref(ref), C.byref(par), C.c_void_p(res if isinstance(res, int) else res.data_ptr()),
                                    C.c_void_p(bmap.data_ptr()) if bmap is not None else None, bmap.numel() * 8 if bmap is not None else 0, stream)


def test_prefilled_buffers_back_to_back_streams_and_sync_false():
    import torch
    bd, w, h, crop = 10, 200, 136, (2, 4, 4, 2)
    a, r, r2 = rand_pic(12, w, h, bd), rand_pic(13, w, h, bd), rand_pic(14, w, h, bd)
    dec, (pa, pr, pr2) = open_pics(bd, a, r, r2)
    with dec:
        want, want2 = mr.compare(a, r, bd, crop=crop, block_map=True), mr.compare(a, r2, bd, crop=crop, block_map=True)
        par = abi.make_compare_params(crop, True, True)
        # result and map pre-filled with 0xFF, two calls back to back into two results, on the context's stream
        res = torch.full((2, 20), -1, dtype=torch.int64, device="cuda")
        maps = torch.full((2,) + want["map"].shape, -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert raw_call(dec, pa, abi.make_compare_ref(pic=pr), par, res[0], maps[0]) == 0
        assert raw_call(dec, pa, abi.make_compare_ref(pic=pr2), par, res[1], maps[1]) == 0
        dec.sync()
        for k, wd in enumerate((want, want2)):
            d = abi.compare_result_dict(res[k].cpu().numpy())
            assert {key: d[key] for key in INT_KEYS} == {key: wd[key] for key in INT_KEYS}, k
            assert np.array_equal(maps[k].cpu().numpy().view(np.uint64), wd["map"]), k
            assert int(res[k].cpu().numpy().view(np.uint32)[27]) == 0      # `reserved` is written too
        # a caller's stream against the context's
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got = dec.pic_compare(pa, pr, crop=crop, block_map=True)
        same(got, want, "caller's stream")
        res_s = torch.full((20,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert raw_call(dec, pa, abi.make_compare_ref(pic=pr), par, res_s, maps[1], stream=C.c_void_p(s.cuda_stream)) == 0
        s.synchronize()
        assert torch.equal(res_s, res[0]) and torch.equal(maps[1], maps[0])
        # sync=False: the raw words, nothing read back; out= takes them
        out = torch.full((20,), -1, dtype=torch.int64, device="cuda")
        t, m = dec.pic_compare(pa, pr2, crop=crop, block_map=True, out=out, sync=False)
        assert t is out and m.dtype == torch.int64
        t2 = dec.pic_compare(pa, pr2, crop=crop, sync=False)
        torch.cuda.synchronize()
        assert torch.equal(t, res[1]) and torch.equal(t2, res[1]) and np.array_equal(m.cpu().numpy().view(np.uint64), want2["map"])
        d = abi.compare_result_dict(t.cpu().numpy())
        assert abi.psnr(d, bd) == abi.psnr(want2, bd) and abi.ssim(d) == abi.ssim(want2)


def test_refusals_queue_nothing():
    """every refusal returns XGPU_ERR_INVALID_ARGUMENT, leaves a message and does not touch a pre-filled result.  Pointer refusals are made with host
    pointers, misaligned addresses and sizes that are too small - never with an address outside an allocation"""
    import torch
    bd, w, h = 10, 72, 40
    a = rand_pic(15, w, h, bd)
    dec, (pa, pb) = open_pics(bd, a, a)
    with dec:
        lib, ctx = dec.lib, dec.ctx
        res = torch.full((20,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        bmap = torch.full((3, 3, 5), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        yuv = yuv_tensor(a)
        nbytes = w * h * 3
        slot, par = abi.make_compare_ref(pic=pb), abi.make_compare_params()
        pmap = abi.make_compare_params(block_map=True)

        def tensor_ref(**kw):
            return abi.make_compare_ref(**dict(dict(d_yuv=yuv.data_ptr(), size=nbytes), **kw))

        def refused(rc, word=None):
            assert rc == INVALID
            msg = lib.xgpu_last_error(ctx)
            assert msg and (word is None or word in msg), msg
            torch.cuda.synchronize()
            assert bool((res == 0x5A5A5A5A5A5A5A5A).all().item()) and bool((bmap == 0x5A5A5A5A5A5A5A5A).all().item())

        assert raw_call(dec, pa, slot, par, res) == 0      # the call these are variations of
        assert raw_call(dec, pa, tensor_ref(), pmap, res, bmap) == 0
        dec.sync()
        res.fill_(0x5A5A5A5A5A5A5A5A); bmap.fill_(0x5A5A5A5A5A5A5A5A)      # noqa: E702
        torch.cuda.synchronize()
        freed = dec.pic_alloc()
        dec.pic_free(freed)
        for bad in (-1, 99, freed):                                                                   # a bad slot, a slot with no picture
            refused(raw_call(dec, bad, slot, par, res), b"no picture")
            refused(raw_call(dec, pa, abi.make_compare_ref(pic=bad), par, res))
        for crop in ((1, 1, 0, 0), (0, 0, 3, 0), (-2, 0, 0, 0), (36, 36, 0, 0), (0, 0, 40, 0)):        # odd, negative, nothing left
            refused(raw_call(dec, pa, slot, abi.make_compare_params(crop), res), b"crop")
        refused(raw_call(dec, pa, tensor_ref(dtype=abi.OUT_U8), par, res), b"XGPU_OUT_U8")            # bytes at 10 bit
        refused(raw_call(dec, pa, tensor_ref(dtype=abi.OUT_F16), par, res), b"dtype")
        refused(raw_call(dec, pa, tensor_ref(row_pitch=2 * w - 4), par, res), b"row_pitch")            # shorter than a row
        refused(raw_call(dec, pa, tensor_ref(row_pitch=2 * w + 2, size=1 << 20), par, res), b"row_pitch")      # not a multiple of 2 elements
        refused(raw_call(dec, pa, tensor_ref(size=nbytes - 1), par, res), b"size")                     # says it is too small
        room = torch.zeros(nbytes // 2 + 4, dtype=torch.int16, device="cuda")
        refused(raw_call(dec, pa, tensor_ref(d_yuv=room.data_ptr() + 1), par, res), b"aligned")       # not aligned to the element
        host = np.zeros(nbytes, np.uint8)
        refused(raw_call(dec, pa, tensor_ref(d_yuv=host.ctypes.data), par, res), b"device memory")    # a host pointer
        refused(raw_call(dec, pa, tensor_ref(d_yuv=None), par, res))
        refused(raw_call(dec, pa, slot, abi.make_compare_params(ssim=2), res))
        hres = np.zeros(20, np.int64)
        refused(raw_call(dec, pa, slot, par, int(hres.ctypes.data)), b"device memory")                # the result in host memory
        assert not hres.any()
        refused(raw_call(dec, pa, slot, par, res.data_ptr() + 4), b"aligned")                         # the result not 8-byte aligned
        refused(raw_call(dec, pa, slot, pmap, res), b"d_map")                                         # a map asked for, none given
        refused(raw_call(dec, pa, slot, pmap, res, bmap[:, :, :4].contiguous()), b"map")              # a map too small
        refused(lib.xgpu_pic_compare(ctx, pa, C.byref(slot), C.byref(pmap), C.c_void_p(res.data_ptr()), C.c_void_p(bmap.data_ptr() + 4), 360, None), b"map")
        refused(lib.xgpu_pic_compare(ctx, pa, None, C.byref(par), C.c_void_p(res.data_ptr()), None, 0, None))
        refused(lib.xgpu_pic_compare(ctx, pa, C.byref(slot), None, C.c_void_p(res.data_ptr()), None, 0, None))
        assert lib.xgpu_pic_compare(ctx, pa, C.byref(slot), C.byref(par), None, None, 0, None) == INVALID
        # the Python layer refuses what it can tell without the library, and hands the rest on
        from xevd_amd.decoder import XgpuError
        with pytest.raises(ValueError):
            dec.pic_compare(pa, yuv.to(torch.float32))
        with pytest.raises(ValueError):
            dec.pic_compare(pa, yuv.view(2, -1))
        with pytest.raises(XgpuError, match="crop"):
            dec.pic_compare(pa, pb, crop=(1, 0, 0, 0))
        with pytest.raises(XgpuError):
            dec.pic_compare(pa, yuv[:-1])
        # an open frame, as xgpu_frame_side_info has it
        dec.frame_begin(pa, 0, {})
        refused(raw_call(dec, pb, slot, par, res), b"a frame is open")
        dec.frame_end()
        assert raw_call(dec, pb, slot, par, res) == 0
        dec.sync()
        assert abi.compare_result_dict(res.cpu().numpy())["n"] == [w * h, w * h // 4, w * h // 4]


# ------------------------------------------------------------------------------------------------ a decoded stream
@pytest.fixture(scope="module")
def short_stream():
    """136x72, 5 pictures, a sub-GOP of 4 with B pictures; the CPU oracle's pictures in decoding order"""
    import stream_util
    data = stream_util.make_stream(136, 72, 5, bit_depth=8, seed=21, max_refs=2, log2_sub_gop=2)
    params = []
    frames = stream_util.decode_oracle(data, order="decoding", keep_params=params)
    assert 4 <= len(frames) <= 6 and any(p["refs"][1] for p in params), "the stream has no B picture"
    return data, params, [[np.ascontiguousarray(pl).view(np.uint16) for pl in f] for f in frames]


def test_stream_compare(short_stream):
    from xevd_amd.player import StreamDecoder
    data, params, frames = short_stream
    refs = [yuv_tensor(f, np.uint8) for f in frames]
    got = [p["compare"] for p, _ in StreamDecoder(data).pictures(download=False, compare=refs)]
    assert len(got) == len(frames)
    for k, d in enumerate(got):
        assert d["n_diff"] == [0, 0, 0] and d["ssim_q30"] == [n << 30 for n in d["ssim_windows"]] and d["n"] == [136 * 72, 68 * 36, 68 * 36], k
    # one expected frame perturbed: metrics_ref's numbers for that picture, through the callable and through output_order
    bad = [[pl.copy() for pl in f] for f in frames]
    bad[2][0][40:48, 60:70] ^= 5
    bad[2][1][3, 3] ^= 1
    by_poc = {p["poc"]: yuv_tensor(f, np.uint8) for p, f in zip(params, bad)}
    pics = StreamDecoder(data).output_order(compare=lambda p: dict(ref=by_poc[p["poc"]], block_map=True) if p["poc"] != params[0]["poc"] else None)
    seen = 0
    for p, planes in pics:
        k = p["decode_index"]
        if k == 0:
            assert p["compare"] is None
            continue
        d = dict(p["compare"])
        want = mr.compare(frames[k], bad[k], 8, block_map=True)
        assert isinstance(d["map"], np.ndarray) and np.array_equal(d["map"].view(np.uint64), want["map"])
        d["map"] = None
        same(d, dict(want, map=None), k)
        assert (sum(d["n_diff"]) != 0) == (k == 2)
        assert all(np.array_equal(np.asarray(g).view(np.uint16), f) for g, f in zip(planes, frames[k]))      # the pictures still come out
        seen += 1
    assert seen == len(frames) - 1


def test_application_ref(short_stream):
    """tools/xevd_gpu_app.py --ref --expect-identical in a fresh process: status 0 and a line per picture for the expected file (in output order, what -o
    writes), status 1 at the perturbed picture of a file in decoding order"""
    data, params, frames = short_stream
    order = sorted(range(len(frames)), key=lambda k: params[k]["poc"])      # one IDR period
    with tempfile.TemporaryDirectory() as td:
        fin, good, bad = (os.path.join(td, n) for n in ("s.evc", "good.yuv", "bad.yuv"))
        with open(fin, "wb") as f:
            f.write(data)
        blob = [b"".join(pl.astype(np.uint8).tobytes() for pl in frames[k]) for k in order]
        with open(good, "wb") as f:
            f.write(b"".join(blob))
        hurt = bytearray(blob[3])
        hurt[136 * 10 + 17] ^= 4
        app = [sys.executable, os.path.join(ROOT, "tools", "xevd_gpu_app.py"), "-i", fin]
        r = subprocess.run(app + ["--ref", good, "--expect-identical"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        lines = r.stdout.decode().splitlines()
        assert len(lines) == len(frames) + 1 and all("n_diff 0" in ln and "PSNR-Y inf" in ln and "SSIM-Y 1.000000" in ln for ln in lines[:-1])
        assert lines[-1].startswith(f"{len(frames)} pictures compared, 0 differ")
        # a file that differs, here in decoding order with --ref-order decoding: status 1 at that picture, whose line is still printed
        k = order[3]
        with open(bad, "wb") as f:
            f.write(b"".join(bytes(hurt) if j == k else b"".join(pl.astype(np.uint8).tobytes() for pl in fr) for j, fr in enumerate(frames)))
        r = subprocess.run(app + ["--ref", bad, "--ref-order", "decoding", "--expect-identical"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 1, r.stderr.decode()
        out = r.stdout.decode()
        assert "first Y(17,10)" in out and "n_diff 1 " in out and len(out.splitlines()) == k + 1 and "pictures compared" not in out
        # without --expect-identical the same file is reported to the end (the tool's compare= object, in this process)
        import importlib.util
        spec = importlib.util.spec_from_file_location("xevd_gpu_app", os.path.join(ROOT, "tools", "xevd_gpu_app.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
        from xevd_amd.player import StreamDecoder
        cmp = tool.RefCompare(bad, "decoding", False, 0)
        pics = StreamDecoder(data).output_order(output_bit_depth=0, compare=cmp)
        cmp.finish()
        assert (cmp.n_cmp, cmp.n_bad) == (len(frames), 1) and [sum(p["compare"]["n_diff"]) for p, _ in pics].count(0) == len(frames) - 1
