"""GPU suite of the picture statistics (xgpu_pic_stats / XgpuDecoder.pic_stats / StreamDecoder(stats=) / tools/xevd_gpu_app.py --stats): pictures are uploaded
with pic_upload and every expectation is tests/stats_ref.py on the uploaded arrays - never GPU output -, bit for bit, the bits of light_sum and light_mean
included.

Sizes are the smallest at which the kernels can go wrong: 8x8 (chroma planes of 4x4: less than one vector), 72x40 (a 64x32 tile and an 8-sample remainder both
ways), 136x72 (several tiles both ways), 200x136 minus (2, 6, 4, 2) = 192x130 (chroma planes of 96x65: an odd height; a left crop that takes the 16-byte loads
away from the luma plane) and one 4096x1088: 3264 tiles for at most 2048 workgroups, so a workgroup walks several tiles, changes plane on the way and must flush
its LDS histogram there."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import golden_io
import stats_ref as sr
from xevd_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -101, -104
NO_CROP = (0, 0, 0, 0)
SIZES = [(8, 8, NO_CROP), (72, 40, NO_CROP), (136, 72, NO_CROP), (200, 136, (2, 6, 4, 2))]
INT_KEYS = ("n", "sum", "sum_sq", "min", "max", "pctl", "light_n", "light_max_code", "light_pctl_code")
FILL = 0xA5
_LIN = {}


def lin_of(transfer, bd):
    if (transfer, bd) not in _LIN:
        _LIN[transfer, bd] = abi.stats_lin(abi.load(), transfer, bd)
    return _LIN[transfer, bd]


def rand_pic(seed, w, h, bd):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, (h >> s, w >> s)).astype(np.uint16) for s in (0, 1, 1)]


def const_pic(w, h, v):
    return [np.full((h >> s, w >> s), v, np.uint16) for s in (0, 1, 1)]


def rails_pic(w, h, bd):
    """0 and 2^bd - 1 alternating along a row, the phase alternating down the rows"""
    out = []
    for s in (0, 1, 1):
        yy, xx = np.mgrid[0:h >> s, 0:w >> s]
        out.append((((yy + xx) & 1) * ((1 << bd) - 1)).astype(np.uint16))
    return out


def any16_pic(seed, w, h):
    """any 16-bit pattern: most of them above 2^10 - 1"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << 16, (h >> s, w >> s)).astype(np.uint16) for s in (0, 1, 1)]


def two_valued_pic(w, h, crop, lo, hi, fewer=0):
    """inside the crop the first quarter of every plane's samples (raster order), less `fewer`, is lo and the rest hi: with n a multiple of 4 the percentile
    2500 lies exactly on its threshold (cum * 10000 == 2500 * n) for fewer = 0 and misses it by one sample for fewer = 1; outside the crop: hi + 1"""
    out = []
    for c, s in enumerate((0, 1, 1)):
        pl = np.full((h >> s, w >> s), hi + 1, np.uint16)
        view = pl[crop[2] >> s:(h - crop[3]) >> s, crop[0] >> s:(w - crop[1]) >> s]
        flat = np.full(view.size, hi, np.uint16)
        assert view.size % 4 == 0
        flat[:view.size // 4 - fewer] = lo
        view[:] = flat.reshape(view.shape)
        out.append(pl)
    return out


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


def bits64(x):
    return int(np.float64(x).view(np.uint64))


def bits32(x):
    return int(np.float32(x).view(np.uint32))


def same(got, want, what=""):
    """pic_stats' dict against stats_ref.stats': the integers, both histograms, and the floats bit for bit"""
    for k in INT_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("hist", "light_hist"):
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
            assert g.shape == want[k].shape and np.array_equal(g.view(np.uint32), want[k]), (what, k)
    if want["hist"] is not None:
        assert [int(h.astype(np.uint64).sum()) for h in want["hist"]] == got["n"], (what, "bins sum to n")
    for k in ("light_sum", "light_mean"):
        assert bits64(got[k]) == bits64(want[k]), (what, k, got[k], want[k])
    assert bits32(got["light_max"]) == bits32(want["light_max"]), (what, "light_max")
    assert [bits32(v) for v in got["light_pctl"]] == [bits32(v) for v in want["light_pctl"]], (what, "light_pctl")
    assert got["mean"] == [s / n for s, n in zip(want["sum"], want["n"])], (what, "mean")


def ref_stats(pic, bd, crop=NO_CROP, hist_bits=8, percentiles=(100, 9999), light=None):
    lin = lin_of(light["transfer"], bd) if light is not None else None
    return sr.stats(pic, bd, crop=crop, hist_bits=hist_bits, pctl_e4=percentiles, light=light, lin=lin)


# ------------------------------------------------------------------------------------------------ the census, the histograms and the percentiles
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("w,h,crop", SIZES)
def test_contents(w, h, crop, bd):
    """uniform random, constant (every lane in one bin), the two rails alternating, a two-valued picture on the percentile's threshold and one sample short of
    it, and - at depth 10 - 16-bit patterns above 2^B; with no histogram and 2^4, 2^8, 2^B bins"""
    top = (1 << bd) - 1
    contents = {"random": rand_pic(1, w, h, bd), "constant": const_pic(w, h, 3 << (bd - 3)), "constant 0": const_pic(w, h, 0), "rails": rails_pic(w, h, bd),
                "threshold": two_valued_pic(w, h, crop, 17, top - 17), "threshold - 1": two_valued_pic(w, h, crop, 17, top - 17, fewer=1)}
    if bd == 10:
        contents["above 2^B"] = any16_pic(2, w, h)
        contents["0xFFFF"] = const_pic(w, h, 0xFFFF)
    dec, (slot,) = open_pics(bd, contents["random"])
    with dec:
        for name, pic in contents.items():
            dec.pic_upload(slot, [p.view(np.int16) for p in pic])
            for hb in (0, 4, 8, bd):
                pct = (2500, 2501) if name.startswith("threshold") else (100, 9999)
                got = dec.pic_stats(slot, crop=crop, hist_bits=hb, percentiles=pct)
                want = ref_stats(pic, bd, crop, hb, pct)
                same(got, want, (name, hb))
                if name.startswith("constant") or name == "0xFFFF":
                    assert got["min"] == got["max"] and got["var"] == [0.0] * 3
                    assert hb == 0 or [int(got["hist"][c].max()) for c in range(3)] == got["n"]
                if hb and name == "threshold":
                    assert got["pctl"] == [[(17 >> (bd - hb)) << (bd - hb), ((top - 17) >> (bd - hb)) << (bd - hb)]] * 3
                if hb and name == "threshold - 1":
                    assert got["pctl"] == [[((top - 17) >> (bd - hb)) << (bd - hb)] * 2] * 3
                if name == "above 2^B" and hb:
                    assert got["max"][0] > top and int(got["hist"][0, -1]) > got["n"][0] // 2      # the last bin takes them; the sums stay exact
        dec.pic_upload(slot, [p.view(np.int16) for p in contents["random"]])
        got = dec.pic_stats(slot, crop=crop, hist_bits=bd, percentiles=(0, 10000))      # the lowest and the highest occupied bin: with 2^B bins, min and max
        assert got["pctl"] == [[m, x] for m, x in zip(got["min"], got["max"])]


def test_more_tiles_than_workgroups():
    """4096x1088: 2176 luma tiles and 2 x 544 chroma tiles"""
    bd, w, h = 10, 4096, 1088
    pic = rand_pic(3, w, h, bd)
    pic[1][:] = 512                    # a flat plane between two busy ones: the wave-wide add, then a flush into another plane's bins
    pic[2] >>= 2
    dec, (slot,) = open_pics(bd, pic)
    with dec:
        for hb in (10, 4, 0):
            same(dec.pic_stats(slot, hist_bits=hb), ref_stats(pic, bd, NO_CROP, hb), hb)
        same(dec.pic_stats(slot, crop=(2, 0, 0, 2), hist_bits=8), ref_stats(pic, bd, (2, 0, 0, 2), 8), "cropped, element loads")
        light = dict(transfer=16, matrix=9)
        same(dec.pic_stats(slot, hist_bits=10, light=light), ref_stats(pic, bd, NO_CROP, 10, light=light), "light")


# ------------------------------------------------------------------------------------------------ the light level
def light_cases():
    """each supported matrix at both ranges; chroma_loc 0 and 2 with both upsampling modes; transfers 1, 16 and 18"""
    out = []
    for k, matrix in enumerate((1, 4, 5, 6, 7, 9)):
        for fr in (False, True):
            out.append(dict(matrix=matrix, full_range=fr, chroma_loc=(0, 2)[(k + fr) & 1], upsample=("linear", "nearest")[k & 1], transfer=(1, 16, 18)[k % 3]))
    for loc in (0, 2):
        for up in ("linear", "nearest"):
            for tc in (1, 16, 18):
                out.append(dict(matrix=9, full_range=False, chroma_loc=loc, upsample=up, transfer=tc))
    return out


def smooth_pic(seed, w, h, bd):
    """a gradient with a little noise, chroma near the middle: R'G'B' codes that stay inside the range, unlike those of random Y'CbCr"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    y = ((yy * 3 + xx * 5) * ((1 << bd) - 1) // (3 * h + 5 * w) + rng.integers(-2, 3, (h, w))).clip(0, (1 << bd) - 1).astype(np.uint16)
    c = [((1 << (bd - 1)) + rng.integers(-(1 << (bd - 3)), 1 << (bd - 3), (h >> 1, w >> 1))).astype(np.uint16) for _ in range(2)]
    return [y] + c


@pytest.mark.parametrize("w,h,crop", [(72, 40, NO_CROP), (200, 136, (2, 6, 4, 2))])
def test_light(w, h, crop):
    import torch
    bd = 10
    pics = {"random": rand_pic(4, w, h, bd), "smooth": smooth_pic(5, w, h, bd), "constant": const_pic(w, h, 700)}
    dec, (slot,) = open_pics(bd, pics["random"])
    with dec:
        for name, pic in pics.items():
            dec.pic_upload(slot, [p.view(np.int16) for p in pic])
            for k, light in enumerate(light_cases()):
                hb = (0, 8, 10)[k % 3]
                got = dec.pic_stats(slot, crop=crop, hist_bits=hb, percentiles=(5000, 9990), light=light)
                want = ref_stats(pic, bd, crop, hb, (5000, 9990), light)
                same(got, want, (name, light))
                assert got["light_n"] == int(got["light_hist"].sum()) == (w - crop[0] - crop[1]) * (h - crop[2] - crop[3])
                if light["transfer"] == 16:
                    assert got["max_cll"] == 10000.0 * float(want["light_max"]) and got["max_fall"] == 10000.0 * float(want["light_mean"])
                else:
                    assert "max_cll" not in got
                if k % 5 == 0:      # the cross-check: the bincount of the channel-wise maximum of the RGB tensor the decoder itself makes
                    opts = {o: light[o] for o in ("matrix", "full_range", "chroma_loc", "upsample")}
                    rgb = dec.pic_output_tensor(slot, layout="rgb", dtype=torch.uint16 if hasattr(torch, "uint16") else torch.int16, crop=crop, **opts)
                    m = rgb.view(torch.int16).to(torch.int64).amax(dim=0).reshape(-1)
                    assert torch.equal(torch.bincount(m, minlength=1 << bd), got["light_hist"].to(torch.int64)), (name, light)


@pytest.mark.parametrize("bd", [8, 12])
def test_light_other_depths(bd):
    w, h, crop = 136, 72, (0, 2, 2, 0)
    pic = smooth_pic(6, w, h, bd)
    dec, (slot,) = open_pics(bd, pic)
    with dec:
        for light in (dict(transfer=16, matrix=9), dict(transfer=18, matrix=9, full_range=True, upsample="nearest"), dict(transfer=13, matrix=1, chroma_loc=1),
                      dict(transfer=1, matrix=5, chroma_loc=5)):
            for hb in (0, bd):
                same(dec.pic_stats(slot, crop=crop, hist_bits=hb, light=light), ref_stats(pic, bd, crop, hb, light=light), (bd, light, hb))
        # the same transfer again after another one: the table of the context is made again
        again = dict(transfer=16, matrix=9)
        same(dec.pic_stats(slot, hist_bits=4, light=again), ref_stats(pic, bd, NO_CROP, 4, light=again), "transfer 16 again")


# ------------------------------------------------------------------------------------------------ the call
def raw_call(dec, pic, par, res, hist=None, hist_size=None, stream=None):
    hp = None if hist is None else C.c_void_p(hist if isinstance(hist, int) else hist.data_ptr())
    if hist_size is None:
        hist_size = 0 if hist is None else hist.numel() * 4
    return dec.lib.xgpu_pic_stats(dec.ctx, pic, C.byref(par) if par is not None else None, C.c_void_p(res if isinstance(res, int) else res.data_ptr()), hp,
                                  hist_size, stream)


def filled(n, dtype):
    import torch
    return torch.full((n * dtype.itemsize,), FILL, dtype=torch.uint8, device="cuda").view(dtype)


def test_prefilled_buffers_second_call_streams_and_sync_false():
    import torch
    bd, w, h, crop = 10, 200, 136, (2, 6, 4, 2)
    pic = smooth_pic(7, w, h, bd)
    light = dict(transfer=16, matrix=9, chroma_loc=2)
    dec, (slot,) = open_pics(bd, pic)
    with dec:
        want = ref_stats(pic, bd, crop, 8, light=light)
        par = abi.make_stats_params(crop, 8, (100, 9999), True, matrix=9, chroma_loc=2, transfer=16)
        nwords = 3 * 256 + 1024
        assert dec.lib.xgpu_stats_hist_size(C.byref(par), bd) == nwords * 4
        # the caller clears nothing: result and histograms pre-filled with 0xA5, on the context's stream
        res, hist = filled(22, torch.int64), filled(nwords, torch.int32)
        assert int(res[0].item()) & 0xFF == FILL
        torch.cuda.synchronize()
        assert raw_call(dec, slot, par, res, hist) == 0
        dec.sync()
        d = abi.stats_result_dict(res.cpu().numpy())
        d["mean"], d["hist"], d["light_hist"] = [s / n for s, n in zip(d["sum"], d["n"])], hist[:768].view(3, 256), hist[768:]
        same(d, want, "raw call")
        raw = res.cpu().numpy().view(np.uint32)
        assert raw[39] == 0 and raw[43] == 0      # `reserved` and `reserved2` are written too
        # a second call into the same buffers leaves identical bytes
        res1, hist1 = res.clone(), hist.clone()
        assert raw_call(dec, slot, par, res, hist) == 0
        dec.sync()
        assert torch.equal(res, res1) and torch.equal(hist, hist1)
        # the same call on a side stream
        s = torch.cuda.Stream()
        res_s, hist_s = filled(22, torch.int64), filled(nwords, torch.int32)
        torch.cuda.synchronize()
        assert raw_call(dec, slot, par, res_s, hist_s, stream=C.c_void_p(s.cuda_stream)) == 0
        s.synchronize()
        assert torch.equal(res_s, res1) and torch.equal(hist_s, hist1)
        with torch.cuda.stream(s):
            same(dec.pic_stats(slot, crop=crop, light=light), want, "caller's stream")
        # without light the light fields are written as 0, and no histogram: d_hist is not read
        res0 = filled(22, torch.int64)
        torch.cuda.synchronize()
        assert raw_call(dec, slot, abi.make_stats_params(crop, 0), res0, None) == 0
        dec.sync()
        assert not res0.cpu().numpy().view(np.uint8)[96:].any()
        assert abi.stats_result_dict(res0.cpu().numpy())["sum"] == want["sum"]
        # sync=False: the raw words and the device tensors, nothing read back; out= takes the words
        out = filled(22, torch.int64)
        t, hg, lh = dec.pic_stats(slot, crop=crop, light=light, out=out, sync=False)
        torch.cuda.synchronize()
        assert t is out and torch.equal(t, res1) and hg.dtype == torch.int32 and tuple(hg.shape) == (3, 256) and tuple(lh.shape) == (1024,)
        assert torch.equal(hg.reshape(-1), hist1[:768]) and torch.equal(lh, hist1[768:])
        d2 = abi.stats_result_dict(t.cpu().numpy())
        full = dec.pic_stats(slot, crop=crop, light=light)
        assert all(d2[k] == full[k] for k in d2)
        t0, h0, l0 = dec.pic_stats(slot, hist_bits=0, sync=False)
        assert h0 is None and l0 is None


def test_refusals_queue_nothing():
    """every refusal returns its code, leaves a message and does not touch the pre-filled result and histogram.  Pointer refusals are made with host pointers,
    misaligned addresses and sizes that are too small - never with an address outside an allocation"""
    import torch
    bd, w, h = 10, 72, 40
    pic = rand_pic(8, w, h, bd)
    dec, (pa, pb) = open_pics(bd, pic, pic)
    with dec:
        lib, ctx = dec.lib, dec.ctx
        nwords = 3 * 256 + 1024
        res, hist = filled(22, torch.int64), filled(nwords + 2, torch.int32)
        good = dict(hist_bits=8, light=True, transfer=16)

        def par(**kw):
            return abi.make_stats_params(**dict(good, **kw))

        def refused(rc, word=None, code=INVALID):
            assert rc == code, rc
            msg = lib.xgpu_last_error(ctx)
            assert msg and (word is None or word in msg), msg
            torch.cuda.synchronize()
            assert bool((res.view(torch.uint8) == FILL).all().item()) and bool((hist.view(torch.uint8) == FILL).all().item())

        assert raw_call(dec, pa, par(), res, hist) == 0      # the call these are variations of
        dec.sync()
        assert abi.stats_result_dict(res.cpu().numpy())["n"] == [w * h, w * h // 4, w * h // 4]
        res.view(torch.uint8).fill_(FILL); hist.view(torch.uint8).fill_(FILL)      # noqa: E702
        torch.cuda.synchronize()
        freed = dec.pic_alloc()
        dec.pic_free(freed)
        for bad in (-1, 99, freed):                                                                   # a bad slot, a slot with no picture
            refused(raw_call(dec, bad, par(), res, hist), b"no picture")
        for crop in ((1, 1, 0, 0), (0, 0, 3, 0), (-2, 0, 0, 0), (36, 36, 0, 0), (0, 0, 40, 0)):        # odd, negative, nothing left
            refused(raw_call(dec, pa, par(crop=crop), res, hist), b"crop")
        for hb in (1, 3, 11, 12, -4):
            refused(raw_call(dec, pa, par(hist_bits=hb), res, hist), b"hist_bits")
        for pct in ((-1, 0), (0, 10001)):
            refused(raw_call(dec, pa, par(pctl_e4=pct), res, hist), b"pctl_e4")
        refused(raw_call(dec, pa, par(light=2), res, hist), b"light")
        refused(raw_call(dec, pa, par(upsample=2), res, hist), b"upsample")
        refused(raw_call(dec, pa, par(chroma_loc=6), res, hist), b"chroma_loc")
        refused(raw_call(dec, pa, par(matrix=2), res, hist), b"matrix", UNSUPPORTED)
        refused(raw_call(dec, pa, par(transfer=2), res, hist), b"transfer", UNSUPPORTED)
        refused(raw_call(dec, pa, par(transfer=17), res, hist), b"transfer", UNSUPPORTED)
        refused(raw_call(dec, pa, None, res, hist), b"NULL")
        hres = np.zeros(22, np.int64)
        refused(raw_call(dec, pa, par(), int(hres.ctypes.data), hist), b"device memory")              # the result in host memory
        assert not hres.any()
        refused(raw_call(dec, pa, par(), res.data_ptr() + 4, hist), b"aligned")                       # the result not 8-byte aligned
        hhist = np.zeros(nwords, np.uint32)
        refused(raw_call(dec, pa, par(), res, int(hhist.ctypes.data), nwords * 4), b"device memory")  # the histogram in host memory
        assert not hhist.any()
        refused(raw_call(dec, pa, par(), res, hist.data_ptr() + 2, nwords * 4), b"aligned")           # not 4-byte aligned
        refused(raw_call(dec, pa, par(), res, hist, nwords * 4 - 4), b"needs")                        # says it is too small
        refused(raw_call(dec, pa, par(), res, hist[:nwords - 1].clone()), b"needs")                   # is too small
        refused(raw_call(dec, pa, par(), res, None), b"d_hist")                                       # a histogram asked for, none given
        assert lib.xgpu_pic_stats(ctx, pa, C.byref(par()), None, C.c_void_p(hist.data_ptr()), nwords * 4, None) == INVALID
        # the Python layer refuses what it can tell without the library, and hands the rest on
        from xevd_amd.decoder import XgpuError
        with pytest.raises(ValueError):
            dec.pic_stats(pa, light=dict(matrix=1))
        with pytest.raises(ValueError):
            dec.pic_stats(pa, light=dict(transfer=1, upsample="cubic"))
        with pytest.raises(XgpuError, match="crop"):
            dec.pic_stats(pa, crop=(1, 0, 0, 0))
        with pytest.raises(XgpuError, match="hist_bits"):
            dec.pic_stats(pa, hist_bits=11)
        # an open frame, as xgpu_pic_compare has it
        dec.frame_begin(pa, 0, {})
        refused(raw_call(dec, pb, par(), res, hist), b"a frame is open")
        dec.frame_end()
        assert raw_call(dec, pb, par(), res, hist) == 0
        dec.sync()
        assert abi.stats_result_dict(res.cpu().numpy())["n"] == [w * h, w * h // 4, w * h // 4]


# ------------------------------------------------------------------------------------------------ a decoded stream
STREAM = "stream_ippp_10b_offsets.npz"


def test_stream_stats():
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, STREAM))["bytes"].tobytes()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]
    light = dict(transfer=1, matrix=1, full_range=False, chroma_loc=0, upsample="linear")      # what a stream without a VUI gets
    got = list(StreamDecoder(data).pictures(download=False, stats=dict(hist_bits=10, light=True)))
    assert len(got) == len(ref) > 1
    for (p, _), (q, planes) in zip(got, ref):
        assert p["poc"] == q["poc"]
        same(p["stats"], ref_stats(planes, p["bit_depth"], NO_CROP, 10, light=light), ("stream", p["poc"]))
    # the callable, a dict that overrides the VUI's transfer, None for a picture; through output_order: the histograms as arrays, the pictures still come out
    skip = ref[1][0]["poc"]
    pics = StreamDecoder(data).output_order(stats=lambda p: None if p["poc"] == skip else dict(light=dict(transfer=16), percentiles=(0, 10000)))
    assert len(pics) == len(ref)
    by_poc = {q["poc"]: planes for q, planes in ref}
    for p, planes in pics:
        assert all(np.array_equal(g, f) for g, f in zip(planes, by_poc[p["poc"]]))
        if p["poc"] == skip:
            assert p["stats"] is None
            continue
        assert isinstance(p["stats"]["hist"], np.ndarray) and isinstance(p["stats"]["light_hist"], np.ndarray) and "max_cll" in p["stats"]
        same(p["stats"], ref_stats(by_poc[p["poc"]], p["bit_depth"], NO_CROP, 8, (0, 10000), dict(light, transfer=16)), ("output_order", p["poc"]))


def test_application_stats():
    """tools/xevd_gpu_app.py --stats in a fresh process: one line per picture in decoding order whose integers are stats_ref's"""
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, STREAM))["bytes"].tobytes()
    ref = [(p, planes) for p, planes in StreamDecoder(data).pictures()]
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "s.evc"), os.path.join(td, "stats.txt")
        with open(fin, "wb") as f:
            f.write(data)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "xevd_gpu_app.py"), "-i", fin, "--stats", fout], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        lines = open(fout).read().splitlines()
    assert len(lines) == len(ref)
    pat = re.compile(r"([YUV]) n (\d+) min (\d+) max (\d+) mean ([0-9.]+) pctl (\d+) (\d+)")
    for ln, (p, planes) in zip(lines, ref):
        want = ref_stats(planes, p["bit_depth"])
        assert ln.startswith(f"POC {p['poc']}  Y n ") and "light" not in ln      # (no VUI in this stream: no transfer characteristic, no light level)
        comps = pat.findall(ln)
        assert [m[0] for m in comps] == ["Y", "U", "V"]
        for c, m in enumerate(comps):
            assert [int(v) for v in m[1:4]] == [want["n"][c], want["min"][c], want["max"][c]] and [int(m[5]), int(m[6])] == want["pctl"][c], (ln, c)
            assert m[4] == f"{want['sum'][c] / want['n'][c]:.4f}"
