"""Device-output rate: an 8K 10-bit picture converted into torch tensors by xgpu_pic_output_device (k_output_rgb / k_output / k_output_semiplanar / k_output_yuv444 / k_output_cm), timed with torch
events on the output stream (median of --iters launches after warm-up), against the plain device copy rate of the same run
(xgpu_measure_copy_bw).  Bytes are algorithmic: 3 bytes of samples read per pixel (luma + two quarter-size chroma planes, 16 bit) and what the
format writes.  Prints one line per form and a JSON line; --out also writes the JSON to a file.
The side-information forms (xgpu_frame_side_info: k_side_blocks / k_side_flow) follow, on a picture decoded from a synthetic B-picture batch: 16 bytes per
4x4 unit read + what the form writes, and the same flow made in torch from the BLOCKS tensor (repeat_interleave twice, crop, scale, cast).

The scaled leg (xgpu_pic_output_device_scaled: k_scale_vertical + k_scale_horizontal) resizes the same picture to 224x224 and to 1920x1080 f32 planar with the
ImageNet normalise, and times next to it - same run, same stream - the route without it: the full-size f32 tensor, torch's
interpolate(mode="bilinear", antialias=True) and the normalise in torch; and the time the measured copy rate needs for the bytes the scaled call must move (the
picture read once, the destination written once).  The call is timed whole; the split between its two kernels is what
rocprofv3 --kernel-trace --stats shows for `--legs scaled`.

The scaled_cm leg (xgpu_pic_output_device_scaled_cm / _rois_cm: the vertical passes + k_scale_horizontal_cm / k_rois_horizontal_cm) takes the picture as PQ / BT.2020
to sRGB / BT.709 through the tone curve at three shapes - 224x224 f32 normalised, 1920x1080 u8, 64 tiles at 224x224 f32 normalised - and alternates each, from an
idle device, with (i) the plain scaled / ROI call at the same shape: the price of the transform, and (ii) the only route without it: the full-size colour= f32
tensor, interpolate(antialias=True) and the normalise (or the u8 rounding) in torch, with the largest difference between the two (on random samples through PQ
that is a record of filtering encoded samples against display light, not an error bound).  device_us is the kernels alone, queued behind a wait.

The scaled_lin leg (xgpu_pic_output_device_scaled_lin / _rois_lin: k_lin_vertical + k_lin_horizontal and their batch forms) takes the same picture the same way at
the same three shapes, filtering linear light, and alternates each with (i) the scaled_cm call of the same shape: the price of correctness, and (ii) the only
correct route without it: the full-size linear-light f32 tensor of the source primaries, interpolate(antialias=True), then matrix, clip, sRGB encode and the
normalise (or the u8 rounding) in torch - the tone curve left out, in the caller's favour.

The rois leg (xgpu_pic_output_device_rois: k_rois_vertical + k_rois_horizontal) makes 64 images of 224x224 f32 planar, normalised, from the same picture by one
call - (a) the 8 x 8 grid of tiles, stretched; (b) 64 seeded boxes with sides of 64..512 samples, letterboxed - and times next to it, alternating with it in the
same run on the same stream, the route without it: 64 calls of xgpu_pic_output_device_scaled with the crop set to the rectangle (for (b) at the inner size, into
tensors of their own; the inner rectangles of the two routes are compared).  Events bracket each whole route as the host queues it, so the time is the device's
from the first kernel to the last, host gaps included; host_us is what the host spends queueing.  The split between the two kernels is what
rocprofv3 --kernel-trace --stats shows for `--legs rois`.

The rois_dev leg (xgpu_pic_output_device_rois_dev: k_rois_prepare + the two kernels of the rois leg) takes the same two workloads with the boxes in a device
tensor, as a detector leaves them, and alternates - same protocol as the rois leg - route A, what the host-box call needs then: boxes.cpu() (a synchronisation
and a read-back) and xgpu_pic_output_device_rois, with route B: the device-box call on the tensor itself, max_roi set to the true maxima of the workload.  The
split of B into its three kernels is what rocprofv3 --kernel-trace --stats shows for `--legs rois_dev`.

The warp leg (xgpu_pic_output_device_warp: k_output_warp) takes the 64 boxes of the rois leg, each turned by a seeded angle, to 224x224 f32 planar, normalised,
and alternates - the rois leg's protocol - route A, what a caller does without it: the full-size f32 R'G'B' tensor, torch's affine_grid + grid_sample(bilinear,
border, align_corners=False) on its expand(64, ...) and the normalise, with route B: the one call, at samples = 1 and at samples = 4.  It also times the same
boxes upright against rois= with the stretch fit: what gathering costs over the two separable passes.

The remap leg (xgpu_pic_output_device_remap: k_output_remap) undistorts the whole picture through a Brown-Conrady lens grid to u8 planar R'G'B' at its own size,
with one node per pixel (step 0) and with a mesh (step 4), S = 1; runs the identity mesh at step 4 beside the plain xgpu_pic_output_device call of the same form,
which is its floor; and cuts four 1920x1080 virtual views out of an equidistant fisheye at S = 4, step 4 (a float32 mesh).  Each is alternated - the rois leg's
protocol - with the torch route: the full-size f32 R'G'B' tensor plus grid_sample(bilinear, border, align_corners=False) through a dense normalised grid made once,
and the largest difference between the two results is recorded in code values of the u8 output (the S = 4 views antialias, grid_sample does not).

The residual leg (xgpu_batch_residual: k_resid_planes / k_resid_energy) writes the residual of a synthetic B-picture batch of the same size as int16 4:2:0
planes, as 4:4:4 planar int16 and float16, and as the per-unit energy.  Bytes are algorithmic: the arena bytes actually coded (2 per sample of every coded
component block), 4 per 4x4 unit of owner map, 32 per CU record, and what the form writes.  The whole measurement - copy rate included - is repeated --repeat
times in the one process; every run is kept.

The compare leg (xgpu_pic_compare: k_compare_init + k_compare) compares the picture with a second slot of other random samples - every sample differs, the most
the census has to do - as the census alone, with the SSIM, with the block map and with both, with the SSIM against the same planes as a tensor (the 16-byte
loads and, one element into its allocation, the element loads), and with both against the picture itself.  `us` is the device time of the call (median of --iters
launches queued behind a wait, as the full-size forms are timed); `alternated_us` the same call from an idle device, as the torch route is timed.  Next to each: (a) the time the measured copy rate
needs for the bytes the call must read, the two pictures once; (b) what a caller does without it, alternated with the call in the same run on the same stream:
two yuv420p tensors from xgpu_pic_output_device and per plane the SSE, the number of differing samples and the largest difference in torch (int32 temporaries;
no SSIM: torch cannot make it exactly).  The split between the two kernels is what rocprofv3 --kernel-trace --stats shows for `--legs compare`.
The stats leg (xgpu_pic_stats: k_stats, k_stats_light, k_stats_finish behind a memset) takes the statistics of three contents - uniform random, constant, a smooth
gradient with +-2 codes of noise: the contention of the LDS histogram depends on the content - in four forms: the census alone, with 2^8 and 2^B bins, and with
the light level.  Each is timed as the other legs are (the median of --iters calls queued behind a wait) and, alternated with it from an idle device, the torch
route: a yuv420p tensor, then bincount, sum, min and max per plane; with light the u16 RGB tensor, amax, bincount and a gather through lin.

The resampled leg (xgpu_pic_output_device_resampled / _rois_resampled: k_resampled_vertical + k_resampled_horizontal) takes the picture to 224x224 f32
normalised, to 1080p u8 and to 64 tiles at 224x224 with the Catmull-Rom kernel and antialias, and alternates - the scaled_cm leg's protocol - each with the plain
bilinear call of the same shape (the price of the window twice as wide) and with the route without it: the full-size f32 tensor, then torch's
interpolate(bicubic, antialias=True) and the normalise or the u8 rounding.  The largest difference to that route is a record, not a test.

The ladder leg (xgpu_pic_output_device_ladder: k_ladder_vertical + k_ladder_horizontal) takes the picture to P010 rungs 3840x2160, 1920x1080, 1280x720 and
640x360 with centre chroma siting on both sides and alternates - the rois leg's protocol - the one call with the route without it (the full-size P010 surface,
then per rung and plane torch's interpolate(bilinear, antialias=True), rounding and repacking) and with the plain full-size surface, the floor of reading the
picture once; four one-rung calls are alternated on their own (each makes its tap tables again: the context keeps those of one key).  `device_us` is the time
of the kernels alone (median of --iters calls queued behind a wait).  The largest difference between each rung's planes and the torch route in float64 is
recorded in code values; it is a record, not a test.
The packed leg (xgpu_pic_output_device_packed: k_output_packed_rgb / k_output_packed_422) writes RGBA u8, RGBA f16, RGBA u8 through PQ / BT.2020 -> sRGB, 10:10:10:2,
YUYV u8 and Y210 and alternates - the rois leg's protocol - each with the nearest call that existed before it (the interleaved RGB tensor of the dtype, NV12, P010) and
with the torch route it replaces on top of that call (a cat with an alpha plane; shifts and ors on an int32 tensor; a row repeat and a stack).  Next to the times:
the ratio of the bytes the two calls move, and whether the packed call takes more than that ratio of its counterpart's time beyond the spread of the run.
The lut3d leg (xgpu_pic_output_device_lut3d / _packed_lut3d: k_output_lut3d / k_output_packed_lut3d) writes U8 / U16 / F32 interleaved RGB, RGBA u8 and 10:10:10:2
through a LUT of n = 17, 33, 65 and alternates - the rois leg's protocol - each with the nearest call without a LUT and with that call's colour-managed form
(PQ / BT.2020 -> sRGB through the tone curve); then the F32 call against the route it replaces, the full-size f32 tensor + a 5-D grid_sample (trilinear, float:
the largest difference is a record, not a test).  All of it on the random picture and on a smooth gradient.  (profiles/output_lut3d_placements_8k_10b.json was
taken while the kernel still had its three placements of the tables side by side - the `global`, `shaper_lds` and `all_lds` columns; `shaper_lds` is the kernel
that stayed, and profiles/output_lut3d_8k_10b.json is this leg as it is now.)
The dither leg (xgpu_pic_output_device_dithered / _packed_dithered: k_output_dither_rgb / k_output_dither_semiplanar) alternates - the rois leg's protocol - each
dithered call with the plain call of the same layout, which reads and writes the same bytes: interleaved RGB u8, RGBA u8 through PQ / BT.2020 -> sRGB with the
tone curve, NV12 u8, and 10:10:10:2 from a 12-bit picture (a second decoder; the other legs' depth is --bit-depth).  RGB u8 runs Bayer 8, blue 64 and blue 128
side by side, the others blue 64.  Then the torch route the call replaces: the full-size f32 tensor, plus a tiled threshold tensor, floor, clamp and to(uint8).

The overlay leg (xgpu_pic_output_device_overlaid / _packed_overlaid: k_output_overlay_rgb / k_output_overlay_semiplanar) alternates, in one run per layout, the
plain call with the overlaid call over no layer, a 512 x 256 logo, a full-size BGRA subtitle plane that is 95 % transparent, and 16 / 64 / 256 boxes read from
device memory; then the torch routes on the written RGB tensor that the calls replace (slice and blend; boxes.cpu() and a loop of slices).

    python tools/bench_output_device.py [--width 7680 --height 4320 --bit-depth 10 --iters 100] [--legs all|full|scaled|scaled_cm|scaled_lin|resampled|rois|rois_dev|ladder|warp|remap|residual|compare|stats|packed|lut3d|dither|overlay] [--out out/output_device.json]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_transform(torch, rgb, to_srgb):
    """PQ / BT.2020 R'G'B' [3, H, W] f32 -> linear BT.709 (1.0 = 100 cd/m2, clipped), or that re-encoded as sRGB u8: the work a caller
    has without the fused kernel (the tone curve left out - in the caller's favour)"""
    m1, m2, c1, c2, c3 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0, 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
    mat = torch.tensor([[1.660491, -0.587641, -0.072850], [-0.124550, 1.132900, -0.008349], [-0.018151, -0.100579, 1.118730]], device=rgb.device)
    p = rgb.pow(1.0 / m2)
    lin = ((p - c1).clamp_min(0) / (c2 - c3 * p)).pow(1.0 / m1)
    lin = (torch.matmul(mat, lin.reshape(3, -1)).reshape(rgb.shape) * 100.0).clamp(0, 1)
    if not to_srgb:
        return lin
    enc = torch.where(lin < 0.0031308, 12.92 * lin, 1.055 * lin.pow(1.0 / 2.4) - 0.055)
    return (enc * 255.0).round().to(torch.uint8)


def torch_flow(torch, blocks, crop, dtype):
    """the dense field of lists 0 and 1 in luma samples from the BLOCKS tensor, in torch: what a caller does without k_side_flow"""
    cl, cr, ct, cb = crop
    v = blocks[:4]
    used = (blocks[4:6] != 0).repeat_interleave(2, 0)
    v = torch.where(used, v.to(torch.float32) * 0.25, torch.zeros((), device=v.device))
    v = v.repeat_interleave(4, 1).repeat_interleave(4, 2)
    return v[:, ct:v.shape[1] - cb, cl:v.shape[2] - cr].to(dtype).contiguous()


def timed(torch, s, fn, n, warm=5, sleep=True):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    if sleep:
        torch.cuda._sleep(int(3e8))      # the GPU waits while the host queues every timed launch: the events then bracket device time only
    for e0, e1 in ev:
        e0.record(s)
        fn()
        e1.record(s)
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]))


SCALED_SIZES = ((224, 224), (1080, 1920))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def scaled_leg(torch, dec, pic, s, a, res, copy_gbps):
    """the scaled call against full-size f32 output + F.interpolate(antialias=True) + normalise, and against the copy-rate time of its own bytes"""
    import torch.nn.functional as F
    w, h = a.width, a.height
    mean = torch.tensor(MEAN, device="cuda:0").view(3, 1, 1)
    inv = (1.0 / torch.tensor(STD, device="cuda:0")).view(3, 1, 1)
    full = dec.pic_output_tensor(pic, dtype=torch.float32)
    res["scaled"] = {}
    for hd, wd in SCALED_SIZES:
        for filt in ("bilinear", "area"):
            kw = dict(dtype=torch.float32, size=(hd, wd), filter=filt, mean=MEAN, std=STD)
            out = dec.pic_output_tensor(pic, **kw)
            us = timed(torch, s, lambda: dec.pic_output_tensor(pic, out=out, **kw), a.iters)
            nbytes = int(w * h * 3 + hd * wd * 12)
            floor_us = nbytes / (copy_gbps * 1e9) * 1e6
            r = {"us": round(us, 2), "bytes": nbytes, "copy_rate_us": round(floor_us, 2), "frac_copy": round(floor_us / us, 3)}
            if filt == "bilinear":
                def route():
                    dec.pic_output_tensor(pic, out=full, dtype=torch.float32)
                    return (F.interpolate(full[None], size=(hd, wd), mode="bilinear", antialias=True, align_corners=False)[0] - mean) * inv
                n = max(a.iters // 10, 5)
                r_us = timed(torch, s, route, n, warm=2, sleep=False)
                diff = float((route() - out).abs().max())
                r.update({"torch_route_us": round(r_us, 2), "speedup": round(r_us / us, 2), "max_abs_diff_vs_torch_route": diff})
                print(f"scaled {w}x{h} -> {wd}x{hd} f32 {filt:8s} {us:9.1f} us   torch route {r_us:9.1f} us ({r_us / us:.1f}x)   copy-rate time {floor_us:7.1f} us ({floor_us / us:.2f})   max |diff| {diff:.2e}")
            else:
                print(f"scaled {w}x{h} -> {wd}x{hd} f32 {filt:8s} {us:9.1f} us   copy-rate time {floor_us:7.1f} us ({floor_us / us:.2f})")
            res["scaled"][f"{wd}x{hd}_f32_planar_{filt}"] = r
    del full


def scaled_cm_leg(torch, dec, pic, s, a, res):
    """the colour-managed scaled call (PQ / BT.2020 -> sRGB through the tone curve) at three shapes, each alternated with (i) the plain scaled / ROI call at the
    same shape - the price of the transform - and (ii) the only route without it: the full-size colour= f32 tensor + F.interpolate(antialias=True) + the normalise
    (or the u8 rounding) in torch, with the max |diff| between the two"""
    import torch.nn.functional as F
    from xevd_amd import abi
    w, h = a.width, a.height
    colour = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
    mean = torch.tensor(MEAN, device="cuda:0").view(3, 1, 1)
    inv = (1.0 / torch.tensor(STD, device="cuda:0")).view(3, 1, 1)
    full = dec.pic_output_tensor(pic, dtype=torch.float32, matrix=9, colour=colour)
    tiles = abi.tile_rois(w, h, (w // 8) & ~1, (h // 8) & ~1)[:64]
    norm = dict(mean=MEAN, std=STD)
    shapes = (("224x224_f32_normalised", (224, 224), None, dict(dtype=torch.float32, **norm)), ("1920x1080_u8", (1080, 1920), None, dict(dtype=torch.uint8)),
              ("64_rois_224x224_f32_normalised", (224, 224), tiles, dict(dtype=torch.float32, **norm)))
    res["scaled_cm"] = {}
    for name, size, rois, kw in shapes:
        is_u8 = kw["dtype"] == torch.uint8
        roi_kw = {} if rois is None else dict(rois=rois)
        out = dec.pic_output_scaled_cm(pic, size, colour, matrix=9, **roi_kw, **kw)
        plain = dec.pic_output_tensor(pic, size=size, matrix=9, **roi_kw, **kw)

        def cm_call():
            dec.pic_output_scaled_cm(pic, size, colour, matrix=9, out=out, **roi_kw, **kw)

        def plain_call():
            dec.pic_output_tensor(pic, size=size, matrix=9, out=plain, **roi_kw, **kw)

        def resize(x):
            y = F.interpolate(x[None], size=size, mode="bilinear", antialias=True, align_corners=False)[0]
            return (y * 255.0).round().clamp(0, 255).to(torch.uint8) if is_u8 else (y - mean) * inv

        def torch_route():
            dec.pic_output_tensor(pic, out=full, dtype=torch.float32, matrix=9, colour=colour)
            if rois is None:
                return resize(full)
            return torch.stack([resize(full[:, y:y + rh, x:x + rw]) for x, y, rw, rh in rois])

        r = alternated(torch, s, {"cm": cm_call, "plain": plain_call}, a.iters)
        rt = alternated(torch, s, {"cm": cm_call, "torch_route": torch_route}, max(a.iters // 10, 5), warm=2)
        r["cm"]["device_us"], r["plain"]["device_us"] = round(timed(torch, s, cm_call, a.iters), 2), round(timed(torch, s, plain_call, a.iters), 2)      # the kernels alone
        r["torch_route"], r["cm_beside_torch_route"] = rt["torch_route"], rt["cm"]
        diff = float((torch_route().float() - out.float()).abs().max())
        r.update({"vs_plain": round(r["cm"]["us"] / r["plain"]["us"], 2), "speedup_vs_torch_route": round(rt["torch_route"]["us"] / rt["cm"]["us"], 2),
                  "max_abs_diff_vs_torch_route": diff, "diff_unit": "code values of the u8 output" if is_u8 else "normalised float"})
        print(f"scaled_cm {name:32s} {r['cm']['us']:9.1f} us (kernels {r['cm']['device_us']:7.1f})   plain call {r['plain']['us']:9.1f} us (kernels {r['plain']['device_us']:7.1f}; {r['vs_plain']:.2f}x)   torch route {rt['torch_route']['us']:10.1f} us "
              f"({r['speedup_vs_torch_route']:.1f}x)   max |diff| {diff:.3g}")
        res["scaled_cm"][name] = r
    del full


def resampled_leg(torch, dec, pic, s, a, res):
    """the bicubic call (Catmull-Rom, antialias) at three shapes, each alternated with (i) the plain bilinear scaled / ROI call of the same shape - the price of the
    wider window - and (ii) the route without it: the full-size f32 tensor + F.interpolate(mode="bicubic", antialias=True) + the normalise (or the u8 rounding)
    in torch, with the max |diff| between the two"""
    import torch.nn.functional as F
    from xevd_amd import abi
    w, h = a.width, a.height
    mean = torch.tensor(MEAN, device="cuda:0").view(3, 1, 1)
    inv = (1.0 / torch.tensor(STD, device="cuda:0")).view(3, 1, 1)
    full = dec.pic_output_tensor(pic, dtype=torch.float32)
    tiles = abi.tile_rois(w, h, (w // 8) & ~1, (h // 8) & ~1)[:64]
    norm = dict(mean=MEAN, std=STD)
    shapes = (("224x224_f32_normalised", (224, 224), None, dict(dtype=torch.float32, **norm)), ("1920x1080_u8", (1080, 1920), None, dict(dtype=torch.uint8)),
              ("64_rois_224x224_f32_normalised", (224, 224), tiles, dict(dtype=torch.float32, **norm)))
    res["resampled"] = {}
    for name, size, rois, kw in shapes:
        is_u8 = kw["dtype"] == torch.uint8
        roi_kw = {} if rois is None else dict(rois=rois)
        out = dec.pic_output_resampled(pic, size, **roi_kw, **kw)
        plain = dec.pic_output_tensor(pic, size=size, **roi_kw, **kw)

        def cubic_call():
            dec.pic_output_resampled(pic, size, out=out, **roi_kw, **kw)

        def plain_call():
            dec.pic_output_tensor(pic, size=size, out=plain, **roi_kw, **kw)

        def resize(x):
            y = F.interpolate(x[None], size=size, mode="bicubic", antialias=True, align_corners=False)[0]
            return (y * 255.0).round().clamp(0, 255).to(torch.uint8) if is_u8 else (y - mean) * inv

        def torch_route():
            dec.pic_output_tensor(pic, out=full, dtype=torch.float32)
            if rois is None:
                return resize(full)
            return torch.stack([resize(full[:, y:y + rh, x:x + rw]) for x, y, rw, rh in rois])

        r = alternated(torch, s, {"bicubic": cubic_call, "plain": plain_call}, a.iters)
        rt = alternated(torch, s, {"bicubic": cubic_call, "torch_route": torch_route}, max(a.iters // 10, 5), warm=2)
        r["bicubic"]["device_us"], r["plain"]["device_us"] = round(timed(torch, s, cubic_call, a.iters), 2), round(timed(torch, s, plain_call, a.iters), 2)      # the kernels alone
        r["torch_route"], r["bicubic_beside_torch_route"] = rt["torch_route"], rt["bicubic"]
        diff = float((torch_route().float() - out.float()).abs().max())
        r.update({"vs_plain": round(r["bicubic"]["us"] / r["plain"]["us"], 2), "speedup_vs_torch_route": round(rt["torch_route"]["us"] / rt["bicubic"]["us"], 2),
                  "max_abs_diff_vs_torch_route": diff, "diff_unit": "code values of the u8 output" if is_u8 else "normalised float"})
        print(f"resampled {name:32s} {r['bicubic']['us']:9.1f} us (kernels {r['bicubic']['device_us']:7.1f})   plain call {r['plain']['us']:9.1f} us (kernels {r['plain']['device_us']:7.1f}; {r['vs_plain']:.2f}x)   "
              f"torch route {rt['torch_route']['us']:10.1f} us ({r['speedup_vs_torch_route']:.1f}x)   max |diff| {diff:.3g}")
        res["resampled"][name] = r
    del full


def scaled_lin_leg(torch, dec, pic, s, a, res):
    """the scaled call filtered in linear light (PQ / BT.2020 -> sRGB through the tone curve) at the scaled_cm leg's three shapes, each alternated with (i) the
    scaled_cm call of the same shape - the price of filtering light instead of code values - and (ii) the only correct route without it: the full-size linear-light
    f32 tensor of the source primaries (400 MB at 8K) + F.interpolate(antialias=True) + matrix, clip, sRGB encode and the normalise (or the u8 rounding) in torch,
    the tone curve left out in the caller's favour.  That route's full-size call runs on a context of its own: a context keeps the tables of one transform, and
    two transforms taking turns on one context would make each call build its tables again.  The max |diff| against that route is taken from a call without
    the tone curve (linear_scale 100, as torch_transform scales), so that both sides compute the same thing; for the rectangles it includes their edges, where
    this call clamps the chroma upsampling to the rectangle and the full-size tensor does not."""
    import torch.nn.functional as F
    from xevd_amd import abi
    from xevd_amd.decoder import XgpuDecoder
    w, h = a.width, a.height
    colour = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
    no_tone = dict(colour, tone_map=False, linear_scale=100.0)
    to_linear = dict(src_primaries=9, src_transfer=16, dst_primaries=9, dst_transfer=8)
    mean = torch.tensor(MEAN, device="cuda:0").view(3, 1, 1)
    inv = (1.0 / torch.tensor(STD, device="cuda:0")).view(3, 1, 1)
    mat = torch.tensor([[1.660491, -0.587641, -0.072850], [-0.124550, 1.132900, -0.008349], [-0.018151, -0.100579, 1.118730]], device="cuda:0")
    dec2 = XgpuDecoder(w, h, a.bit_depth, device=0, max_pics=1)
    pic2 = dec2.pic_alloc()
    dec2.pic_upload(pic2, dec.pic_download(pic))
    full = dec2.pic_output_tensor(pic2, dtype=torch.float32, matrix=9, colour=to_linear)
    tiles = abi.tile_rois(w, h, (w // 8) & ~1, (h // 8) & ~1)[:64]
    norm = dict(mean=MEAN, std=STD)
    shapes = (("224x224_f32_normalised", (224, 224), None, dict(dtype=torch.float32, **norm)), ("1920x1080_u8", (1080, 1920), None, dict(dtype=torch.uint8)),
              ("64_rois_224x224_f32_normalised", (224, 224), tiles, dict(dtype=torch.float32, **norm)))
    res["scaled_lin"] = {}
    for name, size, rois, kw in shapes:
        is_u8 = kw["dtype"] == torch.uint8
        roi_kw = {} if rois is None else dict(rois=rois)
        out = dec.pic_output_scaled_cm(pic, size, colour, matrix=9, linear_light=True, **roi_kw, **kw)
        cm_out = dec.pic_output_scaled_cm(pic, size, colour, matrix=9, **roi_kw, **kw)

        def lin_call():
            dec.pic_output_scaled_cm(pic, size, colour, matrix=9, out=out, linear_light=True, **roi_kw, **kw)

        def cm_call():
            dec.pic_output_scaled_cm(pic, size, colour, matrix=9, out=cm_out, **roi_kw, **kw)

        def finish(x):
            y = F.interpolate(x[None], size=size, mode="bilinear", antialias=True, align_corners=False)[0]
            y = (torch.matmul(mat, y.reshape(3, -1)).reshape(y.shape) * 100.0).clamp(0, 1)
            y = torch.where(y < 0.0031308, 12.92 * y, 1.055 * y.pow(1.0 / 2.4) - 0.055)
            return (y * 255.0).round().clamp(0, 255).to(torch.uint8) if is_u8 else (y - mean) * inv

        def torch_route():
            dec2.pic_output_tensor(pic2, out=full, dtype=torch.float32, matrix=9, colour=to_linear)
            if rois is None:
                return finish(full)
            return torch.stack([finish(full[:, y:y + rh, x:x + rw]) for x, y, rw, rh in rois])

        r = alternated(torch, s, {"lin": lin_call, "cm": cm_call}, a.iters)
        rt = alternated(torch, s, {"lin": lin_call, "torch_route": torch_route}, max(a.iters // 10, 5), warm=2)
        r["lin"]["device_us"], r["cm"]["device_us"] = round(timed(torch, s, lin_call, a.iters), 2), round(timed(torch, s, cm_call, a.iters), 2)      # the kernels alone
        r["torch_route"], r["lin_beside_torch_route"] = rt["torch_route"], rt["lin"]
        same = dec.pic_output_scaled_cm(pic, size, no_tone, matrix=9, linear_light=True, **roi_kw, **kw)      # (after the timed loops: it changes the context's tables)
        diff = float((torch_route().float() - same.float()).abs().max())
        r.update({"vs_cm": round(r["lin"]["us"] / r["cm"]["us"], 2), "speedup_vs_torch_route": round(rt["torch_route"]["us"] / rt["lin"]["us"], 2),
                  "max_abs_diff_vs_torch_route": diff, "diff_unit": "code values of the u8 output" if is_u8 else "normalised float"})
        print(f"scaled_lin {name:32s} {r['lin']['us']:9.1f} us (kernels {r['lin']['device_us']:7.1f})   scaled_cm call {r['cm']['us']:9.1f} us (kernels {r['cm']['device_us']:7.1f}; {r['vs_cm']:.2f}x)   torch route {rt['torch_route']['us']:10.1f} us "
              f"({r['speedup_vs_torch_route']:.1f}x)   max |diff| {diff:.3g}")
        res["scaled_lin"][name] = r
    del full
    dec2.close()


def rois_leg(torch, dec, pic, s, a, res):
    """one batched call against the loop of single-image calls the same pictures cost without it, alternated"""
    import time
    from xevd_amd import abi
    w, h = a.width, a.height
    size, n, pad = (224, 224), 64, 0.447
    rng = np.random.default_rng(7)
    boxes = []
    for _ in range(n):
        bw, bh = (min(int(rng.integers(32, 257)) * 2, v) for v in (w, h))
        boxes.append((int(rng.integers(0, (w - bw) // 2 + 1)) * 2, int(rng.integers(0, (h - bh) // 2 + 1)) * 2, bw, bh))
    kw = dict(dtype=torch.float32, mean=MEAN, std=STD)
    res["rois"] = {}
    for name, rois, fit in (("tiles_stretch", abi.tile_rois(w, h, (w // 8) & ~1, (h // 8) & ~1)[:n], "stretch"), ("boxes_letterbox", boxes, "letterbox")):
        inner = [abi.roi_inner(dec.lib, r, size, abi.FIT_LETTERBOX if fit == "letterbox" else abi.FIT_STRETCH) for r in rois]
        out = dec.pic_output_tensor(pic, size=size, rois=rois, fit=fit, pad=pad, **kw)
        singles = [torch.empty((3, hi, wi), dtype=torch.float32, device="cuda:0") for _, _, wi, hi in inner]
        crops = [(x, w - x - rw, y, h - y - rh) for x, y, rw, rh in rois]

        def batched():
            dec.pic_output_tensor(pic, size=size, rois=rois, fit=fit, pad=pad, out=out, **kw)

        def loop():
            for t, c in zip(singles, crops):
                dec.pic_output_tensor(pic, size=tuple(t.shape[1:]), crop=c, out=t, **kw)

        for _ in range(5):
            batched(); loop()
        torch.cuda.synchronize()
        same = all(torch.equal(out[i][:, y:y + hi, x:x + wi], singles[i]) for i, (x, y, wi, hi) in enumerate(inner))
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)] for k in ("batched", "loop")}
        host = {"batched": [], "loop": []}
        for i in range(a.iters):
            for k, fn in (("batched", batched), ("loop", loop)):
                e0, e1 = ev[k][i]
                torch.cuda.synchronize()      # each route starts on an idle device: its events see its own gaps only
                t0 = time.perf_counter()
                e0.record(s)
                fn()
                e1.record(s)
                host[k].append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        r = {"n": len(rois), "size": list(size), "fit": fit, "inner_equal": bool(same)}
        for k in ("batched", "loop"):
            us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[k]])
            r[k] = {"us": round(float(np.median(us)), 2), "p10_us": round(float(np.percentile(us, 10)), 2), "p90_us": round(float(np.percentile(us, 90)), 2),
                    "host_us": round(float(np.median(host[k])), 2)}
        r["speedup"] = round(r["loop"]["us"] / r["batched"]["us"], 2)
        print(f"rois {name:16s} {len(rois)} x {size[1]}x{size[0]} f32: one call {r['batched']['us']:9.1f} us (host {r['batched']['host_us']:8.1f})   "
              f"loop of single calls {r['loop']['us']:9.1f} us (host {r['loop']['host_us']:8.1f})   {r['speedup']:.2f}x   inner parts equal: {same}")
        res["rois"][name] = r


def rois_dev_leg(torch, dec, pic, s, a, res):
    """boxes in device memory: read back and given to the host-box call (A) against the device-box call (B), alternated"""
    import time
    from xevd_amd import abi
    w, h = a.width, a.height
    size, n, pad = (224, 224), 64, 0.447
    rng = np.random.default_rng(7)      # the boxes of the rois leg
    boxes = []
    for _ in range(n):
        bw, bh = (min(int(rng.integers(32, 257)) * 2, v) for v in (w, h))
        boxes.append((int(rng.integers(0, (w - bw) // 2 + 1)) * 2, int(rng.integers(0, (h - bh) // 2 + 1)) * 2, bw, bh))
    kw = dict(dtype=torch.float32, mean=MEAN, std=STD)
    res["rois_dev"] = {}
    for name, rois, fit in (("tiles_stretch", abi.tile_rois(w, h, (w // 8) & ~1, (h // 8) & ~1)[:n], "stretch"), ("boxes_letterbox", boxes, "letterbox")):
        max_roi = (max(r[3] for r in rois), max(r[2] for r in rois))
        d_boxes = torch.tensor(rois, dtype=torch.int32, device="cuda:0")
        out_a = dec.pic_output_tensor(pic, size=size, rois=rois, fit=fit, pad=pad, **kw)
        out_b, results = dec.pic_output_tensor(pic, size=size, rois=d_boxes, fit=fit, pad=pad, max_roi=max_roi, results=True, **kw)

        def route_a():
            dec.pic_output_tensor(pic, size=size, rois=d_boxes.cpu().tolist(), fit=fit, pad=pad, out=out_a, **kw)

        def route_b():
            dec.pic_output_tensor(pic, size=size, rois=d_boxes, fit=fit, pad=pad, max_roi=max_roi, out=out_b, **kw)

        for _ in range(5):
            route_a(); route_b()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a, out_b)) and bool((results[:, 0] == abi.ROI_OK).all())
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)] for k in ("host_boxes", "device_boxes")}
        host = {"host_boxes": [], "device_boxes": []}
        for i in range(a.iters):
            for k, fn in (("host_boxes", route_a), ("device_boxes", route_b)):
                e0, e1 = ev[k][i]
                torch.cuda.synchronize()      # each route starts on an idle device: its events see its own gaps only
                t0 = time.perf_counter()
                e0.record(s)
                fn()
                e1.record(s)
                host[k].append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        r = {"n": len(rois), "size": list(size), "fit": fit, "max_roi": list(max_roi), "images_equal": same}
        for k in ("host_boxes", "device_boxes"):
            us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[k]])
            r[k] = {"us": round(float(np.median(us)), 2), "p10_us": round(float(np.percentile(us, 10)), 2), "p90_us": round(float(np.percentile(us, 90)), 2),
                    "host_us": round(float(np.median(host[k])), 2)}
        r["speedup"] = round(r["host_boxes"]["us"] / r["device_boxes"]["us"], 2)
        print(f"rois_dev {name:16s} {len(rois)} x {size[1]}x{size[0]} f32: boxes.cpu() + host-box call {r['host_boxes']['us']:9.1f} us (host {r['host_boxes']['host_us']:8.1f})   "
              f"device-box call {r['device_boxes']['us']:9.1f} us (host {r['device_boxes']['host_us']:8.1f})   {r['speedup']:.2f}x   images equal: {same}")
        res["rois_dev"][name] = r


def alternated(torch, s, routes, iters, warm=5):
    """routes {name: fn} run in turn, `iters` rounds, each from an idle device between two events on s -> {name: {us, p10_us, p90_us, host_us}}"""
    import time
    for _ in range(warm):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in routes}
    host = {k: [] for k in routes}
    for i in range(iters):
        for k, fn in routes.items():
            e0, e1 = ev[k][i]
            torch.cuda.synchronize()      # each route starts on an idle device: its events see its own gaps only
            t0 = time.perf_counter()
            e0.record(s)
            fn()
            e1.record(s)
            host[k].append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    r = {}
    for k in routes:
        us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[k]])
        r[k] = {"us": round(float(np.median(us)), 2), "p10_us": round(float(np.percentile(us, 10)), 2), "p90_us": round(float(np.percentile(us, 90)), 2),
                "host_us": round(float(np.median(host[k])), 2)}
    return r


def packed_leg(torch, dec, pic, s, a, res, copy_gbps):
    """every packed call alternated (i) with the nearest call that existed before it - the interleaved RGB tensor of its dtype, NV12, P010 - and (ii) with the torch
    route it replaces on top of that call; next to the times the bytes either side moves per pixel (3 read + what it writes) and whether the packed call takes
    more than that byte ratio of its counterpart's time beyond the spread of the run (its 10th percentile against the counterpart's 90th)"""
    w, h = a.width, a.height
    to_srgb = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)

    def rgba_route(kw, dt, one):      # cat with an alpha plane: a copy of the picture
        rgb = dec.pic_output_tensor(pic, channels_last=True, dtype=dt, **kw)
        return torch.cat([rgb, torch.full((h, w, 1), one, dtype=dt, device=rgb.device)], dim=-1)

    def rgb10_route():                # three shifts and two ors on an int32 tensor
        v = dec.pic_output_tensor(pic, channels_last=True, dtype=torch.int16).to(torch.int32)
        return v[..., 0] | (v[..., 1] << 10) | (v[..., 2] << 20) | (-1 << 30)      # (alpha 3: the two high bits)

    def yuyv_route(kw):               # a row repeat and a stack
        nv = dec.pic_output_tensor(pic, **kw)
        return torch.stack([nv[:h], nv[h:].repeat_interleave(2, 0)], dim=-1)

    u8, f16, i16 = torch.uint8, torch.float16, torch.int16
    p010 = dict(layout="p016", dtype=i16, out_bit_depth=10)
    cases = [("rgba_u8", dict(layout="rgba", dtype=u8), dict(channels_last=True, dtype=u8), lambda: rgba_route({}, u8, 255), 4, 3),
             ("rgba_f16", dict(layout="rgba", dtype=f16), dict(channels_last=True, dtype=f16), lambda: rgba_route({}, f16, 1.0), 8, 6),
             ("rgba_u8_cm_pq2020_srgb", dict(layout="rgba", dtype=u8, matrix=9, colour=to_srgb), dict(channels_last=True, dtype=u8, matrix=9, colour=to_srgb),
              lambda: rgba_route(dict(matrix=9, colour=to_srgb), u8, 255), 4, 3),
             ("rgb10a2", dict(layout="rgb10a2"), dict(channels_last=True, dtype=i16), rgb10_route, 4, 6),
             ("yuyv_u8", dict(layout="yuyv", dtype=u8), dict(layout="nv12", dtype=u8), lambda: yuyv_route(dict(layout="nv12", dtype=u8)), 2, 1.5),
             ("y210", dict(layout="yuyv", dtype=i16, out_bit_depth=10), p010, lambda: yuyv_route(p010), 4, 3)]
    res["packed"] = {"copy_gbps": copy_gbps, "cases": {}}
    for name, pkw, ckw, route, wp, wc in cases:
        out_p, out_c = dec.pic_output_packed(pic, **pkw), dec.pic_output_tensor(pic, **ckw)
        r = alternated(torch, s, {"packed": lambda: dec.pic_output_packed(pic, out=out_p, **pkw), "counterpart": lambda: dec.pic_output_tensor(pic, out=out_c, **ckw)},
                       a.iters)
        rt = alternated(torch, s, {"packed": lambda: dec.pic_output_packed(pic, out=out_p, **pkw), "torch_route": route}, max(a.iters // 10, 5), warm=2)
        r["torch_route"] = rt["torch_route"]
        r["packed_beside_torch_route"] = rt["packed"]
        nbytes = int(w * h * (3 + wp))
        r["packed"].update(bytes=nbytes, gbps=round(nbytes / (r["packed"]["us"] * 1e-6) / 1e9, 1))
        r["packed"]["frac_copy"] = round(r["packed"]["gbps"] / copy_gbps, 3)
        r["byte_ratio"] = round((3 + wp) / (3 + wc), 3)
        r["time_ratio"] = round(r["packed"]["us"] / r["counterpart"]["us"], 3)
        r["over_byte_ratio_beyond_spread"] = bool(r["packed"]["p10_us"] > r["byte_ratio"] * r["counterpart"]["p90_us"])
        r["torch_route_over_packed"] = round(rt["torch_route"]["us"] / rt["packed"]["us"], 2)
        same = route()
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[out_p.element_size()]
        ekw = dict(pkw, upsample="nearest") if pkw["layout"] == "yuyv" else pkw      # (the row repeat is NEAREST; the timed call is the default, LINEAR)
        r["torch_route_equals_kernel"] = bool(torch.equal(same.contiguous().view(it), dec.pic_output_packed(pic, **ekw).view(it)))
        res["packed"]["cases"][name] = r
        print(f"packed {name:24s} {r['packed']['us']:8.1f} us ({r['packed']['p10_us']:.1f} - {r['packed']['p90_us']:.1f})  {r['packed']['gbps']:7.1f} GB/s "
              f"{r['packed']['frac_copy']:.2f} of copy   counterpart {r['counterpart']['us']:8.1f} us ({r['counterpart']['p10_us']:.1f} - {r['counterpart']['p90_us']:.1f})  "
              f"time x{r['time_ratio']:.2f} for bytes x{r['byte_ratio']:.2f}{'  OVER' if r['over_byte_ratio_beyond_spread'] else ''}   "
              f"torch route {rt['torch_route']['us']:8.1f} us = x{r['torch_route_over_packed']:.1f}, equal {r['torch_route_equals_kernel']}")


def lut3d_leg(torch, dec, pic, s, a, res, copy_gbps, planes):
    """the 3D LUT calls at n = 17, 33, 65: U8 / U16 / F32 interleaved RGB, RGBA u8 and 10:10:10:2, each alternated in one loop with
    (i) the nearest call without a LUT and (ii) its colour-managed form (PQ / BT.2020 -> sRGB with the tone curve); then the F32 call against the torch route it
    replaces, the full-size f32 tensor + a 5-D grid_sample (trilinear).  On the picture of random samples of the other legs - the worst case for the gather -
    and on a smooth gradient, where neighbouring pixels share cells."""
    import torch.nn.functional as F
    from xevd_amd import abi
    w, h, bd = a.width, a.height, a.bit_depth
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    gradient = [(xx * top // (w - 1)).astype(np.int16), (cy * top // (h // 2 - 1)).astype(np.int16), ((cx + cy) * top // (w // 2 + h // 2 - 2)).astype(np.int16)]
    del yy, xx, cy, cx
    to_srgb = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
    u8, i16, f32 = torch.uint8, torch.int16, torch.float32
    forms = [("rgb_u8", dict(channels_last=True, dtype=u8), False, 3), ("rgb_u16", dict(channels_last=True, dtype=i16), False, 6),
             ("rgb_f32", dict(channels_last=True, dtype=f32), False, 12), ("rgba_u8", dict(layout="rgba", dtype=u8), True, 4), ("rgb10a2", dict(layout="rgb10a2"), True, 4)]
    res["lut3d"] = {"copy_gbps": copy_gbps, "random": {}, "gradient": {}}
    luts = {n: dec.lut3d_create(abi.lut3d_identity(dec.lib, n)) for n in (17, 33, 65)}
    for content, pl in (("random", planes), ("gradient", gradient)):
        dec.pic_upload(pic, pl)
        for (form, kw, is_packed, wbytes), n in itertools.product(forms, (17, 33, 65)):
            plain = dec.pic_output_packed if is_packed else dec.pic_output_tensor
            out_l, out_c, out_m = dec.pic_output_lut3d(pic, luts[n], matrix=9, **kw), plain(pic, matrix=9, **kw), plain(pic, matrix=9, colour=to_srgb, **kw)
            r = alternated(torch, s, {"lut3d": lambda: dec.pic_output_lut3d(pic, luts[n], matrix=9, out=out_l, **kw), "plain": lambda: plain(pic, matrix=9, out=out_c, **kw),
                                      "cm_pq2020_srgb": lambda: plain(pic, matrix=9, colour=to_srgb, out=out_m, **kw)}, a.iters)
            nbytes = int(w * h * (3 + wbytes))
            for k in r:
                r[k].update(gbps=round(nbytes / (r[k]["us"] * 1e-6) / 1e9, 1), frac_copy=round(nbytes / (r[k]["us"] * 1e-6) / 1e9 / copy_gbps, 3))
            r["bytes"] = nbytes
            res["lut3d"][content][f"{form}_n{n}"] = r
            print(f"lut3d {content:8s} {form:8s} n {n:2d}: " + "  ".join(f"{k} {v['us']:7.1f} us ({v['p10_us']:.1f} - {v['p90_us']:.1f})" for k, v in r.items() if isinstance(v, dict)))
            del out_l, out_c, out_m
        # the route a LUT user has without the call: the full-size f32 tensor, then a 5-D grid_sample over the cube (trilinear, float)
        full = dec.pic_output_tensor(pic, channels_last=True, dtype=f32, matrix=9)
        out = dec.pic_output_lut3d(pic, luts[17], channels_last=True, dtype=f32, matrix=9)
        for n in (17, 33, 65):
            vol = torch.from_numpy(abi.lut3d_identity(dec.lib, n).astype(np.float32) / 65535.0).to("cuda:0").reshape(n, n, n, 3).permute(3, 0, 1, 2)[None].contiguous()

            def route():
                dec.pic_output_tensor(pic, channels_last=True, dtype=f32, matrix=9, out=full)
                return F.grid_sample(vol, (full * 2.0 - 1.0)[None, None], mode="bilinear", padding_mode="border", align_corners=True)

            rt = alternated(torch, s, {"lut3d": lambda: dec.pic_output_lut3d(pic, luts[n], channels_last=True, dtype=f32, matrix=9, out=out), "torch_route": route},
                            max(a.iters // 10, 5), warm=2)
            diff = float((route()[0, :, 0].permute(1, 2, 0) - out).abs().max())
            rt["torch_route_over_lut3d"] = round(rt["torch_route"]["us"] / rt["lut3d"]["us"], 2)
            rt["max_abs_diff_vs_torch_route"] = diff
            res["lut3d"][content][f"torch_route_f32_n{n}"] = rt
            print(f"lut3d {content:8s} f32 n {n:2d}: call {rt['lut3d']['us']:8.1f} us   f32 tensor + grid_sample {rt['torch_route']['us']:9.1f} us = x{rt['torch_route_over_lut3d']:.1f}   "
                  f"max |diff| {diff:.2e}")
        del full, out
    for h_ in luts.values():
        dec.lut3d_destroy(h_)
    dec.pic_upload(pic, planes)      # (the leg uploads its contents into the slot)


def dither_leg(torch, dec, pic, s, a, res, copy_gbps):
    """the dithered calls beside the plain calls of the same layout, and the torch route they replace"""
    from xevd_amd.decoder import XgpuDecoder
    w, h = a.width, a.height
    to_srgb = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
    u8 = torch.uint8
    res["dither"] = {"copy_gbps": copy_gbps, "cases": {}}

    def run(name, d, p, plain, kw, mats, wbytes, phase=(5, 3)):
        hs = {m: d.dither_create(*args) for m, args in mats.items()}
        routes = {"plain": (lambda o=plain(p, **kw): plain(p, out=o, **kw))}
        for m, hd in hs.items():
            routes[m] = (lambda hd=hd, o=d.pic_output_dithered(p, hd, phase=phase, **kw): d.pic_output_dithered(p, hd, phase=phase, out=o, **kw))
        r = alternated(torch, s, routes, a.iters)
        nbytes = int(w * h * (3 + wbytes))
        for k in routes:
            r[k].update(gbps=round(nbytes / (r[k]["us"] * 1e-6) / 1e9, 1), frac_copy=round(nbytes / (r[k]["us"] * 1e-6) / 1e9 / copy_gbps, 3))
        for m in hs:
            r[m]["time_ratio"] = round(r[m]["us"] / r["plain"]["us"], 3)
            r[m]["above_plain_p90"] = bool(r[m]["us"] > r["plain"]["p90_us"])
            d.dither_destroy(hs[m])
        r["bytes"] = nbytes
        res["dither"]["cases"][name] = r
        print(f"dither {name:24s} " + "  ".join(f"{k} {v['us']:7.1f} us ({v['p10_us']:.1f} - {v['p90_us']:.1f})" for k, v in r.items() if isinstance(v, dict)))

    blue64 = {"blue64": ("blue", 64)}
    run("rgb_u8", dec, pic, dec.pic_output_tensor, dict(layout="rgb", channels_last=True, dtype=u8), {"bayer8": ("bayer", 8), "blue64": ("blue", 64), "blue128": ("blue", 128)}, 3)
    run("rgba_u8_cm_pq2020_srgb", dec, pic, dec.pic_output_packed, dict(layout="rgba", dtype=u8, matrix=9, colour=to_srgb), blue64, 4)
    run("nv12_u8", dec, pic, dec.pic_output_tensor, dict(layout="nv12", dtype=u8), blue64, 1.5)
    rng = np.random.default_rng(12)
    with XgpuDecoder(w, h, 12, device=0, max_pics=2) as d12:
        p12 = d12.pic_alloc()
        d12.pic_upload(p12, [rng.integers(0, 1 << 12, sh).astype(np.int16) for sh in ((h, w), (h // 2, w // 2), (h // 2, w // 2))])
        run("rgb10a2_from_12_bit", d12, p12, d12.pic_output_packed, dict(layout="rgb10a2"), blue64, 4)
    # the route a user has without the call: the f32 tensor (400 MB at 8K), a tiled threshold tensor, floor, clamp, to(uint8)
    hd = dec.dither_create("blue", 64)
    from xevd_amd import abi
    m = torch.from_numpy(abi.dither_blue(dec.lib, 6, 1).astype(np.float32) / 4096.0).to("cuda:0")
    thr = m.repeat((h + 63) // 64, (w + 63) // 64)[:h, :w, None].contiguous()
    full = dec.pic_output_tensor(pic, channels_last=True, dtype=torch.float32)
    out = dec.pic_output_dithered(pic, hd, "rgb", channels_last=True)

    def route():
        dec.pic_output_tensor(pic, channels_last=True, dtype=torch.float32, out=full)
        return (full * 255.0 + thr).floor_().clamp_(0.0, 255.0).to(u8)

    rt = alternated(torch, s, {"dithered": lambda: dec.pic_output_dithered(pic, hd, "rgb", channels_last=True, out=out), "torch_route": route}, max(a.iters // 10, 5), warm=2)
    rt["torch_route_over_dithered"] = round(rt["torch_route"]["us"] / rt["dithered"]["us"], 2)
    rt["max_abs_diff_vs_torch_route"] = int((route().to(torch.int16) - out.to(torch.int16)).abs().max())      # (the float matrix is not the integer one: a record)
    res["dither"]["torch_route_rgb_u8_blue64"] = rt
    print(f"dither rgb_u8 blue64: call {rt['dithered']['us']:8.1f} us   f32 tensor + threshold, floor, clamp, to(uint8) {rt['torch_route']['us']:9.1f} us = "
          f"x{rt['torch_route_over_dithered']:.1f}   max |diff| {rt['max_abs_diff_vs_torch_route']}")
    dec.dither_destroy(hd)


def overlay_leg(torch, dec, pic, s, a, res, copy_gbps):
    """the overlaid calls beside the plain calls of the same layout in the same run - no layer, a logo, a full-size subtitle plane,
    16 / 64 / 256 boxes from device memory - and the torch routes they replace"""
    w, h = a.width, a.height
    to_srgb = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)
    u8 = torch.uint8
    rng = np.random.default_rng(31)
    logo = torch.from_numpy(rng.integers(0, 256, (min(256, h), min(512, w), 4)).astype(np.uint8)).to("cuda:0")
    plane = np.zeros((h, w, 4), np.uint8)      # subtitles: 95 % of the plane transparent, two opaque-ish bands of text-like coverage near the bottom
    band = slice(h - h // 20, h)
    plane[band, :, :3] = 255
    plane[band, :, 3] = rng.integers(0, 256, (h // 20, w)).astype(np.uint8)
    plane = torch.from_numpy(plane).to("cuda:0")
    res["overlay"] = {"copy_gbps": copy_gbps, "cases": {}}
    sets = {"none": dict(layers=[]), "logo_512x256": dict(layers=[dict(image=logo, x=w - logo.shape[1] - 64, y=64)]),
            "subtitle_plane_bgra": dict(layers=[dict(image=plane, order="bgra")])}
    pal = [(255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255), (255, 255, 0, 255)]
    box_arrays = {}
    for n in (16, 64, 256):
        bx = np.stack([rng.integers(0, w - 64, n), rng.integers(0, h - 64, n), rng.integers(32, max(w // 8, 64), n), rng.integers(32, max(h // 8, 64), n)], axis=1).astype(np.int32)
        box_arrays[n] = torch.from_numpy(bx).to("cuda:0")
        sets[f"boxes_{n}"] = dict(boxes=dict(tensor=box_arrays[n], count=torch.tensor([n], dtype=torch.int32, device="cuda:0"),
                                             labels=torch.from_numpy(rng.integers(0, 4, n).astype(np.int32)).to("cuda:0"), palette=pal, thickness=4, fill_alpha=0))

    def run(name, plain, kw, wbytes):
        routes = {"plain": (lambda o=plain(pic, **kw): plain(pic, out=o, **kw))}
        for k, ov in sets.items():
            routes[k] = (lambda ov=ov, o=dec.pic_output_overlaid(pic, **ov, **kw): dec.pic_output_overlaid(pic, out=o, **ov, **kw))
        r = alternated(torch, s, routes, a.iters)
        nbytes = int(w * h * (3 + wbytes))
        for k in routes:
            r[k].update(gbps=round(nbytes / (r[k]["us"] * 1e-6) / 1e9, 1))
        for k in sets:
            r[k]["time_ratio"] = round(r[k]["us"] / r["plain"]["us"], 3)
            r[k]["above_plain_p90"] = bool(r[k]["us"] > r["plain"]["p90_us"])
        r["bytes"] = nbytes
        res["overlay"]["cases"][name] = r
        print(f"overlay {name:24s} " + "  ".join(f"{k} {v['us']:7.1f} us ({v['p10_us']:.1f} - {v['p90_us']:.1f})" for k, v in r.items() if isinstance(v, dict)))

    run("rgb_u8", dec.pic_output_tensor, dict(layout="rgb", channels_last=True, dtype=u8), 3)
    run("rgba_u8", dec.pic_output_packed, dict(layout="rgba", dtype=u8), 4)
    run("rgba_u8_cm_pq2020_srgb", dec.pic_output_packed, dict(layout="rgba", dtype=u8, matrix=9, colour=to_srgb), 4)
    run("nv12_u8", dec.pic_output_tensor, dict(layout="nv12", dtype=u8), 1.5)
    run("p010", dec.pic_output_tensor, dict(layout="p016", dtype=torch.int16, out_bit_depth=10), 3)

    # the routes a user has without the calls, on the interleaved RGB u8 tensor: slice and blend in float (logo, subtitle plane); boxes.cpu() and a loop of slices
    out = dec.pic_output_tensor(pic, layout="rgb", channels_last=True, dtype=u8)
    kw = dict(layout="rgb", channels_last=True, dtype=u8)

    def blend(img, x, y):
        hh, ww = img.shape[:2]
        dst = out[y:y + hh, x:x + ww].to(torch.float32)
        al = img[..., 3:4].to(torch.float32) / 255.0
        out[y:y + hh, x:x + ww] = (dst * (1.0 - al) + img[..., :3].to(torch.float32) * al + 0.5).to(u8)

    def torch_logo():
        dec.pic_output_tensor(pic, out=out, **kw)
        blend(logo, w - logo.shape[1] - 64, 64)

    plane_rgba = plane[..., (2, 1, 0, 3)].contiguous()

    def torch_plane():
        dec.pic_output_tensor(pic, out=out, **kw)
        blend(plane_rgba, 0, 0)

    def torch_boxes(n):
        dec.pic_output_tensor(pic, out=out, **kw)
        col = torch.tensor(pal, dtype=u8, device="cuda:0")[:, :3]
        for i, (x, y, bw, bh) in enumerate(box_arrays[n].cpu().tolist()):      # the round trip the device-box call avoids
            x1, y1, c = min(x + bw, w), min(y + bh, h), col[i & 3]
            out[y:y + 4, x:x1] = c; out[max(y1 - 4, y):y1, x:x1] = c; out[y:y1, x:x + 4] = c; out[y:y1, max(x1 - 4, x):x1] = c

    o2 = dec.pic_output_overlaid(pic, **kw)
    routes = {"call_logo": lambda: dec.pic_output_overlaid(pic, out=o2, **sets["logo_512x256"], **kw), "torch_logo": torch_logo,
              "call_plane": lambda: dec.pic_output_overlaid(pic, out=o2, **sets["subtitle_plane_bgra"], **kw), "torch_plane": torch_plane}
    for n in (16, 64, 256):
        routes[f"call_boxes_{n}"] = lambda n=n: dec.pic_output_overlaid(pic, out=o2, **sets[f"boxes_{n}"], **kw)
        routes[f"torch_boxes_{n}"] = lambda n=n: torch_boxes(n)
    rt = alternated(torch, s, routes, max(a.iters // 10, 5), warm=2)
    res["overlay"]["torch_routes_rgb_u8"] = rt
    print("overlay torch routes: " + "  ".join(f"{k} {v['us']:.1f} us (host {v['host_us']:.1f})" for k, v in rt.items()))


def ladder_leg(torch, dec, pic, s, a, res):
    """the picture to P010 rungs 3840x2160, 1920x1080, 1280x720 and 640x360 (those inside the scaled output's limits for the picture): the one call
    (pic_output_surfaces) against four one-rung calls, against the route without it - the full-size P010 surface, then per rung and plane
    torch.nn.functional.interpolate(antialias=True), rounding and repacking in torch - and against the plain full-size surface as the floor, alternated.  Centre
    siting (chroma_loc 1) on both sides, where a chroma plane is a plain plane resize, so that both routes compute the same picture; the largest difference between
    them is reported in code values, the torch route in float64."""
    import torch.nn.functional as F
    w, h, bd = a.width, a.height, a.bit_depth
    sizes = [(hh, ww) for hh, ww in ((2160, 3840), (1080, 1920), (720, 1280), (360, 640)) if h <= 64 * hh <= 512 * h and w <= 64 * ww <= 512 * w]
    kw = dict(layout="p016", dtype=torch.int16, out_bit_depth=10, chroma_loc=1)
    full_kw = dict(layout="p016", dtype=torch.int16, out_bit_depth=10)
    outs = dec.pic_output_surfaces(pic, sizes, **kw)
    singles = [dec.pic_output_surfaces(pic, [sz], **kw) for sz in sizes]
    full = dec.pic_output_tensor(pic, **full_kw)

    def planes_of(surface, hh, ww, ft):      # a P010 surface -> Y [1, 1, H, W] and Cb Cr [1, 2, H / 2, W / 2] as code values
        v = ((surface.to(torch.int32) & 0xFFFF) >> 6).to(ft)
        return v[:hh].view(1, 1, hh, ww), v[hh:].view(1, hh // 2, ww // 2, 2).permute(0, 3, 1, 2)

    def torch_route(ft=torch.float32, pack=True):
        dec.pic_output_tensor(pic, out=full, **full_kw)
        y, c = planes_of(full, h, w, ft)
        made = []
        for hh, ww in sizes:
            ys = F.interpolate(y, size=(hh, ww), mode="bilinear", antialias=True, align_corners=False)
            cs = F.interpolate(c, size=(hh // 2, ww // 2), mode="bilinear", antialias=True, align_corners=False)
            if not pack:
                made.append((ys, cs))
                continue
            o = torch.empty((hh * 3 // 2, ww), dtype=torch.int16, device=full.device)
            o[:hh] = (ys[0, 0].round().clamp(0, 1023).to(torch.int32) << 6).to(torch.int16)
            o[hh:] = (cs[0].permute(1, 2, 0).reshape(hh // 2, ww).round().clamp(0, 1023).to(torch.int32) << 6).to(torch.int16)
            made.append(o)
        return made

    def four_calls():
        for sz, o in zip(sizes, singles):
            dec.pic_output_surfaces(pic, [sz], out=o, **kw)

    routes = {"torch_route": torch_route, "ladder_one_call": lambda: dec.pic_output_surfaces(pic, sizes, out=outs, **kw),
              "full_size_surface": lambda: dec.pic_output_tensor(pic, out=full, **full_kw)}
    r = {"sizes": [[ww, hh] for hh, ww in sizes], "layout": "p010", "chroma_loc": 1, **alternated(torch, s, routes, a.iters)}
    # on their own: the context keeps the tap tables of one key, so each of the four calls makes its tables again - a cost of that route, not of the one call
    r.update(alternated(torch, s, {"ladder_four_calls": four_calls}, a.iters))
    # the kernels alone: the median of --iters calls queued behind a wait, as the full-size forms are timed
    r["ladder_one_call"]["device_us"] = round(timed(torch, s, routes["ladder_one_call"], a.iters), 2)
    r["ladder_four_calls"]["device_us"] = round(timed(torch, s, four_calls, a.iters), 2)
    r["full_size_surface"]["device_us"] = round(timed(torch, s, routes["full_size_surface"], a.iters), 2)
    read = int(w * h * 3)                                              # the 16-bit picture once
    written = sum(hh * ww * 3 for hh, ww in sizes)                     # 16-bit surfaces
    r["bytes_picture"], r["bytes_rungs"], r["bytes_intermediate"] = read, written, sum(2 * (hh * w + 2 * (hh // 2) * (w // 2)) for hh, ww in sizes)
    r["speedup_over_torch_route"] = round(r["torch_route"]["us"] / r["ladder_one_call"]["us"], 2)
    r["four_calls_over_one_call"] = round(r["ladder_four_calls"]["us"] / r["ladder_one_call"]["us"], 2)
    r["one_call_over_full_size_surface"] = round(r["ladder_one_call"]["us"] / r["full_size_surface"]["us"], 2)
    # the minimum traffic of the call as it is built - every rung reads the picture, writes and reads its intermediate, writes its surface - at the copy rate
    traffic = len(sizes) * read + 2 * r["bytes_intermediate"] + written
    r["bytes_moved_as_built"] = traffic
    if res.get("copy_gbps"):
        r["copy_rate_time_as_built_us"] = round(traffic / (res["copy_gbps"] * 1e9) * 1e6, 1)
    diffs = []
    for (ys, cs), o, (hh, ww) in zip(torch_route(torch.float64, pack=False), outs, sizes):
        yo, co = planes_of(o, hh, ww, torch.float64)
        diffs.append({"size": [ww, hh], "luma": round(float((ys - yo).abs().max()), 4), "chroma": round(float((cs - co).abs().max()), 4)})
    r["max_abs_diff_codes_vs_torch_f64"] = diffs
    print(f"ladder {len(sizes)} P010 rungs: torch route {r['torch_route']['us']:9.1f} us   one call {r['ladder_one_call']['us']:9.1f} us ({r['speedup_over_torch_route']:.2f}x)   "
          f"four calls {r['ladder_four_calls']['us']:9.1f} us   kernels alone {r['ladder_one_call']['device_us']:8.1f} us   full-size surface {r['full_size_surface']['us']:8.1f} us   max |diff| "
          + ", ".join(f"{d['size'][0]}x{d['size'][1]}: {d['luma']:.3f} / {d['chroma']:.3f}" for d in diffs))
    res["ladder"] = r


def warp_leg(torch, dec, pic, s, a, res):
    """64 rotated boxes -> 224x224 f32 planar, normalised: the full-size f32 tensor + affine_grid + grid_sample + normalise in torch (A) against the one call at
    S = 1 and S = 4 (B), alternated; and the same boxes upright against rois= with the stretch fit - what gathering costs over the two separable passes"""
    import math
    import torch.nn.functional as F
    from xevd_amd import abi
    w, h = a.width, a.height
    size, n = (224, 224), 64
    hd, wd = size
    rng = np.random.default_rng(7)      # the boxes of the rois leg ...
    boxes = []
    for _ in range(n):
        bw, bh = (min(int(rng.integers(32, 257)) * 2, v) for v in (w, h))
        boxes.append((int(rng.integers(0, (w - bw) // 2 + 1)) * 2, int(rng.integers(0, (h - bh) // 2 + 1)) * 2, bw, bh))
    angles = np.random.default_rng(11).uniform(-180.0, 180.0, n)      # ... each with a seeded angle

    def thetas(angs):
        out = []
        for (x, y, bw, bh), ang in zip(boxes, angs):
            c, sn = math.cos(ang * (math.pi / 180.0)), math.sin(ang * (math.pi / 180.0))
            cx, cy = x + bw / 2, y + bh / 2
            out.append([bw * c / wd, -bh * sn / hd, cx - (bw * c - bh * sn) / 2, bw * sn / wd, bh * c / hd, cy - (bw * sn + bh * c) / 2])
        return out

    def grid_theta(ths):      # destination pixel centres -> source coordinates, as affine_grid's normalised matrix (align_corners=False)
        g = [[[t[0] * wd / w, t[1] * hd / w, 2 * (t[0] * wd / 2 + t[1] * hd / 2 + t[2]) / w - 1],
              [t[3] * wd / h, t[4] * hd / h, 2 * (t[3] * wd / 2 + t[4] * hd / 2 + t[5]) / h - 1]] for t in ths]
        return torch.tensor(g, dtype=torch.float32, device="cuda:0")

    kw = dict(dtype=torch.float32, mean=MEAN, std=STD)
    mean = torch.tensor(MEAN, device="cuda:0").view(1, 3, 1, 1)
    inv = (1.0 / torch.tensor(STD, device="cuda:0")).view(1, 3, 1, 1)
    full = dec.pic_output_tensor(pic, dtype=torch.float32)
    ths = thetas(angles)
    maps = np.asarray([abi.warp_from_matrix(dec.lib, t) for t in ths], np.int64)
    gt = grid_theta(ths)
    outs = {sm: dec.pic_output_warped(pic, maps, size, samples=sm, **kw) for sm in (1, 4)}

    def route_a():
        dec.pic_output_tensor(pic, out=full, dtype=torch.float32)
        grid = F.affine_grid(gt, (n, 3, hd, wd), align_corners=False)
        return (F.grid_sample(full[None].expand(n, -1, -1, -1), grid, mode="bilinear", padding_mode="border", align_corners=False) - mean) * inv

    routes = {"torch_route": route_a, "warp_s1": lambda: dec.pic_output_warped(pic, maps, size, samples=1, out=outs[1], **kw),
              "warp_s4": lambda: dec.pic_output_warped(pic, maps, size, samples=4, out=outs[4], **kw)}
    r = {"n": n, "size": list(size), "rotated": alternated(torch, s, routes, a.iters)}
    r["rotated"]["max_abs_diff_s1_vs_torch_route"] = float((route_a() - outs[1]).abs().max())
    r["rotated"]["speedup_s1"] = round(r["rotated"]["torch_route"]["us"] / r["rotated"]["warp_s1"]["us"], 2)
    r["rotated"]["speedup_s4"] = round(r["rotated"]["torch_route"]["us"] / r["rotated"]["warp_s4"]["us"], 2)
    del full
    # the same boxes upright: the gather against the two separable passes of rois= (stretch); the results differ where a box is reduced (no antialiasing at S = 1)
    up = np.asarray([abi.warp_from_matrix(dec.lib, t) for t in thetas(np.zeros(n))], np.int64)
    out_w = dec.pic_output_warped(pic, up, size, **kw)
    out_r = dec.pic_output_tensor(pic, size=size, rois=boxes, **kw)
    routes = {"rois_stretch": lambda: dec.pic_output_tensor(pic, size=size, rois=boxes, out=out_r, **kw),
              "warp_s1": lambda: dec.pic_output_warped(pic, up, size, samples=1, out=out_w, **kw)}
    r["upright"] = alternated(torch, s, routes, a.iters)
    r["upright"]["warp_over_rois"] = round(r["upright"]["warp_s1"]["us"] / r["upright"]["rois_stretch"]["us"], 2)
    ro, up_ = r["rotated"], r["upright"]
    print(f"warp rotated {n} x {wd}x{hd} f32: torch route {ro['torch_route']['us']:9.1f} us (host {ro['torch_route']['host_us']:8.1f})   one call S=1 {ro['warp_s1']['us']:8.1f} us "
          f"({ro['speedup_s1']:.1f}x)   S=4 {ro['warp_s4']['us']:8.1f} us ({ro['speedup_s4']:.1f}x)   max |diff| S=1 {ro['max_abs_diff_s1_vs_torch_route']:.2e}")
    print(f"warp upright {n} x {wd}x{hd} f32: rois stretch {up_['rois_stretch']['us']:8.1f} us   warp S=1 {up_['warp_s1']['us']:8.1f} us   ({up_['warp_over_rois']:.2f} of rois)")
    res["warp"] = r


def remap_leg(torch, dec, pic, s, a, res):
    """lens undistortion of the whole picture at step 0 and step 4, the identity mesh beside the plain output, four fisheye views at S = 4 - each alternated with the
    full-size f32 tensor + grid_sample in torch"""
    import torch.nn.functional as F
    from xevd_amd import abi
    w, h = a.width, a.height
    dev = "cuda:0"
    kw = dict(dtype=torch.uint8)
    full = dec.pic_output_tensor(pic, dtype=torch.float32)

    def norm_grid(q16):      # Q16 positions [.., 2] -> grid_sample's normalised coordinates (align_corners=False: sample i's centre at (2 i + 1) / n - 1)
        g = torch.from_numpy(q16.astype(np.float32) / np.float32(65536.0)).to(dev)
        return torch.stack([(2 * g[..., 0] + 1) / w - 1, (2 * g[..., 1] + 1) / h - 1], dim=-1)

    def torch_route(ngrid):
        dec.pic_output_tensor(pic, out=full, dtype=torch.float32)
        return F.grid_sample(full[None].expand(ngrid.shape[0], -1, -1, -1), ngrid, mode="bilinear", padding_mode="border", align_corners=False)

    def diff_codes(out_u8, ngrid):      # in code values of the u8 output, image by image (the f32 batch of all views at once is large)
        return max(float((torch_route(ngrid[i:i + 1])[0] * 255.0 - out_u8[i].float()).abs().max()) for i in range(ngrid.shape[0]))

    r = {}
    # ---- the whole picture through a lens, at its own size
    lens = dict(fx=0.8 * w, fy=0.8 * w, cx=w / 2 - 3.3, cy=h / 2 + 2.1, k1=-0.22, k2=0.06, p1=0.0008, p2=-0.0005, k3=-0.008, nfx=0.72 * w, nfy=0.72 * w, ncx=(w - 1) / 2,
                ncy=(h - 1) / 2)
    g0, g4 = (torch.from_numpy(abi.remap_from_lens(dec.lib, lens, (h, w), k)).to(dev) for k in (0, 4))
    ng = norm_grid(abi.remap_from_lens(dec.lib, lens, (h, w), 0))[None]
    outs = {k: dec.pic_output_remapped(pic, g, (h, w), step=k, **kw) for k, g in ((0, g0), (4, g4))}
    routes = {"torch_route": lambda: torch_route(ng), "remap_step0": lambda: dec.pic_output_remapped(pic, g0, (h, w), step=0, out=outs[0], **kw),
              "remap_step4": lambda: dec.pic_output_remapped(pic, g4, (h, w), step=4, out=outs[4], **kw)}
    r["lens_full_size_u8"] = alternated(torch, s, routes, a.iters)
    e = r["lens_full_size_u8"]
    e["grid_bytes"] = {"step0": int(g0.numel() * 4), "step4": int(g4.numel() * 4)}
    e["max_abs_diff_codes_step0_vs_torch_route"] = diff_codes(outs[0], ng)
    e["max_abs_diff_codes_step4_vs_step0"] = int((outs[4].int() - outs[0].int()).abs().max())
    for k in (0, 4):
        e[f"speedup_step{k}"] = round(e["torch_route"]["us"] / e[f"remap_step{k}"]["us"], 2)
    print(f"remap lens {w}x{h} u8: torch route {e['torch_route']['us']:9.1f} us   step 0 {e['remap_step0']['us']:9.1f} us ({e['speedup_step0']:.1f}x)   "
          f"step 4 {e['remap_step4']['us']:9.1f} us ({e['speedup_step4']:.1f}x)   max |diff| step 0 {e['max_abs_diff_codes_step0_vs_torch_route']:.2f} codes")
    del g0, ng
    # ---- the identity mesh beside the plain output of the same form: the floor
    gi = torch.from_numpy(abi.remap_from_warp(dec.lib, (65536, 0, 0, 0, 65536, 0), (h, w), 4)).to(dev)
    plain = dec.pic_output_tensor(pic, upsample="linear", **kw)
    routes = {"plain_output": lambda: dec.pic_output_tensor(pic, upsample="linear", out=plain, **kw),
              "remap_identity_step4": lambda: dec.pic_output_remapped(pic, gi, (h, w), step=4, out=outs[4], **kw)}
    r["identity_step4_vs_plain"] = alternated(torch, s, routes, a.iters)
    e = r["identity_step4_vs_plain"]
    e["equal"] = bool(torch.equal(outs[4][0], plain))
    e["remap_over_plain"] = round(e["remap_identity_step4"]["us"] / e["plain_output"]["us"], 2)
    print(f"remap identity step 4 {e['remap_identity_step4']['us']:9.1f} us   plain output {e['plain_output']['us']:9.1f} us   ({e['remap_over_plain']:.2f} of plain, equal: {e['equal']})")
    del outs, plain, gi, g4
    # ---- four virtual views of an equidistant fisheye (r = f theta), 1920 x 1080, S = 4, a float32 mesh at step 4
    vh, vw, k, n = 1080, 1920, 4, 4
    f_fish, f_view = min(w, h) / np.pi, 0.9 * vw      # a 180-degree circle inscribed in the picture; each view about 94 degrees wide

    def fisheye(ox, oy, yaw, pitch):
        x, y, z = (ox - (vw - 1) / 2) / f_view, (oy - (vh - 1) / 2) / f_view, np.ones_like(ox, dtype=np.float64)
        cy_, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        y, z = y * cp - z * sp, y * sp + z * cp
        x, z = x * cy_ + z * sy_, -x * sy_ + z * cy_
        rho = np.hypot(x, y)
        rad = f_fish * np.arctan2(rho, z) / np.maximum(rho, 1e-12)
        return np.stack([x * rad + (w - 1) / 2, y * rad + (h - 1) / 2], axis=-1)

    views = [(-0.7, -0.3), (0.7, -0.3), (-0.7, 0.3), (0.7, 0.3)]
    gh, gw = abi.remap_grid_dims(dec.lib, (vh, vw), k)
    nx, ny = np.meshgrid(np.arange(gw, dtype=np.float64) * (1 << k), np.arange(gh, dtype=np.float64) * (1 << k))
    mesh = torch.from_numpy(np.stack([fisheye(nx, ny, *v) for v in views]).astype(np.float32)).to(dev)
    px, py = np.meshgrid(np.arange(vw, dtype=np.float64), np.arange(vh, dtype=np.float64))
    dense = np.stack([fisheye(px, py, *v) for v in views])
    ngv = norm_grid(np.rint(dense * 65536.0))
    out_v = dec.pic_output_remapped(pic, mesh, (vh, vw), step=k, samples=4, **kw)
    out_1 = dec.pic_output_remapped(pic, mesh, (vh, vw), step=k, samples=1, **kw)
    routes = {"torch_route": lambda: torch_route(ngv), "remap_s4": lambda: dec.pic_output_remapped(pic, mesh, (vh, vw), step=k, samples=4, out=out_v, **kw),
              "remap_s1": lambda: dec.pic_output_remapped(pic, mesh, (vh, vw), step=k, samples=1, out=out_1, **kw)}
    r["fisheye_4_views_1080p_u8"] = alternated(torch, s, routes, a.iters)
    e = r["fisheye_4_views_1080p_u8"]
    e["max_abs_diff_codes_s1_vs_torch_route"] = diff_codes(out_1, ngv)
    e["max_abs_diff_codes_s4_vs_torch_route"] = diff_codes(out_v, ngv)
    e["speedup_s4"] = round(e["torch_route"]["us"] / e["remap_s4"]["us"], 2)
    e["speedup_s1"] = round(e["torch_route"]["us"] / e["remap_s1"]["us"], 2)
    print(f"remap fisheye {n} x {vw}x{vh} u8 step {k}: torch route {e['torch_route']['us']:9.1f} us   S=4 {e['remap_s4']['us']:9.1f} us ({e['speedup_s4']:.2f}x)   "
          f"S=1 {e['remap_s1']['us']:9.1f} us ({e['speedup_s1']:.2f}x)   max |diff| S=1 {e['max_abs_diff_codes_s1_vs_torch_route']:.2f} codes")
    res["remap"] = r


def residual_leg(torch, dec, pic, s, a, res):
    """the four residual forms on a decoded synthetic batch, --repeat runs, each with the copy rate measured next to it"""
    from xevd_amd import synth
    w, h, bd = a.width, a.height, a.bit_depth
    batch = synth.gen_frame(np.random.default_rng(1), w, h, bd, inter_frac=0.9, bi_frac=0.5, coded_frac=0.6, n_refs=(1, 1), qp_range=(22, 37), mv_sigma_px=8.0, oob_frac=0.05)
    area = (1 << batch["log2w"].astype(np.int64)) << batch["log2h"].astype(np.int64)
    cbf = batch["cbf"].astype(np.int64)
    coded = int((area * (cbf & 1) + (area // 4) * ((cbf >> 1) & 1) + (area // 4) * ((cbf >> 2) & 1)).sum()) * 2      # (no ATS-inter in this batch: whole-CU blocks)
    n_units, n_cu = (w // 4) * (h // 4), len(cbf)
    read = coded + 4 * n_units + 32 * n_cu
    cur = dec.pic_alloc()
    hb = dec.batch_create(batch)
    dec.decode_picture(cur, 8, {(0, 0): (pic, 4), (0, 1): (pic, 16)}, hb, deblock=True)
    dec.sync()
    forms = [("resid_yuv420_s16", dict(kind="yuv420"), 3 * w * h),
             ("resid_444_s16_planar", dict(kind="444", dtype=torch.int16), 6 * w * h),
             ("resid_444_f16_planar", dict(kind="444", dtype=torch.float16), 6 * w * h),
             ("resid_energy", dict(kind="energy"), 12 * n_units)]
    res["residual"] = {"n_cu": n_cu, "coded_arena_bytes": coded, "owner_bytes": 4 * n_units, "record_bytes": 32 * n_cu, "runs": []}
    for rep in range(a.repeat):
        copy_gbps = dec.measure_copy_bw(1 << 30, 20)
        run = {"copy_gbps": copy_gbps, "forms": {}}
        for name, kw, wbytes in forms:
            out = dec.batch_residual(hb, **kw)
            out = out[0] if isinstance(out, tuple) else out
            us = timed(torch, s, lambda: dec.batch_residual(hb, out=out, **kw), a.iters)
            nbytes = int(read + wbytes)
            gbps = nbytes / (us * 1e-6) / 1e9
            run["forms"][name] = {"us": round(us, 2), "bytes": nbytes, "written": int(wbytes), "gbps": round(gbps, 1), "write_gbps": round(wbytes / (us * 1e-6) / 1e9, 1),
                                  "frac_copy": round(gbps / copy_gbps, 3)}
            print(f"run {rep} {name:24s} {us:9.1f} us  {nbytes / 1e6:7.1f} MB  {gbps:7.1f} GB/s  {gbps / copy_gbps:5.2f} of copy ({copy_gbps:.0f} GB/s)")
        res["residual"]["runs"].append(run)
    dec.batch_destroy(hb)


def torch_census(torch, a, b, w, h):
    """per plane the SSE, the differing samples and the largest difference of two flat yuv420p int16 tensors: what a caller computes without xgpu_pic_compare"""
    out = []
    o = 0
    for n in (w * h, w * h // 4, w * h // 4):
        d = a[o:o + n].to(torch.int32) - b[o:o + n].to(torch.int32)
        out += [(d * d).sum(), (d != 0).sum(), d.abs().max()]
        o += n
    return torch.stack(out)


def compare_leg(torch, dec, pic, s, a, res, copy_gbps):
    """xgpu_pic_compare against the copy-rate time of the two pictures and against the torch route, alternated"""
    w, h, bd = a.width, a.height, a.bit_depth
    rng = np.random.default_rng(3)
    other = dec.pic_alloc()
    dec.pic_upload(other, [rng.integers(0, 1 << bd, (h >> k, w >> k)).astype(np.int16) for k in (0, 1, 1)])
    flat = dec.pic_output_tensor(other, layout="yuv420p", dtype=torch.int16)
    shifted = torch.empty(flat.numel() + 8, dtype=torch.int16, device="cuda:0")[1:1 + flat.numel()]
    shifted.copy_(flat)
    nbytes = 2 * 3 * w * h
    floor_us = nbytes / (copy_gbps * 1e9) * 1e6
    out = torch.empty(20, dtype=torch.int64, device="cuda:0")
    forms = [("census", other, dict(ssim=False)), ("census_ssim", other, dict(ssim=True)), ("census_map", other, dict(ssim=False, block_map=True)),
             ("census_ssim_map", other, dict(ssim=True, block_map=True)), ("census_ssim_tensor_ref", flat, dict(ssim=True)),
             ("census_ssim_tensor_ref_unaligned", shifted, dict(ssim=True)), ("census_ssim_map_identical", pic, dict(ssim=True, block_map=True))]
    ya, yb = dec.pic_output_tensor(pic, layout="yuv420p", dtype=torch.int16), torch.empty_like(flat)

    def route():
        dec.pic_output_tensor(pic, layout="yuv420p", dtype=torch.int16, out=ya)
        dec.pic_output_tensor(other, layout="yuv420p", dtype=torch.int16, out=yb)
        return torch_census(torch, ya, yb, w, h)

    def census_only():
        return torch_census(torch, ya, yb, w, h)

    res["compare"] = {"bytes": nbytes, "copy_rate_us": round(floor_us, 2), "forms": {}}
    for name, ref, kw in forms:
        def call():
            dec.pic_compare(pic, ref, out=out, sync=False, **kw)
        for _ in range(5):
            call(); route()
        torch.cuda.synchronize()
        n = max(a.iters // 2, 5)
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for k in ("call", "torch_route", "torch_census_only")}
        for i in range(n):
            for k, fn in (("call", call), ("torch_route", route), ("torch_census_only", census_only)):
                if k != "call" and name != "census":
                    continue      # the torch route does not depend on the form: timed once, next to the census
                e0, e1 = ev[k][i]
                torch.cuda.synchronize()      # each starts on an idle device
                e0.record(s)
                fn()
                e1.record(s)
        torch.cuda.synchronize()
        alt = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev["call"]])      # from an idle device: the launch latency is inside
        r = {"us": round(timed(torch, s, call, a.iters), 2), "alternated_us": round(float(np.median(alt)), 2), "alternated_p10_us": round(float(np.percentile(alt, 10)), 2),
             "alternated_p90_us": round(float(np.percentile(alt, 90)), 2)}
        r["gbps"] = round(nbytes / (r["us"] * 1e-6) / 1e9, 1)
        r["frac_copy"] = round(floor_us / r["us"], 3)
        if name == "census":
            for k in ("torch_route", "torch_census_only"):
                t = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[k]])
                res["compare"][k + "_us"] = round(float(np.median(t)), 2)
            d = abi_dict(out)
            want = route().cpu().numpy().reshape(3, 3)
            res["compare"]["torch_route_agrees"] = bool([d["sse"], d["n_diff"], d["max_abs"]] == want.T.tolist())
        r["torch_route_over_call"] = round(res["compare"]["torch_route_us"] / r["alternated_us"], 2)      # both from an idle device
        r["torch_census_only_over_call"] = round(res["compare"]["torch_census_only_us"] / r["alternated_us"], 2)
        print(f"compare {name:34s} {r['us']:9.1f} us  {r['gbps']:7.1f} GB/s  copy-rate time {floor_us:7.1f} us ({r['frac_copy']:.2f})   torch route {res['compare']['torch_route_us']:9.1f} us "
              f"({r['torch_route_over_call']:.1f}x; its reductions alone {res['compare']['torch_census_only_us']:9.1f} us, {r['torch_census_only_over_call']:.1f}x)")
        res["compare"]["forms"][name] = r
    dec.pic_free(other)


def stats_contents(rng, w, h, bd):
    """the three contents of the stats leg - the contention of the LDS histogram differs between them: uniform random samples, one value everywhere, and a
    smooth diagonal gradient with +-2 codes of noise (chroma: around the middle)"""
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int32)
    grad = ((yy + xx) * top // (h + w - 2) + rng.integers(-2, 3, (h, w))).clip(0, top).astype(np.int16)
    gc = [((1 << (bd - 1)) + (xx[:h // 2, :w // 2] - w // 4) * (top // 4) // w + rng.integers(-2, 3, (h // 2, w // 2))).clip(0, top).astype(np.int16) for _ in range(2)]
    return {"random": [rng.integers(0, 1 << bd, (h >> k, w >> k)).astype(np.int16) for k in (0, 1, 1)],
            "constant": [np.full((h >> k, w >> k), v, np.int16) for k, v in zip((0, 1, 1), (3 << (bd - 3), 1 << (bd - 1), 1 << (bd - 1)))],
            "gradient": [grad] + gc}


def stats_leg(torch, dec, pic, s, a, res, copy_gbps):
    """xgpu_pic_stats - census only, with 2^8 and 2^B bins, with the light level - on three contents, against the copy-rate time of the picture and against the
    torch route (a yuv420p tensor, then bincount, sum, min and max per plane; with light the u16 RGB tensor, amax, bincount and a gather through lin), alternated"""
    from xevd_amd import abi
    w, h, bd = a.width, a.height, a.bit_depth
    nbytes = 3 * w * h
    floor_us = nbytes / (copy_gbps * 1e9) * 1e6
    light = dict(transfer=16, matrix=9)
    lin = torch.from_numpy(abi.stats_lin(dec.lib, 16, bd)).to("cuda:0")
    forms = [("census", dict(hist_bits=0), "census"), ("hist_8", dict(hist_bits=8), "hist"), (f"hist_{bd}", dict(hist_bits=bd), "hist"),
             (f"hist_{bd}_light", dict(hist_bits=bd, light=light), "light")]
    out = torch.empty(22, dtype=torch.int64, device="cuda:0")
    yuv = dec.pic_output_tensor(pic, layout="yuv420p", dtype=torch.int16)
    rgb = dec.pic_output_tensor(pic, layout="rgb", dtype=torch.int16, matrix=9)
    bounds = (0, w * h, w * h * 5 // 4, w * h * 3 // 2)

    def route(kind):
        if kind == "light":
            dec.pic_output_tensor(pic, layout="rgb", dtype=torch.int16, matrix=9, out=rgb)
            m = rgb.amax(dim=0).reshape(-1).to(torch.int64)
            return torch.bincount(m, minlength=1 << bd), m.max(), lin[m].sum(dtype=torch.float64)
        dec.pic_output_tensor(pic, layout="yuv420p", dtype=torch.int16, out=yuv)
        r = []
        for k in range(3):
            pl = yuv[bounds[k]:bounds[k + 1]]
            r.append((torch.bincount(pl.to(torch.int64), minlength=1 << bd) if kind == "hist" else None, pl.sum(dtype=torch.int64), pl.min(), pl.max()))
        return r

    res["stats"] = {"bytes": nbytes, "copy_rate_us": round(floor_us, 2), "contents": {}}
    for cname, planes in stats_contents(np.random.default_rng(4), w, h, bd).items():
        dec.pic_upload(pic, planes)
        rc = res["stats"]["contents"][cname] = {"forms": {}, "torch": {}}
        n = max(a.iters // 4, 5)
        for kind in ("census", "hist", "light"):      # the torch routes, each from an idle device
            for _ in range(2):
                route(kind)
            t = []
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(s)
                route(kind)
                e1.record(s)
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1) * 1e3)
            rc["torch"][kind + "_us"] = round(float(np.median(t)), 2)
        for name, kw, kind in forms:
            def call():
                return dec.pic_stats(pic, out=out, sync=False, **kw)
            for _ in range(5):
                call()
            alt = []
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()      # from an idle device, as the torch route: the launch latency is inside
                e0.record(s)
                call()
                e1.record(s)
                torch.cuda.synchronize()
                alt.append(e0.elapsed_time(e1) * 1e3)
            r = {"us": round(timed(torch, s, call, a.iters), 2), "alternated_us": round(float(np.median(alt)), 2)}
            r["gbps"] = round(nbytes / (r["us"] * 1e-6) / 1e9, 1)
            r["frac_copy"] = round(floor_us / r["us"], 3)
            r["torch_route_us"] = rc["torch"][kind + "_us"]
            r["torch_route_over_call"] = round(r["torch_route_us"] / r["alternated_us"], 2)
            if kind == "hist":
                _, hist, _ = call()
                r["torch_route_agrees"] = bool(all(torch.equal(t[0][:hist.shape[1]] if kw["hist_bits"] == bd else t[0].view(hist.shape[1], -1).sum(1), hist[k].to(torch.int64))
                                                   for k, t in enumerate(route("hist"))))
            if kind == "light":
                _, _, lh = call()
                d = abi.stats_result_dict(out.cpu().numpy())
                th, tm, tsum = route("light")
                r["torch_route_agrees"] = bool(torch.equal(th, lh.to(torch.int64)) and int(tm) == d["light_max_code"] and abs(float(tsum) - d["light_sum"]) <= 1e-9 * d["light_sum"])
            print(f"stats {cname:9s} {name:18s} {r['us']:9.1f} us  {r['gbps']:7.1f} GB/s  copy-rate time {floor_us:7.1f} us ({r['frac_copy']:.2f})   from idle {r['alternated_us']:9.1f} us, "
                  f"torch route {r['torch_route_us']:9.1f} us ({r['torch_route_over_call']:.1f}x)")
            rc["forms"][name] = r


def abi_dict(t):
    from xevd_amd import abi
    return abi.compare_result_dict(t.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--bit-depth", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=3, help="residual leg: runs of the whole measurement in this process")
    ap.add_argument("--legs", choices=("all", "full", "scaled", "scaled_cm", "scaled_lin", "resampled", "rois", "rois_dev", "ladder", "warp", "remap", "residual", "compare", "stats", "packed", "lut3d", "dither", "overlay"), default="all",
                    help="full: the full-size forms and the side information; scaled: the scaled leg alone; scaled_cm: the colour-managed scaled output alone; scaled_lin: the scaled output filtered in linear light alone; resampled: the bicubic resize alone; rois: the batched regions of interest alone; "
                         "rois_dev: the regions of interest from boxes in device memory alone; ladder: the ladder of scaled P010 surfaces alone; warp: the warped regions of interest alone; remap: the remapped output alone; residual: the residual "
                         "export alone; compare: the picture comparison alone; stats: the picture statistics alone; packed: the packed display surfaces alone; "
                         "lut3d: the 3D LUT outputs alone; dither: the dithered outputs alone; overlay: the overlaid outputs alone")
    a = ap.parse_args()
    import torch
    from xevd_amd.decoder import XgpuDecoder
    if not torch.cuda.is_available():
        raise SystemExit("bench_output_device: no GPU")
    w, h, bd = a.width, a.height, a.bit_depth
    rng = np.random.default_rng(0)
    planes = [rng.integers(0, 1 << bd, (h, w)).astype(np.int16), rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(np.int16),
              rng.integers(0, 1 << bd, (h // 2, w // 2)).astype(np.int16)]
    forms = [("rgb_u8_planar", dict(dtype=torch.uint8), 3),
             ("rgb_u8_interleaved", dict(dtype=torch.uint8, channels_last=True), 3),
             ("rgb_f16_planar", dict(dtype=torch.float16), 6),
             ("yuv420p_u8", dict(layout="yuv420p", dtype=torch.uint8), 1.5),
             ("nv12_u8", dict(layout="nv12", dtype=torch.uint8), 1.5),
             ("p010", dict(layout="p016", dtype=torch.int16, out_bit_depth=10), 3),
             ("yuv444_u8_planar", dict(layout="yuv444", dtype=torch.uint8), 3),
             ("yuv444_f16_planar", dict(layout="yuv444", dtype=torch.float16), 6)]
    # colour-managed forms (k_output_cm): PQ / BT.2020 -> sRGB / BT.709 through the tone curve, and -> linear BT.709.
    # rgb_f32_planar is the plain form torch starts from.
    hdr = dict(src_primaries=9, src_transfer=16, dst_primaries=1)
    to_srgb, to_lin = dict(hdr, dst_transfer=13, tone_map=True), dict(hdr, dst_transfer=8, linear_scale=100.0)
    forms += [("rgb_f32_planar", dict(dtype=torch.float32), 12)]
    forms += [("cm_pq2020_srgb_u8_planar", dict(dtype=torch.uint8, matrix=9, colour=to_srgb), 3),
              ("cm_pq2020_linear709_f16_planar", dict(dtype=torch.float16, matrix=9, colour=to_lin), 6),
              ("cm_pq2020_linear709_f32_planar", dict(dtype=torch.float32, matrix=9, colour=to_lin), 12)]
    res = {"width": w, "height": h, "bit_depth": bd, "iters": a.iters, "forms": {}}
    with XgpuDecoder(w, h, bd, device=0, max_pics=3) as dec:
        pic = dec.pic_alloc()
        dec.pic_upload(pic, planes)
        copy_gbps = dec.measure_copy_bw(1 << 30, 20)
        res["copy_gbps"] = copy_gbps
        s = torch.cuda.Stream()      # a stream of its own: the conversion is queued on it directly (torch's default stream goes through a side stream)
        torch.cuda.set_stream(s)
        if a.legs in ("all", "scaled"):
            scaled_leg(torch, dec, pic, s, a, res, copy_gbps)
        if a.legs in ("all", "scaled_cm"):
            scaled_cm_leg(torch, dec, pic, s, a, res)
        if a.legs in ("all", "scaled_lin"):
            scaled_lin_leg(torch, dec, pic, s, a, res)
        if a.legs in ("all", "resampled"):
            resampled_leg(torch, dec, pic, s, a, res)
        if a.legs in ("all", "rois"):
            rois_leg(torch, dec, pic, s, a, res)
        if a.legs in ("all", "rois_dev"):
            rois_dev_leg(torch, dec, pic, s, a, res)
        if a.legs in ("all", "packed"):
            packed_leg(torch, dec, pic, s, a, res, copy_gbps)
        if a.legs in ("all", "lut3d"):
            lut3d_leg(torch, dec, pic, s, a, res, copy_gbps, planes)
        if a.legs in ("all", "dither"):
            dither_leg(torch, dec, pic, s, a, res, copy_gbps)
        if a.legs in ("all", "overlay"):
            overlay_leg(torch, dec, pic, s, a, res, copy_gbps)
        if a.legs in ("all", "ladder"):
            ladder_leg(torch, dec, pic, s, a, res)
        if a.legs in ("all", "warp"):
            warp_leg(torch, dec, pic, s, a, res)
        if a.legs in ("all", "remap"):
            remap_leg(torch, dec, pic, s, a, res)
        if a.legs in ("all", "residual"):
            residual_leg(torch, dec, pic, s, a, res)
        if a.legs in ("all", "compare"):
            compare_leg(torch, dec, pic, s, a, res, copy_gbps)
        if a.legs in ("all", "stats"):
            stats_leg(torch, dec, pic, s, a, res, copy_gbps)
            dec.pic_upload(pic, planes)      # (the leg uploads its contents into the slot)
        if a.legs in ("all", "full"):
            for name, kw, wbytes in forms:
                out = dec.pic_output_tensor(pic, **kw)
                for _ in range(5):
                    dec.pic_output_tensor(pic, out=out, **kw)
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
                torch.cuda._sleep(int(3e8))      # the GPU waits while the host queues every timed launch: the events then bracket device time only
                for e0, e1 in ev:
                    e0.record(s)
                    dec.pic_output_tensor(pic, out=out, **kw)
                    e1.record(s)
                torch.cuda.synchronize()
                us = float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]))
                nbytes = int(w * h * (3 + wbytes))
                gbps = nbytes / (us * 1e-6) / 1e9
                res["forms"][name] = {"us": round(us, 2), "bytes": nbytes, "gbps": round(gbps, 1), "frac_copy": round(gbps / copy_gbps, 3)}
                print(f"{name:20s} {us:9.1f} us  {nbytes / 1e6:7.1f} MB  {gbps:7.1f} GB/s  {gbps / copy_gbps:5.2f} of copy ({copy_gbps:.0f} GB/s)")
            # the same two transforms done afterwards in torch on the plain f32 RGB tensor (pow / where / matmul), timed the same way
            rgb = dec.pic_output_tensor(pic, dtype=torch.float32, matrix=9)
            for name, fn, wbytes in (("torch_pq2020_srgb_u8_after_f32", lambda: torch_transform(torch, rgb, True), 3),
                                     ("torch_pq2020_linear709_f32_after_f32", lambda: torch_transform(torch, rgb, False), 12)):
                n = max(a.iters // 10, 5)
                for _ in range(2):
                    fn()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
                for e0, e1 in ev:
                    e0.record(s)
                    fn()
                    e1.record(s)
                torch.cuda.synchronize()
                us = float(np.median([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]))
                res["forms"][name] = {"us": round(us, 2), "launches": n, "note": "excludes the plain f32 output it starts from"}
                print(f"{name:40s} {us:9.1f} us (torch, after rgb_f32_planar)")
            # ---- coding side information of a decoded picture: the uploaded picture is both references of a synthetic B picture
            from xevd_amd import synth
            batch = synth.gen_frame(np.random.default_rng(1), w, h, bd, inter_frac=0.9, bi_frac=0.5, coded_frac=0.6, n_refs=(1, 1), qp_range=(22, 37), mv_sigma_px=8.0, oob_frac=0.05)
            cur = dec.pic_alloc()
            hb = dec.batch_create(batch)
            dec.decode_picture(cur, 8, {(0, 0): (pic, 4), (0, 1): (pic, 16)}, hb, deblock=True)
            dec.sync()
            n_units = (w // 4) * (h // 4)
            crop = (0, 0, 0, 0)
            side = [("side_blocks", dict(), 18 * n_units),
                    ("side_flow_f16_both_planar", dict(kind="flow", dtype=torch.float16), 8 * w * h),
                    ("side_flow_f16_both_interleaved", dict(kind="flow", dtype=torch.float16, channels_last=True), 8 * w * h),
                    ("side_flow_f16_list0_planar", dict(kind="flow", dtype=torch.float16, lists=0), 4 * w * h),
                    ("side_flow_f32_both_planar", dict(kind="flow", dtype=torch.float32), 16 * w * h),
                    ("side_flow_f32_both_interleaved", dict(kind="flow", dtype=torch.float32, channels_last=True), 16 * w * h),
                    ("side_flow_f32_list0_planar", dict(kind="flow", dtype=torch.float32, lists=0), 8 * w * h),
                    ("side_flow_f16_both_planar_per_poc", dict(kind="flow", dtype=torch.float16, per_poc=True), 8 * w * h)]
            for name, kw, wbytes in side:
                out = dec.frame_side_info(cur, **kw)
                us = timed(torch, s, lambda: dec.frame_side_info(cur, out=out, **kw), a.iters)
                nbytes = int(16 * n_units + wbytes)
                gbps = nbytes / (us * 1e-6) / 1e9
                res["forms"][name] = {"us": round(us, 2), "bytes": nbytes, "written": int(wbytes), "gbps": round(gbps, 1), "write_gbps": round(wbytes / (us * 1e-6) / 1e9, 1),
                                      "frac_copy": round(gbps / copy_gbps, 3)}
                print(f"{name:36s} {us:9.1f} us  {nbytes / 1e6:7.1f} MB  {gbps:7.1f} GB/s  {gbps / copy_gbps:5.2f} of copy ({copy_gbps:.0f} GB/s)")
            blocks = dec.frame_side_info(cur)
            for name, dt in (("torch_flow_f16_both_planar_from_blocks", torch.float16), ("torch_flow_f32_both_planar_from_blocks", torch.float32)):
                n = max(a.iters // 10, 5)
                us = timed(torch, s, lambda: torch_flow(torch, blocks, crop, dt), n, warm=2, sleep=False)
                res["forms"][name] = {"us": round(us, 2), "launches": n, "note": "excludes the BLOCKS export it starts from"}
                print(f"{name:40s} {us:9.1f} us (torch, after side_blocks)")
                kdt = torch.float16 if dt == torch.float16 else torch.float32
                same = torch.equal(torch_flow(torch, blocks, crop, dt).view(torch.int16 if dt == torch.float16 else torch.int32),
                                   dec.frame_side_info(cur, kind="flow", dtype=kdt).view(torch.int16 if dt == torch.float16 else torch.int32))
                res["forms"][name]["equals_kernel"] = bool(same)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
