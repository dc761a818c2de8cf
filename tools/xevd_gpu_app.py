#!/usr/bin/env python3
"""Decode an MPEG-5 EVC Baseline bitstream on the MI355X and write planar YUV - the counterpart of the reference's sample
application (app/xevd_app.c: -i in.evc -o out.yuv --output-bit-depth N).  usage: xevd_gpu_app.py -i in.evc -o out.yuv
--pix-fmt nv12 / p010 writes semi-planar frames instead (what a raw-video reader takes as nv12 / p010le): 8-bit samples, or 10-bit samples in the
high bits of 16-bit words, whatever the stream's depth.
--pix-fmt rgba / bgra / x2bgr10le / x2rgb10le / yuyv422 / uyvy422 / y210le writes packed display surfaces, raw frames a raw-video reader takes
under those names; the RGB ones compose with --to.
--lut look.cube writes every picture through that 3D LUT: interleaved 8-bit RGB frames, or the packed RGB --pix-fmt given with it.
--ladder 3840x2160,1920x1080,... also writes every picture scaled to each of these sizes on the device, in one call per picture: one file per
rung next to -o, the size in its name (out_1920x1080.yuv), in the --pix-fmt layout."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xevd_amd.player import StreamDecoder      # noqa: E402


# --pix-fmt names of the packed display surfaces -> the keyword arguments of XgpuDecoder.pic_output_packed (dtype: torch's name)
PACKED_PIX_FMTS = {"rgba": dict(layout="rgba", dtype="uint8"), "bgra": dict(layout="bgra", dtype="uint8"), "x2bgr10le": dict(layout="rgb10a2"),
                   "x2rgb10le": dict(layout="bgr10a2"), "yuyv422": dict(layout="yuyv", dtype="uint8"), "uyvy422": dict(layout="uyvy", dtype="uint8"),
                   "y210le": dict(layout="yuyv", dtype="int16", out_bit_depth=10)}


class RefCompare:
    """compare= of StreamDecoder for --ref: called per picture in decoding order, returns the picture's frame of the file as a tensor on the device.  The frame of
    the picture expected next is read into pinned memory and copied on a stream of its own while the current picture decodes.  The line of a picture is
    printed - and --expect-identical acted on - when the next picture arrives, or at the end: the result is under params["compare"] only then."""

    def __init__(self, path, order, expect_identical, device):
        self.path, self.order, self.expect_identical, self.device = path, order, expect_identical, device
        self.n = self.epoch_start = 0
        self.last = None           # the picture whose result has not been reported yet
        self.ahead = None          # (frame index, tensor, event)
        self.pinned, self.used = [None, None], [None, None]
        self.seen = set()
        self.n_cmp = self.n_bad = 0
        self.sse, self.cnt, self.q, self.win = [0] * 3, [0] * 3, 0, 0
        self.bit_depth = 8

    def _upload(self, idx, nbytes, dtype):
        import numpy as np
        import torch
        k = idx & 1
        if self.used[k] is not None:
            self.used[k].synchronize()      # the copy out of this pinned buffer is done
        if self.pinned[k] is None or self.pinned[k].numel() * self.pinned[k].element_size() != nbytes or self.pinned[k].dtype != dtype:
            self.pinned[k] = torch.empty(nbytes // dtype.itemsize, dtype=dtype).pin_memory()
        raw = np.fromfile(self.path, dtype=np.uint8, count=nbytes, offset=idx * nbytes)
        if raw.size != nbytes:
            return None
        self.pinned[k].view(torch.uint8).numpy()[:] = raw
        if getattr(self, "_copy", None) is None:
            self._copy = torch.cuda.Stream(device=self.device)
        with torch.cuda.stream(self._copy):
            t = self.pinned[k].to(torch.device("cuda", self.device), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self.used[k] = ev
        return idx, t, ev

    def __call__(self, p):
        import torch
        self.report()
        if p["is_idr"]:
            self.epoch_start = self.n
        idx = self.n if self.order == "decoding" else self.epoch_start + p["poc"]
        self.n += 1
        self.bit_depth = p["bit_depth"]
        dtype = torch.uint8 if p["bit_depth"] == 8 else torch.int16
        nbytes = p["width"] * p["height"] * 3 // 2 * dtype.itemsize
        if idx < 0 or idx in self.seen:
            sys.exit(f"--ref-order output: POC {p['poc']} does not count up from its IDR picture; use --ref-order decoding with a file in that order")
        self.seen.add(idx)
        got = self.ahead if self.ahead is not None and self.ahead[0] == idx else self._upload(idx, nbytes, dtype)
        if got is None:
            sys.exit(f"{self.path}: no frame {idx} of {nbytes} bytes (POC {p['poc']})")
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(got[2])
        got[1].record_stream(cur)
        self.ahead = self._upload(idx + 1, nbytes, dtype)      # the next picture's, in either order, more often than not
        self.last = (p, idx)
        return got[1]

    def report(self):
        if self.last is None:
            return
        (p, idx), self.last = self.last, None
        d = p["compare"]
        first = next((f"{'YUV'[c]}({f[1]},{f[0]})" for c, f in enumerate(d["first_diff"]) if f is not None), "-")
        nd = sum(d["n_diff"])
        print(f"POC {p['poc']:4d} frame {idx:4d}  PSNR-Y {d['psnr'][0]:.4f} U {d['psnr'][1]:.4f} V {d['psnr'][2]:.4f}  SSIM-Y {d['ssim'][0]:.6f}  n_diff {nd}  first {first}")
        self.n_cmp += 1
        self.n_bad += nd != 0
        for c in range(3):
            self.sse[c] += d["sse"][c]
            self.cnt[c] += d["n"][c]
        self.q += d["ssim_q30"][0]
        self.win += d["ssim_windows"][0]
        if nd and self.expect_identical:
            sys.stdout.flush()
            print(f"POC {p['poc']}: {nd} samples differ from frame {idx} of {self.path}, the first at {first}", file=sys.stderr)
            sys.exit(1)

    def finish(self):
        from xevd_amd import abi
        self.report()
        ps = abi.psnr({"n": self.cnt, "sse": self.sse}, self.bit_depth)
        ss = self.q / (self.win * float(1 << 30)) if self.win else float("nan")
        print(f"{self.n_cmp} pictures compared, {self.n_bad} differ  PSNR-Y {ps[0]:.4f} U {ps[1]:.4f} V {ps[2]:.4f}  SSIM-Y {ss:.6f}")
        sys.stdout.flush()


def stats_options(p):
    """stats= of StreamDecoder for --stats: the defaults of XgpuDecoder.pic_stats, and the light level where the stream's VUI names a transfer characteristic
    the library knows"""
    from xevd_amd import abi
    col = p["colour"]
    return {"light": bool(col["vui_present"]) and col["transfer_characteristics"] in abi.STATS_TRANSFERS}


def stats_line(p):
    """one picture's line of --stats: POC, then per component n, min, max, mean and the two percentiles, then - where it was taken - the light level: the highest
    code of max(R', G', B') and its linear light, the two percentiles' linear light, the mean linear light"""
    d = p["stats"]
    parts = [f"POC {p['poc']}"]
    for c, name in enumerate("YUV"):
        parts.append(f"{name} n {d['n'][c]} min {d['min'][c]} max {d['max'][c]} mean {d['mean'][c]:.4f} pctl {d['pctl'][c][0]} {d['pctl'][c][1]}")
    if d["light_hist"] is not None:
        parts.append(f"light max {d['light_max_code']} {d['light_max']:.6f} pctl {d['light_pctl'][0]:.6f} {d['light_pctl'][1]:.6f} mean {d['light_mean']:.6f}")
    return "  ".join(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--input", required=True)
    ap.add_argument("-o", "--output")
    ap.add_argument("--output-bit-depth", type=int, default=0, help="0 = the stream's bit depth (8 -> bytes, else 16-bit little endian)")
    ap.add_argument("--pix-fmt", choices=("yuv420p", "nv12", "p010") + tuple(PACKED_PIX_FMTS), default="yuv420p",
                    help="nv12: 8-bit semi-planar; p010: 10 bit in 16-bit little-endian words, semi-planar; rgba / bgra: four bytes per pixel, alpha 255; "
                    "x2bgr10le / x2rgb10le: one 10:10:10:2 little-endian word per pixel (R / B in the low bits), alpha 3; yuyv422 / uyvy422: packed 8-bit 4:2:2; "
                    "y210le: packed 4:2:2, 10 bit in the high bits of 16-bit words (all ignore --output-bit-depth; the RGB ones take --to)")
    ap.add_argument("--to", default=None, help="write interleaved 8-bit RGB frames in this colour space instead (srgb, bt709, pq-bt2020, ...: "
                    "StreamDecoder.COLOUR_PRESETS), converted on the device from the primaries / transfer characteristics of the stream's VUI")
    ap.add_argument("--lut", default=None, metavar="FILE.cube", help="write every picture through this 3D LUT (a .cube file; tetrahedral interpolation on the device, "
                    "INTEGRATION.md 8q): interleaved 8-bit RGB frames, or - with --pix-fmt rgba / bgra / x2bgr10le / x2rgb10le - that packed surface; not with --to, "
                    "--size or --ladder")
    ap.add_argument("--dither", default=None, choices=("bayer", "blue"), help="dither instead of rounding where the output has fewer bits than the stream (INTEGRATION.md "
                    "8r): with --pix-fmt nv12 / p010 / rgba / bgra / x2bgr10le / x2rgb10le, or with --to (8-bit RGB); not with --lut, --size or --ladder")
    ap.add_argument("--dither-size", type=int, default=None, metavar="N", help="with --dither: the side of the matrix, a power of two (default: bayer 8, blue 64)")
    ap.add_argument("--dither-temporal", action="store_true", help="with --dither: move the matrix from picture to picture (xgpu_dither_phase of the POC)")
    ap.add_argument("--overlay", action="append", default=None, metavar="FILE.npy:X:Y[:OPACITY]", help="blend this bitmap over every picture on the device (INTEGRATION.md "
                    "8s), repeatable, in the order given: an [h, w, 4] uint8 RGBA array with straight alpha, its top left corner at (X, Y) of the picture (either may be "
                    "negative), OPACITY 0 .. 255 (default 255); with --pix-fmt nv12 / p010 / rgba / bgra / x2bgr10le / x2rgb10le, with --to, or alone (interleaved 8-bit "
                    "RGB frames); not with --dither, --lut, --size or --ladder")
    ap.add_argument("--side-info", default=None, metavar="FILE", help="also write the coding side information of every picture, in DECODING order: a text line "
                    "'POC h_scu w_scu', then nine planes of h_scu x w_scu little-endian int16 (list 0 / 1 vectors, POC distances, mode, QP, flags: INTEGRATION.md 8c)")
    ap.add_argument("--residual", default=None, metavar="FILE", help="also write the prediction residual of every picture, in DECODING order: a text line "
                    "'POC w h', then the little-endian int16 planes Y (h x w), Cb, Cr (h/2 x w/2 each) of the uncropped picture (INTEGRATION.md 8g)")
    ap.add_argument("--stats", default=None, metavar="FILE", help="also write the statistics of every picture, taken on the device (INTEGRATION.md 8i), in DECODING order: "
                    "one text line 'POC p  Y n N min A max B mean M pctl P1 P99.99  U ...  V ...' of the uncropped picture, and 'light max CODE L pctl L1 L2 mean LM' "
                    "(linear light, 0 .. 1) when the stream's VUI gives a transfer characteristic")
    ap.add_argument("--size", default=None, metavar="WxH", help="write interleaved 8-bit RGB frames resized to W x H on the device instead (antialiased bilinear, "
                    "the matrix / range / chroma siting of the stream's VUI: INTEGRATION.md 8d); with --to: resized and taken to that colour space in the same call "
                    "(INTEGRATION.md 8m), with --tiles too")
    ap.add_argument("--linear-light", action="store_true", help="with --size and --to: filter the linear light of the source instead of its encoded samples "
                    "(gamma-correct resize, INTEGRATION.md 8n), with --tiles too")
    ap.add_argument("--tiles", default=None, metavar="WxH", help="with --size: every picture as its grid of W x H tiles (the last column / row moved back inside the "
                    "picture), each resized to --size by one call per picture (INTEGRATION.md 8e); the frames written are the tiles, row by row")
    ap.add_argument("--resample", default=None, metavar="NAME", choices=("bicubic", "catmull-rom", "cubic-0.75", "mitchell"), help="with --size: resize with this "
                    "bicubic kernel instead of the antialiased triangle (INTEGRATION.md 8o), with --tiles too; not with --to, --linear-light or --remap")
    ap.add_argument("--remap", default=None, metavar="GRID.npy", help="with --size: every picture pulled through this coordinate grid on the device instead of resized "
                    "(INTEGRATION.md 8k): an int32 (Q16) or float32 (luma samples) array [gh, gw, 2] or [N, gh, gw, 2] of source positions for the W x H image, "
                    "e.g. from abi.remap_from_lens; N > 1 writes N frames per picture")
    ap.add_argument("--remap-step", type=int, default=0, metavar="K", help="with --remap: the grid holds a node every 2^K pixels (0 .. 6; 0: one per pixel)")
    ap.add_argument("--ref", default=None, metavar="FILE.yuv", help="compare every decoded picture with this planar 4:2:0 file on the device (INTEGRATION.md 8h): frames "
                    "of the uncropped picture at the stream's depth (8 bit: bytes, else 16-bit little endian), as -o writes them; prints PSNR, SSIM, the number "
                    "of differing samples and the first differing position per picture, and a summary")
    ap.add_argument("--ref-order", choices=("output", "decoding"), default="output", help="the order of the frames in --ref: output order (what -o and the reference "
                    "application write; needs POCs that count 0, 1, 2, ... from every IDR picture) or decoding order")
    ap.add_argument("--expect-identical", action="store_true", help="with --ref: exit with status 1 at the first picture that differs from its frame")
    ap.add_argument("--ladder", default=None, metavar="WxH,WxH,...", help="also write every picture scaled to each of these even sizes (1 .. 8 of them) on the device, "
                    "as --pix-fmt surfaces: one file per size next to -o, OUT_WxH.EXT; yuv420p takes --output-bit-depth (8: bytes)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    lad, lad_sizes = {}, []
    if args.pix_fmt in PACKED_PIX_FMTS and (args.ladder is not None or args.size is not None):
        ap.error(f"--pix-fmt {args.pix_fmt}: the packed surfaces have no scaled form (--size, --ladder)")
    if args.lut is not None:
        if args.to is not None or args.size is not None or args.ladder is not None:
            ap.error("--lut: the 3D LUT has the full-size RGB and packed outputs only (not --to, --size, --ladder)")
        if args.pix_fmt != "yuv420p" and PACKED_PIX_FMTS.get(args.pix_fmt, {}).get("layout") not in ("rgba", "bgra", "rgb10a2", "bgr10a2"):
            ap.error(f"--lut: a 3D LUT needs an RGB --pix-fmt, not {args.pix_fmt}")
    dith = {}
    if args.dither is not None:
        if args.lut is not None or args.size is not None or args.ladder is not None:
            ap.error("--dither: the dithered output has the full-size forms only (not --lut, --size, --ladder)")
        if args.to is None and (args.pix_fmt not in ("nv12", "p010") and PACKED_PIX_FMTS.get(args.pix_fmt, {}).get("layout") not in ("rgba", "bgra", "rgb10a2", "bgr10a2")):
            ap.error(f"--dither: needs --pix-fmt nv12, p010, rgba, bgra, x2bgr10le or x2rgb10le, or --to; not {args.pix_fmt}")
        dith = dict(dither=dict(kind=args.dither, size=args.dither_size or (8 if args.dither == "bayer" else 64), temporal=args.dither_temporal))
    elif args.dither_size is not None or args.dither_temporal:
        ap.error("--dither-size, --dither-temporal: need --dither")
    ovl = {}
    if args.overlay:
        import numpy as np
        import torch
        if args.dither is not None or args.lut is not None or args.size is not None or args.ladder is not None:
            ap.error("--overlay: the overlaid output has the full-size forms only (not --dither, --lut, --size, --ladder)")
        if args.pix_fmt not in ("yuv420p", "nv12", "p010") and PACKED_PIX_FMTS.get(args.pix_fmt, {}).get("layout") not in ("rgba", "bgra", "rgb10a2", "bgr10a2"):
            ap.error(f"--overlay: needs --pix-fmt nv12, p010, rgba, bgra, x2bgr10le or x2rgb10le, --to, or no --pix-fmt (8-bit RGB); not {args.pix_fmt}")
        layers = []
        for item in args.overlay:
            # X, Y and OPACITY are split from the right, so that FILE may hold colons: four fields if the last three are integers, else three
            def ints(fields):
                try:
                    return [int(v) for v in fields]
                except ValueError:
                    return None
            four, three = item.rsplit(":", 3), item.rsplit(":", 2)
            if len(four) == 4 and ints(four[1:]) is not None:
                name, (x, y, opacity) = four[0], ints(four[1:])
            elif len(three) == 3 and ints(three[1:]) is not None:
                name, (x, y), opacity = three[0], ints(three[1:]), 255
            else:
                ap.error(f"--overlay: expected FILE.npy:X:Y[:OPACITY], not {item!r}")
            img = np.load(name)
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 4:
                ap.error(f"--overlay: {name} is not an [h, w, 4] uint8 array")
            layers.append(dict(image=torch.from_numpy(np.ascontiguousarray(img)).to(f"cuda:{args.device}"), x=x, y=y, opacity=opacity))      # uploaded once
        ovl = dict(overlay=dict(layers=layers))
    if args.ladder is not None:
        import torch
        if not args.output:
            ap.error("--ladder: needs -o, whose name the files of the rungs are made from")
        try:
            lad_sizes = [tuple(int(v) for v in item.lower().split("x")) for item in args.ladder.split(",")]
            assert all(len(sz) == 2 for sz in lad_sizes)
        except (ValueError, AssertionError):
            ap.error(f"--ladder: expected WxH,WxH,..., not {args.ladder!r}")
        if args.pix_fmt == "nv12":
            so = dict(dtype=torch.uint8)
        elif args.pix_fmt == "p010":
            so = dict(dtype=torch.int16, out_bit_depth=10)
        else:
            so = dict(dtype=torch.uint8) if args.output_bit_depth == 8 else dict(dtype=torch.int16, out_bit_depth=args.output_bit_depth)
        lad = dict(surfaces=[(hh, ww) for ww, hh in lad_sizes], surface_layout="p016" if args.pix_fmt == "p010" else args.pix_fmt, surface_options=so)
    if args.expect_identical and args.ref is None:
        ap.error("--expect-identical: needs --ref")
    cmp = RefCompare(args.ref, args.ref_order, args.expect_identical, args.device) if args.ref else None
    if args.tiles is not None and args.size is None:
        ap.error("--tiles: needs --size")
    if args.linear_light and (args.size is None or args.to is None or args.remap is not None):
        ap.error("--linear-light: needs --size and --to, and not --remap")
    if args.resample is not None and (args.size is None or args.to is not None or args.linear_light or args.remap is not None):
        ap.error("--resample: needs --size, and not --to, --linear-light or --remap")
    if args.remap is not None and (args.size is None or args.tiles is not None):
        ap.error("--remap: needs --size, and not --tiles")
    data = open(args.input, "rb").read()
    t0 = time.perf_counter()
    side = {} if args.side_info else None
    resid = {} if args.residual else None
    stats = stats_options if args.stats else None
    # crop-free output like the reference application; bit-depth conversion and plane packing run on the device (xgpu_pic_output)
    if args.size is not None:
        import torch
        if args.to is not None and args.remap is not None:
            ap.error("--remap: the remapped output takes no colour transform (--to)")
        try:
            wd, hd = (int(v) for v in args.size.lower().split("x"))
        except ValueError:
            ap.error(f"--size: expected WxH, not {args.size!r}")
        rois = None
        if args.tiles is not None:
            from xevd_amd import abi
            try:
                tw, th = (int(v) for v in args.tiles.lower().split("x"))
            except ValueError:
                ap.error(f"--tiles: expected WxH, not {args.tiles!r}")
            rois = lambda p: abi.tile_rois(p["width"], p["height"], tw, th)      # noqa: E731
        remap = None
        if args.remap is not None:
            import numpy as np
            remap = np.load(args.remap)
            if remap.dtype not in (np.int32, np.float32):
                ap.error(f"--remap: an int32 or float32 array, not {remap.dtype}")
            remap = torch.from_numpy(remap).to(f"cuda:{args.device}")      # uploaded once, used for every picture
        pics = StreamDecoder(data, device=args.device).output_order(tensor=dict(layout="rgb", channels_last=True, dtype=torch.uint8), size=(hd, wd), to=args.to, side=side, rois=rois, residual=resid, compare=cmp, stats=stats,
                                                                    remap=remap, remap_step=args.remap_step, linear_light=args.linear_light, resample=args.resample, **lad)
    elif args.pix_fmt in PACKED_PIX_FMTS:      # one word per pixel or packed 4:2:2 (xgpu_pic_output_device_packed); --to takes the RGB ones to that colour space
        import torch
        opts = {k: getattr(torch, v) if k == "dtype" else v for k, v in PACKED_PIX_FMTS[args.pix_fmt].items()}
        if args.to is not None and opts["layout"] in ("yuyv", "uyvy"):
            ap.error(f"--to: a colour transform needs an RGB --pix-fmt, not {args.pix_fmt}")
        pics = StreamDecoder(data, device=args.device).output_order(packed=opts, to=args.to, side=side, residual=resid, compare=cmp, stats=stats, lut=args.lut, **lad, **dith, **ovl)
        pics = [(p, p["packed"]) for p, _ in pics]
    elif args.lut is not None:
        import torch
        pics = StreamDecoder(data, device=args.device).output_order(tensor=dict(layout="rgb", channels_last=True, dtype=torch.uint8), lut=args.lut, side=side, residual=resid, compare=cmp, stats=stats)
    elif args.to is not None:
        import torch
        pics = StreamDecoder(data, device=args.device).output_order(tensor=dict(layout="rgb", channels_last=True, dtype=torch.uint8), to=args.to, side=side, residual=resid, compare=cmp, stats=stats, **lad, **dith, **ovl)
    elif args.pix_fmt == "yuv420p" and ovl:      # the layers over the stream's own R'G'B' (matrix, range and siting of its VUI)
        import torch
        pics = StreamDecoder(data, device=args.device).output_order(tensor=dict(layout="rgb", channels_last=True, dtype=torch.uint8), side=side, residual=resid, compare=cmp, stats=stats, **ovl)
    elif args.pix_fmt == "yuv420p":
        pics = StreamDecoder(data, device=args.device).output_order(output_bit_depth=args.output_bit_depth, side=side, residual=resid, compare=cmp, stats=stats, **lad)
    else:      # the same pictures as semi-planar surfaces (xgpu_pic_output_device into a torch tensor, copied to the host picture by picture)
        import torch
        opts = dict(layout="nv12", dtype=torch.uint8) if args.pix_fmt == "nv12" else dict(layout="p016", dtype=torch.int16, out_bit_depth=10)
        pics = StreamDecoder(data, device=args.device).output_order(tensor=opts, side=side, residual=resid, compare=cmp, stats=stats, **lad, **dith, **ovl)
    dt = time.perf_counter() - t0
    if cmp is not None:
        cmp.finish()
    if args.output:
        with open(args.output, "wb") as f:
            for _, frame in pics:
                f.write(frame.tobytes())
    base, ext = os.path.splitext(args.output or "")
    for i, (ww, hh) in enumerate(lad_sizes):
        with open(f"{base}_{ww}x{hh}{ext}", "wb") as f:
            for p, _ in pics:
                f.write(p["surfaces"][i].tobytes())
    if args.side_info:
        with open(args.side_info, "wb") as f:
            for p, _ in sorted(pics, key=lambda t: t[0]["decode_index"]):
                b = p["side_info"]
                f.write(f"{p['poc']} {b.shape[1]} {b.shape[2]}\n".encode())
                f.write(b.astype("<i2").tobytes())
    if args.residual:
        with open(args.residual, "wb") as f:
            for p, _ in sorted(pics, key=lambda t: t[0]["decode_index"]):
                flat, (y, _, _) = p["residual"]
                f.write(f"{p['poc']} {y.shape[1]} {y.shape[0]}\n".encode())
                f.write(flat.astype("<i2").tobytes())
    if args.stats:
        with open(args.stats, "w") as f:
            for p, _ in sorted(pics, key=lambda t: t[0]["decode_index"]):
                f.write(stats_line(p) + "\n")
    print(f"{len(pics)} pictures, {len(pics) / dt:.1f} pictures/s (parse + upload + kernels + download)", file=sys.stderr)


if __name__ == "__main__":
    main()
