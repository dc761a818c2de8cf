#!/usr/bin/env python3
"""Decode an MPEG-5 EVC Baseline bitstream on the MI355X and write planar YUV - the counterpart of the reference's sample
application (app/xevd_app.c: -i in.evc -o out.yuv --output-bit-depth N).  usage: xevd_gpu_app.py -i in.evc -o out.yuv
--pix-fmt nv12 / p010 writes semi-planar frames instead (what a raw-video reader takes as nv12 / p010le): 8-bit samples, or 10-bit samples in the
high bits of 16-bit words, whatever the stream's depth."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xevd_amd.player import StreamDecoder      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--input", required=True)
    ap.add_argument("-o", "--output")
    ap.add_argument("--output-bit-depth", type=int, default=0, help="0 = the stream's bit depth (8 -> bytes, else 16-bit little endian)")
    ap.add_argument("--pix-fmt", choices=("yuv420p", "nv12", "p010"), default="yuv420p",
                    help="nv12: 8-bit semi-planar; p010: 10 bit in 16-bit little-endian words, semi-planar (both ignore --output-bit-depth)")
    ap.add_argument("--to", default=None, help="write interleaved 8-bit RGB frames in this colour space instead (srgb, bt709, pq-bt2020, ...: "
                    "StreamDecoder.COLOUR_PRESETS), converted on the device from the primaries / transfer characteristics of the stream's VUI")
    ap.add_argument("--side-info", default=None, metavar="FILE", help="also write the coding side information of every picture, in DECODING order: a text line "
                    "'POC h_scu w_scu', then nine planes of h_scu x w_scu little-endian int16 (list 0 / 1 vectors, POC distances, mode, QP, flags: INTEGRATION.md 8c)")
    ap.add_argument("--residual", default=None, metavar="FILE", help="also write the prediction residual of every picture, in DECODING order: a text line "
                    "'POC w h', then the little-endian int16 planes Y (h x w), Cb, Cr (h/2 x w/2 each) of the uncropped picture (INTEGRATION.md 8g)")
    ap.add_argument("--size", default=None, metavar="WxH", help="write interleaved 8-bit RGB frames resized to W x H on the device instead (antialiased bilinear, "
                    "the matrix / range / chroma siting of the stream's VUI: INTEGRATION.md 8d); with --to: not supported")
    ap.add_argument("--tiles", default=None, metavar="WxH", help="with --size: every picture as its grid of W x H tiles (the last column / row moved back inside the "
                    "picture), each resized to --size by one call per picture (INTEGRATION.md 8e); the frames written are the tiles, row by row")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.tiles is not None and args.size is None:
        ap.error("--tiles: needs --size")
    data = open(args.input, "rb").read()
    t0 = time.perf_counter()
    side = {} if args.side_info else None
    resid = {} if args.residual else None
    # crop-free output like the reference application; bit-depth conversion and plane packing run on the device (xgpu_pic_output)
    if args.size is not None:
        import torch
        if args.to is not None:
            ap.error("--size: the scaled output takes no colour transform (--to)")
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
        pics = StreamDecoder(data, device=args.device).output_order(tensor=dict(layout="rgb", channels_last=True, dtype=torch.uint8), size=(hd, wd), side=side, rois=rois, residual=resid)
    elif args.to is not None:
        import torch
        pics = StreamDecoder(data, device=args.device).output_order(tensor=dict(layout="rgb", channels_last=True, dtype=torch.uint8), to=args.to, side=side, residual=resid)
    elif args.pix_fmt == "yuv420p":
        pics = StreamDecoder(data, device=args.device).output_order(output_bit_depth=args.output_bit_depth, side=side, residual=resid)
    else:      # the same pictures as semi-planar surfaces (xgpu_pic_output_device into a torch tensor, copied to the host picture by picture)
        import torch
        opts = dict(layout="nv12", dtype=torch.uint8) if args.pix_fmt == "nv12" else dict(layout="p016", dtype=torch.int16, out_bit_depth=10)
        pics = StreamDecoder(data, device=args.device).output_order(tensor=opts, side=side, residual=resid)
    dt = time.perf_counter() - t0
    if args.output:
        with open(args.output, "wb") as f:
            for _, frame in pics:
                f.write(frame.tobytes())
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
    print(f"{len(pics)} pictures, {len(pics) / dt:.1f} pictures/s (parse + upload + kernels + download)", file=sys.stderr)


if __name__ == "__main__":
    main()
