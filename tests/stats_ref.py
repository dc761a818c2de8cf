"""numpy restatement of the picture-statistics contract (include/xevd_hip.h xgpu_pic_stats): the census, the histogram, the
percentile rule, max(R', G', B') and the light level.  Written from the contract, not from the kernel.  Planes are [Y, U, V] arrays of 16-bit patterns (int16 or
uint16) of the whole picture; `lin` is the table xgpu_stats_lin returns (abi.stats_lin)."""
import numpy as np

import colour_ref


def crop_plane(plane, crop, c):
    """the cropped plane of component c as unsigned 16-bit patterns"""
    cl, cr, ct, cb = (v >> (c > 0) for v in crop)
    p = np.ascontiguousarray(plane).view(np.uint16)
    return p[ct:p.shape[0] - cb, cl:p.shape[1] - cr]


def census(s):
    """one cropped plane (uint16) -> n, sum, sum_sq, min, max as Python ints (exact for any contents)"""
    v = s.astype(np.uint64).reshape(-1)
    return {"n": int(v.size), "sum": int(v.sum()), "sum_sq": int((v * v).sum()), "min": int(v.min()), "max": int(v.max())}


def histogram(s, bd, hist_bits):
    """bin = min(s >> (bd - hist_bits), 2^hist_bits - 1), counted: uint32 [2^hist_bits]"""
    nb = 1 << hist_bits
    b = np.minimum(s.astype(np.int64) >> (bd - hist_bits), nb - 1).reshape(-1)
    return np.bincount(b, minlength=nb).astype(np.uint32)


def percentile_bin(hist, p_e4):
    """the smallest bin b with cum(b) * 10000 >= max(p_e4 * n, 1), in Python integers"""
    n = int(hist.astype(np.uint64).sum())
    t = max(p_e4 * n, 1)
    cum = 0
    for b, cnt in enumerate(hist.tolist()):
        cum += cnt
        if cum * 10000 >= t:
            return b
    raise AssertionError("empty histogram")


def max_rgb(planes, bd, crop=(0, 0, 0, 0), matrix=1, full_range=False, chroma_loc=0, upsample="linear"):
    """m per luma sample of the cropped picture: the largest of the three U16 elements of the RGB output (colour_ref.convert), a code in 0 .. 2^bd - 1"""
    signed = [np.ascontiguousarray(p).view(np.int16) for p in planes]      # the RGB output reads the slot's samples as int16
    rgb = colour_ref.convert(signed, bd, matrix=matrix, full_range=full_range, chroma_loc=chroma_loc, mode=upsample, dtype=colour_ref.U16, crop=crop)
    return rgb.max(axis=0)


def light_sum(count, lin):
    """the contract's order in binary64, every operation rounded once: 64 partial sums over k = l, l + 64, ... ascending, then added left to right"""
    count, lin = np.asarray(count), np.asarray(lin, np.float32)
    part = [np.float64(0.0)] * 64
    for k in range(count.size):
        part[k & 63] = part[k & 63] + np.float64(int(count[k])) * np.float64(lin[k])
    total = part[0]
    for l in range(1, 64):
        total = total + part[l]
    return np.float64(total)


def stats(planes, bd, crop=(0, 0, 0, 0), hist_bits=8, pctl_e4=(100, 9999), light=None, lin=None):
    """the whole result: dict of n, sum, sum_sq, min, max (lists of 3 ints), pctl (3 pairs), hist (uint32 [3, 2^hist_bits] or None) and the light fields -
    light_hist (uint32 [2^bd]) or None, light_n, light_max_code, light_pctl_code, light_max, light_pctl (np.float32), light_sum, light_mean (np.float64); all 0
    without light.  light: dict(matrix=, full_range=, chroma_loc=, upsample=) for max_rgb, with `lin` the float32 table of the transfer"""
    cropped = [crop_plane(p, crop, c) for c, p in enumerate(planes)]
    cs = [census(s) for s in cropped]
    d = {k: [c[k] for c in cs] for k in ("n", "sum", "sum_sq", "min", "max")}
    d["hist"], d["pctl"] = None, [[0, 0] for _ in range(3)]
    if hist_bits:
        d["hist"] = np.stack([histogram(s, bd, hist_bits) for s in cropped])
        d["pctl"] = [[percentile_bin(d["hist"][c], p) << (bd - hist_bits) for p in pctl_e4] for c in range(3)]
    d.update(light_hist=None, light_n=0, light_max_code=0, light_pctl_code=[0, 0], light_max=np.float32(0), light_pctl=[np.float32(0)] * 2,
             light_sum=np.float64(0), light_mean=np.float64(0))
    if light is not None:
        opts = {k: v for k, v in light.items() if k != "transfer"}
        m = max_rgb(planes, bd, crop=crop, **opts)
        h = np.bincount(m.reshape(-1).astype(np.int64), minlength=1 << bd).astype(np.uint32)
        lin = np.asarray(lin, np.float32)
        d["light_hist"], d["light_n"] = h, int(m.size)
        d["light_max_code"] = int(np.nonzero(h)[0][-1])
        d["light_pctl_code"] = [percentile_bin(h, p) for p in pctl_e4]
        d["light_max"], d["light_pctl"] = lin[d["light_max_code"]], [lin[c] for c in d["light_pctl_code"]]
        d["light_sum"] = light_sum(h, lin)
        d["light_mean"] = d["light_sum"] / np.float64(d["light_n"])
    return d
