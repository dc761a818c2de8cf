"""numpy restatement of the scaled device output (include/xevd_hip.h xgpu_pic_output_device_scaled): the taps with
fractions.Fraction, the two integer passes in int64, the conversion of the unscaled contract (colour_ref / yuv_ref) and the normalise in float32, one
operation at a time.  Written from the contract, not from the kernel."""
from fractions import Fraction
import math

import numpy as np

import colour_ref as cr
import yuv_ref as yr

BILINEAR, AREA = 0, 1
U8, U16, F16, BF16, F32 = cr.U8, cr.U16, cr.F16, cr.BF16, cr.F32
ONE = 16384
# ChromaSampleLocType -> (dx, dy) in half luma samples
SITING = {0: (0, 1), 1: (1, 1), 2: (0, 0), 3: (1, 0), 4: (0, 2), 5: (1, 2)}


def taps(n, s, half, N, filt, outputs=None):
    """one axis of one plane: n plane samples, subsampling s, siting half / 2 luma samples, N destination samples -> [(first, [q ...]) per destination sample]
    (outputs: of these destination samples only)"""
    r = Fraction(n * s, N)
    f = max(Fraction(1), r / s)
    d = Fraction(half, 2)
    rows = []
    for o in (range(N) if outputs is None else outputs):
        c = ((o + Fraction(1, 2)) * r - Fraction(1, 2) - d) / s
        reach = f if filt == BILINEAR else (f + 1) / 2
        ws = {}
        for i in range(max(math.floor(c - reach) - 1, 0), min(math.ceil(c + reach) + 1, n - 1) + 1):
            if filt == BILINEAR:
                w = 1 - abs(i - c) / f
            else:
                w = min(i + Fraction(1, 2), c + f / 2) - max(i - Fraction(1, 2), c - f / 2)
            if w > 0:
                ws[i] = w
        if not ws:          # the window lies off the plane: the nearest sample alone
            ws = {min(max(math.floor(c + Fraction(1, 2)), 0), n - 1): Fraction(1)}
        idx = sorted(ws)
        assert idx == list(range(idx[0], idx[0] + len(idx)))
        total = sum(ws.values())
        q = [math.floor(ws[i] / total * ONE + Fraction(1, 2)) for i in idx]
        q[q.index(max(q))] += ONE - sum(q)
        rows.append((idx[0], q))
    return rows


def table_rows(first, count, w):
    """the library's arrays (abi.scale_taps) as taps() returns them"""
    return [(int(first[o]), [int(v) for v in w[o, :count[o]]]) for o in range(len(first))]


def vertical(plane, rows):
    """t = (sum qy * sample + 2^10) >> 11"""
    plane = np.asarray(plane, np.int64)
    out = np.zeros((len(rows), plane.shape[1]), np.int64)
    for o, (first, q) in enumerate(rows):
        out[o] = ((np.asarray(q, np.int64)[:, None] * plane[first:first + len(q)]).sum(0) + (1 << 10)) >> 11
    return out


def horizontal(mid, rows):
    """v = (sum qx * t + 2^16) >> 17"""
    out = np.zeros((mid.shape[0], len(rows)), np.int64)
    for o, (first, q) in enumerate(rows):
        out[:, o] = ((mid[:, first:first + len(q)] * np.asarray(q, np.int64)[None, :]).sum(1) + (1 << 16)) >> 17
    return out


def resize_plane(plane, rows_y, rows_x):
    mid = vertical(plane, rows_y)
    assert mid.min() >= 0 and mid.max() <= 0xFFFF
    return horizontal(mid, rows_x)


def make_tables(ws, hs, wd, hd, filt, chroma_loc, lib=None):
    """the four tap tables (luma rows, chroma rows, luma columns, chroma columns): from taps(), or - lib given - the library's own"""
    dx, dy = SITING[chroma_loc]
    spec = ((hs, 1, 0, hd), (hs // 2, 2, dy, hd), (ws, 1, 0, wd), (ws // 2, 2, dx, wd))
    if lib is None:
        return [taps(n, s, h, N, filt) for n, s, h, N in spec]
    from xevd_amd import abi
    return [table_rows(*abi.scale_taps(lib, n, s, h, N, filt)) for n, s, h, N in spec]


def scaled_ycbcr(planes, bd, size, filt=BILINEAR, chroma_loc=0, crop=(0, 0, 0, 0), dra=None, lib=None):
    """decoded [Y, U, V] of the whole picture -> Y, Cb, Cr [Hd][Wd] at the coding depth"""
    planes = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        planes = cr.dra_apply(planes, dra)
    y, u, v = (np.clip(p, 0, (1 << bd) - 1) for p in cr.crop_planes(planes, crop))
    hd, wd = size
    hs, ws = y.shape
    yl, yc, xl, xc = make_tables(ws, hs, wd, hd, filt, chroma_loc, lib)
    return resize_plane(y, yl, xl), resize_plane(u, yc, xc), resize_plane(v, yc, xc)


def normalise(x, mean, inv_std):
    """[3][H][W] float32, channel k: (x - mean[k]) * inv_std[k], two float32 roundings"""
    m, i = np.asarray(mean, np.float32).reshape(3, 1, 1), np.asarray(inv_std, np.float32).reshape(3, 1, 1)
    return ((np.asarray(x, np.float32) - m).astype(np.float32) * i).astype(np.float32)


def convert(planes, bd, size, layout="rgb", filt=BILINEAR, matrix=1, full_range=False, chroma_loc=0, dtype=U8, crop=(0, 0, 0, 0), dra=None, bgr=False,
            mean=None, inv_std=None, lib=None):
    """-> [3][Hd][Wd] in output channel order: uint8 / uint16 for the integer dtypes, float32 (before any f16 / bf16 rounding) otherwise"""
    y, cb, crr = scaled_ycbcr(planes, bd, size, filt, chroma_loc, crop, dra, lib)
    if layout == "rgb":
        out = cr.ycbcr_to_rgb(y, cb, crr, bd, matrix, full_range, dtype)
    elif dtype == U8:
        out = np.stack([yr.depth_convert(p, bd, 8) for p in (y, cb, crr)]).astype(np.uint8)
    elif dtype == U16:
        out = np.stack([y, cb, crr]).astype(np.uint16)
    else:
        out = yr.normalised(y, cb, crr, bd, full_range)
    if bgr:
        out = out[::-1]
    if mean is not None or inv_std is not None:
        assert dtype not in (U8, U16)
        out = normalise(out, np.zeros(3, np.float32) if mean is None else mean, np.ones(3, np.float32) if inv_std is None else inv_std)
    return np.ascontiguousarray(out)
