"""numpy restatement of the bicubic resize (include/xevd_hip.h xgpu_pic_output_device_resampled / _rois_resampled): the taps with
fractions.Fraction, the two signed integer passes in int64 - the intermediate asserted to stay inside int16 -, then the conversion and the normalise of the
scaled output's restatement (scale_ref on colour_ref / yuv_ref) and the batch by roi_ref's letterbox rule.  Written from the contract, not from the kernel.
`census` (a dict, optional) collects what the tests assert was exercised: the intermediate's and the unclipped second pass' minimum and maximum."""
from fractions import Fraction
import math

import numpy as np

import colour_ref as cr
import roi_ref as rr
import scale_ref as sr
import yuv_ref as yr

CATMULL_ROM, CUBIC_075, MITCHELL = 0, 1, 2
BC = {CATMULL_ROM: (Fraction(0), Fraction(1, 2)), CUBIC_075: (Fraction(0), Fraction(3, 4)), MITCHELL: (Fraction(1, 3), Fraction(1, 3))}
U8, U16, F16, BF16, F32 = sr.U8, sr.U16, sr.F16, sr.BF16, sr.F32
ONE = sr.ONE


def spline(kernel, x):
    """the BC-spline of `kernel` at x"""
    b, c = BC[kernel]
    x = abs(x)
    if x < 1:
        return ((12 - 9 * b - 6 * c) * x ** 3 + (-18 + 12 * b + 6 * c) * x ** 2 + (6 - 2 * b)) / 6
    if x < 2:
        return ((-b - 6 * c) * x ** 3 + (6 * b + 30 * c) * x ** 2 + (-12 * b - 48 * c) * x + (8 * b + 24 * c)) / 6
    return Fraction(0)


def taps(n, s, half, N, kernel, antialias):
    """one axis of one plane: n plane samples, subsampling s, siting half / 2 luma samples, N destination samples -> [(first, [q ...]) per destination sample]"""
    r = Fraction(n * s, N)
    f = max(Fraction(1), Fraction(n, N)) if antialias else Fraction(1)
    d = Fraction(half, 2)
    rows = []
    for o in range(N):
        c = ((o + Fraction(1, 2)) * r - Fraction(1, 2) - d) / s
        idx = [i for i in range(max(math.floor(c - 2 * f) - 1, 0), min(math.ceil(c + 2 * f) + 1, n - 1) + 1) if abs(i - c) < 2 * f]
        if idx:
            assert idx == list(range(idx[0], idx[0] + len(idx)))
            w = [spline(kernel, (i - c) / f) for i in idx]
        else:               # the window lies off the plane: the nearest sample alone
            idx, w = [min(max(math.floor(c + Fraction(1, 2)), 0), n - 1)], [Fraction(1)]
        total = sum(w)
        assert total > 0
        q = [math.floor(v / total * ONE + Fraction(1, 2)) for v in w]
        q[q.index(max(q))] += ONE - sum(q)
        assert sum(abs(v) for v in q) <= 2 * ONE
        rows.append((idx[0], q))
    return rows


def _note(census, key, a):
    if census is not None:
        lo, hi = census.get(key, (int(a.min()), int(a.max())))
        census[key] = (min(lo, int(a.min())), max(hi, int(a.max())))


def vertical(plane, rows):
    """t = (sum qy * sample + 2^11) >> 12 (arithmetic), not clipped"""
    plane = np.asarray(plane, np.int64)
    out = np.zeros((len(rows), plane.shape[1]), np.int64)
    for o, (first, q) in enumerate(rows):
        out[o] = ((np.asarray(q, np.int64)[:, None] * plane[first:first + len(q)]).sum(0) + (1 << 11)) >> 12
    return out


def horizontal(mid, rows):
    """(sum qx * t + 2^15) >> 16 (arithmetic), before the clip"""
    out = np.zeros((mid.shape[0], len(rows)), np.int64)
    for o, (first, q) in enumerate(rows):
        out[:, o] = ((mid[:, first:first + len(q)] * np.asarray(q, np.int64)[None, :]).sum(1) + (1 << 15)) >> 16
    return out


def resize_plane(plane, rows_y, rows_x, bd, census=None):
    mid = vertical(plane, rows_y)
    assert mid.min() >= -32768 and mid.max() <= 32767
    raw = horizontal(mid, rows_x)
    _note(census, "mid", mid)
    _note(census, "raw", raw)
    return np.clip(raw, 0, (1 << bd) - 1)


def make_tables(ws, hs, wd, hd, kernel, antialias, chroma_loc, lib=None):
    """the four tap tables (luma rows, chroma rows, luma columns, chroma columns): from taps(), or - lib given - the library's own"""
    dx, dy = sr.SITING[chroma_loc]
    spec = ((hs, 1, 0, hd), (hs // 2, 2, dy, hd), (ws, 1, 0, wd), (ws // 2, 2, dx, wd))
    if lib is None:
        return [taps(n, s, h, N, kernel, antialias) for n, s, h, N in spec]
    from xevd_amd import abi
    return [sr.table_rows(*abi.resample_taps(lib, n, s, h, N, kernel, antialias)) for n, s, h, N in spec]


def resampled_ycbcr(planes, bd, size, kernel=CATMULL_ROM, antialias=True, chroma_loc=0, crop=(0, 0, 0, 0), dra=None, lib=None, census=None):
    """decoded [Y, U, V] of the whole picture -> Y, Cb, Cr [Hd][Wd] at the coding depth"""
    planes = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        planes = cr.dra_apply(planes, dra)
    y, u, v = (np.clip(p, 0, (1 << bd) - 1) for p in cr.crop_planes(planes, crop))
    hd, wd = size
    hs, ws = y.shape
    yl, yc, xl, xc = make_tables(ws, hs, wd, hd, kernel, antialias, chroma_loc, lib)
    return resize_plane(y, yl, xl, bd, census), resize_plane(u, yc, xc, bd, census), resize_plane(v, yc, xc, bd, census)


def convert(planes, bd, size, layout="rgb", kernel=CATMULL_ROM, antialias=True, matrix=1, full_range=False, chroma_loc=0, dtype=U8, crop=(0, 0, 0, 0), dra=None,
            bgr=False, mean=None, inv_std=None, lib=None, census=None):
    """-> [3][Hd][Wd] in output channel order: uint8 / uint16 for the integer dtypes, float32 (before any f16 / bf16 rounding) otherwise"""
    y, cb, crr = resampled_ycbcr(planes, bd, size, kernel, antialias, chroma_loc, crop, dra, lib, census)
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
        out = sr.normalise(out, np.zeros(3, np.float32) if mean is None else mean, np.ones(3, np.float32) if inv_std is None else inv_std)
    return np.ascontiguousarray(out)


def batch(planes, bd, size, rois, fit=rr.STRETCH, pad=0.0, crop=(0, 0, 0, 0), dtype=U8, mean=None, inv_std=None, **kw):
    """decoded [Y, U, V] of the whole picture -> [N][3][Hd][Wd] in output channel order; rois: (x, y, w, h) inside the picture minus crop; kw: convert's"""
    hd, wd = size
    h, w = np.asarray(planes[0]).shape
    fill = rr.pad_elements(pad, dtype, mean, inv_std)
    out = []
    for x, y, rw, rh in rois:
        ix, iy, wi, hi = rr.inner(rw, rh, wd, hd, fit)
        rect = (crop[0] + x, w - crop[0] - x - rw, crop[2] + y, h - crop[2] - y - rh)      # the rectangle as a crop of the whole picture
        part = convert(planes, bd, (hi, wi), dtype=dtype, crop=rect, mean=mean, inv_std=inv_std, **kw)
        img = np.empty((3, hd, wd), part.dtype)
        img[:] = fill.astype(part.dtype).reshape(3, 1, 1)
        img[:, iy:iy + hi, ix:ix + wi] = part
        out.append(img)
    return np.stack(out)
