"""numpy restatement of the device-output conversion contract (include/xevd_hip.h xgpu_output_format): DRA, crop,
4:2:0 chroma upsampling, Y'CbCr -> R'G'B' in fixed point (u8 / u16) or float32 (f32 / f16 / bf16).  Written from the contract, not from the kernel."""
import math

import numpy as np

KR_KB = {1: (0.2126, 0.0722), 4: (0.30, 0.11), 5: (0.299, 0.114), 6: (0.299, 0.114), 7: (0.212, 0.087), 9: (0.2627, 0.0593)}
U8, U16, F16, BF16, F32 = 0, 1, 2, 3, 4


def round_half_away(x):
    """round half away from zero, exactly, in double"""
    a = abs(x)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1
    return int(math.copysign(r, x)) if r else 0


def ranges(bd, full_range):
    """(yo, yr, cr): luma offset, luma and chroma excursions at coding depth bd"""
    if full_range:
        return 0, float((1 << bd) - 1), float((1 << bd) - 1)
    return 16 << (bd - 8), float(219 << (bd - 8)), float(224 << (bd - 8))


def _terms(matrix, full_range, bd, m, sc):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    _, yr, cr = ranges(bd, full_range)
    return [m / yr * sc,
            2.0 * (1.0 - kr) * m / cr * sc,
            -(2.0 * kb * (1.0 - kb) / kg * m / cr * sc),
            -(2.0 * kr * (1.0 - kr) / kg * m / cr * sc),
            2.0 * (1.0 - kb) * m / cr * sc]


def out_depth(dtype, bd):
    return 8 if dtype == U8 else bd


def coeffs(matrix, full_range, bd, dtype):
    """-> ([cy, crv, cgu, cgv, cbu], S) of an integer dtype ([0] * 5, 0 for float ones), float32 [cy, crv, cgu, cgv, cbu] with M = 1"""
    f = [np.float32(t) for t in _terms(matrix, full_range, bd, 1.0, 1.0)]
    if dtype not in (U8, U16):
        return [0] * 5, 0, f
    d = out_depth(dtype, bd)
    s = 27 - d
    mags = _terms(matrix, full_range, bd, float((1 << d) - 1), float(1 << s))
    return [round_half_away(t) for t in mags], s, f


def dra_apply(planes, luts):
    """the DRA post-filter (the output kernel's per-sample mapping): chroma scaled around 512 by the factor of the UNMAPPED luma at (2y, 2x), luma through its table"""
    y, u, v = (np.asarray(p, np.int64) for p in planes)
    luts = [np.asarray(t, np.int64) for t in luts]
    out = [luts[0][np.clip(y, 0, 1023)].astype(np.int16).astype(np.int64)]
    lum = y[0::2, 0::2]
    for c, pl in ((1, u), (2, v)):
        sv = pl - 512
        off = (np.abs(sv) * luts[c][np.clip(lum, 0, 1023)] + 256) >> 9
        off = np.where(sv < 0, -off, off)
        out.append((512 + off).astype(np.int16).astype(np.int64))
    return out


# quarter weights of ChromaSampleLocType 0..5: horizontal (even x, odd x) as {offset from j: weight}, vertical (even y, odd y) as {offset from i: weight}
_H_COSITED = ({0: 4}, {0: 2, 1: 2})
_H_CENTRED = ({0: 3, -1: 1}, {0: 3, 1: 1})
_V = {"centre": ({0: 3, -1: 1}, {0: 3, 1: 1}), "top": ({0: 4}, {0: 2, 1: 2}), "bottom": ({-1: 2, 0: 2}, {0: 4})}


def upsample(c, w, h, mode, loc):
    """cropped chroma plane c [h/2][w/2] -> [h][w] at luma resolution, indices clamped to the plane"""
    c = np.asarray(c, np.int64)
    ch, cw = c.shape
    ys, xs = np.arange(h), np.arange(w)
    if mode == "nearest":
        return c[(ys >> 1)[:, None], (xs >> 1)[None, :]]
    hw = _H_CENTRED if loc in (1, 3, 5) else _H_COSITED
    vw = _V["centre" if loc in (0, 1) else ("top" if loc in (2, 3) else "bottom")]
    out = np.zeros((h, w), np.int64)
    for py in range(2):
        rows = ys[py::2]
        i = rows >> 1
        for px in range(2):
            cols = xs[px::2]
            j = cols >> 1
            acc = np.zeros((len(rows), len(cols)), np.int64)
            for di, wv in vw[py].items():
                for dj, wh in hw[px].items():
                    acc += wv * wh * c[np.clip(i + di, 0, ch - 1)[:, None], np.clip(j + dj, 0, cw - 1)[None, :]]
            out[np.ix_(rows, cols)] = (acc + 8) >> 4
    return out


def crop_planes(planes, crop):
    cl, cr, ct, cb = crop
    y, u, v = planes
    h, w = y.shape
    return [y[ct:h - cb, cl:w - cr], u[ct // 2:(h - cb) // 2, cl // 2:(w - cr) // 2], v[ct // 2:(h - cb) // 2, cl // 2:(w - cr) // 2]]


def ycbcr_to_rgb(y, cb, cr, bd, matrix, full_range, dtype):
    """full-resolution Y, Cb, Cr (int) -> [3][h][w] R, G, B: uint8 / uint16 for integer dtypes, float32 (before any f16 / bf16 rounding) otherwise"""
    yo, _, _ = ranges(bd, full_range)
    co = 1 << (bd - 1)
    yy, u, v = np.asarray(y, np.int64) - yo, np.asarray(cb, np.int64) - co, np.asarray(cr, np.int64) - co
    k, s, f = coeffs(matrix, full_range, bd, dtype)
    if dtype in (U8, U16):
        m = (1 << out_depth(dtype, bd)) - 1
        rnd = 1 << (s - 1)
        chans = [k[0] * yy + k[1] * v + rnd, k[0] * yy + k[2] * u + k[3] * v + rnd, k[0] * yy + k[4] * u + rnd]
        return np.stack([np.clip(c >> s, 0, m) for c in chans]).astype(np.uint8 if dtype == U8 else np.uint16)
    fy, fu, fv = f[0] * yy.astype(np.float32), u.astype(np.float32), v.astype(np.float32)
    chans = [fy + f[1] * fv, fy + f[2] * fu + f[3] * fv, fy + f[4] * fu]
    return np.stack([np.clip(c, np.float32(0), np.float32(1)) for c in chans]).astype(np.float32)


def convert(planes, bd, matrix=1, full_range=False, chroma_loc=0, mode="linear", dtype=U8, crop=(0, 0, 0, 0), dra=None):
    """decoded [Y, U, V] of the whole picture -> [3][H][W] R, G, B of the contract"""
    planes = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        planes = dra_apply(planes, dra)
    y, u, v = crop_planes(planes, crop)
    h, w = y.shape
    return ycbcr_to_rgb(y, upsample(u, w, h, mode, chroma_loc), upsample(v, w, h, mode, chroma_loc), bd, matrix, full_range, dtype)


def h273_float64(y, cb, cr, bd, matrix, full_range, d):
    """the same conversion in float64 without fixed point, rounded to D-bit integers"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    yo, yr, crr = ranges(bd, full_range)
    m = (1 << d) - 1
    e_y = (np.asarray(y, np.float64) - yo) / yr
    e_b = (np.asarray(cb, np.float64) - (1 << (bd - 1))) / crr
    e_r = (np.asarray(cr, np.float64) - (1 << (bd - 1))) / crr
    r = e_y + 2 * (1 - kr) * e_r
    b = e_y + 2 * (1 - kb) * e_b
    g = (e_y - kr * r - kb * b) / kg
    return np.stack([np.clip(np.floor(c * m + 0.5), 0, m) for c in (r, g, b)]).astype(np.int64)


def to_f16_bits(f):
    return np.asarray(f, np.float32).astype(np.float16).view(np.uint16)


def to_bf16_bits(f):
    u = np.asarray(f, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
