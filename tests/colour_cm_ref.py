"""numpy restatement of the colour-managed RGB output (include/xevd_hip.h xgpu_colour_transform), in two parts:
the standards' formulae in float64 (H.273 transfer characteristics and chromaticities, BT.2100 PQ / HLG, the BT.2390 EETF) that the library's tables are
checked against, and the kernel's arithmetic - table lookups and float32 operations rounded one by one - fed with the library's own tables, which the
GPU output must equal bit for bit.  Written from the contract, not from the kernel."""
import math

import numpy as np

import colour_ref

U8, U16, F16, BF16, F32 = 0, 1, 2, 3, 4
CURVE_U0, CURVE_SIZE = 0x1F800000, 64 * 32 + 3

# ---------------------------------------------------------------------------------------------- the standards, float64
A709, B709 = 1.09929682680944, 0.018053968510807
ASRGB, BSRGB = 1.055, 0.0031308
PQ_M1, PQ_M2, PQ_C1, PQ_C2, PQ_C3 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0, 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
HLG_A = 0.17883277
HLG_B = 1.0 - 4.0 * HLG_A
HLG_C = 0.5 - HLG_A * math.log(4.0 * HLG_A)
TRANSFERS = (1, 4, 5, 6, 8, 13, 14, 15, 16, 18)
PRIMARIES = {1: (0.640, 0.330, 0.300, 0.600, 0.150, 0.060), 5: (0.640, 0.330, 0.290, 0.600, 0.150, 0.060), 6: (0.630, 0.340, 0.310, 0.595, 0.155, 0.070),
             7: (0.630, 0.340, 0.310, 0.595, 0.155, 0.070), 9: (0.708, 0.292, 0.170, 0.797, 0.131, 0.046), 12: (0.680, 0.320, 0.265, 0.690, 0.150, 0.060)}
D65 = (0.3127, 0.3290)


def _cls(tc):
    return 1 if tc in (1, 6, 14, 15) else tc


def tc_forward(tc, v):
    """linear light in [0, 1] -> encoded value (the OETF of H.273; 16: the inverse EOTF of ST 2084; 18: the HLG OETF)"""
    v = np.asarray(v, np.float64)
    c = _cls(tc)
    with np.errstate(invalid="ignore", divide="ignore"):
        if c == 1:
            return np.where(v < B709, 4.5 * v, A709 * np.power(v, 0.45) - (A709 - 1.0))
        if c == 4:
            return np.power(v, 1.0 / 2.2)
        if c == 5:
            return np.power(v, 1.0 / 2.8)
        if c == 13:
            return np.where(v < BSRGB, 12.92 * v, ASRGB * np.power(v, 1.0 / 2.4) - (ASRGB - 1.0))
        if c == 16:
            p = np.power(v, PQ_M1)
            return np.power((PQ_C1 + PQ_C2 * p) / (1.0 + PQ_C3 * p), PQ_M2)
        if c == 18:
            return np.where(v <= 1.0 / 12.0, np.sqrt(3.0 * v), HLG_A * np.log(np.maximum(12.0 * v - HLG_B, 1e-300)) + HLG_C)
    return v


def tc_inverse(tc, e):
    """encoded value in [0, 1] -> linear light"""
    e = np.asarray(e, np.float64)
    c = _cls(tc)
    if c == 1:
        return np.where(e < 4.5 * B709, e / 4.5, np.power((e + (A709 - 1.0)) / A709, 1.0 / 0.45))
    if c == 4:
        return np.power(e, 2.2)
    if c == 5:
        return np.power(e, 2.8)
    if c == 13:
        return np.where(e < 12.92 * BSRGB, e / 12.92, np.power((e + (ASRGB - 1.0)) / ASRGB, 2.4))
    if c == 16:
        p = np.power(e, 1.0 / PQ_M2)
        return np.power(np.maximum(p - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * p), 1.0 / PQ_M1)
    if c == 18:
        return np.where(e <= 0.5, e * e / 3.0, (np.exp((e - HLG_C) / HLG_A) + HLG_B) / 12.0)
    return e


def rgb_to_xyz(cp):
    """RGB -> XYZ of H.273 ColourPrimaries cp, white D65 with Y = 1"""
    xr, yr, xg, yg, xb, yb = PRIMARIES[cp]
    p = np.array([[xr / yr, xg / yg, xb / yb], [1.0, 1.0, 1.0], [(1 - xr - yr) / yr, (1 - xg - yg) / yg, (1 - xb - yb) / yb]])
    w = np.array([D65[0] / D65[1], 1.0, (1 - D65[0] - D65[1]) / D65[1]])
    return p * np.linalg.solve(p, w)[None, :]


def primaries_matrix(src, dst):
    return np.linalg.solve(rgb_to_xyz(dst), rgb_to_xyz(src))


def default_peak(tc):
    return 1000.0 if tc in (16, 18) else 100.0


def eetf(lum, lw, lmax):
    """Report BT.2390 section 5.4.1, black levels 0: luminance (cd/m2) on a display of peak lw -> on one of peak lmax"""
    lum = np.asarray(lum, np.float64)
    if lmax >= lw:
        return lum
    pw = float(tc_forward(16, lw / 10000.0))
    max_lum = float(tc_forward(16, lmax / 10000.0)) / pw
    ks = 1.5 * max_lum - 0.5
    e1 = np.minimum(tc_forward(16, lum / 10000.0) / pw, 1.0)
    t = (e1 - ks) / (1.0 - ks)
    t2, t3 = t * t, t * t * t
    p = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * max_lum
    return 10000.0 * tc_inverse(16, np.where(e1 >= ks, p, e1) * pw)


def tone_curve(cm, y):
    """g(Y) of the tone curve of transform cm (a dict as abi.make_colour_transform takes it): source luminance y in [0, 1] -> destination linear light"""
    y = np.asarray(y, np.float64)
    st, dt = _cls(cm["src_transfer"]), _cls(cm["dst_transfer"])
    sp = float(np.float32(cm.get("src_peak", 0.0))) or default_peak(st)
    dp = float(np.float32(cm.get("dst_peak", 0.0))) or default_peak(dt)
    white = 10000.0 if dt == 16 else dp
    if st == 16:
        ld = 10000.0 * y
    elif st == 18:
        ld = sp * np.power(y, 1.2 + 0.42 * math.log10(sp / 1000.0))      # the BT.2100 OOTF on the luminance
    else:
        ld = sp * y
    return eetf(ld, sp, dp) / white


def curve_x():
    """the sample points of entries 1 .. CURVE_SIZE - 2 of a curve table (entry 0 is at 0, the last entry repeats the one before)"""
    return (CURVE_U0 + (np.arange(2049, dtype=np.uint32) << 18)).view(np.float32)


def curve_table64(fn):
    x = curve_x().astype(np.float64)
    t = np.concatenate([[float(fn(np.float64(0.0)))], fn(x)])
    return np.concatenate([t, t[-1:]])


def tables64(cm, bd):
    """what xgpu_colour_tables returns, in float64 straight from the formulae"""
    n = 1 << bd
    same = PRIMARIES[cm["src_primaries"]] == PRIMARIES[cm["dst_primaries"]]
    return {"lin": tc_inverse(cm["src_transfer"], np.arange(n) / float(n - 1)),
            "matrix": np.eye(3) if same else primaries_matrix(cm["src_primaries"], cm["dst_primaries"]), "use_matrix": not same,
            "luma": rgb_to_xyz(cm["src_primaries"])[1], "scale": np.float64(np.float32(cm.get("linear_scale", 1.0) or 1.0)),
            "tone": curve_table64(lambda y: tone_curve(cm, y)) if cm.get("tone_map") else None,
            "encode": curve_table64(lambda v: tc_forward(cm["dst_transfer"], v)) if _cls(cm["dst_transfer"]) != 8 else None}


def exact64(codes, cm, bd):
    """the four steps on R'G'B' codes [3, ...] in float64 with exact pow and no tables -> [3, ...] in [0, 1]"""
    e = tc_inverse(cm["src_transfer"], np.asarray(codes, np.float64) / float((1 << bd) - 1))
    t = tables64(cm, bd)
    p = np.tensordot(t["matrix"], e, axes=(1, 0))
    if cm.get("tone_map"):
        yl = np.clip(np.tensordot(t["luma"], e, axes=(0, 0)), 0.0, 1.0)
        s = np.where(yl > 0, tone_curve(cm, yl) / np.where(yl > 0, yl, 1.0), 0.0)
    else:
        s = t["scale"]
    q = np.clip(p * s, 0.0, 1.0)
    return tc_forward(cm["dst_transfer"], q)


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic, float32
def clip01(v):
    """-0 and NaN -> +0, above 1 -> 1"""
    with np.errstate(invalid="ignore"):
        return np.minimum(np.where(v > 0, v, np.float32(0)), np.float32(1)).astype(np.float32)


def curve_eval(t, v):
    """a curve table at float32 v in [+0, 1]: T[k] + frac * (T[k + 1] - T[k]), every operation rounded to float32"""
    t, v = np.asarray(t, np.float32), np.asarray(v, np.float32)
    u = v.view(np.uint32).astype(np.int64)
    low = u < CURVE_U0
    k = np.where(low, 0, np.minimum(((u - CURVE_U0) >> 18) + 1, CURVE_SIZE - 2))
    fr = np.where(low, v * np.float32(2.0 ** 64), (u & 0x3FFFF).astype(np.float32) * np.float32(2.0 ** -18)).astype(np.float32)
    t0, t1 = t[k], t[k + 1]
    return (t0 + fr * (t1 - t0)).astype(np.float32)


def _dot(m, e):
    m = np.asarray(m, np.float32)
    return ((m[0] * e[0] + m[1] * e[1]) + m[2] * e[2]).astype(np.float32)


def transform(codes, tab, dtype, bd):
    """R'G'B' codes at the coding depth [3, ...] (int) through tables `tab` (abi.colour_tables) -> uint8 / uint16, or float32 before any f16 / bf16 rounding"""
    e = [np.asarray(tab["lin"], np.float32)[np.asarray(c, np.int64)] for c in codes]
    p = [_dot(tab["matrix"][r], e) for r in range(3)] if tab["use_matrix"] else e
    if tab["tone"] is not None:      # g(Y) / Y, one IEEE division; black stays black
        yl = clip01(_dot(tab["luma"], e))
        s = np.where(yl > 0, curve_eval(tab["tone"], yl) / np.where(yl > 0, yl, np.float32(1)), np.float32(0)).astype(np.float32)
    else:
        s = np.float32(tab["scale"])
    out = []
    for c in range(3):
        q = clip01((p[c] * s).astype(np.float32))
        if tab["encode"] is not None:
            q = curve_eval(tab["encode"], q)
        if dtype in (U8, U16):
            m = np.float32((1 << colour_ref.out_depth(dtype, bd)) - 1)
            q = np.rint((q * m).astype(np.float32)).astype(np.uint8 if dtype == U8 else np.uint16)      # round to nearest, ties to even
        out.append(q)
    return np.stack(out)


def convert(planes, bd, tab, matrix=1, full_range=False, chroma_loc=0, mode="linear", dtype=U8, crop=(0, 0, 0, 0), dra=None):
    """decoded [Y, U, V] of the whole picture -> [3][H][W] of the colour-managed contract: colour_ref's U16 R'G'B' codes, then transform"""
    codes = colour_ref.convert(planes, bd, matrix=matrix, full_range=full_range, chroma_loc=chroma_loc, mode=mode, dtype=U16, crop=crop, dra=dra)
    return transform(codes.astype(np.int64), tab, dtype, bd)
