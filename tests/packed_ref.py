"""numpy restatement of the packed display surfaces (include/xevd_hip.h xgpu_packed_format): RGBA, 10:10:10:2 and packed 4:2:2.
Written from the contract, not from the kernel; DRA, crop, chroma upsampling and the matrix are colour_ref's, the colour transform is colour_cm_ref's and the depth
conversion is yuv_ref's."""
import math

import numpy as np

import colour_cm_ref as cmr
import colour_ref as cr
import yuv_ref as yr

U8, U16, F16, BF16, F32 = cr.U8, cr.U16, cr.F16, cr.BF16, cr.F32
RGBA, RGB10A2, YUYV, UYVY = 0, 1, 2, 3


def alpha_code(alpha, d):
    """floor(alpha * (2^d - 1) + 0.5) in double"""
    return int(math.floor(float(np.float32(alpha)) * float((1 << d) - 1) + 0.5))


def alpha_element(alpha, dtype, bd):
    """the A element of RGBA as the bits the dtype stores: the integer code (D = 8 for U8, else the coding depth), or float32(alpha) through the dtype's rounding"""
    if dtype in (U8, U16):
        return alpha_code(alpha, 8 if dtype == U8 else bd)
    f = np.float32(alpha)
    if dtype == F32:
        return int(f.view(np.uint32))
    return int(cr.to_f16_bits(f)) if dtype == F16 else int(cr.to_bf16_bits(f))


def coeffs10(matrix, full_range, bd):
    """-> ([cy, crv, cgu, cgv, cbu], 17): section 8a's integer rule with D = 10 whatever the coding depth - colour_ref.coeffs' expressions, term for term"""
    return [cr.round_half_away(t) for t in cr._terms(matrix, full_range, bd, float(1023), float(1 << 17))], 17


def rgb10_codes(y, cb, crr, bd, matrix, full_range):
    """full-resolution Y, Cb, Cr at the coding depth -> [3][h][w] 10-bit R, G, B codes"""
    yo, _, _ = cr.ranges(bd, full_range)
    co = 1 << (bd - 1)
    yy, u, v = np.asarray(y, np.int64) - yo, np.asarray(cb, np.int64) - co, np.asarray(crr, np.int64) - co
    k, s = coeffs10(matrix, full_range, bd)
    rnd = 1 << (s - 1)
    chans = [k[0] * yy + k[1] * v + rnd, k[0] * yy + k[2] * u + k[3] * v + rnd, k[0] * yy + k[4] * u + rnd]
    assert all(np.abs(c).max() < (1 << 31) for c in chans)      # the kernel's int32 holds every sum
    return np.stack([np.clip(c >> s, 0, 1023) for c in chans])


def transform10(codes, tab):
    """colour_cm_ref.transform with the store rint(q * 1023): R'G'B' codes at the coding depth [3, ...] through tables `tab` -> 10-bit codes"""
    q = cmr.transform(codes, tab, F32, 0)
    return np.rint((q * np.float32(1023)).astype(np.float32)).astype(np.int64)


def rgb10a2(planes, bd, matrix=1, full_range=False, chroma_loc=0, mode="linear", crop=(0, 0, 0, 0), dra=None, bgr=False, alpha=1.0, tab=None):
    """decoded [Y, U, V] of the whole picture -> [H][W] uint32 words R | G << 10 | B << 20 | A << 30 (bgr: B low, R at 20); tab: abi.colour_tables' dict for a
    colour transform - then the U16 code at the coding depth goes through it"""
    if tab is not None:
        codes = cr.convert(planes, bd, matrix=matrix, full_range=full_range, chroma_loc=chroma_loc, mode=mode, dtype=U16, crop=crop, dra=dra)
        c = transform10(codes.astype(np.int64), tab)
    else:
        pl = [np.asarray(p, np.int64) for p in planes]
        if dra is not None:
            pl = cr.dra_apply(pl, dra)
        y, u, v = cr.crop_planes(pl, crop)
        h, w = y.shape
        c = rgb10_codes(y, cr.upsample(u, w, h, mode, chroma_loc), cr.upsample(v, w, h, mode, chroma_loc), bd, matrix, full_range)
    c = c.astype(np.uint64)
    lo, hi = (c[2], c[0]) if bgr else (c[0], c[2])
    return (lo | (c[1] << 10) | (hi << 20) | (np.uint64(alpha_code(alpha, 2)) << 30)).astype(np.uint32)


_VERTICAL = {0: ((1, 3), (3, 1)), 1: ((0, 4), (2, 2)), 2: ((2, 2), (4, 0))}      # chroma_loc >> 1: centred, top, bottom - (ve0, ve1), (vo0, vo1)


def chroma_full_height(c, mode, chroma_loc):
    """cropped chroma plane [ch][cw] -> [2 ch][cw]: row r from the rows around i = r >> 1, edge-clamped"""
    c = np.asarray(c, np.int64)
    ch = c.shape[0]
    i = np.arange(ch)
    out = np.zeros((2 * ch, c.shape[1]), np.int64)
    if mode == "nearest":
        out[0::2] = out[1::2] = c
        return out
    ve, vo = _VERTICAL[chroma_loc >> 1]
    out[0::2] = (ve[0] * c[np.maximum(i - 1, 0)] + ve[1] * c + 2) >> 2
    out[1::2] = (vo[0] * c + vo[1] * c[np.minimum(i + 1, ch - 1)] + 2) >> 2
    return out


def yuv422(planes, bd, d, dtype=U8, uyvy=False, chroma_loc=0, mode="linear", crop=(0, 0, 0, 0), dra=None):
    """decoded [Y, U, V] of the whole picture -> [H][W][2] uint8 (d = 8, dtype U8) or uint16 words sample << (16 - d): pixel x holds Y and Cb (even x) or Cr
    (odd x) - the luma sample first for YUYV, second for UYVY"""
    pl = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        pl = cr.dra_apply(pl, dra)
    y, u, v = cr.crop_planes(pl, crop)
    h, w = y.shape
    ys = yr.depth_convert(y, bd, d)
    cb = yr.depth_convert(chroma_full_height(u, mode, chroma_loc), bd, d)
    crr = yr.depth_convert(chroma_full_height(v, mode, chroma_loc), bd, d)
    out = np.zeros((h, w, 2), np.int64)
    out[:, :, 1 if uyvy else 0] = ys
    out[:, 0::2, 0 if uyvy else 1] = cb
    out[:, 1::2, 0 if uyvy else 1] = crr
    if dtype == U8:
        assert d == 8
        return out.astype(np.uint8)
    return ((out << (16 - d)) & 0xFFFF).astype(np.uint16)
