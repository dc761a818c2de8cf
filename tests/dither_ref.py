"""numpy restatement of the dithered device outputs (include/xevd_hip.h xgpu_dither_params): the three quantisation rules, the Bayer and
the blue-noise constructor and the per-picture phase.  Written from the contract, not from the kernel; everything in front of the final quantisation is
colour_ref's (DRA, crop, chroma upsampling, the matrix' coefficients), colour_cm_ref's (the transform up to its float32 q), yuv_ref's (the surfaces' layout) and
packed_ref's (the 10-bit matrix, the alpha codes)."""
import numpy as np

import colour_cm_ref as cmr
import colour_ref as cr
import packed_ref as pr
import yuv_ref as yr

U8, U16 = cr.U8, cr.U16


# ---------------------------------------------------------------------------------------------- matrices
def bayer(log2n):
    """the recursive Bayer matrix of side 2^log2n, L = n^2: uint16 [n, n]"""
    n = 1 << log2n
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    r = np.zeros((n, n), np.int64)
    for b in range(log2n):
        hi = 2 * (log2n - 1 - b)
        r |= (((x ^ y) >> b) & 1) << (hi + 1)
        r |= ((y >> b) & 1) << hi
    return r.astype(np.uint16)


# floor(2^20 * exp(-d2 / 4.5) + 0.5) by d2 = dx^2 + dy^2, |dx|, |dy| <= 6: the same integers as the library's table
GAUSS = np.array([
    1048576, 839634, 672326, 538357, 431082, 345184, 276402, 221325, 177223, 141909, 113632, 90989, 72859, 58341, 46716, 37407, 29953, 23985, 19205, 15378,
    12314, 9860, 7896, 6322, 5062, 4054, 3246, 2599, 2081, 1667, 1334, 1069, 856, 685, 549, 439, 352, 282, 226, 181, 145, 116, 93, 74, 59, 48, 38, 31, 24, 20,
    16, 13, 10, 8, 6, 5, 4, 3, 3, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], np.int64)


def tie_permutation(nn, seed):
    """Fisher-Yates from the back; before every draw s = s * 6364136223846793005 + 1442695040888963407 mod 2^64 (s0 = seed), j = (s >> 33) % (i + 1)"""
    tie = list(range(nn))
    s = seed & 0xFFFFFFFF
    for i in range(nn - 1, 0, -1):
        s = (s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        j = (s >> 33) % (i + 1)
        tie[i], tie[j] = tie[j], tie[i]
    return np.array(tie, np.int64)


def blue(log2n, seed):
    """greedy void filling on the torus: uint16 [n, n], a permutation of 0 .. n^2 - 1"""
    n = 1 << log2n
    nn = n * n
    d = np.arange(-6, 7)
    kern = GAUSS[d[:, None] ** 2 + d[None, :] ** 2] * nn      # [13, 13], already at the key's scale
    key = tie_permutation(nn, seed).reshape(n, n).copy()      # E * n^2 + tie
    filled = np.int64(1) << 62
    rank = np.zeros((n, n), np.uint16)
    for r in range(nn):
        best = int(np.argmin(key))      # the keys of unfilled cells are distinct
        by, bx = divmod(best, n)
        rank[by, bx] = r
        np.add.at(key, (((by + d) % n)[:, None], ((bx + d) % n)[None, :]), kern)
        key[by, bx] = filled
        key[key >= filled] = filled      # (a filled cell stays above every unfilled one)
    return rank


def phase(index, mw, mh):
    index &= 0xFFFFFFFF
    return ((((index * 0x9E3779B1) & 0xFFFFFFFF) >> 16) & (mw - 1), (((index * 0x85EBCA6B) & 0xFFFFFFFF) >> 16) & (mh - 1))


def low_frequency_share(m):
    """the share of the spectral power of matrix m (mean removed) at 0 < max(|fx|, |fy|) <= n / 8"""
    m = np.asarray(m, np.float64)
    n = m.shape[0]
    p = np.abs(np.fft.fft2(m - m.mean())) ** 2
    f = np.abs(np.fft.fftfreq(n, 1.0 / n))
    r = np.maximum(f[:, None], f[None, :])
    return p[(r > 0) & (r <= n / 8)].sum() / p.sum()


def ranks(m, h, w, ph=(0, 0)):
    """the rank of every pixel of an h x w plane: M[(y + phase_y) & (mh - 1)][(x + phase_x) & (mw - 1)] as int64 [h, w]"""
    m = np.asarray(m, np.int64)
    mh, mw = m.shape
    return m[((np.arange(h) + ph[1]) & (mh - 1))[:, None], ((np.arange(w) + ph[0]) & (mw - 1))[None, :]]


# ---------------------------------------------------------------------------------------------- the three rules
def quantise_sum(s, r, k, shift, maxv):
    """matrix path: clip((sum + (r << (S - k))) >> S, 0, maxv)"""
    assert k <= shift
    return np.clip((s + (r << (shift - k))) >> shift, 0, maxv)


def depth_convert(v, bd, d, r, k):
    """yuv_ref.depth_convert with the rounding constant replaced by (r << shift) >> k; with shift <= 0 the sample is that function's"""
    v = np.asarray(v, np.int64)
    s = bd - d
    if s <= 0:
        return yr.depth_convert(v, bd, d)
    add = (r << s) >> k
    if d == 8:
        return np.clip((v + add) >> s, 0, 255)
    return np.minimum(((v & 0xFFFF) + add) >> s, (1 << d) - 1)


def quantise_cm(q, r, k, outmax):
    """with a transform: min(floor(float32(float32(q * outmax) + r / L)), outmax); r / L is exact in float32"""
    m = np.float32(outmax)
    t = ((np.asarray(q, np.float32) * m).astype(np.float32) + (r.astype(np.float32) * np.float32(2.0 ** -k)).astype(np.float32)).astype(np.float32)
    return np.minimum(np.floor(t).astype(np.int64), int(outmax))


# ---------------------------------------------------------------------------------------------- the outputs
def _sums(planes, bd, k5, matrix, full_range, chroma_loc, mode, crop, dra):
    """the three sums of the matrix before its rounding constant, [3][H][W] int64"""
    pl = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        pl = cr.dra_apply(pl, dra)
    y, u, v = cr.crop_planes(pl, crop)
    h, w = y.shape
    cb, crr = cr.upsample(u, w, h, mode, chroma_loc), cr.upsample(v, w, h, mode, chroma_loc)
    yo, _, _ = cr.ranges(bd, full_range)
    co = 1 << (bd - 1)
    yy, uu, vv = y - yo, cb - co, crr - co
    s = np.stack([k5[0] * yy + k5[1] * vv, k5[0] * yy + k5[2] * uu + k5[3] * vv, k5[0] * yy + k5[4] * uu])
    assert np.abs(s).max() + (1 << 27) < (1 << 31)      # the kernel's int32 holds every sum and the threshold
    return s


def rgb_codes(planes, bd, m, k, ph=(0, 0), d=8, tab=None, matrix=1, full_range=False, chroma_loc=0, mode="linear", crop=(0, 0, 0, 0), dra=None):
    """decoded [Y, U, V] of the whole picture -> [3][H][W] int64 R, G, B codes at depth d (8: U8, the coding depth: U16, 10: RGB10A2) dithered with matrix m of
    2^k levels at phase ph; tab: abi.colour_tables' dict for a colour transform"""
    if tab is not None:
        codes = cr.convert(planes, bd, matrix=matrix, full_range=full_range, chroma_loc=chroma_loc, mode=mode, dtype=U16, crop=crop, dra=dra)
        q = cmr.transform(codes.astype(np.int64), tab, cr.F32, 0)
        return quantise_cm(q, ranks(m, q.shape[1], q.shape[2], ph)[None], k, (1 << d) - 1)
    if d == 10 and bd != 10:
        k5, s = pr.coeffs10(matrix, full_range, bd)
    else:
        k5, s, _ = cr.coeffs(matrix, full_range, bd, U8 if d == 8 else U16)
        if d == 10:
            assert (k5, s) == tuple(pr.coeffs10(matrix, full_range, bd))
    sums = _sums(planes, bd, k5, matrix, full_range, chroma_loc, mode, crop, dra)
    return quantise_sum(sums, ranks(m, sums.shape[1], sums.shape[2], ph)[None], k, s, (1 << d) - 1)


def rgb(planes, bd, m, k, ph=(0, 0), dtype=U8, bgr=False, channels_last=False, **kw):
    """the RGB layouts: [3][H][W] or [H][W][3], uint8 / uint16"""
    c = rgb_codes(planes, bd, m, k, ph, d=8 if dtype == U8 else bd, **kw)
    if bgr:
        c = c[::-1]
    c = c.astype(np.uint8 if dtype == U8 else np.uint16)
    return np.ascontiguousarray(c.transpose(1, 2, 0)) if channels_last else c


def rgba(planes, bd, m, k, ph=(0, 0), dtype=U8, bgr=False, alpha=1.0, **kw):
    """[H][W][4] R G B A (bgr: B G R A), uint8 / uint16; A is the plain call's"""
    c = rgb(planes, bd, m, k, ph, dtype=dtype, bgr=bgr, channels_last=True, **kw)
    a = np.full(c.shape[:2] + (1,), pr.alpha_element(alpha, dtype, bd), c.dtype)
    return np.concatenate([c, a], axis=2)


def rgb10a2(planes, bd, m, k, ph=(0, 0), bgr=False, alpha=1.0, **kw):
    """[H][W] uint32 words R | G << 10 | B << 20 | A << 30 (bgr: B low, R at 20)"""
    c = rgb_codes(planes, bd, m, k, ph, d=10, **kw).astype(np.uint64)
    lo, hi = (c[2], c[0]) if bgr else (c[0], c[2])
    return (lo | (c[1] << 10) | (hi << 20) | (np.uint64(pr.alpha_code(alpha, 2)) << 30)).astype(np.uint32)


def nv12(planes, bd, d, m, k, ph=(0, 0), crop=(0, 0, 0, 0), dra=None, dtype=None):
    """yuv_ref.nv12 with the dithered depth conversion: luma by its position, chroma by its chroma-plane position, Cb and Cr alike"""
    y, u, v = yr._prepared(planes, crop, dra)
    h, w = y.shape
    out = np.zeros((h * 3 // 2, w), np.int64)
    out[:h] = depth_convert(y, bd, d, ranks(m, h, w, ph), k)
    rc = ranks(m, h // 2, w // 2, ph)
    out[h:, 0::2] = depth_convert(u, bd, d, rc, k)
    out[h:, 1::2] = depth_convert(v, bd, d, rc, k)
    return out.astype(dtype or (np.uint8 if d == 8 else np.uint16))


def p016(planes, bd, d, m, k, ph=(0, 0), crop=(0, 0, 0, 0), dra=None):
    return (nv12(planes, bd, d, m, k, ph, crop, dra, np.uint16).astype(np.int64) << (16 - d)).astype(np.uint16)
