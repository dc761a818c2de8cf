"""numpy restatement of the remapped output (include/xevd_hip.h xgpu_pic_output_device_remap): the float32 -> Q16 conversion of a
node, the mesh interpolation, the derivatives and the validity of a pixel in int64; then warp_ref's bilinear gather, and the conversion and normalise that
warp_ref uses (colour_ref / yuv_ref / scale_ref), taken by import.  The three host helpers (xgpu_remap_from_warp, _from_homography, _from_lens) are restated in
Python floats, which are IEEE doubles evaluated operation by operation.  Written from the contract, not from the kernel."""
import math

import numpy as np

import colour_ref as cr
import roi_ref as rr
import scale_ref as sr
import warp_ref as wr
import yuv_ref as yr

CLAMP, PAD = wr.CLAMP, wr.PAD
U8, U16, F16, BF16, F32 = sr.U8, sr.U16, sr.F16, sr.BF16, sr.F32
INVALID = -(1 << 31)
I32_MAX = (1 << 31) - 1


def grid_dims(size, k):
    """(gh, gw) of the grid of an image of size = (H, W) with a node every 2^k pixels"""
    assert 0 <= k <= 6
    return tuple(((d - 1) >> k) + 1 + (k > 0) for d in size)


def nodes_q16(grid):
    """one grid [gh, gw, 2], int32 (Q16) or float32 (luma samples) -> (int64 Q16 [gh, gw, 2], valid [gh, gw])"""
    grid = np.asarray(grid)
    if grid.dtype == np.float32:
        valid = np.isfinite(grid).all(axis=-1)
        c = np.minimum(np.maximum(np.where(np.isfinite(grid), grid, np.float32(0)), np.float32(-32767.0)), np.float32(32767.0))
        q = np.rint(c * np.float32(65536.0))
        assert q.dtype == np.float32
        return q.astype(np.int64), valid
    assert grid.dtype == np.int32
    return grid.astype(np.int64), (grid != INVALID).all(axis=-1)


def positions(grid, size, k, samples):
    """-> X, Y, (D0x, D0y, D1x, D1y) (zeros for samples = 1), ok: per destination pixel, int64 / bool [H, W]"""
    hd, wd = size
    q, valid = nodes_q16(grid)
    assert q.shape == (*grid_dims(size, k), 2)
    ox, oy = np.meshgrid(np.arange(wd, dtype=np.int64), np.arange(hd, dtype=np.int64))
    zero = np.zeros((hd, wd), np.int64)
    if k == 0:
        P, ok = q[oy, ox], valid[oy, ox]
        d = [zero] * 4
        if samples > 1:
            xa, ya = np.minimum(ox, wd - 2), np.minimum(oy, hd - 2)
            d0, d1 = q[oy, xa + 1] - q[oy, xa], q[ya + 1, ox] - q[ya, ox]
            ok = ok & valid[oy, xa + 1] & valid[oy, xa] & valid[ya + 1, ox] & valid[ya, ox]
            d = [d0[..., 0], d0[..., 1], d1[..., 0], d1[..., 1]]
        return P[..., 0], P[..., 1], d, ok
    M = 1 << k
    i, fx, j, fy = ox >> k, ox & (M - 1), oy >> k, oy & (M - 1)
    assert int(i.max()) + 1 <= q.shape[1] - 1 and int(j.max()) + 1 <= q.shape[0] - 1
    p00, p01, p10, p11 = q[j, i], q[j, i + 1], q[j + 1, i], q[j + 1, i + 1]
    ok = valid[j, i] & valid[j, i + 1] & valid[j + 1, i] & valid[j + 1, i + 1]
    rnd = 1 << (2 * k - 1)
    pos, d = [], []
    for c in range(2):
        v00, v01, v10, v11 = p00[..., c], p01[..., c], p10[..., c], p11[..., c]
        pos.append(((M - fx) * (M - fy) * v00 + fx * (M - fy) * v01 + (M - fx) * fy * v10 + fx * fy * v11 + rnd) >> (2 * k))
        if samples > 1:
            d.append((((M - fy) * (v01 - v00) + fy * (v11 - v10) + rnd) >> (2 * k), ((M - fx) * (v10 - v00) + fx * (v11 - v01) + rnd) >> (2 * k)))
        else:
            d.append((zero, zero))
    return pos[0], pos[1], [d[0][0], d[1][0], d[0][1], d[1][1]], ok


def remapped_ycbcr(planes, bd, size, grid, k=0, samples=1, chroma_loc=0, crop=(0, 0, 0, 0), dra=None):
    """decoded [Y, U, V] of the whole picture and one grid -> (Y, Cb, Cr [Hd][Wd] at the coding depth, outside [Hd][Wd]: the pixels XGPU_WARP_PAD pads,
    invalid [Hd][Wd]: the pixels that are pad under either border)"""
    planes = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        planes = cr.dra_apply(planes, dra)
    y, u, v = (np.clip(p, 0, (1 << bd) - 1) for p in cr.crop_planes(planes, crop))
    hs, ws = y.shape
    assert samples in (1, 2, 4)
    S, ls = samples, {1: 0, 2: 1, 4: 2}[samples]
    sh, sv = sr.SITING[chroma_loc]
    X, Y, (D0x, D0y, D1x, D1y), ok = positions(grid, size, k, samples)
    x0, y0 = (X + 128) >> 8, (Y + 128) >> 8
    outside = (x0 < 0) | (x0 > (ws - 1) << 8) | (y0 < 0) | (y0 > (hs - 1) << 8)
    acc = [np.zeros(size, np.int64) for _ in range(3)]
    for j in range(S):
        for i in range(S):
            Xs = X + ((D0x * (2 * i + 1 - S) + D1x * (2 * j + 1 - S)) >> (ls + 1))
            Ys = Y + ((D0y * (2 * i + 1 - S) + D1y * (2 * j + 1 - S)) >> (ls + 1))
            acc[0] += wr._bilinear(y, np.clip((Xs + 128) >> 8, 0, (ws - 1) << 8), np.clip((Ys + 128) >> 8, 0, (hs - 1) << 8))
            xc = np.clip((Xs - sh * 32768 + 256) >> 9, 0, (ws // 2 - 1) << 8)
            yc = np.clip((Ys - sv * 32768 + 256) >> 9, 0, (hs // 2 - 1) << 8)
            acc[1] += wr._bilinear(u, xc, yc)
            acc[2] += wr._bilinear(v, xc, yc)
    assert max(int(a.max()) for a in acc) < 1 << 32
    return [(a + (1 << (15 + 2 * ls))) >> (16 + 2 * ls) for a in acc], outside, ~ok


def batch(planes, bd, size, grids, k=0, samples=1, border=CLAMP, pad=0.0, layout="rgb", matrix=1, full_range=False, chroma_loc=0, dtype=U8, crop=(0, 0, 0, 0),
          dra=None, bgr=False, mean=None, inv_std=None):
    """decoded [Y, U, V] of the whole picture and grids [N][gh][gw][2] (int32 or float32) -> [N][3][Hd][Wd] in output channel order (uint8 / uint16, or float32
    before any f16 / bf16 rounding)"""
    fill = rr.pad_elements(pad, dtype, mean, inv_std)
    out = []
    for grid in grids:
        (y, cb, crr), outside, invalid = remapped_ycbcr(planes, bd, size, grid, k, samples, chroma_loc, crop, dra)
        if layout == "rgb":
            img = cr.ycbcr_to_rgb(y, cb, crr, bd, matrix, full_range, dtype)
        elif dtype == U8:
            img = np.stack([yr.depth_convert(p, bd, 8) for p in (y, cb, crr)]).astype(np.uint8)
        elif dtype == U16:
            img = np.stack([y, cb, crr]).astype(np.uint16)
        else:
            img = yr.normalised(y, cb, crr, bd, full_range)
        if bgr:
            img = img[::-1]
        if mean is not None or inv_std is not None:
            assert dtype not in (U8, U16)
            img = sr.normalise(img, np.zeros(3, np.float32) if mean is None else mean, np.ones(3, np.float32) if inv_std is None else inv_std)
        padded = invalid | outside if border == PAD else invalid
        out.append(np.where(padded[None], fill.astype(img.dtype).reshape(3, 1, 1), np.ascontiguousarray(img)))
    return np.stack(out)


# ---- the host helpers
def _q16(x, y):
    """a helper's node from luma samples: non-finite -> invalid, else llround of the clamped product"""
    tx, ty = x * 65536.0, y * 65536.0
    if not (math.isfinite(tx) and math.isfinite(ty)):
        return (INVALID, INVALID)
    return tuple(wr._llround(min(max(t, -2147483647.0), 2147483647.0)) for t in (tx, ty))


def _fill(size, k, node):
    gh, gw = grid_dims(size, k)
    g = np.empty((gh, gw, 2), np.int32)
    for j in range(gh):
        for i in range(gw):
            g[j, i] = node(i << k, j << k)
    return g


def from_warp(m, size, k=0):
    m = [int(v) for v in m]
    assert wr.map_ok(m)
    return _fill(size, k, lambda ox, oy: (min(max(m[0] * ox + m[1] * oy + m[2], -I32_MAX), I32_MAX), min(max(m[3] * ox + m[4] * oy + m[5], -I32_MAX), I32_MAX)))


def from_homography(h, size, k=0):
    h = [float(v) for v in np.asarray(h, np.float64).reshape(9)]

    def node(ox, oy):
        u, v = ox + 0.5, oy + 0.5
        den = h[6] * u + h[7] * v + h[8]
        if not den > 0.0:
            return (INVALID, INVALID)
        return _q16((h[0] * u + h[1] * v + h[2]) / den - 0.5, (h[3] * u + h[4] * v + h[5]) / den - 0.5)
    return _fill(size, k, node)


def from_lens(lens, size, k=0):
    d = dict(lens)
    for n in ("fx", "fy", "cx", "cy"):
        d.setdefault("n" + n, d[n])
    fx, fy, cx, cy, nfx, nfy, ncx, ncy = (float(d[n]) for n in ("fx", "fy", "cx", "cy", "nfx", "nfy", "ncx", "ncy"))
    k1, k2, p1, p2, k3 = (float(d.get(n, 0.0)) for n in ("k1", "k2", "p1", "p2", "k3"))

    def node(ox, oy):
        x, y = (float(ox) - ncx) / nfx, (float(oy) - ncy) / nfy
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        return _q16(fx * xd + cx, fy * yd + cy)
    return _fill(size, k, node)
