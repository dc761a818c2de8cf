"""numpy restatement of the warped regions of interest (include/xevd_hip.h xgpu_pic_output_device_warp): the affine maps, the
supersampled bilinear gather and the border rule in int64 throughout, the conversion of the unscaled contract (colour_ref / yuv_ref) and the normalise of the
scaled output (scale_ref) on top - the way roi_ref.py sits on scale_ref.py.  The two host helpers (xgpu_warp_from_matrix, xgpu_warp_from_rotated_box) are restated
too.  Written from the contract, not from the kernel."""
import math

import numpy as np

import colour_ref as cr
import roi_ref as rr
import scale_ref as sr
import yuv_ref as yr

CLAMP, PAD = 0, 1
U8, U16, F16, BF16, F32 = sr.U8, sr.U16, sr.F16, sr.BF16, sr.F32
LIN_LIMIT, OFF_LIMIT = 64 << 16, 1 << 36
IDENTITY = (65536, 0, 0, 0, 65536, 0)


def map_ok(m):
    return all(abs(int(v)) <= (OFF_LIMIT if k in (2, 5) else LIN_LIMIT) for k, v in enumerate(m))


def _llround(v):
    """C's llround on a double: half away from zero (|v| < 2^52: the sum is exact)"""
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def from_matrix(theta):
    """theta (six doubles: destination pixel centres -> continuous source coordinates) -> the six Q16 integers, or None where the library refuses"""
    t = [float(v) for v in theta]
    if not all(math.isfinite(v) for v in t):
        return None
    m = []
    for r in (0, 3):
        m += [_llround(t[r] * 65536.0), _llround(t[r + 1] * 65536.0), _llround(((t[r] + t[r + 1]) * 0.5 + t[r + 2] - 0.5) * 65536.0)]
    return tuple(m) if map_ok(m) else None


def box_theta(cx, cy, w, h, angle_deg, dst_w, dst_h):
    rad = angle_deg * (math.pi / 180.0)
    c, s = math.cos(rad), math.sin(rad)
    return [w * c / dst_w, -h * s / dst_h, cx - (w * c - h * s) / 2, w * s / dst_w, h * c / dst_h, cy - (w * s + h * c) / 2]


def from_rotated_box(cx, cy, w, h, angle_deg, dst_size):
    """the map showing the w x h box centred at (cx, cy), turned by angle_deg (y down), in an image of dst_size = (H, W)"""
    return from_matrix(box_theta(cx, cy, w, h, angle_deg, dst_size[1], dst_size[0]))


def _bilinear(p, xr, yr):
    """plane p (int64) at the clamped Q8 positions xr, yr -> the weighted sum (16 fraction bits)"""
    ph, pw = p.shape
    ix, fx, iy, fy = xr >> 8, xr & 255, yr >> 8, yr & 255
    ix1, iy1 = np.minimum(ix + 1, pw - 1), np.minimum(iy + 1, ph - 1)
    return (256 - fx) * (256 - fy) * p[iy, ix] + fx * (256 - fy) * p[iy, ix1] + (256 - fx) * fy * p[iy1, ix] + fx * fy * p[iy1, ix1]


def warped_ycbcr(planes, bd, size, m, samples=1, chroma_loc=0, crop=(0, 0, 0, 0), dra=None):
    """decoded [Y, U, V] of the whole picture and one map (inside the limits) -> (Y, Cb, Cr [Hd][Wd] at the coding depth, outside [Hd][Wd]: the pixels that
    XGPU_WARP_PAD pads)"""
    planes = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        planes = cr.dra_apply(planes, dra)
    y, u, v = (np.clip(p, 0, (1 << bd) - 1) for p in cr.crop_planes(planes, crop))
    hs, ws = y.shape
    hd, wd = size
    m = [int(t) for t in m]
    assert map_ok(m) and samples in (1, 2, 4)
    S, ls = samples, {1: 0, 2: 1, 4: 2}[samples]
    sh, sv = sr.SITING[chroma_loc]
    ox, oy = np.arange(wd, dtype=np.int64)[None, :], np.arange(hd, dtype=np.int64)[:, None]
    X = m[0] * ox + m[1] * oy + m[2]
    Y = m[3] * ox + m[4] * oy + m[5]
    x0, y0 = (X + 128) >> 8, (Y + 128) >> 8
    outside = (x0 < 0) | (x0 > (ws - 1) << 8) | (y0 < 0) | (y0 > (hs - 1) << 8)
    acc = [np.zeros((hd, wd), np.int64) for _ in range(3)]
    for j in range(S):
        for i in range(S):
            Xs = X + ((m[0] * (2 * i + 1 - S) + m[1] * (2 * j + 1 - S)) >> (ls + 1))
            Ys = Y + ((m[3] * (2 * i + 1 - S) + m[4] * (2 * j + 1 - S)) >> (ls + 1))
            acc[0] += _bilinear(y, np.clip((Xs + 128) >> 8, 0, (ws - 1) << 8), np.clip((Ys + 128) >> 8, 0, (hs - 1) << 8))
            xc = np.clip((Xs - sh * 32768 + 256) >> 9, 0, (ws // 2 - 1) << 8)
            yc = np.clip((Ys - sv * 32768 + 256) >> 9, 0, (hs // 2 - 1) << 8)
            acc[1] += _bilinear(u, xc, yc)
            acc[2] += _bilinear(v, xc, yc)
    assert max(int(a.max()) for a in acc) < 1 << 32
    return [(a + (1 << (15 + 2 * ls))) >> (16 + 2 * ls) for a in acc], outside


def batch(planes, bd, size, maps, samples=1, border=CLAMP, pad=0.0, layout="rgb", matrix=1, full_range=False, chroma_loc=0, dtype=U8, crop=(0, 0, 0, 0), dra=None,
          bgr=False, mean=None, inv_std=None):
    """decoded [Y, U, V] of the whole picture -> [N][3][Hd][Wd] in output channel order (uint8 / uint16, or float32 before any f16 / bf16 rounding); a map outside
    the limits (the device-map call) gives an image that is all pad"""
    hd, wd = size
    fill = rr.pad_elements(pad, dtype, mean, inv_std)
    out = []
    for m in maps:
        if not map_ok(m):
            img = np.empty((3, hd, wd), fill.dtype)
            img[:] = fill.reshape(3, 1, 1)
            out.append(img)
            continue
        (y, cb, crr), outside = warped_ycbcr(planes, bd, size, m, samples, chroma_loc, crop, dra)
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
        img = np.ascontiguousarray(img)
        if border == PAD:
            img = np.where(outside[None], fill.astype(img.dtype).reshape(3, 1, 1), img)
        out.append(img)
    return np.stack(out)
