"""numpy restatement of the video-surface layouts of the device-output contract (include/xevd_hip.h xgpu_output_format):
YUV420P / NV12 / P016 from the depth conversion of xgpu_pic_output, Y'CbCr 4:4:4 as integers or H.273's normalised floats.  Written from the
contract, not from the kernel; DRA, crop and chroma upsampling are colour_ref's (the RGB contract's steps 1 and 2)."""
import numpy as np

import colour_ref as cr

U8, U16, F16, BF16, F32 = cr.U8, cr.U16, cr.F16, cr.BF16, cr.F32


def depth_convert(v, bd, d):
    """xgpu_pic_output's conversion of samples at coding depth bd to depth d: 8 bit - rounding shift of the signed sample clipped to [0, 255]; a
    lower depth - the same on the unsigned 16-bit sample clipped to 2^d - 1; a higher depth - left shift (16-bit wrap); equal - copy"""
    v = np.asarray(v, np.int64)
    s = bd - d
    if d == 8:
        return np.clip((v + ((1 << (s - 1)) if s else 0)) >> s, 0, 255)
    if s > 0:
        return np.minimum(((v & 0xFFFF) + (1 << (s - 1))) >> s, (1 << d) - 1)
    return (v << -s) & 0xFFFF if s < 0 else v & 0xFFFF


def _prepared(planes, crop, dra):
    planes = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        planes = cr.dra_apply(planes, dra)
    return cr.crop_planes(planes, crop)


def yuv420p(planes, bd, d, crop=(0, 0, 0, 0), dra=None):
    """the YUV420P layout: Y, U, V planes back to back, tight rows -> 1-D uint8 (d = 8) or uint16"""
    return np.concatenate([depth_convert(p, bd, d).ravel() for p in _prepared(planes, crop, dra)]).astype(np.uint8 if d == 8 else np.uint16)


def nv12(planes, bd, d, crop=(0, 0, 0, 0), dra=None, dtype=None):
    """[H * 3 // 2][W]: H luma rows, then H / 2 rows Cb0 Cr0 Cb1 Cr1 ...; uint8 for d = 8 (or uint16 when dtype says so: P016 at D = 8)"""
    y, u, v = (depth_convert(p, bd, d) for p in _prepared(planes, crop, dra))
    h, w = y.shape
    out = np.zeros((h * 3 // 2, w), np.int64)
    out[:h] = y
    out[h:, 0::2] = u
    out[h:, 1::2] = v
    return out.astype(dtype or (np.uint8 if d == 8 else np.uint16))


def p016(planes, bd, d, crop=(0, 0, 0, 0), dra=None):
    """NV12's samples at depth d in the high bits of 16-bit words (d = 10: P010, 12: P012)"""
    return (nv12(planes, bd, d, crop, dra, np.uint16).astype(np.int64) << (16 - d)).astype(np.uint16)


def interleave_420p(flat, w, h):
    """the bytes / words of a YUV420P frame (1-D, tight) re-interleaved as NV12 [H * 3 // 2][W]"""
    flat = np.asarray(flat)
    n, q = w * h, (w // 2) * (h // 2)
    out = np.zeros((h * 3 // 2, w), flat.dtype)
    out[:h] = flat[:n].reshape(h, w)
    out[h:, 0::2] = flat[n:n + q].reshape(h // 2, w // 2)
    out[h:, 1::2] = flat[n + q:n + 2 * q].reshape(h // 2, w // 2)
    return out


def normalised(y, cb, crr, bd, full_range):
    """H.273's E'Y, E'Cb, E'Cr in float32: one float32 multiplication by a reciprocal rounded once from double, then the clip"""
    yo, yr, crng = cr.ranges(bd, full_range)
    fy, fc = np.float32(1.0 / yr), np.float32(1.0 / crng)
    co = 1 << (bd - 1)
    ey = np.clip((np.asarray(y, np.int64) - yo).astype(np.float32) * fy, np.float32(0), np.float32(1))
    ecb = np.clip((np.asarray(cb, np.int64) - co).astype(np.float32) * fc, np.float32(-0.5), np.float32(0.5))
    ecr = np.clip((np.asarray(crr, np.int64) - co).astype(np.float32) * fc, np.float32(-0.5), np.float32(0.5))
    return np.stack([ey, ecb, ecr]).astype(np.float32)


def yuv444(planes, bd, full_range=False, chroma_loc=0, mode="linear", dtype=U8, crop=(0, 0, 0, 0), dra=None):
    """decoded [Y, U, V] of the whole picture -> [3][H][W] Y, Cb, Cr: uint8 / uint16 for the integer dtypes, float32 (before any f16 / bf16
    rounding) otherwise"""
    y, u, v = _prepared(planes, crop, dra)
    h, w = y.shape
    cb, crr = cr.upsample(u, w, h, mode, chroma_loc), cr.upsample(v, w, h, mode, chroma_loc)
    if dtype == U8:
        return np.stack([depth_convert(p, bd, 8) for p in (y, cb, crr)]).astype(np.uint8)
    if dtype == U16:
        return np.stack([y, cb, crr]).astype(np.uint16)
    return normalised(y, cb, crr, bd, full_range)
