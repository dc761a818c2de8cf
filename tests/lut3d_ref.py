"""numpy restatement of the 3D LUT output (include/xevd_hip.h xgpu_pic_output_device_lut3d): the host helpers that make the uint16
tables, the shaper, the tetrahedral interpolation, the store, and a census of the branches a call reaches.  Written from the contract, not from the kernel: the
axes are sorted and the vertices are walked as the contract words them.  DRA, crop, chroma upsampling and the matrix are colour_ref's."""
import itertools

import numpy as np

import colour_ref as cr
import packed_ref as pr

U8, U16, F16, BF16, F32 = cr.U8, cr.U16, cr.F16, cr.BF16, cr.F32
ORDERINGS = ["".join(p) for p in itertools.permutations("RGB")]      # "RGB": f_R > f_G > f_B, ...


# ---- the host helpers (double arithmetic: + - * / and floor)
def quantise(v):
    """floor(clip(v, 0, 1) * 65535 + 0.5), NaN -> 0"""
    v = np.asarray(v, np.float64)
    v = np.where(v > 0.0, v, 0.0)
    v = np.where(v > 1.0, 1.0, v)
    return np.floor(v * 65535.0 + 0.5).astype(np.uint16)


def from_float(rgb):
    """float32 nodes [n^3, 3] -> uint16 nodes"""
    return quantise(np.asarray(rgb, np.float32).astype(np.float64)).reshape(-1, 3)


def identity_shaper(bd):
    """S[c] = floor((2 * 65535 * c + M) / (2 M)) in integers, [3][2^bd]"""
    m = (1 << bd) - 1
    c = np.arange(m + 1, dtype=np.int64)
    return np.tile(((2 * 65535 * c + m) // (2 * m)).astype(np.uint16), (3, 1))


def identity_cube(n):
    """e_i = floor((2 * 65535 * i + n - 1) / (2 (n - 1))) per axis, [n^3][3] in .cube order (red fastest)"""
    e = (2 * 65535 * np.arange(n, dtype=np.int64) + n - 1) // (2 * (n - 1))
    b, g, r = np.meshgrid(e, e, e, indexing="ij")
    return np.stack([r.ravel(), g.ravel(), b.ravel()], axis=1).astype(np.uint16)


def shaper(bd, curve=None, in_min=(0.0, 0.0, 0.0), in_max=(1.0, 1.0, 1.0)):
    """xgpu_lut3d_shaper: [3][2^bd] positions"""
    m = (1 << bd) - 1
    x = np.arange(m + 1, dtype=np.float64) / float(m)
    out = np.zeros((3, m + 1), np.uint16)
    for k in range(3):
        lo, hi = float(np.float32(in_min[k])), float(np.float32(in_max[k]))
        t = (x - lo) / (hi - lo)
        t = np.where(t > 0.0, t, 0.0)
        t = np.where(t > 1.0, 1.0, t)
        if curve is not None:
            cv = np.asarray(curve, np.float32).astype(np.float64).reshape(-1, 3)[:, k]
            nc = cv.shape[0]
            u = t * float(nc - 1)
            j = np.minimum(np.floor(u).astype(np.int64), nc - 2)
            with np.errstate(invalid="ignore"):
                t = cv[j] + (u - j.astype(np.float64)) * (cv[j + 1] - cv[j])
        out[k] = quantise(t)
    return out


# ---- the interpolation
def interpolate(codes, shp, nodes, n):
    """R'G'B' codes at the coding depth [3, ...] -> (v [3, ...] int64 in 0 .. 65535, census).  shp: [3][2^B] uint16, nodes: [n^3][3] uint16 in .cube order."""
    codes = np.asarray(codes, np.int64)
    shape = codes.shape[1:]
    c = codes.reshape(3, -1)
    shp = np.asarray(shp, np.int64)
    nodes = np.asarray(nodes, np.int64).reshape(n, n, n, 3)      # [b][g][r]
    p = np.stack([shp[k][c[k]] for k in range(3)])
    q = p * (n - 1)
    i = np.minimum(q // 65535, n - 2)
    f = q - 65535 * i
    assert f.min() >= 0 and f.max() <= 65535
    order = np.argsort(-f, axis=0, kind="stable")                # axes a, b, c with f_a >= f_b >= f_c
    fs = np.take_along_axis(f, order, axis=0)
    px = np.arange(c.shape[1])

    def node(idx):
        return nodes[idx[2], idx[1], idx[0]]                      # [pixels][3]
    v0i = i.copy()
    v1i = v0i.copy()
    v1i[order[0], px] += 1
    v2i = v1i.copy()
    v2i[order[1], px] += 1
    v3i = i + 1
    w = [65535 - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2]]
    s = sum(wk[:, None] * node(vi) for wk, vi in zip(w, (v0i, v1i, v2i, v3i)))
    assert s.max() + 32767 < (1 << 32)
    v = ((s + 32767) // 65535).T
    strict = (f[0] != f[1]) & (f[1] != f[2]) & (f[0] != f[2])
    census = {name: int((strict & (order[0] == "RGB".index(name[0])) & (order[1] == "RGB".index(name[1]))).sum()) for name in ORDERINGS}
    census["tie"] = int((~strict).sum())
    census["clamp"] = int((f == 65535).any(axis=0).sum())
    census["node"] = int(((f == 0) | (f == 65535)).all(axis=0).sum())
    return v.reshape((3,) + shape), census


def store_depth(dtype, bd, out_bit_depth=0):
    return 8 if dtype == U8 else (16 if out_bit_depth == 16 else bd)


def store(v, dtype, d):
    """v in 0 .. 65535 -> the elements as unsigned integers: the D-bit code, or the bits of the float dtype"""
    v = np.asarray(v, np.int64)
    if dtype in (U8, U16):
        return ((v * ((1 << d) - 1) + 32767) // 65535).astype(np.uint8 if dtype == U8 else np.uint16)
    f = (v.astype(np.float32) * (np.float32(1) / np.float32(65535))).astype(np.float32)
    if dtype == F32:
        return f.view(np.uint32)
    return cr.to_f16_bits(f) if dtype == F16 else cr.to_bf16_bits(f)


def codes_of(planes, bd, matrix=1, full_range=False, chroma_loc=0, mode="linear", crop=(0, 0, 0, 0), dra=None):
    """the input of the LUT: the U16 form's R'G'B' codes [3][H][W]"""
    return cr.convert(planes, bd, matrix=matrix, full_range=full_range, chroma_loc=chroma_loc, mode=mode, dtype=U16, crop=crop, dra=dra).astype(np.int64)


def lut3d(planes, bd, nodes, n, shp=None, dtype=U8, out_bit_depth=0, bgr=False, **conv):
    """decoded [Y, U, V] of the whole picture -> ([3][H][W] elements in R, G, B (bgr: B, G, R) order as unsigned integers / float bits, census)"""
    v, census = interpolate(codes_of(planes, bd, **conv), identity_shaper(bd) if shp is None else shp, nodes, n)
    e = store(v, dtype, store_depth(dtype, bd, out_bit_depth))
    return (e[::-1] if bgr else e), census


def rgb10a2(planes, bd, nodes, n, shp=None, bgr=False, alpha=1.0, **conv):
    """-> [H][W] uint32 words R | G << 10 | B << 20 | A << 30 (bgr: B low, R at 20)"""
    v, _ = interpolate(codes_of(planes, bd, **conv), identity_shaper(bd) if shp is None else shp, nodes, n)
    c = store(v, U16, 10).astype(np.uint64)
    lo, hi = (c[2], c[0]) if bgr else (c[0], c[2])
    return (lo | (c[1] << 10) | (hi << 20) | (np.uint64(pr.alpha_code(alpha, 2)) << 30)).astype(np.uint32)


def div65535_shift(x):
    """the kernel's form of x / 65535 (the contract says they are equal for x <= 65535^2 + 32767)"""
    x = np.asarray(x, np.uint64)
    return (x + (x >> np.uint64(16)) + np.uint64(1)) >> np.uint64(16)
