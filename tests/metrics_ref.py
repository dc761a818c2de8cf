"""The picture comparison of xgpu_pic_compare restated in numpy: the census of the differences, the exact integer SSIM and the
per-block SSE map.  Every figure is an integer - the SSIM of a window is made of individually rounded binary64 operations, quantised to 2^-30 and summed as an
integer - so the GPU is held to these numbers bit for bit.  Planes are 2-D arrays of unsigned 16-bit patterns (anything numpy converts to uint16 without loss);
nothing is clipped or masked."""
import numpy as np

NO_DIFF = (1 << 64) - 1


def ssim_constants(bit_depth):
    """c1, c2 of the 8x8-window integer SSIM at depth B: L = 2^B - 1, c1 = (64 L^2 + 5000) // 10000, c2 = (9 * 64 * 63 L^2 + 5000) // 10000"""
    peak = (1 << bit_depth) - 1
    return (64 * peak * peak + 5000) // 10000, (9 * 64 * 63 * peak * peak + 5000) // 10000


def _u16(p):
    p = np.asarray(p)
    if p.dtype == np.int16:
        p = p.view(np.uint16)
    assert p.ndim == 2 and p.min() >= 0 and p.max() <= 0xFFFF
    return p.astype(np.int64)


def crop_plane(p, crop, c):
    """plane c (0 luma, 1 / 2 chroma) of a picture minus crop = (left, right, top, bottom) luma samples"""
    s = 1 if c else 0
    l, r, t, b = (v >> s for v in crop)
    h, w = p.shape
    return p[t:h - b, l:w - r]


def census(a, r):
    """dict(n, sse, n_diff, max_abs, first_diff) of one plane: first_diff = (y << 32) | x of the first differing sample in raster order, NO_DIFF: none"""
    a, r = _u16(a), _u16(r)
    d = a - r
    nz = np.flatnonzero(d)
    first = NO_DIFF if nz.size == 0 else (int(nz[0] // a.shape[1]) << 32) | int(nz[0] % a.shape[1])
    return {"n": int(a.size), "sse": int((d * d).sum()), "n_diff": int(nz.size), "max_abs": int(np.abs(d).max()) if a.size else 0, "first_diff": first}


def window_sums(a, r):
    """(s1, s2, ss, s12) of every 8x8 window at (4i, 4j), i < (w >> 2) - 1, j < (h >> 2) - 1, as int64 arrays [windows down, windows across] (empty for w < 8 or h < 8)"""
    a, r = _u16(a), _u16(r)
    h, w = a.shape
    nbx, nby = w >> 2, h >> 2
    if nbx < 2 or nby < 2:
        z = np.zeros((0, 0), np.int64)
        return z, z, z, z

    def blocks(v):      # sums of the 4x4 blocks
        return v[:nby * 4, :nbx * 4].reshape(nby, 4, nbx, 4).sum(axis=(1, 3))

    def windows(v):     # a window is 2x2 of them
        b = blocks(v)
        return b[:-1, :-1] + b[:-1, 1:] + b[1:, :-1] + b[1:, 1:]

    return windows(a), windows(r), windows(a * a + r * r), windows(a * r)


def ssim_q30_windows(a, r, bit_depth):
    """q of every window: int64 [windows down, windows across]"""
    s1, s2, ss, s12 = window_sums(a, r)
    c1, c2 = ssim_constants(bit_depth)
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    cov = 64 * s12 - s1 * s2
    # the four integers are below 2^53: exact in binary64; then one rounding per written operation
    num = (2 * s1 * s2 + c1).astype(np.float64) * (2 * cov + c2).astype(np.float64)
    den = (s1 * s1 + s2 * s2 + c1).astype(np.float64) * (vars_ + c2).astype(np.float64)
    return np.floor(num / den * np.float64(1 << 30) + np.float64(0.5)).astype(np.int64)


def ssim_q30(a, r, bit_depth):
    """(ssim_windows, ssim_q30) of one plane"""
    q = ssim_q30_windows(a, r, bit_depth)
    return int(q.size), int(q.sum())


def block_sse(a, r, block):
    """SSE of the block x block blocks of one plane, clipped at its edge: int64 [ceil(h / block), ceil(w / block)]"""
    a, r = _u16(a), _u16(r)
    h, w = a.shape
    mh, mw = -(-h // block), -(-w // block)
    d2 = np.zeros((mh * block, mw * block), np.int64)
    d2[:h, :w] = (a - r) ** 2
    return d2.reshape(mh, block, mw, block).sum(axis=(1, 3))


def compare(pic, ref, bit_depth, crop=(0, 0, 0, 0), ssim=True, block_map=False):
    """xgpu_pic_compare of two pictures (lists of the planes Y, Cb, Cr of the uncropped pictures): the dict XgpuDecoder.pic_compare returns without its floats -
    n, sse, n_diff, first_diff, max_abs, ssim_windows, ssim_q30 as lists of three ints - and "map": uint64 [3, ceil(h / 16), ceil(w / 16)] or None"""
    out = {k: [] for k in ("n", "sse", "n_diff", "first_diff", "max_abs", "ssim_windows", "ssim_q30")}
    maps = []
    for c in range(3):
        a, r = crop_plane(pic[c], crop, c), crop_plane(ref[c], crop, c)
        for k, v in census(a, r).items():
            out[k].append(v)
        nw, q = ssim_q30(a, r, bit_depth) if ssim else (0, 0)
        out["ssim_windows"].append(nw)
        out["ssim_q30"].append(q)
        if block_map:
            maps.append(block_sse(a, r, 8 if c else 16))
    out["map"] = np.stack(maps).astype(np.uint64) if block_map else None
    return out


def ssim_float(a, r, bit_depth):
    """The textbook formula in plain float64 over the same windows: (2 mx my + C1)(2 cxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)) from the means, the unbiased
    variances and the covariance of the 64 samples, one value per window in raster order.  C1 = c1 / 64^2 and C2 = c2 / (64 * 63) are the integer form's own
    constants per sample (s1 = 64 mx, vars = 64 * 63 (vx + vy)): x264's c1 carries a factor 64 where the algebra asks for 64^2, so its effective C1 is
    (0.01 L)^2 / 64 - the integer form is what is specified, and this restatement follows it.  What is left between the two is the 2^-30 quantisation of a
    window (at most 2^-31) and float rounding."""
    a, r = _u16(a).astype(np.float64), _u16(r).astype(np.float64)
    h, w = a.shape
    c1, c2 = ssim_constants(bit_depth)
    k1, k2 = c1 / 4096.0, c2 / 4032.0
    vals = []
    for j in range((h >> 2) - 1):
        for i in range((w >> 2) - 1):
            x, y = a[4 * j:4 * j + 8, 4 * i:4 * i + 8], r[4 * j:4 * j + 8, 4 * i:4 * i + 8]
            mx, my = x.mean(), y.mean()
            vx, vy, cxy = ((x - mx) ** 2).sum() / 63.0, ((y - my) ** 2).sum() / 63.0, ((x - mx) * (y - my)).sum() / 63.0
            vals.append((2 * mx * my + k1) * (2 * cxy + k2) / ((mx * mx + my * my + k1) * (vx + vy + k2)))
    return np.array(vals, np.float64)
