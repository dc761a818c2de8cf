"""numpy restatement of the surface ladder (include/xevd_hip.h xgpu_pic_output_device_ladder): the taps of a destination with a
subsampling and a siting of its own with fractions.Fraction, the two integer passes of the scaled output (scale_ref), the depth conversion and the packing of the
video surfaces (yuv_ref).  Written from the contract, not from the kernel."""
from fractions import Fraction
import math

import numpy as np

import colour_ref as cr
import scale_ref as sr
import yuv_ref as yr

BILINEAR, AREA = sr.BILINEAR, sr.AREA
ONE = sr.ONE
SITING = sr.SITING      # ChromaSampleLocType -> (dx, dy) in half luma samples


def taps_ex(n, s, half, N, S=1, Half=0, filt=BILINEAR, outputs=None):
    """one axis: n plane samples of subsampling s and siting half / 2 luma samples onto N samples of subsampling S and siting Half / 2 luma samples of the
    destination grid -> [(first, [q ...]) per destination sample]"""
    r = Fraction(n * s, N * S)
    f = max(Fraction(1), r * S / s)
    d, D = Fraction(half, 2), Fraction(Half, 2)
    rows = []
    for o in (range(N) if outputs is None else outputs):
        c = ((S * o + D + Fraction(1, 2)) * r - Fraction(1, 2) - d) / s
        reach = f if filt == BILINEAR else (f + 1) / 2
        ws = {}
        for i in range(max(math.floor(c - reach) - 1, 0), min(math.ceil(c + reach) + 1, n - 1) + 1):
            if filt == BILINEAR:
                w = 1 - abs(i - c) / f
            else:
                w = min(i + Fraction(1, 2), c + f / 2) - max(i - Fraction(1, 2), c - f / 2)
            if w > 0:
                ws[i] = w
        if not ws:          # the window lies off the plane: the nearest sample alone
            ws = {min(max(math.floor(c + Fraction(1, 2)), 0), n - 1): Fraction(1)}
        idx = sorted(ws)
        assert idx == list(range(idx[0], idx[0] + len(idx)))
        total = sum(ws.values())
        q = [math.floor(ws[i] / total * ONE + Fraction(1, 2)) for i in idx]
        q[q.index(max(q))] += ONE - sum(q)
        rows.append((idx[0], q))
    return rows


def make_tables(ws, hs, wd, hd, filt=BILINEAR, chroma_loc=0, dst_chroma_loc=None, lib=None):
    """the four tap tables of one rung (luma rows, chroma rows, luma columns, chroma columns): from taps_ex(), or - lib given - the library's own"""
    dx, dy = SITING[chroma_loc]
    Dx, Dy = SITING[chroma_loc if dst_chroma_loc is None else dst_chroma_loc]
    spec = ((hs, 1, 0, hd, 1, 0), (hs // 2, 2, dy, hd // 2, 2, Dy), (ws, 1, 0, wd, 1, 0), (ws // 2, 2, dx, wd // 2, 2, Dx))
    if lib is None:
        return [taps_ex(*a, filt) for a in spec]
    from xevd_amd import abi
    return [sr.table_rows(*abi.scale_taps_ex(lib, *a, filt)) for a in spec]


def source_planes(planes, bd, crop=(0, 0, 0, 0), dra=None):
    """decoded [Y, U, V] of the whole picture -> the source of a ladder: DRA, crop, the clip to [0, 2^B - 1]"""
    planes = [np.asarray(p, np.int64) for p in planes]
    if dra is not None:
        planes = cr.dra_apply(planes, dra)
    return [np.clip(p, 0, (1 << bd) - 1) for p in cr.crop_planes(planes, crop)]


def resize_planes(src, size, tables):
    """the source planes through the tables of one rung -> Y [Hd][Wd], Cb and Cr [Hd / 2][Wd / 2] at the coding depth"""
    yl, yc, xl, xc = tables
    out = [sr.resize_plane(src[0], yl, xl), sr.resize_plane(src[1], yc, xc), sr.resize_plane(src[2], yc, xc)]
    hd, wd = size
    assert out[0].shape == (hd, wd) and out[1].shape == (hd // 2, wd // 2)
    return out


def pack(ycc, bd, layout, d):
    """Y, Cb, Cr of a rung at the coding depth -> the surface: the depth rule of xgpu_pic_output to depth d, then the layout of section 8a.  "nv12" at d = 8 is
    uint8; "nv12_u16": NV12 in 16-bit words whatever d"""
    if layout == "yuv420p":
        return yr.yuv420p(ycc, bd, d)
    if layout == "p016":
        return yr.p016(ycc, bd, d)
    return yr.nv12(ycc, bd, d, dtype=np.uint16 if layout == "nv12_u16" else None)


def rung(planes, bd, size, layout="nv12", d=None, filt=BILINEAR, chroma_loc=0, dst_chroma_loc=None, crop=(0, 0, 0, 0), dra=None, lib=None, tables=None):
    """one rung of (H, W) = size as the array its tensor must hold"""
    src = source_planes(planes, bd, crop, dra)
    hs, ws = src[0].shape
    if tables is None:
        tables = make_tables(ws, hs, size[1], size[0], filt, chroma_loc, dst_chroma_loc, lib)
    return pack(resize_planes(src, size, tables), bd, layout, bd if d is None else d)
