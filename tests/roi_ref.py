"""numpy restatement of the batched regions of interest (include/xevd_hip.h xgpu_pic_output_device_rois) on top of the scaled
output's (tests/scale_ref.py): the letterbox rule in Python integers, and the batch as scale_ref.convert(crop=rectangle, size=inner size) placed into an image
filled with the pad value.  Written from the contract, not from the kernel."""
import numpy as np

import scale_ref as sr

STRETCH, LETTERBOX = 0, 1
U8, U16 = sr.U8, sr.U16


def inner(ws, hs, wd, hd, fit=LETTERBOX):
    """(x, y, width, height) of the filtered part of a ws x hs rectangle inside a wd x hd image"""
    wi, hi = wd, hd
    if fit == LETTERBOX:
        if ws * hd >= hs * wd:
            hi = min(hd, max(2, (2 * hs * wd + ws) // (2 * ws)))
        else:
            wi = min(wd, max(2, (2 * ws * hd + hs) // (2 * hs)))
    return (wd - wi) >> 1, (hd - hi) >> 1, wi, hi


def pad_elements(pad, dtype, mean=None, inv_std=None):
    """[3] the pad value as the image holds it: the integer, or the float32 through the normalise (before any f16 / bf16 rounding)"""
    p = np.broadcast_to(np.asarray(pad, np.float32), (3,))
    if dtype in (U8, U16):
        assert (p == np.floor(p)).all()
        return p.astype(np.uint8 if dtype == U8 else np.uint16)
    if mean is not None or inv_std is not None:
        p = sr.normalise(p.reshape(3, 1, 1), np.zeros(3, np.float32) if mean is None else mean, np.ones(3, np.float32) if inv_std is None else inv_std).reshape(3)
    return p.astype(np.float32)


def batch(planes, bd, size, rois, fit=STRETCH, pad=0.0, crop=(0, 0, 0, 0), dtype=U8, mean=None, inv_std=None, **kw):
    """decoded [Y, U, V] of the whole picture -> [N][3][Hd][Wd] in output channel order; rois: (x, y, w, h) inside the picture minus crop; kw: scale_ref.convert's"""
    hd, wd = size
    h, w = np.asarray(planes[0]).shape
    fill = pad_elements(pad, dtype, mean, inv_std)
    out = []
    for x, y, rw, rh in rois:
        ix, iy, wi, hi = inner(rw, rh, wd, hd, fit)
        rect = (crop[0] + x, w - crop[0] - x - rw, crop[2] + y, h - crop[2] - y - rh)      # the rectangle as a crop of the whole picture
        part = sr.convert(planes, bd, (hi, wi), dtype=dtype, crop=rect, mean=mean, inv_std=inv_std, **kw)
        img = np.empty((3, hd, wd), part.dtype)
        img[:] = fill.astype(part.dtype).reshape(3, 1, 1)
        img[:, iy:iy + hi, ix:ix + wi] = part
        out.append(img)
    return np.stack(out)
