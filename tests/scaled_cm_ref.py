"""numpy restatement of the colour-managed scaled output (include/xevd_hip.h xgpu_pic_output_device_scaled_cm / _rois_cm).  No
arithmetic of its own: the scaled output's filter (scale_ref.scaled_ycbcr), the U16 form's matrix (colour_ref.ycbcr_to_rgb), the transform
(colour_cm_ref.transform), bgr, the scaled output's normalise (scale_ref.normalise), and roi_ref's letterbox rule and pad value for the batch.  Written from the
contract, not from the kernel."""
import numpy as np

import colour_cm_ref as cmr
import colour_ref as cr
import roi_ref
import scale_ref as sr

U8, U16 = sr.U8, sr.U16
STRETCH, LETTERBOX = roi_ref.STRETCH, roi_ref.LETTERBOX


def convert(planes, bd, size, tab, filt=sr.BILINEAR, matrix=1, full_range=False, chroma_loc=0, dtype=U8, crop=(0, 0, 0, 0), dra=None, bgr=False,
            mean=None, inv_std=None, lib=None):
    """decoded [Y, U, V] of the whole picture through tables `tab` (abi.colour_tables) -> [3][Hd][Wd] in output channel order: uint8 / uint16 for the integer
    dtypes, float32 (before any f16 / bf16 rounding) otherwise"""
    y, cb, crr = sr.scaled_ycbcr(planes, bd, size, filt, chroma_loc, crop, dra, lib)
    return from_ycbcr(y, cb, crr, bd, tab, matrix, full_range, dtype, bgr, mean, inv_std)


def from_ycbcr(y, cb, crr, bd, tab, matrix=1, full_range=False, dtype=U8, bgr=False, mean=None, inv_std=None):
    """the steps behind the filter, for planes scale_ref.scaled_ycbcr has made (a test that wants several dtypes of one size filters once)"""
    codes = cr.ycbcr_to_rgb(y, cb, crr, bd, matrix, full_range, U16)      # the code at the coding depth, whatever the output dtype
    out = cmr.transform(np.asarray(codes).astype(np.int64), tab, dtype, bd)
    if bgr:
        out = out[::-1]
    if mean is not None or inv_std is not None:
        assert dtype not in (U8, U16)
        out = sr.normalise(out, np.zeros(3, np.float32) if mean is None else mean, np.ones(3, np.float32) if inv_std is None else inv_std)
    return np.ascontiguousarray(out)


def batch(planes, bd, size, rois, tab, fit=STRETCH, pad=0.0, crop=(0, 0, 0, 0), dtype=U8, mean=None, inv_std=None, **kw):
    """-> [N][3][Hd][Wd]; rois: (x, y, w, h) inside the picture minus crop; the pad value is roi_ref's - a value of the destination space, never transformed"""
    hd, wd = size
    h, w = np.asarray(planes[0]).shape
    fill = roi_ref.pad_elements(pad, dtype, mean, inv_std)
    out = []
    for x, y, rw, rh in rois:
        ix, iy, wi, hi = roi_ref.inner(rw, rh, wd, hd, fit)
        rect = (crop[0] + x, w - crop[0] - x - rw, crop[2] + y, h - crop[2] - y - rh)      # the rectangle as a crop of the whole picture
        part = convert(planes, bd, (hi, wi), tab, dtype=dtype, crop=rect, mean=mean, inv_std=inv_std, **kw)
        img = np.empty((3, hd, wd), part.dtype)
        img[:] = fill.astype(part.dtype).reshape(3, 1, 1)
        img[:, iy:iy + hi, ix:ix + wi] = part
        out.append(img)
    return np.stack(out)
