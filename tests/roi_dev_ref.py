"""numpy restatement of what the device decides per box in xgpu_pic_output_device_rois_dev (include/xevd_hip.h), on top of
roi_ref.py and scale_ref.py: the snapping rule of both box formats, the status, the rectangle used and its inner part.  The images themselves need no
restatement of their own: image i is roi_ref.batch on the rectangle used, or all pad.  Written from the contract, not from the kernel."""
import numpy as np

import roi_ref as rr

XYWH_I32, XYXY_F32 = 0, 1
OK, UNUSED, INVALID, EMPTY, TOO_LARGE, RATIO = range(6)
NONE = (0, 0, 0, 0)


def snap(box, pic_size, fmt):
    """box (x, y, w, h) of ints or (x1, y1, x2, y2) of floats, pic_size = (H, W) of the picture minus the crop -> (status, (x, y, width, height))"""
    ph, pw = pic_size
    if fmt == XYWH_I32:
        x, y, w, h = (int(v) for v in box)
        x0, y0 = max(x & ~1, 0), max(y & ~1, 0)
        x1, y1 = min((x + w + 1) & ~1, pw), min((y + h + 1) & ~1, ph)
    else:
        b = np.asarray(box, np.float32)
        if not np.isfinite(b).all():
            return INVALID, NONE
        b = np.minimum(np.maximum(b, np.float32(-2 ** 20)), np.float32(2 ** 20))
        half = (b * np.float32(0.5)).astype(np.float32)      # exact: a power of two
        x0, y0 = max(2 * int(np.floor(half[0])), 0), max(2 * int(np.floor(half[1])), 0)
        x1, y1 = min(2 * int(np.ceil(half[2])), pw), min(2 * int(np.ceil(half[3])), ph)
    if x1 - x0 < 2 or y1 - y0 < 2:
        return EMPTY, NONE
    return OK, (x0, y0, x1 - x0, y1 - y0)


def ratio_ok(n, N):
    return N >= 2 and n <= 64 * N and N <= 8 * n


def result(box, fmt, pic_size, size, fit=rr.STRETCH, max_roi=None):
    """one live box -> the nine ints of its xgpu_roi_result: status, the rectangle used, its inner part (zeros unless OK)"""
    status, used = snap(box, pic_size, fmt)
    mh, mw = max_roi if max_roi else pic_size
    if status == OK and (used[2] > (mw or pic_size[1]) or used[3] > (mh or pic_size[0])):
        status = TOO_LARGE
    inner = NONE
    if status == OK:
        inner = rr.inner(used[2], used[3], size[1], size[0], fit)
        if not ratio_ok(used[2], inner[2]) or not ratio_ok(used[3], inner[3]):
            status = RATIO
    if status != OK:
        used, inner = NONE, NONE
    return (status, *used, *inner)


def results(boxes, fmt, pic_size, size, fit=rr.STRETCH, max_roi=None, count=None):
    """[N][9] int32 for a batch: the first min(max(count, 0), N) boxes are live, the others UNUSED"""
    n = len(boxes)
    live = n if count is None else min(max(int(count), 0), n)
    return np.array([result(b, fmt, pic_size, size, fit, max_roi) if i < live else (UNUSED,) + NONE + NONE for i, b in enumerate(boxes)], np.int32).reshape(n, 9)
