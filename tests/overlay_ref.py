"""The overlaid output restated in numpy: layers alpha-blended over the plain call's picture in the output's own code domain, integers
only.  Every function takes the plain call's output array as `v` and returns what xgpu_pic_output_device_overlaid / _packed_overlaid write in its place.

A layer is a dict:
  bitmaps  dict(kind="rgba" | "bgra" | "a8", pixels=<uint8 [h, w, 4] or [h, w], in the byte order of the kind>, x=, y=, opacity=255, colour=(r, g, b, a))
  boxes    dict(kind="box", box=(x, y, w, h), thickness=1, colour=(r, g, b, a), fill=(r, g, b, a), opacity=255)
Device boxes are a dict(array=<int32 [n, 4] x y w h | float32 [n, 4] x1 y1 x2 y2>, count=None | int, labels=None | int32 [n], palette=[(r, g, b, a)],
thickness=, fill_alpha=); box_layers turns them into box layers, painted before the host layers."""
import math

import numpy as np

LIMIT = 1 << 20
KR_KB = {1: (0.2126, 0.0722), 4: (0.30, 0.11), 5: (0.299, 0.114), 6: (0.299, 0.114), 7: (0.212, 0.087), 9: (0.2627, 0.0593)}


def c_round(x):
    """C's round(): half away from zero"""
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def forward_matrix(matrix, full_range, d):
    """R'G'B' in 0 .. 255 -> Y', Cb, Cr codes of depth d: (m [3][3], offsets [3], S) - m[i][j] = round(k[i][j] * range_i / 255 * 2^S), S = 28 - d"""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    k = [kr, kg, kb,
         -kr / (2.0 * (1.0 - kb)), -kg / (2.0 * (1.0 - kb)), 0.5,
         0.5, -kg / (2.0 * (1.0 - kr)), -kb / (2.0 * (1.0 - kr))]
    s = 28 - d
    yr = float((1 << d) - 1) if full_range else float(219 << (d - 8))
    cr = float((1 << d) - 1) if full_range else float(224 << (d - 8))
    m = [c_round(k[i] * (yr if i < 3 else cr) / 255.0 * float(1 << s)) for i in range(9)]
    off = [0 if full_range else 16 << (d - 8), 1 << (d - 1), 1 << (d - 1)]
    return np.array(m, np.int64).reshape(3, 3), off, s


def to_ycc(rgb, matrix, full_range, d):
    """colours [..., 3] in 0 .. 255 -> Y', Cb, Cr codes [..., 3] of depth d, clipped to [0, 2^d - 1]"""
    m, off, s = forward_matrix(matrix, full_range, d)
    rgb = np.asarray(rgb, np.int64)
    out = np.empty(rgb.shape, np.int64)
    for i in range(3):
        out[..., i] = off[i] + (((rgb * m[i]).sum(axis=-1) + (1 << (s - 1))) >> s)      # (>> of a negative int64 is the floor, as the device's arithmetic shift)
    return np.clip(out, 0, (1 << d) - 1)


def box_snap(box, xyxy):
    """a device box -> the unclipped rectangle (x0, y0, x1, y1), or None: skipped"""
    if xyxy:
        b = np.asarray(box, np.float32)
        if not np.all(np.isfinite(b)):
            return None
        b = np.clip(b, np.float32(-LIMIT), np.float32(LIMIT))
        r = (int(np.floor(b[0])), int(np.floor(b[1])), int(np.ceil(b[2])), int(np.ceil(b[3])))
    else:
        x, y, w, h = (int(v) for v in box)
        if w < 1 or h < 1:
            return None
        cl = lambda v: max(-LIMIT, min(LIMIT, v))
        r = (cl(x), cl(y), cl(x + w), cl(y + h))
    return r if r[2] > r[0] and r[3] > r[1] else None


def box_layers(boxes):
    """the device boxes as box layers, in index order"""
    if boxes is None:
        return []
    arr = np.asarray(boxes["array"])
    xyxy = arr.dtype.kind == "f"
    cap = arr.shape[0]
    count = boxes.get("count")
    live = cap if count is None else min(max(int(count), 0), cap)
    pal = boxes.get("palette", [(255, 0, 0, 255)])
    out = []
    for i in range(live):
        r = box_snap(arr[i], xyxy)
        if r is None:
            continue
        lab = 0 if boxes.get("labels") is None else int(boxes["labels"][i])
        c = tuple(int(v) for v in pal[lab % len(pal)])      # (Python's % is ((label % n) + n) % n)
        out.append(dict(kind="box", box=(r[0], r[1], r[2] - r[0], r[3] - r[1]), thickness=boxes.get("thickness", 2), colour=c,
                        fill=c[:3] + (int(boxes.get("fill_alpha", 0)),), opacity=255))
    return out


def layer_field(layer, w, h):
    """one layer over the w x h image -> (colour [h, w, 3] int64 in R, G, B order, effective alpha a [h, w] int64; 0 where the layer is not)"""
    yy, xx = np.mgrid[0:h, 0:w]
    if layer["kind"] == "box":
        x0, y0, bw, bh = (int(v) for v in layer["box"])
        x1, y1 = x0 + bw, y0 + bh
        inside = (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
        dist = np.minimum(np.minimum(xx - x0, x1 - 1 - xx), np.minimum(yy - y0, y1 - 1 - yy))      # of the unclipped rectangle
        frame = dist < int(layer.get("thickness", 1))
        col, fill = np.array(layer.get("colour", (255, 255, 255, 255)), np.int64), np.array(layer.get("fill", (0, 0, 0, 0)), np.int64)
        rgba = np.where(frame[..., None], col, fill)
        rgb, a8 = rgba[..., :3], rgba[..., 3]
    else:
        px = np.asarray(layer["pixels"])
        x0, y0 = int(layer.get("x", 0)), int(layer.get("y", 0))
        ph, pw = px.shape[:2]
        inside = (xx >= x0) & (xx < x0 + pw) & (yy >= y0) & (yy < y0 + ph)
        s = px[np.clip(yy - y0, 0, ph - 1), np.clip(xx - x0, 0, pw - 1)].astype(np.int64)
        if layer["kind"] == "a8":
            col = np.array(layer.get("colour", (255, 255, 255, 255)), np.int64)
            rgb = np.broadcast_to(col[:3], (h, w, 3))
            a8 = (s * col[3] + 127) // 255
        else:
            rgb = s[..., :3][..., ::-1] if layer["kind"] == "bgra" else s[..., :3]
            a8 = s[..., 3]
    a = (a8 * int(layer.get("opacity", 255)) + 127) // 255
    return np.asarray(rgb, np.int64), np.where(inside, a, 0)


def all_layers(layers, boxes):
    return box_layers(boxes) + list(layers or [])


def blend_rgb(v, maxv, layers, boxes=None):
    """v [h, w, 3] in R, G, B order, elements of maximum maxv -> the same with the layers over it"""
    out = np.clip(np.asarray(v, np.int64), 0, maxv)
    h, w = out.shape[:2]
    for l in all_layers(layers, boxes):
        rgb, a = layer_field(l, w, h)
        cd = (rgb * maxv + 127) // 255
        a = a[..., None]
        out = np.where(a == 0, out, (out * (255 - a) + cd * a + 127) // 255)
    return out


def rgb(v, maxv, layers, boxes=None, channels_last=False, bgr=False):
    """the plain RGB image v ([3, h, w] or [h, w, 3]; bgr: B, G, R) with the layers over it"""
    x = np.asarray(v).astype(np.int64)
    x = x if channels_last else x.transpose(1, 2, 0)
    x = x[..., ::-1] if bgr else x
    out = blend_rgb(x, maxv, layers, boxes)
    out = out[..., ::-1] if bgr else out
    out = out if channels_last else out.transpose(2, 0, 1)
    return np.ascontiguousarray(out).astype(np.asarray(v).dtype)


def rgba(v, maxv, layers, boxes=None, bgr=False):
    """the plain RGBA surface v [h, w, 4] with the layers over it: the A element stays"""
    out = np.array(v)
    out[..., :3] = rgb(out[..., :3], maxv, layers, boxes, channels_last=True, bgr=bgr)
    return out


def rgb10a2(v, layers, boxes=None, bgr=False):
    """the plain 10:10:10:2 words v [h, w] (uint32) with the layers over them: the two alpha bits stay"""
    w = np.asarray(v).astype(np.uint32)
    ch = np.stack([(w >> np.uint32(10 * k)) & np.uint32(1023) for k in range(3)], axis=-1)
    out = rgb(ch, 1023, layers, boxes, channels_last=True, bgr=bgr).astype(np.uint32)
    return (w & np.uint32(0xC0000000)) | out[..., 0] | (out[..., 1] << np.uint32(10)) | (out[..., 2] << np.uint32(20))


def chroma_blend(v, maxv, a, c):
    """one layer on one chroma plane: v [h/2, w/2], a [h, w] the layer's alphas, c [h, w] its converted chroma -> (clip(v) * (1020 - A) + C + 510) // 1020, or v"""
    h2, w2 = v.shape
    q = lambda t: t.reshape(h2, 2, w2, 2).sum(axis=(1, 3))
    A, C = q(a), q(a * c)
    return np.where(A == 0, v, (np.clip(v, 0, maxv) * (1020 - A) + C + 510) // 1020)


def semiplanar(v, d, layers, boxes=None, matrix=1, full_range=False, lsh=0):
    """the plain NV12 / P016 surface v [h * 3 / 2, w] at depth d (P016: lsh = 16 - d) with the layers over it, blended in Y'CbCr on the d-bit sample"""
    src = np.asarray(v)
    x = src.astype(np.int64) >> lsh
    maxv = (1 << d) - 1
    h = x.shape[0] * 2 // 3
    w = x.shape[1]
    y, cb, cr = x[:h].copy(), x[h:, 0::2].copy(), x[h:, 1::2].copy()
    for l in all_layers(layers, boxes):
        col, a = layer_field(l, w, h)
        ycc = to_ycc(col, matrix, full_range, d)
        y = np.where(a == 0, y, (np.clip(y, 0, maxv) * (255 - a) + ycc[..., 0] * a + 127) // 255)
        cb = chroma_blend(cb, maxv, a, ycc[..., 1])
        cr = chroma_blend(cr, maxv, a, ycc[..., 2])
    out = np.empty_like(x)
    out[:h], out[h:, 0::2], out[h:, 1::2] = y, cb, cr
    return (out << lsh).astype(src.dtype)
