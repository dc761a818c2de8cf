"""ctypes view of include/xevd_hip.h - struct layouts and the loader for the product library.

Plumbing only: the product is xevd_amd/libxevd_hip.so (hand-written HIP for gfx950 behind a C ABI).  This
module never falls back to a CPU path: if the shared library is missing, `load()` raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libxevd_hip.so")

XGPU_MAX_REFS = 17
PAD_L, PAD_C = 144, 72
MODE_INTRA, MODE_INTER, MODE_SKIP, MODE_DIR = 0, 1, 2, 3
K_NAMES = ["itdq", "inter", "dbk_v", "dbk_h", "pad", "intra", "alf", "affine", "dmvr"]
K_COUNT = 9


class SeqParams(C.Structure):
    _fields_ = [
        ("device", C.c_int), ("width", C.c_int), ("height", C.c_int),
        ("bit_depth_luma", C.c_int), ("bit_depth_chroma", C.c_int), ("chroma_format_idc", C.c_int),
        ("log2_ctu", C.c_int), ("tool_iqt", C.c_int), ("tool_admvp", C.c_int), ("tool_addb", C.c_int),
        ("tool_alf", C.c_int), ("max_pics", C.c_int),
        ("chroma_qp_table", C.POINTER(C.c_int8) * 2),
        ("tool_eipd", C.c_int),
    ]


class DraLuts(C.Structure):
    _fields_ = [("luma_inv_scale_lut", C.c_void_p), ("chroma_inv_scale_lut", C.c_void_p * 2)]


OUT_YUV420P, OUT_RGB_PLANAR, OUT_RGB_INTERLEAVED = 0, 1, 2
OUT_NV12, OUT_P016, OUT_YUV444_PLANAR, OUT_YUV444_INTERLEAVED = 3, 4, 5, 6
OUT_U8, OUT_U16, OUT_F16, OUT_BF16, OUT_F32 = 0, 1, 2, 3, 4
UPSAMPLE_NEAREST, UPSAMPLE_LINEAR = 0, 1


class OutputFormat(C.Structure):
    _fields_ = [("layout", C.c_int), ("bgr", C.c_int), ("dtype", C.c_int), ("out_bit_depth", C.c_int),
                ("matrix", C.c_int), ("full_range", C.c_int), ("chroma_loc", C.c_int), ("upsample", C.c_int),
                ("crop", C.c_int * 4), ("row_pitch", C.c_size_t)]


def make_output_format(layout=OUT_RGB_PLANAR, dtype=OUT_U8, bgr=False, out_bit_depth=0, matrix=1, full_range=False, chroma_loc=0,
                       upsample=UPSAMPLE_LINEAR, crop=(0, 0, 0, 0), row_pitch=0):
    f = OutputFormat()
    f.layout, f.bgr, f.dtype, f.out_bit_depth = int(layout), int(bool(bgr)), int(dtype), int(out_bit_depth)
    f.matrix, f.full_range, f.chroma_loc, f.upsample = int(matrix), int(bool(full_range)), int(chroma_loc), int(upsample)
    for i in range(4):
        f.crop[i] = int(crop[i])
    f.row_pitch = int(row_pitch)
    return f


PACKED_RGBA, PACKED_RGB10A2, PACKED_YUYV, PACKED_UYVY = 0, 1, 2, 3


class PackedFormat(C.Structure):
    _fields_ = [("layout", C.c_int), ("bgr", C.c_int), ("dtype", C.c_int), ("out_bit_depth", C.c_int),
                ("matrix", C.c_int), ("full_range", C.c_int), ("chroma_loc", C.c_int), ("upsample", C.c_int),
                ("crop", C.c_int * 4), ("row_pitch", C.c_size_t), ("alpha", C.c_float)]


def make_packed_format(layout=PACKED_RGBA, dtype=OUT_U8, bgr=False, out_bit_depth=0, matrix=1, full_range=False, chroma_loc=0,
                       upsample=UPSAMPLE_LINEAR, crop=(0, 0, 0, 0), row_pitch=0, alpha=1.0):
    """xgpu_packed_format (include/xevd_hip.h): the packed display surfaces of xgpu_pic_output_device_packed"""
    f = PackedFormat()
    f.layout, f.bgr, f.dtype, f.out_bit_depth = int(layout), int(bool(bgr)), int(dtype), int(out_bit_depth)
    f.matrix, f.full_range, f.chroma_loc, f.upsample = int(matrix), int(bool(full_range)), int(chroma_loc), int(upsample)
    for i in range(4):
        f.crop[i] = int(crop[i])
    f.row_pitch, f.alpha = int(row_pitch), float(alpha)
    return f


def packed_coeffs(lib, fmt, bit_depth):
    """xgpu_output_packed_coeffs -> (coef [5], shift, fcoef float32 [5], alpha_code), or the negative code"""
    coef, shift, fcoef, alpha = (C.c_int32 * 5)(), C.c_int(), (C.c_float * 5)(), C.c_uint32()
    rc = lib.xgpu_output_packed_coeffs(C.byref(fmt), int(bit_depth), coef, C.byref(shift), fcoef, C.byref(alpha))
    if rc < 0:
        return rc
    return list(coef), shift.value, np.array(list(fcoef), np.float32), alpha.value


MAX_LUT3D = 8


def lut3d_from_float(lib, rgb):
    """xgpu_lut3d_from_float: float32 [n, n, n, 3] (or [n^3, 3]) in .cube order -> uint16 [n^3, 3], or the negative code"""
    rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    n = int(round(rgb.shape[0] ** (1.0 / 3.0)))
    if n * n * n != rgb.shape[0]:
        raise ValueError(f"{rgb.shape[0]} nodes are no cube")
    nodes = np.empty((n * n * n, 3), np.uint16)
    rc = lib.xgpu_lut3d_from_float(rgb.ctypes.data_as(C.POINTER(C.c_float)), n, nodes.ctypes.data_as(C.POINTER(C.c_uint16)))
    return rc if rc < 0 else nodes


def lut3d_identity(lib, n):
    """xgpu_lut3d_identity -> uint16 [n^3, 3], or the negative code"""
    nodes = np.empty((max(int(n), 0) ** 3, 3), np.uint16)
    rc = lib.xgpu_lut3d_identity(int(n), nodes.ctypes.data_as(C.POINTER(C.c_uint16)))
    return rc if rc < 0 else nodes


def lut3d_shaper(lib, bit_depth, curve=None, in_min=None, in_max=None):
    """xgpu_lut3d_shaper -> uint16 [3, 2^bit_depth], or the negative code.  curve: None or float32 [n_curve, 3]"""
    fp = C.POINTER(C.c_float)
    if curve is not None:
        curve = np.ascontiguousarray(curve, np.float32).reshape(-1, 3)
    lo = None if in_min is None else (C.c_float * 3)(*[float(v) for v in in_min])
    hi = None if in_max is None else (C.c_float * 3)(*[float(v) for v in in_max])
    out = np.empty((3, 1 << max(min(int(bit_depth), 16), 0)), np.uint16)
    rc = lib.xgpu_lut3d_shaper(int(bit_depth), None if curve is None else curve.ctypes.data_as(fp), 0 if curve is None else curve.shape[0], lo, hi,
                               out.ctypes.data_as(C.POINTER(C.c_uint16)))
    return rc if rc < 0 else out


MAX_DITHER = 4


class DitherParams(C.Structure):
    _fields_ = [("handle", C.c_int), ("phase_x", C.c_int), ("phase_y", C.c_int)]


def make_dither_params(handle, phase=(0, 0)):
    """xgpu_dither_params (include/xevd_hip.h): the matrix of a dithered output call and its phase (x, y)"""
    d = DitherParams()
    d.handle, d.phase_x, d.phase_y = int(handle), int(phase[0]), int(phase[1])
    return d


def dither_bayer(lib, log2n):
    """xgpu_dither_bayer -> uint16 [n, n] ranks below n^2, or the negative code"""
    n = 1 << max(min(int(log2n), 7), 0)
    rank = np.empty((n, n), np.uint16)
    rc = lib.xgpu_dither_bayer(int(log2n), rank.ctypes.data_as(C.POINTER(C.c_uint16)))
    return rc if rc < 0 else rank


def dither_blue(lib, log2n, seed=1):
    """xgpu_dither_blue -> uint16 [n, n], a permutation of 0 .. n^2 - 1, or the negative code"""
    n = 1 << max(min(int(log2n), 7), 0)
    rank = np.empty((n, n), np.uint16)
    rc = lib.xgpu_dither_blue(int(log2n), int(seed) & 0xFFFFFFFF, rank.ctypes.data_as(C.POINTER(C.c_uint16)))
    return rc if rc < 0 else rank


def dither_phase(lib, index, mw, mh):
    """xgpu_dither_phase -> (phase_x, phase_y) of picture `index`, or the negative code"""
    px, py = C.c_int(), C.c_int()
    rc = lib.xgpu_dither_phase(int(index) & 0xFFFFFFFF, int(mw), int(mh), C.byref(px), C.byref(py))
    return rc if rc < 0 else (px.value, py.value)


MAX_OVERLAY_LAYERS, MAX_OVERLAY_BOXES = 16, 256
OVL_RGBA8, OVL_BGRA8, OVL_A8, OVL_BOX = 0, 1, 2, 3


class OverlayLayer(C.Structure):
    _fields_ = [("kind", C.c_int), ("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int), ("opacity", C.c_int),
                ("d_pixels", C.c_void_p), ("pitch", C.c_size_t), ("colour", C.c_uint8 * 4), ("fill", C.c_uint8 * 4), ("thickness", C.c_int)]


class OverlayBoxes(C.Structure):
    _fields_ = [("box_format", C.c_int), ("d_boxes", C.c_void_p), ("capacity", C.c_int), ("d_count", C.c_void_p), ("d_labels", C.c_void_p),
                ("palette", (C.c_uint8 * 4) * 16), ("n_palette", C.c_int), ("thickness", C.c_int), ("fill_alpha", C.c_int)]


def make_overlay_layer(kind, x, y, width, height, opacity=255, d_pixels=0, pitch=0, colour=(255, 255, 255, 255), fill=(0, 0, 0, 0), thickness=1):
    """xgpu_overlay_layer (include/xevd_hip.h): one layer of an overlaid output call"""
    l = OverlayLayer()
    l.kind, l.x, l.y, l.width, l.height, l.opacity = int(kind), int(x), int(y), int(width), int(height), int(opacity)
    l.d_pixels, l.pitch, l.thickness = int(d_pixels) or None, int(pitch), int(thickness)
    for i in range(4):
        l.colour[i], l.fill[i] = int(colour[i]), int(fill[i])
    return l


def make_overlay_boxes(box_format, d_boxes, capacity, d_count=0, d_labels=0, palette=((255, 0, 0, 255),), thickness=2, fill_alpha=0, n_palette=None):
    """xgpu_overlay_boxes (include/xevd_hip.h): the boxes in device memory of an overlaid output call"""
    b = OverlayBoxes()
    b.box_format, b.d_boxes, b.capacity = int(box_format), int(d_boxes) or None, int(capacity)
    b.d_count, b.d_labels = int(d_count) or None, int(d_labels) or None
    for i, p in enumerate(list(palette)[:16]):
        for k in range(4):
            b.palette[i][k] = int(p[k])
    b.n_palette = len(palette) if n_palette is None else int(n_palette)
    b.thickness, b.fill_alpha = int(thickness), int(fill_alpha)
    return b


def overlay_coeffs(lib, fmt, bit_depth):
    """xgpu_overlay_coeffs -> (m [9], offsets [3], shift), or the negative code"""
    m, off, shift = (C.c_int32 * 9)(), (C.c_int32 * 3)(), C.c_int()
    rc = lib.xgpu_overlay_coeffs(C.byref(fmt), int(bit_depth), m, off, C.byref(shift))
    return rc if rc < 0 else (list(m), list(off), shift.value)


def overlay_box_snap(lib, box, box_format=None):
    """xgpu_overlay_box_snap, the device's snapping rule on the host: box (x, y, w, h) of ints (BOX_XYWH_I32) or (x1, y1, x2, y2) of floats (BOX_XYXY_F32; the
    default for a float box) -> (x0, y0, x1, y1), None for a skipped box, or the negative code"""
    raw = np.ascontiguousarray(box)
    if box_format is None:
        box_format = BOX_XYXY_F32 if raw.dtype.kind == "f" else BOX_XYWH_I32
    raw = raw.astype(np.float32 if box_format == BOX_XYXY_F32 else np.int32)
    r = (C.c_int * 4)()
    rc = lib.xgpu_overlay_box_snap(int(box_format), raw.ctypes.data_as(C.c_void_p), r)
    return rc if rc < 0 else (tuple(r) if rc else None)


SIDE_BLOCKS, SIDE_FLOW_PLANAR, SIDE_FLOW_INTERLEAVED = 0, 1, 2
MODE_IBC = 6


class SideFormat(C.Structure):
    _fields_ = [("layout", C.c_int), ("dtype", C.c_int), ("lists", C.c_int), ("per_poc", C.c_int), ("crop", C.c_int * 4), ("row_pitch", C.c_size_t)]


def make_side_format(layout=SIDE_BLOCKS, dtype=OUT_U16, lists=3, per_poc=False, crop=(0, 0, 0, 0), row_pitch=0):
    """xgpu_side_format (include/xevd_hip.h): BLOCKS - nine int16 planes per 4x4 unit (dtype OUT_U16, no crop); FLOW - a dense motion field, OUT_F16 / OUT_F32,
    lists 1 = list 0, 2 = list 1, 3 = both"""
    f = SideFormat()
    f.layout, f.dtype, f.lists, f.per_poc = int(layout), int(dtype), int(lists), int(per_poc)
    for i in range(4):
        f.crop[i] = int(crop[i])
    f.row_pitch = int(row_pitch)
    return f


RESID_YUV420, RESID_444_PLANAR, RESID_444_INTERLEAVED, RESID_ENERGY = 0, 1, 2, 3


class ResidFormat(C.Structure):
    _fields_ = [("layout", C.c_int), ("dtype", C.c_int), ("crop", C.c_int * 4), ("row_pitch", C.c_size_t)]


def make_resid_format(layout=RESID_YUV420, dtype=OUT_U16, crop=(0, 0, 0, 0), row_pitch=0):
    """xgpu_resid_format (include/xevd_hip.h): YUV420 - int16 planes Y, Cb, Cr (dtype OUT_U16); 444 planar / interleaved - OUT_U16 / OUT_F16 / OUT_F32, chroma
    replicated; ENERGY - sum |r| per 4x4 luma unit and component, OUT_F32, no crop"""
    f = ResidFormat()
    f.layout, f.dtype = int(layout), int(dtype)
    for i in range(4):
        f.crop[i] = int(crop[i])
    f.row_pitch = int(row_pitch)
    return f


CMP_REF_PIC, CMP_REF_YUV420 = 0, 1


class CompareRef(C.Structure):
    _fields_ = [("kind", C.c_int), ("pic", C.c_int), ("d_yuv", C.c_void_p), ("size", C.c_size_t), ("dtype", C.c_int), ("row_pitch", C.c_size_t)]


class CompareParams(C.Structure):
    _fields_ = [("crop", C.c_int * 4), ("ssim", C.c_int), ("block_map", C.c_int)]


class CompareResult(C.Structure):
    """xgpu_compare_result: 160 bytes, written by the device"""
    _fields_ = [("n", C.c_uint64 * 3), ("sse", C.c_uint64 * 3), ("n_diff", C.c_uint64 * 3), ("first_diff", C.c_uint64 * 3), ("max_abs", C.c_uint32 * 3),
                ("reserved", C.c_uint32), ("ssim_windows", C.c_uint64 * 3), ("ssim_q30", C.c_int64 * 3)]


def make_compare_ref(pic=None, d_yuv=None, size=0, dtype=OUT_U16, row_pitch=0):
    """xgpu_compare_ref (include/xevd_hip.h): a slot (pic=), or 4:2:0 planes in device memory (d_yuv= the address, size= the bytes there, dtype OUT_U8 / OUT_U16,
    row_pitch= the luma pitch in bytes, 0 = tight)"""
    r = CompareRef()
    if pic is not None:
        r.kind, r.pic = CMP_REF_PIC, int(pic)
    else:
        r.kind, r.d_yuv, r.size, r.dtype, r.row_pitch = CMP_REF_YUV420, d_yuv, int(size), int(dtype), int(row_pitch)
    return r


def make_compare_params(crop=(0, 0, 0, 0), ssim=True, block_map=False):
    p = CompareParams()
    for i in range(4):
        p.crop[i] = int(crop[i])
    p.ssim, p.block_map = int(ssim), int(block_map)
    return p


def compare_result_dict(res):
    """a CompareResult, or its 160 bytes as anything numpy reads -> dict of lists of Python ints, one entry per component Y, Cb, Cr"""
    if not isinstance(res, CompareResult):
        res = CompareResult.from_buffer_copy(np.ascontiguousarray(res).tobytes())
    return {k: [int(v) for v in getattr(res, k)] for k in ("n", "sse", "n_diff", "first_diff", "max_abs", "ssim_windows", "ssim_q30")}


def psnr(result, bit_depth):
    """host only: [Y, Cb, Cr] 10 log10(L^2 n / sse) with L = 2^bit_depth - 1 of a compare result (CompareResult or compare_result_dict's dict); inf for sse == 0"""
    import math
    d = result if isinstance(result, dict) else compare_result_dict(result)
    peak = ((1 << int(bit_depth)) - 1) ** 2
    return [math.inf if s == 0 else 10.0 * math.log10(peak * n / s) for n, s in zip(d["n"], d["sse"])]


def ssim(result):
    """host only: [Y, Cb, Cr] ssim_q30 / (ssim_windows 2^30) of a compare result; nan for a plane without windows (or a call with ssim off)"""
    d = result if isinstance(result, dict) else compare_result_dict(result)
    return [q / (n * float(1 << 30)) if n else float("nan") for q, n in zip(d["ssim_q30"], d["ssim_windows"])]


class StatsParams(C.Structure):
    _fields_ = [("crop", C.c_int * 4), ("hist_bits", C.c_int), ("pctl_e4", C.c_int * 2), ("light", C.c_int), ("matrix", C.c_int), ("full_range", C.c_int),
                ("chroma_loc", C.c_int), ("upsample", C.c_int), ("transfer", C.c_int)]


class StatsResult(C.Structure):
    """xgpu_stats_result: 176 bytes, written by the device"""
    _fields_ = [("n", C.c_uint64 * 3), ("sum", C.c_uint64 * 3), ("sum_sq", C.c_uint64 * 3), ("min", C.c_uint32 * 3), ("max", C.c_uint32 * 3),
                ("pctl", (C.c_uint32 * 2) * 3), ("light_n", C.c_uint64), ("light_sum", C.c_double), ("light_mean", C.c_double),
                ("light_max_code", C.c_uint32), ("light_pctl_code", C.c_uint32 * 2), ("reserved", C.c_uint32),
                ("light_max", C.c_float), ("light_pctl", C.c_float * 2), ("reserved2", C.c_float)]


STATS_TRANSFERS = (1, 4, 5, 6, 8, 13, 14, 15, 16, 18)      # the H.273 TransferCharacteristics xgpu_stats_lin knows (xgpu_colour_transform's list)


def make_stats_params(crop=(0, 0, 0, 0), hist_bits=8, pctl_e4=(100, 9999), light=False, matrix=1, full_range=False, chroma_loc=0, upsample=UPSAMPLE_LINEAR,
                      transfer=1):
    """xgpu_stats_params (include/xevd_hip.h): the crop, 2^hist_bits bins per component (0: none), two percentiles in 1 / 10000; light: also the histogram of
    max(R', G', B') and the light level, with the matrix / range / chroma siting / upsampling of xgpu_output_format and the stream's transfer characteristic"""
    p = StatsParams()
    for i in range(4):
        p.crop[i] = int(crop[i])
    p.hist_bits, p.light = int(hist_bits), int(light)
    p.pctl_e4[0], p.pctl_e4[1] = int(pctl_e4[0]), int(pctl_e4[1])
    p.matrix, p.full_range, p.chroma_loc, p.upsample, p.transfer = int(matrix), int(full_range), int(chroma_loc), int(upsample), int(transfer)
    return p


def stats_result_dict(res):
    """a StatsResult, or its 176 bytes as anything numpy reads -> dict: n, sum, sum_sq, min, max as lists of three Python ints, pctl as three pairs, the light
    fields as ints and floats (light_sum, light_mean: float64; light_max, light_pctl: the float32 values)"""
    if not isinstance(res, StatsResult):
        res = StatsResult.from_buffer_copy(np.ascontiguousarray(res).tobytes())
    d = {k: [int(v) for v in getattr(res, k)] for k in ("n", "sum", "sum_sq", "min", "max")}
    d["pctl"] = [[int(v) for v in row] for row in res.pctl]
    d.update(light_n=int(res.light_n), light_sum=float(res.light_sum), light_mean=float(res.light_mean), light_max_code=int(res.light_max_code),
             light_pctl_code=[int(v) for v in res.light_pctl_code], light_max=float(res.light_max), light_pctl=[float(v) for v in res.light_pctl])
    return d


def stats_moments(d):
    """host only: ([Y, Cb, Cr] mean, [Y, Cb, Cr] population variance) of a stats result's integers as exact fractions.Fraction (float() them as needed)"""
    from fractions import Fraction
    mean = [Fraction(s, n) for s, n in zip(d["sum"], d["n"])]
    return mean, [Fraction(q, n) - m * m for q, n, m in zip(d["sum_sq"], d["n"], mean)]


def stats_lin(lib, transfer, bit_depth):
    """xgpu_stats_lin as a float32 array of 2^bit_depth entries, or the negative code"""
    buf = (C.c_float * 4096)()
    rc = lib.xgpu_stats_lin(int(transfer), int(bit_depth), buf)
    return rc if rc < 0 else np.frombuffer(buf, np.float32, 1 << int(bit_depth)).copy()


SCALE_BILINEAR, SCALE_AREA = 0, 1


class ScaleParams(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("filter", C.c_int), ("normalize", C.c_int), ("mean", C.c_float * 3), ("inv_std", C.c_float * 3)]


def make_scale_params(width, height, filter=SCALE_BILINEAR, mean=None, std=None, inv_std=None):
    """xgpu_scale_params (include/xevd_hip.h): the destination size, the filter, and - when mean or std (or inv_std) is given - the normalise
    out = (v - mean[k]) * inv_std[k], k the channel's position in the output; inv_std = float32(1) / float32(std), one float32 division"""
    p = ScaleParams()
    p.width, p.height, p.filter = int(width), int(height), int(filter)
    p.normalize = int(mean is not None or std is not None or inv_std is not None)
    m = np.zeros(3, np.float32) if mean is None else np.broadcast_to(np.asarray(mean, np.float32), (3,))
    if inv_std is not None:
        i = np.broadcast_to(np.asarray(inv_std, np.float32), (3,))
    elif std is not None:
        i = np.float32(1) / np.broadcast_to(np.asarray(std, np.float32), (3,))
    else:
        i = np.ones(3, np.float32)
    for k in range(3):
        p.mean[k], p.inv_std[k] = float(m[k]), float(i[k])
    return p


def scale_taps(lib, n_plane, subsampling, siting_half_luma, n_dst, filter=SCALE_BILINEAR):
    """xgpu_scale_taps as numpy arrays: (first [n_dst] int32, count [n_dst] int32, w [n_dst][widest] int16 - row o: count[o] weights of sum 16384, then
    zeros), or the negative code"""
    first, count = np.zeros(max(int(n_dst), 1), np.int32), np.zeros(max(int(n_dst), 1), np.int32)
    pi, pc = first.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_int32))
    widest = lib.xgpu_scale_taps(int(n_plane), int(subsampling), int(siting_half_luma), int(n_dst), int(filter), pi, pc, None, 0)
    if widest < 0:
        return widest
    w = np.zeros((int(n_dst), widest), np.int16)
    rc = lib.xgpu_scale_taps(int(n_plane), int(subsampling), int(siting_half_luma), int(n_dst), int(filter), pi, pc, w.ctypes.data_as(C.POINTER(C.c_int16)), widest)
    return rc if rc < 0 else (first, count, w)


RESAMPLE_CATMULL_ROM, RESAMPLE_CUBIC_075, RESAMPLE_MITCHELL = 0, 1, 2
RESAMPLE_KERNELS = {"catmull-rom": RESAMPLE_CATMULL_ROM, "bicubic": RESAMPLE_CATMULL_ROM, "cubic-0.75": RESAMPLE_CUBIC_075, "mitchell": RESAMPLE_MITCHELL}


class ResampleParams(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("kernel", C.c_int), ("antialias", C.c_int), ("normalize", C.c_int), ("mean", C.c_float * 3),
                ("inv_std", C.c_float * 3)]


def make_resample_params(width, height, kernel=RESAMPLE_CATMULL_ROM, antialias=True, mean=None, std=None, inv_std=None):
    """xgpu_resample_params (include/xevd_hip.h): the destination size, the cubic kernel (a RESAMPLE_* code or a name of RESAMPLE_KERNELS), antialias, and the
    normalise of make_scale_params"""
    sc = make_scale_params(width, height, mean=mean, std=std, inv_std=inv_std)
    p = ResampleParams()
    p.width, p.height, p.kernel, p.antialias, p.normalize = sc.width, sc.height, int(RESAMPLE_KERNELS.get(kernel, kernel)), int(antialias), sc.normalize
    for k in range(3):
        p.mean[k], p.inv_std[k] = sc.mean[k], sc.inv_std[k]
    return p


def resample_taps(lib, n_plane, subsampling, siting_half_luma, n_dst, kernel=RESAMPLE_CATMULL_ROM, antialias=True):
    """xgpu_resample_taps as numpy arrays: (first [n_dst] int32, count [n_dst] int32, w [n_dst][widest] int16 - row o: count[o] weights of either sign and of
    sum 16384, then zeros), or the negative code"""
    first, count = np.zeros(max(int(n_dst), 1), np.int32), np.zeros(max(int(n_dst), 1), np.int32)
    pi, pc = first.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_int32))
    args = (int(n_plane), int(subsampling), int(siting_half_luma), int(n_dst), int(RESAMPLE_KERNELS.get(kernel, kernel)), int(antialias))
    widest = lib.xgpu_resample_taps(*args, pi, pc, None, 0)
    if widest < 0:
        return widest
    w = np.zeros((int(n_dst), widest), np.int16)
    rc = lib.xgpu_resample_taps(*args, pi, pc, w.ctypes.data_as(C.POINTER(C.c_int16)), widest)
    return rc if rc < 0 else (first, count, w)


def scale_taps_device(lib, ctx, n_plane, subsampling, siting_half_luma, n_dst, filter=SCALE_BILINEAR, extra=0):
    """xgpu_test_scale_taps_device - scale_taps' arrays made by the device's row builder (ctx: an open context); extra: columns beyond the widest row"""
    first, count = np.zeros(max(int(n_dst), 1), np.int32), np.zeros(max(int(n_dst), 1), np.int32)
    pi, pc = first.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_int32))
    widest = lib.xgpu_test_scale_taps_device(ctx, int(n_plane), int(subsampling), int(siting_half_luma), int(n_dst), int(filter), pi, pc, None, 0)
    if widest < 0:
        return widest
    w = np.full((int(n_dst), widest + int(extra)), -1, np.int16)
    rc = lib.xgpu_test_scale_taps_device(ctx, int(n_plane), int(subsampling), int(siting_half_luma), int(n_dst), int(filter), pi, pc,
                                         w.ctypes.data_as(C.POINTER(C.c_int16)), w.shape[1])
    return rc if rc < 0 else (first, count, w)


def scale_taps_ex(lib, n_plane, subsampling, siting_half_luma, n_dst, dst_subsampling=1, dst_siting_half_luma=0, filter=SCALE_BILINEAR):
    """xgpu_scale_taps_ex as numpy arrays - scale_taps for a destination with a subsampling and a siting of its own (the chroma planes of a surface ladder):
    (first, count, w) as scale_taps gives them, or the negative code"""
    first, count = np.zeros(max(int(n_dst), 1), np.int32), np.zeros(max(int(n_dst), 1), np.int32)
    pi, pc = first.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_int32))
    args = (int(n_plane), int(subsampling), int(siting_half_luma), int(n_dst), int(dst_subsampling), int(dst_siting_half_luma), int(filter))
    widest = lib.xgpu_scale_taps_ex(*args, pi, pc, None, 0)
    if widest < 0:
        return widest
    w = np.zeros((int(n_dst), widest), np.int16)
    rc = lib.xgpu_scale_taps_ex(*args, pi, pc, w.ctypes.data_as(C.POINTER(C.c_int16)), widest)
    return rc if rc < 0 else (first, count, w)


MAX_RUNGS = 8


class SurfaceRung(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("row_pitch", C.c_size_t), ("d_dst", C.c_void_p), ("dst_size", C.c_size_t)]


class LadderParams(C.Structure):
    _fields_ = [("filter", C.c_int), ("dst_chroma_loc", C.c_int)]


def make_ladder_params(filter=SCALE_BILINEAR, dst_chroma_loc=None):
    """xgpu_ladder_params (include/xevd_hip.h): the filter and the chroma siting of the rungs (None: the source's, f->chroma_loc)"""
    p = LadderParams()
    p.filter, p.dst_chroma_loc = int(filter), -1 if dst_chroma_loc is None else int(dst_chroma_loc)
    return p


def make_rungs(rungs):
    """[(width, height, row_pitch, d_dst, dst_size), ...] -> an array of xgpu_surface_rung (d_dst may be None)"""
    arr = (SurfaceRung * max(len(rungs), 1))()
    for i, (w, h, pitch, ptr, size) in enumerate(rungs):
        arr[i].width, arr[i].height, arr[i].row_pitch, arr[i].d_dst, arr[i].dst_size = int(w), int(h), int(pitch), ptr, int(size)
    return arr


FIT_STRETCH, FIT_LETTERBOX = 0, 1
MAX_ROIS = 1024


class Roi(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class RoiParams(C.Structure):
    _fields_ = [("fit", C.c_int), ("pad", C.c_float * 3), ("image_pitch", C.c_size_t)]


def make_rois(rois):
    """[(x, y, width, height), ...] in luma samples -> an array of xgpu_roi"""
    a = (Roi * max(len(rois), 1))()
    for i, r in enumerate(rois):
        a[i].x, a[i].y, a[i].width, a[i].height = (int(v) for v in r)
    return a


def make_roi_params(fit=FIT_STRETCH, pad=0.0, image_pitch=0):
    """xgpu_roi_params (include/xevd_hip.h): fit FIT_STRETCH / FIT_LETTERBOX, the letterbox's pad value - one value or three, by the channel's position in the
    output, before the normalise - and the bytes between two images (0: tight)"""
    p = RoiParams()
    p.fit, p.image_pitch = int(fit), int(image_pitch)
    v = np.broadcast_to(np.asarray(pad, np.float32), (3,))
    for k in range(3):
        p.pad[k] = float(v[k])
    return p


def roi_inner(lib, roi, size, fit=FIT_LETTERBOX):
    """xgpu_roi_inner: (x, y, width, height) of the filtered part of rectangle roi = (x, y, width, height) inside an image of size = (H, W), or the negative code"""
    r = make_rois([roi])
    sc = make_scale_params(size[1], size[0])
    inner = (C.c_int * 4)()
    rc = lib.xgpu_roi_inner(r, C.byref(sc), int(fit), inner)
    return rc if rc < 0 else tuple(inner)


BOX_XYWH_I32, BOX_XYXY_F32 = 0, 1
ROI_OK, ROI_UNUSED, ROI_INVALID, ROI_EMPTY, ROI_TOO_LARGE, ROI_RATIO = range(6)


class RoiBounds(C.Structure):
    _fields_ = [("max_width", C.c_int), ("max_height", C.c_int)]


class RoiResult(C.Structure):
    _fields_ = [("status", C.c_int), ("used", Roi), ("inner", C.c_int * 4)]


def make_roi_bounds(max_roi=None):
    """xgpu_roi_bounds from max_roi = (H, W), the largest snapped rectangle a device-box call is sized for; None or 0: the picture minus the crop"""
    b = RoiBounds()
    if max_roi is not None:
        b.max_height, b.max_width = int(max_roi[0]), int(max_roi[1])
    return b


def roi_snap(lib, box, pic_size, box_format=None):
    """xgpu_roi_snap, the device's snapping rule on the host: box (x, y, w, h) of ints (BOX_XYWH_I32) or (x1, y1, x2, y2) of floats (BOX_XYXY_F32; the default
    for a box that holds a float), pic_size = (H, W) of the picture minus the crop -> (status, (x, y, width, height)), or the negative code"""
    if box_format is None:
        box_format = BOX_XYXY_F32 if any(isinstance(v, (float, np.floating)) for v in box) else BOX_XYWH_I32
    raw = (C.c_float * 4)(*[float(np.float32(v)) for v in box]) if box_format == BOX_XYXY_F32 else (C.c_int * 4)(*[int(v) for v in box])
    used = Roi()
    rc = lib.xgpu_roi_snap(int(box_format), raw, int(pic_size[1]), int(pic_size[0]), C.byref(used))
    return rc if rc < 0 else (rc, (used.x, used.y, used.width, used.height))


def tile_rois(width, height, tile_w, tile_h):
    """the grid of tile_w x tile_h tiles (even) that covers a width x height picture, row by row: where the size is no multiple of the tile the last column / row
    is moved back inside the picture (it overlaps its neighbour), so every tile has the same size and the tiles share one set of tap tables"""
    tile_w, tile_h = min(int(tile_w), int(width)), min(int(tile_h), int(height))
    if tile_w < 2 or tile_h < 2 or (tile_w | tile_h | int(width) | int(height)) & 1:
        raise ValueError(f"tile_rois: tile {tile_w}x{tile_h} in {width}x{height}: sizes must be even and at least 2")
    xs = [min(x, width - tile_w) for x in range(0, width, tile_w)]
    ys = [min(y, height - tile_h) for y in range(0, height, tile_h)]
    return [(x, y, tile_w, tile_h) for y in ys for x in xs]


WARP_CLAMP, WARP_PAD = 0, 1
WARP_LIN_LIMIT, WARP_OFF_LIMIT = 64 << 16, 1 << 36      # |m[0]|, |m[1]|, |m[3]|, |m[4]| / |m[2]|, |m[5]|


class WarpMap(C.Structure):
    _fields_ = [("m", C.c_int64 * 6)]


class WarpParams(C.Structure):
    _fields_ = [("samples", C.c_int), ("border", C.c_int), ("pad", C.c_float * 3), ("image_pitch", C.c_size_t)]


def make_warp_params(samples=1, border=WARP_CLAMP, pad=0.0, image_pitch=0):
    """xgpu_warp_params (include/xevd_hip.h): sub-positions per axis (1, 2, 4), WARP_CLAMP / WARP_PAD, the pad value - one value or three, by the channel's
    position in the output, before the normalise - and the bytes between two images (0: tight)"""
    p = WarpParams()
    p.samples, p.border, p.image_pitch = int(samples), int(border), int(image_pitch)
    v = np.broadcast_to(np.asarray(pad, np.float32), (3,))
    for k in range(3):
        p.pad[k] = float(v[k])
    return p


def make_warp_maps(maps):
    """[(m0 .. m5), ...] or an int64 array [N, 6] of Q16 maps -> an array of xgpu_warp_map"""
    m = np.ascontiguousarray(maps, np.int64).reshape(-1, 6)
    return (WarpMap * len(m)).from_buffer_copy(m.tobytes()) if len(m) else (WarpMap * 1)()


def warp_from_matrix(lib, theta):
    """xgpu_warp_from_matrix: theta (six floats, destination pixel centres -> continuous source coordinates) -> the six Q16 integers, or the negative code"""
    out = WarpMap()
    rc = lib.xgpu_warp_from_matrix((C.c_double * 6)(*[float(v) for v in theta]), C.byref(out))
    return rc if rc < 0 else tuple(int(v) for v in out.m)


def warp_from_rotated_box(lib, cx, cy, w, h, angle_deg, dst_size):
    """xgpu_warp_from_rotated_box: the map that shows the w x h box centred at (cx, cy), turned by angle_deg, in an image of dst_size = (H, W); or the negative code"""
    out = WarpMap()
    rc = lib.xgpu_warp_from_rotated_box(float(cx), float(cy), float(w), float(h), float(angle_deg), int(dst_size[1]), int(dst_size[0]), C.byref(out))
    return rc if rc < 0 else tuple(int(v) for v in out.m)


def output_warp_check(lib, fmt, sc, wp, maps, n, width, height, bit_depth):
    """xgpu_output_warp_check -> (code, bad_index); maps: make_warp_maps' array, or None for maps in device memory"""
    bad = C.c_int(-1)
    rc = lib.xgpu_output_warp_check(C.byref(fmt), C.byref(sc), C.byref(wp), maps, int(n), int(width), int(height), int(bit_depth), C.byref(bad))
    return rc, bad.value


def output_warp_size(lib, fmt, sc, wp, n, width, height, bit_depth):
    """xgpu_output_warp_size: the bytes the batch needs, 0 = refused"""
    return lib.xgpu_output_warp_size(C.byref(fmt), C.byref(sc), C.byref(wp), int(n), int(width), int(height), int(bit_depth))


GRID_Q16_I32, GRID_F32 = 0, 1
GRID_INVALID = -(1 << 31)      # INT32_MIN in either coordinate of a Q16 node: the node is invalid


class RemapParams(C.Structure):
    _fields_ = [("grid_format", C.c_int), ("step_log2", C.c_int), ("samples", C.c_int), ("border", C.c_int), ("pad", C.c_float * 3), ("grid_pitch", C.c_size_t),
                ("image_pitch", C.c_size_t)]


class RemapLens(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "nfx", "nfy", "ncx", "ncy")]


def make_remap_params(grid_format=GRID_Q16_I32, step_log2=0, samples=1, border=WARP_CLAMP, pad=0.0, grid_pitch=0, image_pitch=0):
    """xgpu_remap_params (include/xevd_hip.h): GRID_Q16_I32 / GRID_F32, a node every 2^step_log2 pixels, sub-positions per axis (1, 2, 4), WARP_CLAMP / WARP_PAD,
    the pad value - one value or three, by the channel's position in the output, before the normalise - and the bytes between two grids / two images (0: tight)"""
    p = RemapParams()
    p.grid_format, p.step_log2, p.samples, p.border = int(grid_format), int(step_log2), int(samples), int(border)
    p.grid_pitch, p.image_pitch = int(grid_pitch), int(image_pitch)
    v = np.broadcast_to(np.asarray(pad, np.float32), (3,))
    for k in range(3):
        p.pad[k] = float(v[k])
    return p


def remap_grid_dims(lib, dst_size, step=0):
    """xgpu_remap_grid_dims: (gh, gw) of the grid of an image of dst_size = (H, W) with a node every 2^step pixels, or the negative code"""
    gw, gh = C.c_int(), C.c_int()
    rc = lib.xgpu_remap_grid_dims(int(dst_size[1]), int(dst_size[0]), int(step), C.byref(gw), C.byref(gh))
    return rc if rc < 0 else (gh.value, gw.value)


def remap_grid_size(lib, sc, rp, n):
    """xgpu_remap_grid_size: the bytes the call reads at d_grid, 0 = refused"""
    return lib.xgpu_remap_grid_size(C.byref(sc), C.byref(rp), int(n))


def output_remap_check(lib, fmt, sc, rp, n, width, height, bit_depth):
    """xgpu_output_remap_check: 0 or the code the call refuses with"""
    return lib.xgpu_output_remap_check(C.byref(fmt), C.byref(sc), C.byref(rp), int(n), int(width), int(height), int(bit_depth))


def output_remap_size(lib, fmt, sc, rp, n, width, height, bit_depth):
    """xgpu_output_remap_size: the bytes the batch needs, 0 = refused"""
    return lib.xgpu_output_remap_size(C.byref(fmt), C.byref(sc), C.byref(rp), int(n), int(width), int(height), int(bit_depth))


def _remap_helper(lib, name, arg, dst_size, step):
    dims = remap_grid_dims(lib, dst_size, step)
    if not isinstance(dims, tuple):
        return dims
    grid = np.empty((*dims, 2), np.int32)
    rc = getattr(lib, name)(arg, int(dst_size[1]), int(dst_size[0]), int(step), grid.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc if rc < 0 else grid


def remap_from_warp(lib, m, dst_size, step=0):
    """xgpu_remap_from_warp: the Q16 grid int32 [gh, gw, 2] of the affine map m (six Q16 integers) for an image of dst_size = (H, W), or the negative code"""
    return _remap_helper(lib, "xgpu_remap_from_warp", make_warp_maps([m]), dst_size, step)


def remap_from_homography(lib, h, dst_size, step=0):
    """xgpu_remap_from_homography: the Q16 grid of the 3 x 3 matrix h (nine floats, row-major; destination pixel centres -> continuous source coordinates)"""
    return _remap_helper(lib, "xgpu_remap_from_homography", (C.c_double * 9)(*[float(v) for v in np.asarray(h, np.float64).reshape(9)]), dst_size, step)


def remap_from_lens(lib, lens, dst_size, step=0):
    """xgpu_remap_from_lens: the Q16 grid that undistorts a Brown-Conrady lens; lens: a dict with fx, fy, cx, cy, the new camera nfx, nfy, ncx, ncy (default: the
    old one) and any of k1, k2, p1, p2, k3 (default 0)"""
    l = RemapLens()
    d = dict(lens)
    for k in ("fx", "fy", "cx", "cy"):
        d.setdefault("n" + k, d[k])
    for k, _ in RemapLens._fields_:
        setattr(l, k, float(d.get(k, 0.0)))
    return _remap_helper(lib, "xgpu_remap_from_lens", C.byref(l), dst_size, step)


CM_CURVE_U0, CM_CURVE_SIZE = 0x1F800000, 64 * 32 + 3


class ColourTransform(C.Structure):
    _fields_ = [("src_primaries", C.c_int), ("src_transfer", C.c_int), ("dst_primaries", C.c_int), ("dst_transfer", C.c_int),
                ("tone_map", C.c_int), ("src_peak", C.c_float), ("dst_peak", C.c_float), ("linear_scale", C.c_float)]


class ColourTables(C.Structure):
    _fields_ = [("n_lin", C.c_int), ("use_matrix", C.c_int), ("use_tone", C.c_int), ("use_encode", C.c_int),
                ("lin", C.c_float * 4096), ("matrix", C.c_float * 9), ("luma", C.c_float * 3), ("scale", C.c_float),
                ("tone", C.c_float * CM_CURVE_SIZE), ("encode", C.c_float * CM_CURVE_SIZE)]


def make_colour_transform(src_primaries=1, src_transfer=1, dst_primaries=1, dst_transfer=13, tone_map=False, src_peak=0.0, dst_peak=0.0, linear_scale=1.0):
    """xgpu_colour_transform (include/xevd_hip.h): H.273 code points of the stream and of the output; peaks in cd/m2, 0 = the default of the transfer"""
    t = ColourTransform()
    t.src_primaries, t.src_transfer, t.dst_primaries, t.dst_transfer = int(src_primaries), int(src_transfer), int(dst_primaries), int(dst_transfer)
    t.tone_map, t.src_peak, t.dst_peak, t.linear_scale = int(bool(tone_map)), float(src_peak), float(dst_peak), float(linear_scale)
    return t


def colour_tables(lib, fmt, cm, bit_depth):
    """xgpu_colour_tables as numpy arrays: dict(lin, matrix [3][3], luma, scale, tone or None, encode or None, use_matrix)"""
    t = ColourTables()
    rc = lib.xgpu_colour_tables(C.byref(fmt), C.byref(cm), int(bit_depth), C.byref(t))
    if rc < 0:
        return rc
    f32 = lambda a, n: np.frombuffer(a, np.float32, n).copy()      # noqa: E731
    return {"lin": f32(t.lin, t.n_lin), "matrix": f32(t.matrix, 9).reshape(3, 3), "luma": f32(t.luma, 3), "scale": np.float32(t.scale),
            "use_matrix": bool(t.use_matrix), "tone": f32(t.tone, CM_CURVE_SIZE) if t.use_tone else None,
            "encode": f32(t.encode, CM_CURVE_SIZE) if t.use_encode else None}


class FrameParams(C.Structure):
    _fields_ = [
        ("pic", C.c_int), ("poc", C.c_int), ("num_refp", C.c_int * 2),
        ("refp_pic", (C.c_int * 2) * XGPU_MAX_REFS), ("refp_poc", (C.c_int * 2) * XGPU_MAX_REFS),
        ("qp_u_offset", C.c_int), ("qp_v_offset", C.c_int),
        ("deblock_alpha_offset", C.c_int), ("deblock_beta_offset", C.c_int),
        ("deblock_on", C.c_int), ("alf_on", C.c_int),
    ]


XGPU_MAX_TILE_COLS, XGPU_MAX_TILE_ROWS = 20, 22


class TileGrid(C.Structure):
    _fields_ = [("n_cols", C.c_int), ("n_rows", C.c_int), ("col_bd", C.c_int * (XGPU_MAX_TILE_COLS + 1)), ("row_bd", C.c_int * (XGPU_MAX_TILE_ROWS + 1)),
                ("loop_filter_across_tiles", C.c_int)]


def make_tile_grid(d):
    """{'col_bd': [...], 'row_bd': [...], 'across': 0/1} (borders in CTUs, first 0, last = CTUs per row / column) -> TileGrid"""
    g = TileGrid()
    g.n_cols, g.n_rows = len(d["col_bd"]) - 1, len(d["row_bd"]) - 1
    for i, v in enumerate(d["col_bd"]):
        g.col_bd[i] = int(v)
    for i, v in enumerate(d["row_bd"]):
        g.row_bd[i] = int(v)
    g.loop_filter_across_tiles = int(d.get("across", 0))
    return g


def tile_grid_dict(g):
    return {"col_bd": [g.col_bd[i] for i in range(g.n_cols + 1)], "row_bd": [g.row_bd[i] for i in range(g.n_rows + 1)], "across": int(g.loop_filter_across_tiles)}


class CuBatch(C.Structure):
    _fields_ = [
        ("n_cu", C.c_int),
        ("x", C.POINTER(C.c_uint16)), ("y", C.POINTER(C.c_uint16)),
        ("log2w", C.POINTER(C.c_uint8)), ("log2h", C.POINTER(C.c_uint8)),
        ("pred_mode", C.POINTER(C.c_uint8)),
        ("refi", C.POINTER(C.c_int8)), ("mv", C.POINTER(C.c_int16)),
        ("qp", C.POINTER(C.c_uint8)), ("cbf", C.POINTER(C.c_uint8)), ("cbf_sub", C.POINTER(C.c_uint16)), ("ipm", C.POINTER(C.c_uint8)), ("ats", C.POINTER(C.c_uint8)), ("ats_inter", C.POINTER(C.c_uint8)),
        ("coef_off", C.POINTER(C.c_uint32)), ("coef", C.POINTER(C.c_int16)), ("n_coef", C.c_size_t),
        ("n_ctu", C.c_int), ("ctu_cu_start", C.POINTER(C.c_uint32)), ("constrained_intra_pred", C.c_int),
        ("affine", C.POINTER(C.c_uint8)), ("affine_mv", C.POINTER(C.c_int16)), ("dmvr", C.POINTER(C.c_uint8)), ("htdf_slice_qp", C.c_int),
        ("tiles", C.POINTER(TileGrid)), ("tree", C.POINTER(C.c_uint8)),
    ]


class AlfParams(C.Structure):
    _fields_ = [("enable", C.c_int * 3), ("luma_coef", C.POINTER(C.c_int16)), ("chroma_coef", C.POINTER(C.c_int16)),
                ("ctb_flag", C.POINTER(C.c_uint8)), ("across_tiles", C.c_int), ("tiles", C.POINTER(TileGrid))]


def make_alf_params(d):
    """{'enable': (y,u,v), 'luma_coef': [25][13], 'chroma_coef': [7], 'ctb_flag': [n_ctu] or None, 'across_tiles': 0/1}"""
    keep = {"luma": np.ascontiguousarray(d["luma_coef"], np.int16).reshape(25 * 13),
            "chroma": np.ascontiguousarray(d["chroma_coef"], np.int16).reshape(7),
            "flag": None if d.get("ctb_flag") is None else np.ascontiguousarray(d["ctb_flag"], np.uint8)}
    ap = AlfParams()
    for i in range(3):
        ap.enable[i] = int(d["enable"][i])
    ap.luma_coef = keep["luma"].ctypes.data_as(C.POINTER(C.c_int16))
    ap.chroma_coef = keep["chroma"].ctypes.data_as(C.POINTER(C.c_int16))
    if keep["flag"] is not None:
        ap.ctb_flag = keep["flag"].ctypes.data_as(C.POINTER(C.c_uint8))
    ap.across_tiles = int(d.get("across_tiles", 0))
    if d.get("tiles") is not None:
        keep["tiles"] = make_tile_grid(d["tiles"])
        ap.tiles = C.pointer(keep["tiles"])
    return ap, keep


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def make_cu_batch(b):
    """dict of numpy arrays (see synth.gen_frame) -> (CuBatch, keepalive)."""
    keep = {
        "x": np.ascontiguousarray(b["x"], np.uint16), "y": np.ascontiguousarray(b["y"], np.uint16),
        "log2w": np.ascontiguousarray(b["log2w"], np.uint8), "log2h": np.ascontiguousarray(b["log2h"], np.uint8),
        "pred_mode": np.ascontiguousarray(b["pred_mode"], np.uint8),
        "refi": np.ascontiguousarray(b["refi"], np.int8), "mv": np.ascontiguousarray(b["mv"], np.int16),
        "qp": np.ascontiguousarray(b["qp"], np.uint8), "cbf": np.ascontiguousarray(b["cbf"], np.uint8),
        "ipm": np.ascontiguousarray(b["ipm"], np.uint8),
        "cbf_sub": None if b.get("cbf_sub") is None else np.ascontiguousarray(b["cbf_sub"], np.uint16),
        "ats": None if b.get("ats") is None else np.ascontiguousarray(b["ats"], np.uint8),
        "ats_inter": None if b.get("ats_inter") is None else np.ascontiguousarray(b["ats_inter"], np.uint8),
        "affine": None if b.get("affine") is None else np.ascontiguousarray(b["affine"], np.uint8),
        "affine_mv": None if b.get("affine") is None else np.ascontiguousarray(b["affine_mv"], np.int16),
        "dmvr": None if b.get("dmvr") is None else np.ascontiguousarray(b["dmvr"], np.uint8),
        "tree": None if b.get("tree") is None else np.ascontiguousarray(b["tree"], np.uint8),
        "coef_off": np.ascontiguousarray(b["coef_off"], np.uint32),
        "coef": np.ascontiguousarray(b["coef"], np.int16),
        "ctu_cu_start": np.ascontiguousarray(b["ctu_cu_start"], np.uint32),
    }
    cb = CuBatch()
    cb.n_cu = len(keep["x"])
    cb.x, cb.y = _ptr(keep["x"], C.c_uint16), _ptr(keep["y"], C.c_uint16)
    cb.log2w, cb.log2h = _ptr(keep["log2w"], C.c_uint8), _ptr(keep["log2h"], C.c_uint8)
    cb.pred_mode = _ptr(keep["pred_mode"], C.c_uint8)
    cb.refi, cb.mv = _ptr(keep["refi"], C.c_int8), _ptr(keep["mv"], C.c_int16)
    cb.qp, cb.cbf, cb.ipm = _ptr(keep["qp"], C.c_uint8), _ptr(keep["cbf"], C.c_uint8), _ptr(keep["ipm"], C.c_uint8)
    if keep["cbf_sub"] is not None:
        cb.cbf_sub = _ptr(keep["cbf_sub"], C.c_uint16)
    if keep["ats"] is not None:
        cb.ats = _ptr(keep["ats"], C.c_uint8)
    if keep["ats_inter"] is not None:
        cb.ats_inter = _ptr(keep["ats_inter"], C.c_uint8)
    if keep["affine"] is not None:
        cb.affine, cb.affine_mv = _ptr(keep["affine"], C.c_uint8), _ptr(keep["affine_mv"], C.c_int16)
    if keep["dmvr"] is not None:
        cb.dmvr = _ptr(keep["dmvr"], C.c_uint8)
    if keep["tree"] is not None:
        cb.tree = _ptr(keep["tree"], C.c_uint8)
    cb.coef_off, cb.coef = _ptr(keep["coef_off"], C.c_uint32), _ptr(keep["coef"], C.c_int16)
    cb.n_coef = len(keep["coef"])
    cb.n_ctu = len(keep["ctu_cu_start"]) - 1
    cb.ctu_cu_start = _ptr(keep["ctu_cu_start"], C.c_uint32)
    cb.constrained_intra_pred = int(b.get("constrained_intra_pred", 0) or 0)
    cb.htdf_slice_qp = int(b.get("htdf_slice_qp", 0) or 0)
    if b.get("tiles") is not None:
        keep["tiles"] = make_tile_grid(b["tiles"])
        cb.tiles = C.pointer(keep["tiles"])
    return cb, keep


def make_seq_params(width, height, bit_depth=8, log2_ctu=6, device=0, iqt=0, admvp=0, addb=0, alf=0, max_pics=4,
                    bit_depth_chroma=None, eipd=0):
    sp = SeqParams()
    sp.device, sp.width, sp.height = device, width, height
    sp.bit_depth_luma = bit_depth
    sp.bit_depth_chroma = bit_depth if bit_depth_chroma is None else bit_depth_chroma
    sp.chroma_format_idc = 1
    sp.log2_ctu = log2_ctu
    sp.tool_iqt, sp.tool_admvp, sp.tool_addb, sp.tool_alf = iqt, admvp, addb, alf
    sp.max_pics = max_pics
    sp.tool_eipd = eipd
    return sp


_EXPORTS = {
    # name: (restype, argtypes)
    "xgpu_open": (C.c_int, [C.POINTER(SeqParams), C.POINTER(C.c_void_p)]),
    "xgpu_close": (None, [C.c_void_p]),
    "xgpu_sync": (C.c_int, [C.c_void_p]),
    "xgpu_last_error": (C.c_char_p, [C.c_void_p]),
    "xgpu_version": (C.c_char_p, []),
    "xgpu_pic_alloc": (C.c_int, [C.c_void_p]),
    "xgpu_pic_free": (C.c_int, [C.c_void_p, C.c_int]),
    "xgpu_pic_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "xgpu_pic_download": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "xgpu_pic_output_size": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_output": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "xgpu_pic_output_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    "xgpu_pic_output_wait": (C.c_int, [C.c_void_p, C.c_int]),
    "xgpu_pic_md5": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "xgpu_output_format_size": (C.c_size_t, [C.POINTER(OutputFormat), C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_output_device_size": (C.c_size_t, [C.c_void_p, C.POINTER(OutputFormat)]),
    "xgpu_pic_output_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_output_coeffs": (C.c_int, [C.POINTER(OutputFormat), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "xgpu_colour_tables": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ColourTransform), C.c_int, C.POINTER(ColourTables)]),
    "xgpu_pic_output_device_cm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ColourTransform), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_output_packed_size": (C.c_size_t, [C.POINTER(PackedFormat), C.c_int, C.c_int, C.c_int]),
    "xgpu_output_packed_check": (C.c_int, [C.POINTER(PackedFormat), C.POINTER(ColourTransform), C.c_int, C.c_int, C.c_int]),
    "xgpu_output_packed_coeffs": (C.c_int, [C.POINTER(PackedFormat), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "xgpu_pic_output_device_packed": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PackedFormat), C.POINTER(ColourTransform), C.c_void_p, C.c_size_t,
                                                C.c_void_p]),
    "xgpu_lut3d_from_float": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_uint16)]),
    "xgpu_lut3d_identity": (C.c_int, [C.c_int, C.POINTER(C.c_uint16)]),
    "xgpu_lut3d_shaper": (C.c_int, [C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint16)]),
    "xgpu_output_lut3d_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(PackedFormat), C.c_int, C.c_int, C.c_int, C.c_int]),
    "xgpu_lut3d_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_int)]),
    "xgpu_lut3d_destroy": (C.c_int, [C.c_void_p, C.c_int]),
    "xgpu_pic_output_device_lut3d": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_pic_output_device_packed_lut3d": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PackedFormat), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_dither_bayer": (C.c_int, [C.c_int, C.POINTER(C.c_uint16)]),
    "xgpu_dither_blue": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(C.c_uint16)]),
    "xgpu_dither_phase": (C.c_int, [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "xgpu_output_dither_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(PackedFormat), C.POINTER(ColourTransform), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int]),
    "xgpu_dither_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_int)]),
    "xgpu_dither_destroy": (C.c_int, [C.c_void_p, C.c_int]),
    "xgpu_pic_output_device_dithered": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ColourTransform), C.POINTER(DitherParams),
                                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_pic_output_device_packed_dithered": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PackedFormat), C.POINTER(ColourTransform),
                                                         C.POINTER(DitherParams), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_overlay_coeffs": (C.c_int, [C.POINTER(OutputFormat), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "xgpu_overlay_box_snap": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "xgpu_output_overlay_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(PackedFormat), C.POINTER(ColourTransform), C.POINTER(OverlayLayer), C.c_int,
                                            C.POINTER(OverlayBoxes), C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_output_device_overlaid": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ColourTransform), C.POINTER(OverlayLayer),
                                                  C.c_int, C.POINTER(OverlayBoxes), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_pic_output_device_packed_overlaid": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(PackedFormat), C.POINTER(ColourTransform),
                                                         C.POINTER(OverlayLayer), C.c_int, C.POINTER(OverlayBoxes), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_scale_taps": (C.c_int, [C.c_int] * 5 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int16), C.c_int]),
    "xgpu_output_scaled_size": (C.c_size_t, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.c_int, C.c_int, C.c_int]),
    "xgpu_output_scaled_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_output_device_scaled": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_scale_taps_ex": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int16), C.c_int]),
    "xgpu_output_ladder_rung_size": (C.c_size_t, [C.POINTER(OutputFormat), C.c_int, C.c_int, C.c_size_t, C.c_int]),
    "xgpu_output_ladder_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(LadderParams), C.POINTER(SurfaceRung), C.c_int, C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_output_device_ladder": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(LadderParams), C.POINTER(SurfaceRung), C.c_int,
                                                C.c_void_p]),
    "xgpu_roi_inner": (C.c_int, [C.POINTER(Roi), C.POINTER(ScaleParams), C.c_int, C.POINTER(C.c_int)]),
    "xgpu_output_rois_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RoiParams), C.POINTER(Roi), C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_int)]),
    "xgpu_output_rois_size": (C.c_size_t, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RoiParams), C.POINTER(Roi), C.c_int, C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_output_device_rois": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RoiParams), C.POINTER(Roi),
                                              C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_output_scaled_cm_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(ColourTransform), C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_output_device_scaled_cm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(ColourTransform),
                                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_pic_output_device_rois_cm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RoiParams), C.POINTER(Roi),
                                                 C.c_int, C.POINTER(ColourTransform), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_output_scaled_lin_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(ColourTransform), C.c_int, C.c_int, C.c_int]),
    "xgpu_output_rois_lin_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RoiParams), C.POINTER(Roi), C.c_int, C.POINTER(ColourTransform),
                                             C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "xgpu_pic_output_device_scaled_lin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(ColourTransform),
                                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_pic_output_device_rois_lin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RoiParams), C.POINTER(Roi),
                                                  C.c_int, C.POINTER(ColourTransform), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_resample_taps": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int16), C.c_int]),
    "xgpu_output_resampled_size": (C.c_size_t, [C.POINTER(OutputFormat), C.POINTER(ResampleParams), C.c_int, C.c_int, C.c_int]),
    "xgpu_output_resampled_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ResampleParams), C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_output_device_resampled": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ResampleParams), C.c_void_p, C.c_size_t,
                                                   C.c_void_p]),
    "xgpu_output_rois_resampled_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ResampleParams), C.POINTER(RoiParams), C.POINTER(Roi), C.c_int, C.c_int, C.c_int,
                                                   C.c_int, C.POINTER(C.c_int)]),
    "xgpu_output_rois_resampled_size": (C.c_size_t, [C.POINTER(OutputFormat), C.POINTER(ResampleParams), C.POINTER(RoiParams), C.POINTER(Roi), C.c_int, C.c_int, C.c_int,
                                                     C.c_int]),
    "xgpu_pic_output_device_rois_resampled": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ResampleParams), C.POINTER(RoiParams),
                                                        C.POINTER(Roi), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_roi_snap": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(Roi)]),
    "xgpu_output_rois_dev_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RoiParams), C.POINTER(RoiBounds)] + [C.c_int] * 5),
    "xgpu_output_rois_dev_size": (C.c_size_t, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RoiParams), C.POINTER(RoiBounds)] + [C.c_int] * 5),
    "xgpu_pic_output_device_rois_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RoiParams),
                                                  C.POINTER(RoiBounds), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_warp_from_matrix": (C.c_int, [C.POINTER(C.c_double), C.POINTER(WarpMap)]),
    "xgpu_warp_from_rotated_box": (C.c_int, [C.c_double] * 5 + [C.c_int, C.c_int, C.POINTER(WarpMap)]),
    "xgpu_output_warp_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(WarpParams), C.POINTER(WarpMap), C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_int)]),
    "xgpu_output_warp_size": (C.c_size_t, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(WarpParams), C.c_int, C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_output_device_warp": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(WarpParams), C.c_void_p,
                                              C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_remap_grid_dims": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "xgpu_remap_grid_size": (C.c_size_t, [C.POINTER(ScaleParams), C.POINTER(RemapParams), C.c_int]),
    "xgpu_output_remap_check": (C.c_int, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RemapParams), C.c_int, C.c_int, C.c_int, C.c_int]),
    "xgpu_output_remap_size": (C.c_size_t, [C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RemapParams), C.c_int, C.c_int, C.c_int, C.c_int]),
    "xgpu_remap_from_warp": (C.c_int, [C.POINTER(WarpMap), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "xgpu_remap_from_homography": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "xgpu_remap_from_lens": (C.c_int, [C.POINTER(RemapLens), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "xgpu_pic_output_device_remap": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(OutputFormat), C.POINTER(ScaleParams), C.POINTER(RemapParams), C.c_void_p,
                                               C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_side_info_size": (C.c_size_t, [C.POINTER(SideFormat), C.c_int, C.c_int]),
    "xgpu_frame_side_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SideFormat), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_resid_size": (C.c_size_t, [C.POINTER(ResidFormat), C.c_int, C.c_int]),
    "xgpu_batch_residual": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ResidFormat), C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_compare_ref_size": (C.c_size_t, [C.POINTER(CompareRef), C.c_int, C.c_int]),
    "xgpu_compare_map_size": (C.c_size_t, [C.POINTER(CompareParams), C.c_int, C.c_int]),
    "xgpu_compare_check": (C.c_int, [C.POINTER(CompareRef), C.POINTER(CompareParams), C.c_int, C.c_int, C.c_int]),
    "xgpu_pic_compare": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(CompareRef), C.POINTER(CompareParams), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_stats_hist_size": (C.c_size_t, [C.POINTER(StatsParams), C.c_int]),
    "xgpu_stats_check": (C.c_int, [C.POINTER(StatsParams), C.c_int, C.c_int, C.c_int]),
    "xgpu_stats_lin": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "xgpu_pic_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(StatsParams), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "xgpu_host_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "xgpu_host_free": (None, [C.c_void_p, C.c_void_p]),
    "xgpu_batch_wait_upload": (C.c_int, [C.c_void_p, C.c_void_p]),
    "xgpu_set_builder_threads": (C.c_int, [C.c_void_p, C.c_int]),
    "xgpu_batch_prepare": (C.c_int, [C.c_void_p, C.c_void_p]),
    "xgpu_batch_info": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "xgpu_batch_dmvr_mvs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "xgpu_pic_download_padded": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "xgpu_pic_upload_padded": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "xgpu_frame_begin": (C.c_int, [C.c_void_p, C.POINTER(FrameParams)]),
    "xgpu_batch_create": (C.c_int, [C.c_void_p, C.POINTER(CuBatch), C.POINTER(C.c_void_p)]),
    "xgpu_batch_destroy": (None, [C.c_void_p, C.c_void_p]),
    "xgpu_batch_recon": (C.c_int, [C.c_void_p, C.c_void_p]),
    "xgpu_batch_recon_ahead": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "xgpu_deblock": (C.c_int, [C.c_void_p]),
    "xgpu_alf": (C.c_int, [C.c_void_p, C.POINTER(AlfParams)]),
    "xgpu_pad": (C.c_int, [C.c_void_p]),
    "xgpu_frame_end": (C.c_int, [C.c_void_p]),
    "xgpu_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "xgpu_timing_reset": (C.c_int, [C.c_void_p]),
    "xgpu_timing_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "xgpu_measure_copy_bw": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "xgpu_test_mc_l": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p] + [C.c_int] * 3),
    "xgpu_test_mc_c": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p] + [C.c_int] * 3),
    "xgpu_test_batch_resid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "xgpu_test_build_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "xgpu_test_inter_lists": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int)]),
    "xgpu_test_recon": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int]),
    "xgpu_test_dbk": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 7),
    "xgpu_test_dbk_chroma": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 8),
    "xgpu_test_itdq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "xgpu_test_itdq_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "xgpu_test_itdq_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "xgpu_test_itdq_pairs_mixed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "xgpu_test_scale_taps_device": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int16), C.c_int]),
}

_lib = None


def exported_names():
    return sorted(_EXPORTS)


def _share_torch_hip_runtime():
    """torch's ROCm wheel carries its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7) and its libraries ask for it by that FILE
    name.  Loaded after this library - which asks for libamdhip64.so.7 and gets ROCm's - torch maps a second runtime, and a second runtime in one
    process finds no GPU.  So when torch is installed its runtime is mapped first (without importing torch): this library then binds to it by
    SONAME, and torch finds it already there, in either import order."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return                                   # torch's runtime is mapped already
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    rt = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(rt):
        C.CDLL(rt, mode=C.RTLD_GLOBAL)


def load():
    """Load the product library.  Fails loudly when it has not been built - there is no CPU fallback."""
    global _lib
    if _lib is None:
        _share_torch_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  xevd_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _EXPORTS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib
