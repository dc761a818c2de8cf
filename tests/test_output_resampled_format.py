"""CPU suite for the bicubic resize: xgpu_resample_taps against the fractions.Fraction restatement (tests/resample_ref.py), the
size / check functions against the scaled output's and the batch's on the same shapes, the integer contract against torch's bicubic resize in float64, and what
the Python surface refuses on its arguments alone.  No GPU: the functions tested are the host-only ones."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import resample_ref as rf
import scale_ref as sr
import stub_decoder
from xevd_amd import abi

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -101, -104
KERNELS = (rf.CATMULL_ROM, rf.CUBIC_075, rf.MITCHELL)
PLANES = (2, 3, 5, 33, 34, 64, 127, 540)


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def test_codes_are_the_headers():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xevd_hip.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(XGPU_RESAMPLE_\w+)\s+(\d+)", src)}
    assert vals == {"XGPU_RESAMPLE_CATMULL_ROM": abi.RESAMPLE_CATMULL_ROM, "XGPU_RESAMPLE_CUBIC_075": abi.RESAMPLE_CUBIC_075, "XGPU_RESAMPLE_MITCHELL": abi.RESAMPLE_MITCHELL}
    assert (abi.RESAMPLE_CATMULL_ROM, abi.RESAMPLE_CUBIC_075, abi.RESAMPLE_MITCHELL) == KERNELS
    assert abi.RESAMPLE_KERNELS["bicubic"] == abi.RESAMPLE_KERNELS["catmull-rom"] == rf.CATMULL_ROM
    assert C.sizeof(abi.ResampleParams) == 5 * 4 + 6 * 4


def _destinations(n, s):
    """the destination sizes of the sweep that lie inside the limits for n plane samples of subsampling s"""
    return [N for N in sorted({2, 3, 7, 9, 31, 64, n, 2 * n, 8 * n, -(-n // 64), n // 3}) if 2 <= N <= 16384 and n * s <= 64 * N and N <= 8 * n * s]


@pytest.mark.parametrize("antialias", (0, 1))
@pytest.mark.parametrize("kernel", KERNELS)
def test_taps_equal_the_fraction_restatement(lib, kernel, antialias):
    done, widest_mag = 0, 0
    for (s, half), n in itertools.product(((1, 0), (2, 0), (2, 1), (2, 2)), PLANES):
        for N in _destinations(n, s):
            what = (kernel, antialias, s, half, n, N)
            got = abi.resample_taps(lib, n, s, half, N, kernel, antialias)
            assert not isinstance(got, int), (what, got)      # no row of the sweep has W <= 0 or sum |q| > 32768
            first, count, w = got
            assert sr.table_rows(first, count, w) == rf.taps(n, s, half, N, kernel, antialias), what
            wide = w.astype(np.int64)
            assert (wide.sum(1) == 16384).all() and (np.abs(wide).sum(1) <= 32768).all(), what
            assert (count >= 1).all() and (first >= 0).all() and (first + count <= n).all() and w.shape[1] == count.max(), what
            assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all(), what      # pass 2 takes a workgroup's span from its first and last column
            assert not (w * (np.arange(w.shape[1])[None, :] >= count[:, None])).any(), what
            widest_mag = max(widest_mag, int(np.abs(wide).sum(1).max()))
            done += 1
    assert done >= 200
    assert widest_mag > 16384      # negative lobes are there


def test_window_and_negative_weights_stay_in_the_row(lib):
    """count is the number of samples in the window |i - c| < 2 f: nothing is trimmed, zero and negative weights included"""
    first, count, w = abi.resample_taps(lib, 64, 1, 0, 64, rf.CATMULL_ROM, 1)      # same size: c = o, the window is o - 1 .. o + 1, weights 0, 1, 0
    assert list(count[1:-1]) == [3] * 62 and (count[0], count[-1]) == (2, 2)
    assert [int(v) for v in w[5, :3]] == [0, 16384, 0]
    first, count, w = abi.resample_taps(lib, 64, 1, 0, 128, rf.CUBIC_075, 0)
    assert count.max() == 4 and (w < 0).any()
    first, count, w = abi.resample_taps(lib, 640, 1, 0, 10, rf.MITCHELL, 1)           # f = 64: 4 f samples
    assert count.max() == 256
    assert abi.resample_taps(lib, 640, 1, 0, 10, rf.MITCHELL, 0)[1].max() == 4        # without antialias the window does not widen


def test_invalid_tap_arguments(lib):
    f, c = (C.c_int32 * 64)(), (C.c_int32 * 64)()
    w = (C.c_int16 * 64)()
    taps = lib.xgpu_resample_taps
    assert taps(0, 1, 0, 16, 0, 1, f, c, None, 0) == ERR_INVALID_ARGUMENT
    assert taps(16, 3, 0, 16, 0, 1, f, c, None, 0) == ERR_INVALID_ARGUMENT
    assert taps(16, 1, 3, 16, 0, 1, f, c, None, 0) == ERR_INVALID_ARGUMENT
    assert taps(16, 1, 0, 16, 3, 1, f, c, None, 0) == ERR_INVALID_ARGUMENT and taps(16, 1, 0, 16, -1, 1, f, c, None, 0) == ERR_INVALID_ARGUMENT
    assert taps(16, 1, 0, 16, 0, 2, f, c, None, 0) == ERR_INVALID_ARGUMENT
    assert taps(16, 1, 0, 16, 0, 1, None, c, None, 0) == ERR_INVALID_ARGUMENT
    assert taps(64, 1, 0, 16, 0, 1, f, c, w, 2) == ERR_INVALID_ARGUMENT      # rows of 16 do not fit a stride of 2
    assert taps(16, 1, 0, 1, 0, 1, f, c, None, 0) == ERR_UNSUPPORTED
    assert taps(130, 1, 0, 2, 0, 1, f, c, None, 0) == ERR_UNSUPPORTED          # below 1 / 64
    assert taps(4, 1, 0, 33, 0, 1, f, c, None, 0) == ERR_UNSUPPORTED           # above 8
    assert taps(128, 1, 0, 2, 0, 1, f, c, None, 0) == 128 and taps(4, 1, 0, 32, 0, 1, f, c, None, 0) == 4      # both rows of the first hold the whole axis


# ---------------------------------------------------------------------------------------------------------------- sizes and refusals
W, H, BD = 1920, 1080, 10
RGB = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32)


def _both(lib, fmt, **shape):
    """(size, check) of the bicubic call and of the scaled output for the same format and shape"""
    normalize = shape.pop("normalize", None)
    rs, sc = abi.make_resample_params(**shape), abi.make_scale_params(**shape)
    if normalize is not None:
        rs.normalize = sc.normalize = normalize
    r = lib.xgpu_output_resampled_size(C.byref(fmt), C.byref(rs), W, H, BD), lib.xgpu_output_resampled_check(C.byref(fmt), C.byref(rs), W, H, BD)
    s = lib.xgpu_output_scaled_size(C.byref(fmt), C.byref(sc), W, H, BD), lib.xgpu_output_scaled_check(C.byref(fmt), C.byref(sc), W, H, BD)
    return r, s


def test_sizes_and_refusals_are_the_scaled_outputs(lib):
    layouts = (abi.OUT_RGB_PLANAR, abi.OUT_RGB_INTERLEAVED, abi.OUT_YUV444_PLANAR, abi.OUT_YUV444_INTERLEAVED)
    for layout, dtype in itertools.product(layouts, (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16, abi.OUT_BF16, abi.OUT_F32)):
        es = {abi.OUT_U8: 1, abi.OUT_F32: 4}.get(dtype, 2)
        r, s = _both(lib, abi.make_output_format(layout, dtype), width=224, height=200)
        assert r == s == (3 * 224 * 200 * es, 0)
        row = (224 if layout in (abi.OUT_RGB_PLANAR, abi.OUT_YUV444_PLANAR) else 3 * 224) * es
        for pitch in (row + 64, row - es):
            r, s = _both(lib, abi.make_output_format(layout, dtype, row_pitch=pitch), width=224, height=200)
            assert r == s and (r[1] == 0) == (pitch > row)
    refused = 0
    cases = [(abi.make_output_format(lay, abi.OUT_U16), dict(width=224, height=224)) for lay in (abi.OUT_YUV420P, abi.OUT_NV12, abi.OUT_P016, 7)]
    cases += [(RGB, dict(width=w, height=h)) for w, h in ((29, 224), (224, 16), (15361, 224), (224, 8641), (1, 224), (224, 16385), (30, 17), (15360, 8640))]
    cases += [(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, crop=(0, 1856, 0, 0)), dict(width=513, height=224))]
    cases += [(abi.make_output_format(abi.OUT_RGB_PLANAR, dt), dict(width=224, height=224, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25))) for dt in (abi.OUT_U8, abi.OUT_U16, abi.OUT_F16)]
    cases += [(RGB, dict(width=224, height=224, mean=(0.5, float("nan"), 0.5))), (RGB, dict(width=224, height=224, inv_std=(1.0, 1.0, float("inf"))))]
    cases += [(abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, crop=crop), dict(width=224, height=224)) for crop in ((1, 0, 0, 0), (0, 0, 0, 3), (0, -2, 0, 0), (960, 960, 0, 0))]
    cases += [(RGB, dict(width=224, height=224, normalize=2)), (abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32, matrix=2), dict(width=224, height=224))]
    for fmt, shape in cases:
        r, s = _both(lib, fmt, **shape)
        assert r == s, shape
        refused += r[1] < 0
    assert refused == len(cases) - 3      # (30, 17), (15360, 8640) and the float16 normalise are served
    ok = abi.make_resample_params(224, 224)
    assert lib.xgpu_output_resampled_size(None, C.byref(ok), W, H, BD) == 0 and lib.xgpu_output_resampled_check(None, C.byref(ok), W, H, BD) == ERR_INVALID_ARGUMENT
    assert lib.xgpu_output_resampled_size(C.byref(RGB), None, W, H, BD) == 0 and lib.xgpu_output_resampled_check(C.byref(RGB), None, W, H, BD) == ERR_INVALID_ARGUMENT
    # the call's own: an unknown kernel, an antialias outside 0 / 1
    for kernel, antialias, good in ((0, 0, True), (2, 1, True), (3, 1, False), (-1, 1, False), (0, 2, False), (0, -1, False)):
        rs = abi.make_resample_params(224, 224, kernel, antialias)
        rs.antialias = antialias
        assert lib.xgpu_output_resampled_check(C.byref(RGB), C.byref(rs), W, H, BD) == (0 if good else ERR_INVALID_ARGUMENT), (kernel, antialias)
        assert (lib.xgpu_output_resampled_size(C.byref(RGB), C.byref(rs), W, H, BD) != 0) == good


def test_batch_sizes_and_refusals_are_the_batchs(lib):
    def both(rects, n=None, fmt=RGB, fit=abi.FIT_STRETCH, pad=0.0, image_pitch=0, size=(48, 64), kernel=0, antialias=1):
        n = len(rects) if n is None else n
        ra, rp = abi.make_rois(rects), abi.make_roi_params(fit, pad, image_pitch)
        rs, sc = abi.make_resample_params(size[1], size[0], kernel, antialias), abi.make_scale_params(size[1], size[0])
        rs.antialias = antialias
        b0, b1 = C.c_int(-7), C.c_int(-7)
        r = (lib.xgpu_output_rois_resampled_size(C.byref(fmt), C.byref(rs), C.byref(rp), ra, n, W, H, BD),
             lib.xgpu_output_rois_resampled_check(C.byref(fmt), C.byref(rs), C.byref(rp), ra, n, W, H, BD, C.byref(b0)), b0.value)
        s = (lib.xgpu_output_rois_size(C.byref(fmt), C.byref(sc), C.byref(rp), ra, n, W, H, BD),
             lib.xgpu_output_rois_check(C.byref(fmt), C.byref(sc), C.byref(rp), ra, n, W, H, BD, C.byref(b1)), b1.value)
        return r, s
    good = [(0, 0, W, H), (100, 50, 640, 360), (W - 8, H - 6, 8, 6)]
    r, s = both(good)
    assert r == s == (3 * 3 * 48 * 64 * 4, 0, -1)
    r, s = both(good, image_pitch=3 * 48 * 64 * 4 + 256)
    assert r == s and r[1] == 0
    refused = 0
    for kw in (dict(rects=good, n=0), dict(rects=good * 400), dict(rects=good[:2] + [(1, 0, 64, 64)]), dict(rects=good[:1] + [(W - 62, 0, 64, 64)]),
               dict(rects=good, fit=2), dict(rects=good, fit=abi.FIT_LETTERBOX, pad=float("nan")),
               dict(rects=good, fmt=abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8), fit=abi.FIT_LETTERBOX, pad=0.5),
               dict(rects=good, image_pitch=3 * 48 * 64 * 4 - 4), dict(rects=good, image_pitch=3 * 48 * 64 * 4 + 2),
               dict(rects=good + [(0, 0, 2, 2)], size=(32, 32)), dict(rects=good, size=(2, 2)), dict(rects=good, size=(1, 224)),
               dict(rects=[(0, 0, W, H)] * 70, size=(1080, 224)),      # 70 x 1080 x 3840 x 2 bytes pass 512 MiB
               dict(rects=good, fmt=abi.make_output_format(abi.OUT_NV12, abi.OUT_U8))):
        r, s = both(**kw)
        assert r == s and r[1] < 0 and r[0] == 0, kw
        refused += 1
    assert refused == 14
    for kernel, antialias in ((3, 1), (0, 2)):
        r, _ = both(good, kernel=kernel, antialias=antialias)
        assert r == (0, ERR_INVALID_ARGUMENT, -1)


# ---------------------------------------------------------------------------------------------------------------- accuracy
# The yardstick is torch's own bicubic resize in float64 on the CPU.  Catmull-Rom with antialias is torch's antialias=True form on every shape; CUBIC_075 without
# antialias is its antialias=False form on the enlargement, away from the border: torch replicates the edge sample where this contract ends the row at the edge and
# renormalises, so the destination samples whose window reaches the two outermost source samples - ceil(2 N / n) of them on either side - are left out.
# The bound per bit depth is the largest difference measured over the shapes and patterns below, rounded up to the next quarter of a code value (INTEGRATION.md
# section 8o has the table): 0.62, 0.65 and 1.04 code values at 8, 10 and 12 bit - the last one at the 32 : 1 reduction, where 128 weights of 2^-14 each carry 12-bit
# samples.
SHAPES = (((96, 128), (30, 50)), ((40, 56), (90, 100)), ((256, 64), (8, 60)))      # (Hs, Ws) -> (Hd, Wd)
BOUND = {8: 0.75, 10: 0.75, 12: 1.25}


def _patterns(hs, ws, bd):
    top = (1 << bd) - 1
    yy, xx = np.mgrid[0:hs, 0:ws]
    return {"random": np.random.default_rng(bd * 7 + hs).integers(0, top + 1, (hs, ws), dtype=np.int64), "checker": ((yy + xx) & 1) * top,
            "ramp": (xx * top) // (ws - 1)}


@pytest.fixture(scope="module")
def shape_taps():
    """the Fraction taps of the three shapes, made once: (rows, columns) per (shape, kernel, antialias)"""
    out = {}
    for (hs, ws), (hd, wd) in SHAPES:
        out[(hs, ws), rf.CATMULL_ROM, 1] = rf.taps(hs, 1, 0, hd, rf.CATMULL_ROM, 1), rf.taps(ws, 1, 0, wd, rf.CATMULL_ROM, 1)
        if hd >= hs and wd >= ws:
            out[(hs, ws), rf.CUBIC_075, 0] = rf.taps(hs, 1, 0, hd, rf.CUBIC_075, 0), rf.taps(ws, 1, 0, wd, rf.CUBIC_075, 0)
    return out


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_restatement_against_torch_bicubic(shape_taps, bd):
    import torch
    top, worst, compared = (1 << bd) - 1, 0.0, 0
    for ((hs, ws), (hd, wd)), (name, plane) in ((sh, pt) for sh in SHAPES for pt in _patterns(*sh[0], bd).items()):
        t = torch.from_numpy(plane.astype(np.float64))[None, None]
        for (kernel, antialias), border in (((rf.CATMULL_ROM, 1), (0, 0)), ((rf.CUBIC_075, 0), (math.ceil(2 * hd / hs), math.ceil(2 * wd / ws)))):
            if ((hs, ws), kernel, antialias) not in shape_taps:
                continue
            ty, tx = shape_taps[(hs, ws), kernel, antialias]
            census = {}
            got = rf.resize_plane(plane, ty, tx, bd, census)
            ref = torch.nn.functional.interpolate(t, size=(hd, wd), mode="bicubic", antialias=bool(antialias), align_corners=False)[0, 0].numpy()
            by, bx = border
            err = np.abs(got - np.clip(ref, 0, top))[by:hd - by, bx:wd - bx].max()
            print(f"{bd} bit {ws}x{hs} -> {wd}x{hd} {name} kernel {kernel} antialias {antialias}: max |integer contract - torch float64| = {err:.3f} code values")
            assert err <= BOUND[bd], (bd, (hs, ws), (hd, wd), name, kernel, antialias)
            worst, compared = max(worst, err), compared + 1
    assert compared == 12
    assert worst > BOUND[bd] - 0.25      # the bound is the measured maximum rounded up, not a wider one


def test_rails_stay_on_the_rails_and_same_size_is_the_identity():
    for bd, kernel, antialias in itertools.product((8, 10, 12), KERNELS, (0, 1)):
        ty, tx = rf.taps(54, 1, 0, 20, kernel, antialias), rf.taps(96, 1, 0, 131, kernel, antialias)
        for v in (0, (1 << bd) - 1):
            assert (rf.resize_plane(np.full((54, 96), v, np.int64), ty, tx, bd) == v).all(), (bd, kernel, antialias, v)
    plane = np.random.default_rng(5).integers(0, 4096, (34, 50), dtype=np.int64)
    for kernel in (rf.CATMULL_ROM, rf.CUBIC_075):      # the Keys kernels interpolate: k(0) = 1, k(+-1) = 0
        assert np.array_equal(rf.resize_plane(plane, rf.taps(34, 1, 0, 34, kernel, 1), rf.taps(50, 1, 0, 50, kernel, 1), 12), plane)
    assert not np.array_equal(rf.resize_plane(plane, rf.taps(34, 1, 0, 34, rf.MITCHELL, 1), rf.taps(50, 1, 0, 50, rf.MITCHELL, 1), 12), plane)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def _decoder(lib, w=320, h=200, bd=10):
    """a decoder object without a context: what the arguments alone decide"""
    from xevd_amd.decoder import XgpuDecoder
    dec = stub_decoder.XgpuDecoder(w, h, bd)
    dec.lib, dec.sp, dec.ctx = lib, abi.make_seq_params(w, h, bd), None
    dec._scaled_setup = XgpuDecoder._scaled_setup.__get__(dec)
    dec._rois_fit = XgpuDecoder._rois_fit
    return dec, XgpuDecoder.pic_output_resampled


def test_pic_output_resampled_argument_errors(lib, monkeypatch):
    import torch
    from xevd_amd import decoder
    dec, call = _decoder(lib)
    for bad in (dict(kernel="lanczos"), dict(kernel=2), dict(antialias=2), dict(antialias="yes"), dict(fit="letterbox"), dict(pad=3), dict(layout="nv12"),
                dict(rois=torch.zeros((1, 4), dtype=torch.int32)), dict(rois=[(0, 0, 64, 64)], fit="crop"), dict(rois=[(1, 0, 64, 64)]), dict(rois=[]),
                dict(dtype=torch.uint8, mean=(0.5, 0.5, 0.5)), dict(dtype=torch.float64), dict(crop=(1, 0, 0, 0)), dict(matrix=2),
                dict(rois=[(0, 0, 64, 64)], fit="letterbox", pad=0.5)):
        with pytest.raises(ValueError):
            call(dec, 0, (48, 64), **bad)
    for size in ((1, 64), (48, 4), (48, 2561), (16385, 64)):
        with pytest.raises(ValueError):
            call(dec, 0, size)
    with pytest.raises(TypeError):
        call(dec, 0, (48, 64), filter="bilinear")
    # what reaches the library: the entry, the kernel's code and the antialias flag
    seen = []
    dec._device_call = lambda name, out, *args: seen.append((name, args))
    dec._dra_luts = lambda dra: (None, None)
    monkeypatch.setattr(decoder, "_out_tensor", lambda out, shape, dtype, dev: torch.empty(shape, dtype=dtype))      # no device here: a host tensor of the shape
    for name in abi.RESAMPLE_KERNELS:
        call(dec, 0, (48, 64), kernel=name, antialias=False)
        call(dec, 0, (48, 64), kernel=name, rois=[(0, 0, 64, 64), (2, 2, 32, 48)], fit="letterbox", pad=0, dtype=torch.float32, mean=0.5, std=0.25)
    assert len(seen) == 2 * len(abi.RESAMPLE_KERNELS)
    for (entry, args), (name, batch) in zip(seen, itertools.product(abi.RESAMPLE_KERNELS, (False, True))):
        assert entry == ("xgpu_pic_output_device_rois_resampled" if batch else "xgpu_pic_output_device_resampled")
        rs = args[3]._obj
        assert (rs.width, rs.height, rs.kernel, rs.antialias, rs.normalize) == (64, 48, abi.RESAMPLE_KERNELS[name], int(batch), int(batch))
        if batch:
            assert args[4]._obj.fit == abi.FIT_LETTERBOX and args[6] == 2


def test_pictures_resample_combinations_that_raise():
    import torch
    from xevd_amd.player import StreamDecoder
    t = dict(layout="rgb")
    for bad in (dict(resample="bicubic"), dict(resample="bicubic", tensor=t), dict(resample="bicubic", size=(48, 64)),
                dict(resample="bicubic", tensor=t, size=(48, 64), to="srgb"), dict(resample="bicubic", tensor=t, size=(48, 64), to="srgb", linear_light=True),
                dict(resample="bicubic", tensor=t, size=(48, 64), warp=[0.0]), dict(resample="bicubic", tensor=t, size=(48, 64), remap=np.zeros((48, 64, 2), np.float32)),
                dict(resample="bicubic", tensor=t, size=(48, 64), rois=torch.zeros((1, 4), dtype=torch.int32)),
                dict(resample=dict(kernel="mitchell", filter="area"), tensor=t, size=(48, 64)), dict(resample="bicubic", tensor=t, size=(48, 64), fit="letterbox")):
        with pytest.raises(ValueError):
            next(StreamDecoder(b"").pictures(**bad))
        with pytest.raises(ValueError):
            StreamDecoder(b"").output_order(**bad)
