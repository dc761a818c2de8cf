"""CPU suite for the regions of interest from device memory (xgpu_roi_snap, xgpu_output_rois_dev_check, xgpu_output_rois_dev_size):
the snapping rule of both box formats against its restatement (tests/roi_dev_ref.py), sizes, every refusal with its code, the worst-case intermediate at its
boundary - all without a device - and the tap rows of the function the host and the device share against the Fraction restatement (tests/scale_ref.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import roi_dev_ref as rd
import scale_ref as sr
from xevd_amd import abi

INVALID, UNSUPPORTED = -101, -104
W, H = 320, 200


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def test_status_codes_are_the_headers():
    assert (abi.ROI_OK, abi.ROI_UNUSED, abi.ROI_INVALID, abi.ROI_EMPTY, abi.ROI_TOO_LARGE, abi.ROI_RATIO) == (rd.OK, rd.UNUSED, rd.INVALID, rd.EMPTY, rd.TOO_LARGE, rd.RATIO)
    assert (abi.BOX_XYWH_I32, abi.BOX_XYXY_F32) == (rd.XYWH_I32, rd.XYXY_F32)
    assert C.sizeof(abi.RoiResult) == 36 and C.sizeof(abi.RoiBounds) == 8


def test_snap_i32_follows_the_rule(lib):
    boxes = [(1, 1, 15, 15), (3, 5, 1, 1), (0, 0, W, H), (0, 0, 2, 2),                                   # odd boxes, whole picture
             (-5, 33, 21, 10), (-7, -9, 30, 40), (-40, 10, 20, 20), (-40, 10, 41, 20), (-40, 10, 42, 20),      # negative: cut, gone, one column left, two
             (300, 190, 40, 40), (318, 198, 9, 9), (319, 199, 1, 1), (320, 0, 10, 10), (400, 300, 10, 10),     # past the edge
             (10, 10, 0, 8), (11, 10, 0, 8), (10, 10, -4, 8), (10, 11, 8, 0), (10, 10, 1, 1), (11, 11, 1, 1),   # widths of 0 and what snaps to 2
             (2 ** 31 - 1, 0, 2 ** 31 - 1, 8), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (0, 0, 2 ** 31 - 1, 2 ** 31 - 1)]
    rng = np.random.default_rng(5)
    boxes += [tuple(int(v) for v in rng.integers(-60, 380, 4)) for _ in range(2000)]
    seen = set()
    for b in boxes:
        got = abi.roi_snap(lib, b, (H, W), abi.BOX_XYWH_I32)
        assert got == rd.snap(b, (H, W), rd.XYWH_I32), b
        seen.add(got[0])
        if got[0] == rd.OK:
            x, y, w, h = got[1]
            assert not (x | y | w | h) & 1 and x >= 0 and y >= 0 and w >= 2 and h >= 2 and x + w <= W and y + h <= H
    assert seen == {rd.OK, rd.EMPTY}
    # what pic_output_tensor(snap=True) makes of the boxes of the host-box suite
    assert [abi.roi_snap(lib, b, (H, W))[1] for b in ((1, 1, 15, 15), (300, 190, 40, 40), (-5, 33, 21, 10))] == [(0, 0, 16, 16), (300, 190, 20, 10), (0, 32, 16, 12)]


def test_snap_f32_follows_the_rule(lib):
    inf, nan = float("inf"), float("nan")
    boxes = [(10.0, 20.0, 50.0, 60.0), (10.5, 20.5, 50.5, 60.5), (10.999, 20.999, 50.999, 60.999), (11.0, 21.0, 51.0, 61.0), (11.5, 21.999, 51.0, 61.5),
             (0.0, 0.0, 320.0, 200.0), (-0.001, -0.5, 320.001, 200.5), (-3.5, -1e-30, 10.0, 10.0), (-30.0, 5.0, -10.0, 50.0), (-30.0, 5.0, 0.0, 50.0),
             (-30.0, 5.0, 0.001, 50.0), (319.0, 199.0, 500.0, 500.0), (320.0, 10.0, 330.0, 20.0), (319.999, 10.0, 330.0, 20.0),
             (inf, 0.0, 10.0, 10.0), (0.0, -inf, 10.0, 10.0), (0.0, 0.0, inf, 10.0), (0.0, 0.0, 10.0, nan), (nan, nan, nan, nan),
             (1e30, 0.0, 2e30, 10.0), (-1e30, -1e30, 1e30, 1e30), (0.0, 0.0, 1e30, 3e38), (-3e38, 4.0, 9.0, 8.0),
             (10.0, 10.0, 10.0, 30.0), (10.0, 10.0, 9.0, 30.0), (10.5, 10.0, 10.6, 30.0), (12.0, 10.0, 12.0, 30.0), (12.0, 10.0, 12.001, 30.0),
             (50.0, 60.0, 10.0, 20.0), (1048575.0, 0.0, 1048577.0, 10.0), (0.0, 16777217.0, 5.0, 16777300.0)]
    rng = np.random.default_rng(6)
    for _ in range(2000):
        c = rng.uniform(-40, 360, 2)
        d = rng.uniform(-4, 120, 2)
        boxes.append(tuple(float(np.float32(v)) for v in (c[0], c[1], c[0] + d[0], c[1] + d[1])))
    seen = set()
    for b in boxes:
        got = abi.roi_snap(lib, b, (H, W), abi.BOX_XYXY_F32)
        assert got == rd.snap(b, (H, W), rd.XYXY_F32), b
        seen.add(got[0])
    assert seen == {rd.OK, rd.EMPTY, rd.INVALID}
    assert abi.roi_snap(lib, (10.5, 20.5, 50.5, 60.5), (H, W)) == (rd.OK, (10, 20, 42, 42))
    assert abi.roi_snap(lib, (10.999, 20.0, 12.0, 22.0), (H, W)) == (rd.OK, (10, 20, 2, 2))
    assert abi.roi_snap(lib, (12.0, 20.0, 12.0, 22.0), (H, W)) == (rd.EMPTY, (0, 0, 0, 0))
    assert abi.roi_snap(lib, (1e30, 0.0, 2e30, 10.0), (H, W)) == (rd.EMPTY, (0, 0, 0, 0))
    assert abi.roi_snap(lib, (-1e30, -1e30, 1e30, 1e30), (H, W)) == (rd.OK, (0, 0, W, H))
    # bad arguments of the function itself
    box = (C.c_int * 4)(0, 0, 8, 8)
    used = abi.Roi()
    assert lib.xgpu_roi_snap(2, box, W, H, C.byref(used)) == INVALID
    assert lib.xgpu_roi_snap(0, None, W, H, C.byref(used)) == INVALID and lib.xgpu_roi_snap(0, box, W, H, None) == INVALID
    assert lib.xgpu_roi_snap(0, box, W + 1, H, C.byref(used)) == INVALID and lib.xgpu_roi_snap(0, box, W, 0, C.byref(used)) == INVALID


def check(lib, capacity=6, size=(48, 64), width=W, height=H, bd=10, fmt=None, rp=None, sc=None, max_roi=None, box_format=abi.BOX_XYWH_I32, bounds=True):
    """(code, bytes) of one call's arguments"""
    fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8) if fmt is None else fmt
    sc = abi.make_scale_params(size[1], size[0]) if sc is None else sc
    rp = abi.make_roi_params() if rp is None else rp
    b = C.byref(abi.make_roi_bounds(max_roi)) if bounds else None
    rc = lib.xgpu_output_rois_dev_check(C.byref(fmt), C.byref(sc), C.byref(rp), b, box_format, capacity, width, height, bd)
    n = lib.xgpu_output_rois_dev_size(C.byref(fmt), C.byref(sc), C.byref(rp), b, box_format, capacity, width, height, bd)
    assert (n == 0) == (rc < 0)
    return rc, n


def test_sizes_and_pitches(lib):
    for layout, dtype, es in ((abi.OUT_RGB_PLANAR, abi.OUT_U8, 1), (abi.OUT_RGB_INTERLEAVED, abi.OUT_F16, 2), (abi.OUT_YUV444_PLANAR, abi.OUT_F32, 4),
                              (abi.OUT_YUV444_INTERLEAVED, abi.OUT_U16, 2)):
        fmt = abi.make_output_format(layout, dtype)
        image = 3 * 48 * 64 * es
        assert check(lib, 3, fmt=fmt) == (0, 3 * image)                      # tight: (capacity - 1) * image_pitch + one image
        assert check(lib, 1, fmt=fmt) == (0, image)
        assert check(lib, 3, fmt=fmt, rp=abi.make_roi_params(image_pitch=image + 4 * es)) == (0, 2 * (image + 4 * es) + image)      # padded
        assert check(lib, 3, fmt=fmt, rp=abi.make_roi_params(image_pitch=image - es))[0] == INVALID
        # it is the host-box call's size for as many rectangles
        rois = abi.make_rois([(0, 0, 64, 64)] * 3)
        for rp in (abi.make_roi_params(), abi.make_roi_params(image_pitch=image + 4 * es)):
            sc = abi.make_scale_params(64, 48)
            assert check(lib, 3, fmt=fmt, rp=rp)[1] == lib.xgpu_output_rois_size(C.byref(fmt), C.byref(sc), C.byref(rp), rois, 3, W, H, 10)
    assert check(lib, abi.MAX_ROIS)[0] == 0
    for fmt_code in (abi.BOX_XYWH_I32, abi.BOX_XYXY_F32):
        assert check(lib, box_format=fmt_code, rp=abi.make_roi_params(abi.FIT_LETTERBOX, 114))[0] == 0


def test_every_refusal_has_its_code(lib):
    assert check(lib)[0] == 0
    # what this call adds: the box format, the bounds, the capacity
    assert check(lib, box_format=2)[0] == INVALID and check(lib, box_format=-1)[0] == INVALID
    assert check(lib, max_roi=(-2, 64))[0] == INVALID and check(lib, max_roi=(64, -2))[0] == INVALID
    assert check(lib, max_roi=(H + 2, 64))[0] == INVALID and check(lib, max_roi=(64, W + 2))[0] == INVALID
    assert check(lib, max_roi=(H, W))[0] == 0 and check(lib, max_roi=(0, 0))[0] == 0 and check(lib, max_roi=(2, 2))[0] == 0
    crop = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, crop=(4, 2, 6, 0))      # the bounds are of the picture minus the crop
    assert check(lib, fmt=crop, max_roi=(194, 314))[0] == 0
    assert check(lib, fmt=crop, max_roi=(194, 316))[0] == INVALID and check(lib, fmt=crop, max_roi=(196, 314))[0] == INVALID
    assert check(lib, 0)[0] == INVALID and check(lib, -3)[0] == INVALID and check(lib, abi.MAX_ROIS + 1)[0] == INVALID
    assert check(lib, bounds=False)[0] == INVALID
    fmt, sc = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8), abi.make_scale_params(64, 48)
    assert lib.xgpu_output_rois_dev_check(C.byref(fmt), C.byref(sc), None, C.byref(abi.make_roi_bounds()), 0, 4, W, H, 10) == INVALID
    assert lib.xgpu_output_rois_dev_check(None, None, None, None, 0, 1, W, H, 10) == INVALID
    # fit, batch stride
    assert check(lib, rp=abi.make_roi_params(fit=2))[0] == INVALID and check(lib, rp=abi.make_roi_params(fit=-1))[0] == INVALID
    assert check(lib, fmt=abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), rp=abi.make_roi_params(image_pitch=3 * 48 * 64 * 2 + 1))[0] == INVALID
    assert check(lib, rp=abi.make_roi_params(image_pitch=3 * 48 * 64 - 1))[0] == INVALID
    # the pad value fills every refused box, so it is validated for BOTH fits
    for dtype, pads_ok, pads_bad in ((abi.OUT_U8, (0, 114, 255), (256, -1, 0.5, float("nan"))), (abi.OUT_U16, (0, 1023), (1024, 7.25, float("inf"))),
                                     (abi.OUT_F32, (0.447, -3.0, 1e6), (float("nan"), float("-inf"))), (abi.OUT_BF16, (0.5,), (float("inf"),))):
        fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, dtype)
        for fit, p in itertools.product((abi.FIT_STRETCH, abi.FIT_LETTERBOX), pads_ok):
            assert check(lib, fmt=fmt, rp=abi.make_roi_params(fit, (0, p, 0)))[0] == 0, (dtype, fit, p)
        for fit, p in itertools.product((abi.FIT_STRETCH, abi.FIT_LETTERBOX), pads_bad):
            assert check(lib, fmt=fmt, rp=abi.make_roi_params(fit, (0, 0, p)))[0] == INVALID, (dtype, fit, p)
    # what the host-box call refuses without looking at a rectangle
    for fmt in (abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8), abi.make_output_format(abi.OUT_YUV420P, abi.OUT_U16),
                abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, crop=(1, 0, 0, 0)), abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, row_pitch=63)):
        assert check(lib, fmt=fmt)[0] == INVALID
    assert check(lib, sc=abi.make_scale_params(64, 48, mean=(0.5, 0.5, 0.5)))[0] == INVALID            # normalise into integers
    assert check(lib, sc=abi.make_scale_params(64, 48, filter=7))[0] == INVALID
    assert check(lib, fmt=abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, matrix=2))[0] == UNSUPPORTED
    assert check(lib, size=(1, 64))[0] == UNSUPPORTED and check(lib, size=(48, 16385))[0] == UNSUPPORTED
    assert check(lib, bd=13)[0] == INVALID and check(lib, width=W + 1)[0] == INVALID


def test_worst_case_intermediate_at_its_boundary(lib):
    """capacity x sc->height * (align8(Mw) + 2 * align8(Mw / 2)) * 2 bytes against 512 MiB: allowed at the limit itself, refused one box above"""
    w, h = 7680, 4320
    slot = 1024 * (1024 + 2 * 512) * 2                          # boxes up to 1024 columns to 1024 rows: 4 MiB each
    assert (512 << 20) % slot == 0 and (512 << 20) // slot == 128
    for capacity, rc in ((127, 0), (128, 0), (129, UNSUPPORTED)):
        assert check(lib, capacity, size=(1024, 1024), width=w, height=h, max_roi=(h, 1024))[0] == rc, capacity
    # the width rounds up to 8 samples per plane: 1026 -> 1032 + 2 * 520, so 128 boxes no longer fit; the height of the bounds does not count
    assert check(lib, 128, size=(1024, 1024), width=w, height=h, max_roi=(2, 1026))[0] == UNSUPPORTED
    assert check(lib, (512 << 20) // (1024 * (1032 + 2 * 520) * 2), size=(1024, 1024), width=w, height=h, max_roi=(2, 1026))[0] == 0
    # bounds of 0 are the picture: 224 rows of 7680 + 2 * 3840 samples are 6.6 MiB a box
    per = 224 * (7680 + 2 * 3840) * 2
    n = (512 << 20) // per
    assert check(lib, n, size=(224, 224), width=w, height=h)[0] == 0 and check(lib, n + 1, size=(224, 224), width=w, height=h)[0] == UNSUPPORTED
    # the detector's second stage: 1024 boxes of up to 512 x 512 to 224 x 224 are 224 MiB
    assert check(lib, abi.MAX_ROIS, size=(224, 224), width=w, height=h, max_roi=(512, 512))[0] == 0


PAIRS = ((128, 24), (24, 128), (64, 64), (130, 3), (2, 16), (96, 2))      # down, up, identity, a ratio near 64, the 8x enlargement limit, the narrowest output


@pytest.mark.parametrize("n,N", PAIRS + ((320, 48), (200, 64), (100, 37), (54, 20), (96, 131), (1088, 16)))
def test_shared_tap_rows_on_the_host(lib, n, N):
    """xgpu_scale_taps is now a loop over the row function the device runs too: first, count and every weight against the Fraction restatement, zeros behind
    count, and the same rows at a wider stride"""
    for filt, (s, half) in itertools.product((sr.BILINEAR, sr.AREA), ((1, 0), (2, 0), (2, 1), (2, 2))):
        if n * s > 64 * N or N > 8 * n * s:
            assert abi.scale_taps(lib, n, s, half, N, filt) == UNSUPPORTED
            continue
        first, count, w = abi.scale_taps(lib, n, s, half, N, filt)
        assert sr.table_rows(first, count, w) == sr.taps(n, s, half, N, filt), (n, s, half, N, filt)
        assert w.shape[1] == count.max() and all((w[o, count[o]:] == 0).all() for o in range(N))
        wide = np.full((N, w.shape[1] + 3), -1, np.int16)
        f2, c2 = np.zeros(N, np.int32), np.zeros(N, np.int32)
        assert lib.xgpu_scale_taps(n, s, half, N, filt, f2.ctypes.data_as(C.POINTER(C.c_int32)), c2.ctypes.data_as(C.POINTER(C.c_int32)),
                                   wide.ctypes.data_as(C.POINTER(C.c_int16)), wide.shape[1]) == w.shape[1]
        assert np.array_equal(f2, first) and np.array_equal(c2, count) and np.array_equal(wide[:, :w.shape[1]], w) and (wide[:, w.shape[1]:] == 0).all()
