"""CPU suite for the batched regions of interest (xgpu_roi_inner, xgpu_output_rois_check, xgpu_output_rois_size): the letterbox
rule against its restatement in Python integers (tests/roi_ref.py), sizes and pitches, and every refusal with the rectangle it names - all without a device."""
import ctypes as C

import numpy as np
import pytest

import roi_ref as rr
from xevd_amd import abi

INVALID, UNSUPPORTED = -101, -104


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def check(lib, rois, size=(48, 64), width=320, height=200, bd=10, fmt=None, rp=None, sc=None):
    """(code, bad_index, bytes) of one call's arguments"""
    fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8) if fmt is None else fmt
    sc = abi.make_scale_params(size[1], size[0]) if sc is None else sc
    rp = abi.make_roi_params() if rp is None else rp
    ra = abi.make_rois(rois)
    bad = C.c_int(12345)
    rc = lib.xgpu_output_rois_check(C.byref(fmt), C.byref(sc), C.byref(rp), ra, len(rois), width, height, bd, C.byref(bad))
    n = lib.xgpu_output_rois_size(C.byref(fmt), C.byref(sc), C.byref(rp), ra, len(rois), width, height, bd)
    assert (n == 0) == (rc < 0)
    return rc, bad.value, n


def test_inner_rectangle_follows_the_integer_rule(lib):
    rng = np.random.default_rng(2024)
    cases = [((2, 2), (2, 2)), ((8192, 2), (16384, 16384)), ((2, 8192), (16384, 16384)), ((7680, 4320), (224, 224)), ((160, 50), (48, 64)), ((20, 200), (48, 64))]
    for _ in range(3000):
        cases.append(((int(rng.integers(1, 4097)) * 2, int(rng.integers(1, 4097)) * 2), (int(rng.integers(2, 1025)), int(rng.integers(2, 1025)))))
    for (ws, hs), (hd, wd) in cases:
        for fit in (rr.STRETCH, rr.LETTERBOX):
            got = abi.roi_inner(lib, (0, 0, ws, hs), (hd, wd), fit)
            assert got == rr.inner(ws, hs, wd, hd, fit), (ws, hs, wd, hd, fit)
            x, y, wi, hi = got
            assert 0 <= x and x + wi <= wd and 0 <= y and y + hi <= hd and wi >= 2 and hi >= 2
            assert fit == rr.LETTERBOX or got == (0, 0, wd, hd)
            assert wi == wd or hi == hd                      # one axis is filled
    assert abi.roi_inner(lib, (0, 0, 16, 16), (48, 64), 2) == INVALID
    assert abi.roi_inner(lib, (0, 0, 0, 16), (48, 64), 1) == INVALID
    assert lib.xgpu_roi_inner(None, None, 0, None) == INVALID


def test_sizes_and_pitches(lib):
    rois = [(0, 0, 320, 200), (40, 30, 160, 50), (40, 30, 160, 50)]      # duplicates are accepted
    for layout, dtype, es in ((abi.OUT_RGB_PLANAR, abi.OUT_U8, 1), (abi.OUT_RGB_INTERLEAVED, abi.OUT_F16, 2), (abi.OUT_YUV444_PLANAR, abi.OUT_F32, 4),
                              (abi.OUT_YUV444_INTERLEAVED, abi.OUT_U16, 2)):
        fmt = abi.make_output_format(layout, dtype)
        image = 3 * 48 * 64 * es
        assert check(lib, rois, fmt=fmt) == (0, -1, 3 * image)
        assert check(lib, rois[:1], fmt=fmt) == (0, -1, image)
        # a batch stride of one's own: the last image is not followed by a stride's worth of bytes
        assert check(lib, rois, fmt=fmt, rp=abi.make_roi_params(image_pitch=image + 4 * es)) == (0, -1, 2 * (image + 4 * es) + image)
        # padded rows: the tight batch stride is whole rows, one image ends with its last element
        interleaved = layout in (abi.OUT_RGB_INTERLEAVED, abi.OUT_YUV444_INTERLEAVED)
        row = (3 if interleaved else 1) * 64 * es
        fmt.row_pitch = row + 32
        rows = 48 if interleaved else 3 * 48
        one = (rows - 1) * (row + 32) + row
        assert check(lib, rois, fmt=fmt) == (0, -1, 2 * rows * (row + 32) + one)
        assert check(lib, rois, fmt=fmt, rp=abi.make_roi_params(image_pitch=one)) == (0, -1, 3 * one)
        assert check(lib, rois, fmt=fmt, rp=abi.make_roi_params(image_pitch=one - es))[:2] == (INVALID, -1)
    # the stretch fit equals the scaled output's own size per image
    fmt, sc = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F32), abi.make_scale_params(64, 48)
    assert check(lib, rois[:1], fmt=fmt)[2] == lib.xgpu_output_scaled_size(C.byref(fmt), C.byref(sc), 320, 200, 10)
    assert check(lib, [(0, 0, 320, 200)] * abi.MAX_ROIS)[0] == 0


def test_every_refusal_names_its_rectangle(lib):
    good = [(0, 0, 320, 200), (312, 194, 8, 6), (2, 2, 64, 64)]
    assert check(lib, good)[:2] == (0, -1)
    # the count
    assert check(lib, [])[:2] == (INVALID, -1)
    assert check(lib, [(0, 0, 16, 16)] * (abi.MAX_ROIS + 1))[:2] == (INVALID, -1)
    # odd, or outside the picture (minus the crop)
    for bad in ((1, 0, 16, 16), (0, 3, 16, 16), (0, 0, 15, 16), (0, 0, 16, 17), (-2, 0, 16, 16), (0, -2, 16, 16), (306, 0, 16, 16), (0, 186, 16, 16), (0, 0, 322, 16),
                (0, 0, 0, 16), (0, 0, 16, -4)):
        for at in range(3):
            rois = list(good)
            rois.insert(at, bad)
            assert check(lib, rois)[:2] == (INVALID, at), (bad, at)
    crop = abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, crop=(4, 2, 6, 0))
    assert check(lib, [(0, 0, 314, 194)], fmt=crop)[:2] == (0, -1)
    assert check(lib, [(0, 0, 8, 8), (2, 0, 314, 8)], fmt=crop)[:2] == (INVALID, 1)
    assert check(lib, [(0, 2, 8, 194)], fmt=crop)[:2] == (INVALID, 0)
    # the first offender is the one named
    assert check(lib, [good[0], (0, 0, 16, 16), (1, 1, 3, 3), (500, 0, 2, 2)])[:2] == (INVALID, 2)
    # fit, pad, batch stride
    assert check(lib, good, rp=abi.make_roi_params(fit=2))[:2] == (INVALID, -1)
    assert check(lib, good, rp=abi.make_roi_params(fit=-1))[:2] == (INVALID, -1)
    for dtype, pads_ok, pads_bad in ((abi.OUT_U8, (0, 114, 255), (256, -1, 0.5, float("nan"))), (abi.OUT_U16, (0, 1023), (1024, 7.25, float("inf"))),
                                     (abi.OUT_F32, (0.447, -3.0, 1e6), (float("nan"), float("-inf"))), (abi.OUT_BF16, (0.5,), (float("inf"),))):
        fmt = abi.make_output_format(abi.OUT_RGB_PLANAR, dtype)
        for p in pads_ok:
            assert check(lib, good, fmt=fmt, rp=abi.make_roi_params(abi.FIT_LETTERBOX, p))[:2] == (0, -1), (dtype, p)
            assert check(lib, good, fmt=fmt, rp=abi.make_roi_params(abi.FIT_LETTERBOX, (0, p, 0)))[:2] == (0, -1), (dtype, p)
        for p in pads_bad:
            assert check(lib, good, fmt=fmt, rp=abi.make_roi_params(abi.FIT_LETTERBOX, (0, 0, p)))[:2] == (INVALID, -1), (dtype, p)
            assert check(lib, good, fmt=fmt, rp=abi.make_roi_params(abi.FIT_STRETCH, p))[:2] == (0, -1), (dtype, p)      # not read
    assert check(lib, good, fmt=abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), rp=abi.make_roi_params(image_pitch=3 * 48 * 64 * 2 + 1))[:2] == (INVALID, -1)
    assert check(lib, good, rp=abi.make_roi_params(image_pitch=3 * 48 * 64 - 1))[:2] == (INVALID, -1)
    # what the scaled output refuses with the same code
    for fmt in (abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8), abi.make_output_format(abi.OUT_YUV420P, abi.OUT_U16),
                abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, crop=(1, 0, 0, 0)), abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, row_pitch=63)):
        assert check(lib, good, fmt=fmt)[:2] == (INVALID, -1)
    assert check(lib, good, sc=abi.make_scale_params(64, 48, mean=(0.5, 0.5, 0.5)))[:2] == (INVALID, -1)            # normalise into integers
    assert check(lib, good, sc=abi.make_scale_params(64, 48, filter=7))[:2] == (INVALID, -1)
    assert check(lib, good, fmt=abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U8, matrix=2))[:2] == (UNSUPPORTED, -1)
    assert check(lib, good, size=(1, 64))[:2] == (UNSUPPORTED, -1)
    assert check(lib, good, size=(48, 16385))[:2] == (UNSUPPORTED, -1)
    assert check(lib, good, bd=13)[:2] == (INVALID, -1)
    assert lib.xgpu_output_rois_check(None, None, None, None, 1, 320, 200, 10, None) == INVALID
    # the limits of the scaled output, per rectangle and axis, on the inner size
    assert check(lib, [good[2], (0, 0, 320, 192)], size=(3, 5))[:2] == (0, -1)                  # 64 times on both axes
    assert check(lib, [good[2], (0, 0, 320, 194)], size=(3, 5))[:2] == (UNSUPPORTED, 1)         # 194 rows to 3
    assert check(lib, [(0, 0, 6, 8)], size=(48, 64))[:2] == (UNSUPPORTED, 0)                   # 6 columns to 64
    assert check(lib, [(0, 0, 8, 6)], size=(48, 64))[:2] == (0, -1)
    # the same rectangle letterboxed: 6 x 8 becomes 36 x 48 inside 64 x 48 and is fine; a long thin one keeps 2 rows, 200 / 2 > 64
    box = abi.make_roi_params(abi.FIT_LETTERBOX, 0)
    assert check(lib, [(0, 0, 6, 8)], size=(48, 64), rp=box)[:2] == (0, -1)
    assert rr.inner(2, 200, 64, 48) == (31, 0, 2, 48)
    assert check(lib, [good[0], (0, 0, 2, 200)], size=(48, 64), rp=box)[:2] == (0, -1)
    assert rr.inner(320, 2, 4, 4)[3] == 2
    assert check(lib, [good[2], good[2], (0, 0, 320, 2)], size=(4, 4), rp=box)[:2] == (UNSUPPORTED, 2)      # 320 columns to 4


def test_intermediate_limit_without_a_device(lib):
    """the intermediate of a call: the sum over the rectangles of Hi * (align8(Ws) + 2 * align8(Ws / 2)) * 2 bytes, refused above 512 MiB at the rectangle
    where the sum passes it"""
    w, h = 7680, 4320
    full = (0, 0, w, h)
    per = 1080 * (7680 + 2 * 3840) * 2                         # one whole 8K picture to 1080 rows
    n_fit = (512 << 20) // per
    assert n_fit == 16
    assert check(lib, [full] * n_fit, size=(1080, 1920), width=w, height=h)[:2] == (0, -1)
    assert check(lib, [full] * (n_fit + 1) + [(0, 0, 16, 16)], size=(1080, 1920), width=w, height=h)[:2] == (UNSUPPORTED, n_fit)
    # widths round up to 8 samples per plane: 68 -> 72 + 2 * 40
    small = 224 * (72 + 2 * 40) * 2
    n_small = (512 << 20) // small
    assert n_small > abi.MAX_ROIS                             # small boxes never reach the limit
    # 64 tiles of an 8K picture to 224 x 224, the detector's grid: 64 * 224 * 1920 * 2 bytes
    assert check(lib, abi.tile_rois(w, h, 960, 540), size=(224, 224), width=w, height=h)[:2] == (0, -1)
    # letterbox shrinks the intermediate with the inner height
    rois = [full] * 40
    assert check(lib, rois, size=(1080, 1080), width=w, height=h)[:2] == (UNSUPPORTED, 16)
    assert rr.inner(w, h, 1080, 1080)[3] == 608
    assert check(lib, rois[:28], size=(1080, 1080), width=w, height=h, rp=abi.make_roi_params(abi.FIT_LETTERBOX, 0))[:2] == (0, -1)
    assert check(lib, rois[:30], size=(1080, 1080), width=w, height=h, rp=abi.make_roi_params(abi.FIT_LETTERBOX, 0))[:2] == (UNSUPPORTED, 28)


def test_tile_grid():
    t = abi.tile_rois(7680, 4320, 960, 540)
    assert len(t) == 64 and t[0] == (0, 0, 960, 540) and t[9] == (960, 540, 960, 540) and t[-1] == (6720, 3780, 960, 540)
    t = abi.tile_rois(320, 200, 128, 96)                      # no multiple: the last column and row move back inside
    assert t == [(0, 0, 128, 96), (128, 0, 128, 96), (192, 0, 128, 96), (0, 96, 128, 96), (128, 96, 128, 96), (192, 96, 128, 96),
                 (0, 104, 128, 96), (128, 104, 128, 96), (192, 104, 128, 96)]
    assert abi.tile_rois(320, 200, 640, 640) == [(0, 0, 320, 200)]
    with pytest.raises(ValueError):
        abi.tile_rois(320, 200, 63, 64)
