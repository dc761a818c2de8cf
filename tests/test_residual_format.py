"""CPU suite of the residual export (xgpu_batch_residual): the host-only size function, the numpy restatement of the contract (tests/residual_ref.py) tied to the
decoder itself - prediction + restated residual, clipped, is the oracle's reconstruction -, and a census of what the cases of the GPU suite hold."""
import ctypes as C

import numpy as np
import pytest

import cases
import residual_ref as rr
from xevd_amd import abi


def size(w, h, **kw):
    return abi.load().xgpu_resid_size(C.byref(abi.make_resid_format(**kw)), w, h)


# ------------------------------------------------------------------------------------------------ xgpu_resid_size
def test_size_yuv420():
    w, h = 200, 136
    assert size(w, h) == w * h * 3
    assert size(w, h, row_pitch=w * 2) == w * h * 3
    assert size(w, h, row_pitch=512) == h * 512 + (h - 1) * 256 + w
    crop = (2, 6, 4, 10)
    cw, ch = w - 8, h - 14
    assert size(w, h, crop=crop) == cw * ch * 3
    assert size(w, h, crop=crop, row_pitch=(cw + 6) * 2) == ch * (cw + 6) * 2 + (ch - 1) * (cw + 6) + cw
    assert size(7680, 4320) == 7680 * 4320 * 3


@pytest.mark.parametrize("dtype,es", [(abi.OUT_U16, 2), (abi.OUT_F16, 2), (abi.OUT_F32, 4)])
def test_size_444(dtype, es):
    w, h = 200, 136
    for layout in (abi.RESID_444_PLANAR, abi.RESID_444_INTERLEAVED):
        assert size(w, h, layout=layout, dtype=dtype) == 3 * w * h * es
    crop = (2, 6, 4, 10)
    cw, ch = w - 8, h - 14
    assert size(w, h, layout=abi.RESID_444_PLANAR, dtype=dtype, crop=crop) == 3 * cw * ch * es
    assert size(w, h, layout=abi.RESID_444_PLANAR, dtype=dtype, crop=crop, row_pitch=1024) == (3 * ch - 1) * 1024 + cw * es
    assert size(w, h, layout=abi.RESID_444_INTERLEAVED, dtype=dtype, crop=crop, row_pitch=4096) == (ch - 1) * 4096 + 3 * cw * es
    assert size(w, h, layout=abi.RESID_444_PLANAR, dtype=dtype, row_pitch=(w + 6) * es) == (3 * h - 1) * (w + 6) * es + w * es


def test_size_energy():
    w, h = 200, 136
    ws, hs = w // 4, h // 4
    assert size(w, h, layout=abi.RESID_ENERGY, dtype=abi.OUT_F32) == 3 * hs * ws * 4
    assert size(w, h, layout=abi.RESID_ENERGY, dtype=abi.OUT_F32, row_pitch=256) == (3 * hs - 1) * 256 + ws * 4
    assert size(7680, 4320, layout=abi.RESID_ENERGY, dtype=abi.OUT_F32) == 3 * 1080 * 1920 * 4


def test_size_refusals():
    w, h = 200, 136
    lib = abi.load()
    assert lib.xgpu_resid_size(None, w, h) == 0
    p444 = dict(layout=abi.RESID_444_PLANAR, dtype=abi.OUT_F16)
    i444 = dict(layout=abi.RESID_444_INTERLEAVED, dtype=abi.OUT_F32)
    en = dict(layout=abi.RESID_ENERGY, dtype=abi.OUT_F32)
    for good in ({}, p444, i444, en):
        assert size(w, h, **good) > 0
    for f in ({}, p444, i444):
        for crop in ((1, 0, 0, 0), (0, 3, 0, 0), (0, 0, 5, 0), (0, 0, 0, 7), (-2, 0, 0, 0)):      # odd / negative crops
            assert size(w, h, crop=crop, **f) == 0
        assert size(w, h, crop=(100, 100, 0, 0), **f) == 0                   # a crop that leaves nothing
        assert size(w, h, crop=(0, 0, 100, 36), **f) == 0
        assert size(w, h, crop=(0, 0, 0, 140), **f) == 0
    assert size(w, h, crop=(2, 0, 0, 0), **en) == 0                          # ENERGY with a crop
    assert size(w, h, crop=(0, 0, 0, 4), **en) == 0
    for dt in (abi.OUT_U16, abi.OUT_F16, abi.OUT_BF16, abi.OUT_U8):
        assert size(w, h, layout=abi.RESID_ENERGY, dtype=dt) == 0            # ENERGY is float32
    for dt in (abi.OUT_F16, abi.OUT_F32, abi.OUT_BF16, abi.OUT_U8, 7, -1):
        assert size(w, h, dtype=dt) == 0                                     # YUV420 is int16
    for dt in (abi.OUT_U8, abi.OUT_BF16, 7, -1):
        assert size(w, h, layout=abi.RESID_444_PLANAR, dtype=dt) == 0
    assert size(w, h, layout=4) == 0 and size(w, h, layout=-1) == 0
    assert size(w, h, row_pitch=w * 2 - 4) == 0                              # short pitches
    assert size(w, h, row_pitch=w * 2 - 2, **p444) == 0
    assert size(w, h, row_pitch=3 * w * 4 - 4, **i444) == 0
    assert size(w, h, row_pitch=(w // 4) * 4 - 4, **en) == 0
    assert size(w, h, row_pitch=w * 2 + 2) == 0                              # misaligned: YUV420 halves its pitch for chroma (a multiple of 4)
    assert size(w, h, row_pitch=w * 2 + 3) == 0
    assert size(w, h, row_pitch=w * 2 + 1, **p444) == 0
    assert size(w, h, row_pitch=3 * w * 4 + 2, **i444) == 0
    assert size(w, h, row_pitch=w + 2, **en) == 0
    for bad in ((0, 136), (200, 0), (-8, 136), (204, 136), (200, 132), (201, 136)):      # sizes that are not positive multiples of 8
        for f in ({}, p444, i444, en):
            assert size(*bad, **f) == 0


# ------------------------------------------------------------------------------------------------ the restatement against the decoder
def spec_of(name):
    return next(s for s in cases.CASES if s[0] == name)


def test_prediction_plus_restated_residual_is_the_reconstruction():
    """inter CUs only, no filter: the oracle's picture before the filters is clip(P + R), P the same batch reconstructed with every cbf cleared and R the
    restatement applied to the oracle's arena - the addressing (TU rectangles, component order, strides) is the decoder's own"""
    case = cases.build_case(*spec_of("main_atsinter_noaddb"))
    b = case["batch"]
    assert (b["pred_mode"] != 0).all() and (b["pred_mode"] != 6).all()
    _, pre, _, arena = cases.run_cpu("oracle", case, deblock=False, pad=False)
    pred_case = dict(case)
    pred_case["batch"] = dict(b, cbf=np.zeros_like(b["cbf"]))
    _, pred, _, _ = cases.run_cpu("oracle", pred_case, deblock=False, pad=False)
    r = rr.planes(b, arena, case["w"], case["h"])
    assert all((p != 0).any() for p in r)
    ats = [rr.ats_inter_of(b, i) for i in range(len(b["x"])) if b["cbf"][i] & 7]
    assert {a & 15 for a in ats} >= {0, 1, 2} and {a >> 4 for a in ats if a} == {0, 1}
    hi = (1 << case["bd"]) - 1
    for c in range(3):
        want = np.clip(pred.active(c).astype(np.int32) + r[c].astype(np.int32), 0, hi)
        assert np.array_equal(pre.active(c).astype(np.int32), want), f"component {c}"
        assert not np.array_equal(pre.active(c), pred.active(c))


def test_forms_on_a_hand_made_picture():
    """the output forms of the restatement on planes small enough to write down"""
    y = np.arange(-32, 32, dtype=np.int16).reshape(8, 8) * 100
    cb = np.array([[1, -2, 3, -4], [5, -6, 7, -8], [9, -10, 11, -12], [13, -14, 15, -16]], np.int16)
    cr = (-cb * 3).astype(np.int16)
    pl = [y, cb, cr]
    assert np.array_equal(rr.yuv420(pl), np.concatenate([y.ravel(), cb.ravel(), cr.ravel()]))
    c = rr.yuv420(pl, (2, 0, 0, 4))
    assert np.array_equal(c, np.concatenate([y[:4, 2:].ravel(), cb[:2, 1:].ravel(), cr[:2, 1:].ravel()]))
    f = rr.f444(pl, 10, 8, (2, 2, 2, 0), np.float32)
    assert f.shape == (3, 6, 4) and f[0, 0, 0] == np.float32(y[2, 2]) / 1024 and f[1, 0, 0] == np.float32(cb[1, 1]) / 256 and f[2, 5, 3] == np.float32(cr[3, 2]) / 256
    assert f[1, 0, 0] == f[1, 1, 0] == f[1, 0, 1] and f[1, 0, 2] == np.float32(cb[1, 2]) / 256
    i = rr.f444(pl, 10, 8, dtype=np.int16, interleaved=True)
    assert i.shape == (8, 8, 3) and i[3, 5].tolist() == [y[3, 5], cb[1, 2], cr[1, 2]]
    e = rr.energy(pl)
    assert e.dtype == np.float32 and e.shape == (3, 2, 2)
    assert e[0, 1, 0] == np.abs(y[4:, :4].astype(np.int64)).sum() and e[1, 0, 1] == 3 + 4 + 7 + 8 and e[2, 1, 1] == 3 * (11 + 12 + 15 + 16)


# ------------------------------------------------------------------------------------------------ what the cases of the GPU suite hold
def test_census_of_the_gpu_cases():
    """asserted, not assumed: the batches of cases.CASES (tests/test_gpu_residual.py runs every one) reach every branch of the addressing"""
    ats, sub_mixed, cu4, chroma_only_cbf = set(), False, False, False
    for spec in cases.CASES:
        b = cases.build_case(*spec)["batch"]
        lw, lh, cbf = b["log2w"].astype(int), b["log2h"].astype(int), b["cbf"].astype(int) & 7
        for i in np.nonzero(cbf)[0]:
            a = rr.ats_inter_of(b, i)
            if a:
                ats.add((a & 15, a >> 4))
        cu4 |= bool(((lw == 2) & (lh == 2) & (cbf != 0)).any())
        chroma_only_cbf |= bool((((cbf & 1) == 0) & ((cbf & 6) != 0)).any())
        if b.get("cbf_sub") is not None:
            for i in np.nonzero(((lw > 6) | (lh > 6)) & (cbf != 0))[0]:
                n_sub = (2 if lw[i] > 6 else 1) * (2 if lh[i] > 6 else 1)
                present = [sb for sb in range(4) if (sb & 1) < (2 if lw[i] > 6 else 1) and (sb >> 1) < (2 if lh[i] > 6 else 1)]
                assert len(present) == n_sub
                for c in range(3):
                    if (cbf[i] >> c) & 1:
                        bits = [(int(b["cbf_sub"][i]) >> (4 * c + sb)) & 1 for sb in present]
                        sub_mixed |= 0 in bits and 1 in bits
    assert ats == {(idx, pos) for idx in (1, 2, 3, 4) for pos in (0, 1)}, f"ATS-inter (idx, pos) reached: {sorted(ats)}"
    assert sub_mixed, "no CU above 64 with one cbf_sub bit clear and another set"
    assert cu4, "no coded 4x4 CU"
    assert chroma_only_cbf, "no CU with luma cbf clear and chroma cbf set"


def test_census_nonzero_in_all_planes():
    """the arena of a case with large CUs: values in all three planes, and the restatement's zeroing of empty 64x64 sub-blocks agrees with the arena"""
    case = cases.build_case(*spec_of("main_btt_ctu128_8b"))
    _, _, _, arena = cases.run_cpu("oracle", case, pad=False)
    r = rr.planes(case["batch"], arena, case["w"], case["h"])
    assert all((p != 0).any() for p in r)
    r_arena = rr.planes(dict(case["batch"], cbf_sub=None), arena, case["w"], case["h"])      # the arena alone: zeros where no sub-block was coded
    assert all(np.array_equal(a, z) for a, z in zip(r_arena, r))
