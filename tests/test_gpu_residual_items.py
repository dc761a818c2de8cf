"""The residual pass (k_itdq, and the same body inside k_intra_itdq) at the edges of its work items, against the oracle (orc_itdq / cases.run_cpu("oracle", ...),
which tests/test_oracle_vs_ref.py pins to the reference): partial last items of every class that keeps its TBs in registers and of the classes around them, the
ends of the dequantisation's range on the 32-bit path of the even classes and on the 64-bit path that the odd ones keep, and both launch forms on small pictures.
Bar: bit-exact."""
import ctypes as C

import numpy as np
import pytest

import cases
import oracle_lib as ol
from xevd_amd import abi

pytestmark = pytest.mark.gpu

SCALE = {0: (40, 45, 51, 57, 64, 71), 1: (40, 45, 51, 57, 64, 72)}      # xevd_tbl_dq_scale_b / xevd_tbl_dq_scale


def itdq_group(lw, lh):
    """TBs per 256-thread work item of a size class (itdq_group in xevd_amd/csrc/itdq_body.h)"""
    w, h = 1 << lw, 1 << lh
    return 256 // max(w * (h // 16 if h > 16 else 1), h * (w // 16 if w > 16 else 1))


@pytest.fixture(scope="module")
def decs():
    from xevd_amd.decoder import XgpuDecoder
    d = {(0, iqt): XgpuDecoder(64, 64, 8, admvp=0, iqt=iqt, max_pics=2) for iqt in (0, 1)}
    yield d
    for v in d.values():
        v.close()


def oracle_blocks(coef, lw, lh, qps, bd, iqt):
    orc = ol.oracle()
    n = 1 << (lw + lh)
    out = coef.copy()
    for i, qp in enumerate(qps):
        blk = np.ascontiguousarray(out[i * n:(i + 1) * n])
        orc.orc_itdq(blk.ctypes.data_as(C.c_void_p), lw, lh, int(qp), bd, iqt)
        out[i * n:(i + 1) * n] = blk
    return out


def sparse_blocks(rng, lw, lh, n_blocks, qps, bd, iqt):
    """content like synth.gen_frame's: a DC-ish level and a few low-frequency ones per block, capped so that the residual stays near the sample range; 64-point
    dimensions carry coefficients in their first 32 positions only"""
    w, h = 1 << lw, 1 << lh
    coef = np.zeros((n_blocks, h, w), np.int16)
    shift = bd - 9 + ((lw + lh) >> 1) + 8 * ((lw + lh) & 1)
    for b in range(n_blocks):
        gain = (SCALE[iqt][qps[b] % 6] << (qps[b] // 6)) * (181 if (lw + lh) & 1 else 1) / 2.0 ** shift
        cap = int(np.clip(np.floor(2.0 * (1 << bd) / gain), 1, 32767))
        nnz = int(min(rng.geometric(0.25), 24))
        px = np.minimum((np.abs(rng.normal(0, 1.0, nnz)) * w / 5.0).astype(np.int64), min(w, 32) - 1)
        py = np.minimum((np.abs(rng.normal(0, 1.0, nnz)) * h / 5.0).astype(np.int64), min(h, 32) - 1)
        lev = np.round(rng.laplace(0, 2.0, nnz)).astype(np.int64)
        lev[lev == 0] = 1
        coef[b, py, px] = np.clip(lev, -cap, cap)
        dc = int(np.round(rng.laplace(0, 6.0))) or 1
        coef[b, 0, 0] = np.clip(dc, -cap, cap)
    return coef


# the classes whose TBs stay in registers (W * H <= 16), the first class beside them, a class with masks, and two whose chunk index is not wave-uniform
BOUNDARY_CLASSES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 3), (3, 1), (3, 3), (4, 4), (2, 5), (5, 2)]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("iqt", [0, 1])
@pytest.mark.parametrize("lw,lh", BOUNDARY_CLASSES, ids=[f"{1 << a}x{1 << b}" for a, b in BOUNDARY_CLASSES])
def test_gpu_item_boundaries(decs, lw, lh, iqt, bd):
    """G - 1, G, G + 1 and 2G + 1 blocks of a class (a full item, items whose last lanes / waves / load units have no TB), every block its own QP; the block in the
    middle of each batch holds one coefficient only, in the last row pair and the last column pair the sparsity masks cover"""
    g, w, h = itdq_group(lw, lh), 1 << lw, 1 << lh
    rng = np.random.default_rng(1000 * lw + 100 * lh + 10 * iqt + bd)
    for n_blocks in (g - 1, g, g + 1, 2 * g + 1):
        if n_blocks == 0:
            continue
        qps = rng.integers(0, 52, n_blocks) + 6 * (bd - 8) * rng.integers(0, 2, n_blocks)
        coef = sparse_blocks(rng, lw, lh, n_blocks, qps, bd, iqt)
        coef[n_blocks // 2] = 0
        coef[n_blocks // 2, min(h, 32) - 1, min(w, 32) - 1] = -3
        coef = coef.reshape(-1)
        exp = oracle_blocks(coef, lw, lh, qps, bd, iqt)
        got = decs[(0, iqt)].test_itdq(coef, lw, lh, qps, bd)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (n_blocks, "first differing block", int(bad[0]) >> (lw + lh), "of", n_blocks, got[bad[:4]], exp[bad[:4]])


EVEN_CLASSES = [(a, b) for a in range(1, 7) for b in range(1, 7) if (a + b) % 2 == 0]
RANGE_CLASSES = EVEN_CLASSES + [(2, 3), (4, 5)]      # + 4x8 and 16x32: the s64 form the odd classes keep


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("lw,lh", RANGE_CLASSES, ids=[f"{1 << a}x{1 << b}" for a, b in RANGE_CLASSES])
def test_gpu_dequant_range(decs, lw, lh, bd):
    """levels +-1, +-32767 and -32768 at QP 0, 5, 17, 51 and at the top of the bit depth's range (51 + 6 (bd - 8): the scale's shift is past 8 there, where the
    32-bit product holds the level to a bound beyond which the result is clipped anyway), both scale tables: one level per block at three positions, and all
    five levels in one block (five clipped s16 values keep every sum of both transforms far inside 32 bits)."""
    w, h = 1 << lw, 1 << lh
    levels = (1, -1, 32767, -32767, -32768)
    qp_list = sorted({0, 5, 17, 51, 51 + 6 * (bd - 8)})
    # positions: DC, the last position the masks cover, one in between
    spots = sorted({(0, 0), (min(h, 32) - 1, min(w, 32) - 1), (h // 2 - 1 if h > 2 else 0, w // 2)})
    blocks, qps = [], []
    for qp in qp_list:
        for i, lev in enumerate(levels):
            for (y, x) in spots:
                b = np.zeros((h, w), np.int16)
                b[y, x] = lev
                blocks.append(b)
                qps.append(qp)
        # and all five levels in one block
        b = np.zeros((h, w), np.int16)
        for i, lev in enumerate(levels):
            b[(i * 3) % min(h, 32), (i * 5) % min(w, 32)] = lev
        blocks.append(b)
        qps.append(qp)
    coef = np.stack(blocks).reshape(-1)
    for iqt in (0, 1):
        exp = oracle_blocks(coef, lw, lh, qps, bd, iqt)
        got = decs[(0, iqt)].test_itdq(coef, lw, lh, qps, bd)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (iqt, "first differing block", int(bad[0]) >> (lw + lh), "qp", qps[int(bad[0]) >> (lw + lh)], got[bad[:4]], exp[bad[:4]])


FORMS = [      # cases.build_case's arguments, then its seed
    # CTU 128, so that a 64x64 sub-block of a larger CU keeps the CU's row stride; ATS (DST-VII / DCT-VIII work items, 4x4 among them), ATS-inter and BTT classes
    ("items_main_10b", 192, 136, 10, 1, 1, (2, 2), 0.5, {"addb": 1, "alf": 1, "log2_ctu": 7, "inter_frac": 0.5, "split_prob": 0.35, "ats_frac": 0.6, "ats_inter_frac": 0.5,
                                                         "btt_frac": 0.5, "coded_frac": 0.8}, 1),
    # Baseline, 8 bit: the 32-bit intermediate of the non-IQT instantiation (hi * 2^15 + lo)
    ("items_base_8b", 192, 136, 8, 0, 0, (1, 1), 0.4, {"inter_frac": 0.5, "split_prob": 0.6, "coded_frac": 0.8}, 0),
]


@pytest.fixture(scope="module")
def form_refs():
    out = {}
    for spec in FORMS:
        cs = cases.build_case(*spec[:9], seed=spec[9])
        ref, _, _, resid = cases.run_cpu("oracle", cs)
        out[spec[0]] = (cs, ref, resid)
    return out


@pytest.mark.parametrize("ahead", [False, True], ids=["own_launch", "inside_intra_launch"])
@pytest.mark.parametrize("name", [s[0] for s in FORMS])
def test_gpu_both_launch_forms(form_refs, name, ahead):
    """the pass as a launch of its own and queued with the previous picture's kernels (inside its data-flow intra launch): residual arena and all planes"""
    cs, ref, resid = form_refs[name]
    b = cs["batch"]
    assert (b["pred_mode"] == abi.MODE_INTRA).sum() >= 32, "the picture needs intra CUs for a data-flow launch"
    if name == "items_main_10b":
        assert (b["log2w"] == 7).any() and (b["log2h"] == 7).any(), "a CU above 64: its 64x64 sub-blocks keep the CU's stride"
    out, got = cases.run_gpu(cs, resid=True, ahead=ahead)
    bad = np.nonzero(got[:len(resid)] != resid)[0]
    assert bad.size == 0, ("residual arena", bad[:4], got[bad[:4]], resid[bad[:4]])
    for c in range(3):
        assert np.array_equal(out[c], ref.bufs[c]), f"{name} plane {c}: {np.argwhere(out[c] != ref.bufs[c])[:4]}"
