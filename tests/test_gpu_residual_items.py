"""The residual pass (k_itdq, and the same body inside k_intra_itdq) at the edges of its work items, against the oracle (orc_itdq / cases.run_cpu("oracle", ...),
which tests/test_oracle_vs_ref.py pins to the reference): partial last items of every class that keeps its TBs in registers and of the classes around them, the
ends of the dequantisation's range on the 32-bit path of the even classes and on the 64-bit path that the odd ones keep, and both launch forms on small pictures.

Then every range argument of xevd_amd/csrc/itdq_body.h at block level, through xgpu_test_itdq_ex (which names the transform pair and the row stride), on the blocks of
tests/residual_inputs.py - the same blocks tests/test_oracle_extremes.py feeds the reference: single levels at every position (32 .. 63 of a 64-point dimension among them),
blocks whose terms all add at one output, aimed at each side of the stage-1 clip and of the final clip, every threshold level of the dequantiser at every QP (its clips,
2^23 >> (qp / 6) and its neighbours, the last level that dequantises to 0), work items that mix dense and near-empty blocks (the wave's union of sparsity masks against a
TB's own, LDS an earlier workgroup filled), for all 36 classes, 8 / 10 / 12 bit, both instantiations, DCT-II and the four ATS pairs on 4 .. 32; blocks that keep a row stride
beyond their width; and two promises of the kernel's own that no reference pins: the 32-bit intermediate beyond the range on which the reference's second stage is
defined, and the dequantiser's hold at the shift of 13 that a bit depth of 16 gives.
Bar: bit-exact."""
import ctypes as C

import numpy as np
import pytest

import cases
import oracle_lib as ol
import residual_inputs as ri
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


# ------------------------------------------------------------------------------------------------ every branch of the arithmetic, block level
ALL_IDS = [f"{1 << a}x{1 << b}" for a, b in ri.CLASSES]


def _launch_and_compare(dec, blk, lw, lh, qps, bd, iqt, tr, what):
    """ALL blocks in one launch - nothing is cut off - and then launches of G - 1, G + 1 and 2G + 1 blocks, so that partial items occur with these inputs too: the first
    blocks of the batch, which wraps around where it is shorter than that"""
    g = ri.itdq_group(lw, lh)
    n = len(qps)
    qps = np.asarray(qps)
    exp = ri.oracle_blocks(blk, lw, lh, qps, bd, iqt, tr)
    for m in (n, g - 1, g + 1, 2 * g + 1):
        if m < 1:
            continue
        idx = np.arange(m) % n
        got = dec.test_itdq(blk[idx].reshape(-1), lw, lh, qps[idx], bd, tr_v=tr[0], tr_h=tr[1]).reshape(blk[idx].shape)
        bad = np.nonzero((got != exp[idx]).reshape(m, -1).any(1))[0]
        assert bad.size == 0, (what, lw, lh, bd, iqt, tr, "blocks", m, "first differing block", int(bad[0]), "qp", int(qps[idx][bad[0]]), got[bad[0]].ravel()[:6], exp[idx][bad[0]].ravel()[:6])


def _check_single_walk(blk, lw, lh, cen):
    """every position of single_positions was fed, one level per block, and - for a class with a side of 16 or more, which the census counts - the oracle saw a single level
    in exactly the (row pair, column pair) cells those positions lie in"""
    assert ((blk != 0).reshape(len(blk), -1).sum(1) == 1).all()
    fed = {(int(y), int(x)) for _, y, x in np.argwhere(blk != 0)}
    assert fed == set(ri.single_positions(lw, lh)), sorted(set(ri.single_positions(lw, lh)) - fed)[:8]
    cells = np.zeros((32, 32), bool)
    if max(lw, lh) >= 4:
        for y, x in fed:
            cells[y >> 1, x >> 1] = True
        assert cells.sum() == (1 << (lw + lh)) // 4, "every (row pair, column pair) of the class"
    assert ((cen["it_single"] > 0) == cells).all(), np.argwhere((cen["it_single"] > 0) != cells)[:8].tolist()


def _blocks(kind, lw, lh, bd, iqt, tr):
    g = ri.itdq_group(lw, lh)
    n = max(ri.n_blocks_for(kind, lw, lh), 2 * g + 1)
    qps = ri.walk_qps(n, bd, start=lw + 2 * lh)
    return ri.blocks(kind, lw, lh, qps, bd, iqt, tr, sub="defined" if kind == "dense_signed" else None), qps


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("kind", ["single", "dense_signed", "mixed_item"])
@pytest.mark.parametrize("lw,lh", ri.CLASSES, ids=ALL_IDS)
def test_gpu_residual_blocks(decs, lw, lh, kind, bd):
    """one generator on one class, both instantiations (iqt 0 / 1), against orc_itdq: at least 2G + 1 blocks in one launch, then G - 1 and G + 1.  The 32-bit intermediate
    keeps to the `defined` sub-kind here - these are the blocks the oracle is pinned to the reference on; beyond it: test_gpu_residual_beyond_the_defined_range.
    `single`: every position of the class (above 256 samples: every pair of rows x pair of columns) is fed, held by the walk itself and by the oracle's it_single"""
    for iqt in (0, 1):
        blk, qps = _blocks(kind, lw, lh, bd, iqt, (0, 0))
        ol.census_reset()
        _launch_and_compare(decs[(0, iqt)], blk, lw, lh, qps, bd, iqt, (0, 0), kind)
        if kind == "single":
            _check_single_walk(blk, lw, lh, ol.census())


ATS_IDS = [f"{1 << a}x{1 << b}" for a, b in ri.ATS_CLASSES]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("kind", ["single", "dense_signed", "thresholds", "mixed_item"])
@pytest.mark.parametrize("lw,lh", ri.ATS_CLASSES, ids=ATS_IDS)
def test_gpu_residual_blocks_ats(decs, lw, lh, kind, bd):
    """the same on 4 .. 32 for the four pairs of DST-VII / DCT-VIII, against orc_itdq_ats: the clipped s16 intermediate also where IQT is 0"""
    for iqt in (0, 1):
        for tr in ri.ATS_PAIRS:
            blk, qps = _blocks(kind, lw, lh, bd, iqt, tr)
            _launch_and_compare(decs[(0, iqt)], blk, lw, lh, qps, bd, iqt, tr, kind)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("lw,lh", ri.CLASSES, ids=ALL_IDS)
def test_gpu_residual_thresholds_at_every_qp(decs, lw, lh, bd):
    """every threshold level of the dequantiser that s16 holds, at every QP of 0 .. 51 + 6 (bd - 8): the last level that does not clip and the first that does, both
    signs; 2^23 >> (qp / 6) - the bound the 32-bit product of the even classes holds a level to - with its neighbours; the last level that dequantises to 0 and the first
    that does not.  One level per block, at DC, in the middle or in the last position."""
    for iqt in (0, 1):
        blk, qps = ri.thresholds_all(lw, lh, bd, iqt, range(ri.qp_top(bd) + 1))
        assert set(qps.tolist()) == set(range(ri.qp_top(bd) + 1)), "every QP is fed"
        for qp in (0, ri.qp_top(bd)):      # and every level of a QP that s16 holds (the first and the last QP stand for the rest: thresholds_all walks them alike)
            want = sorted(v for nm, v in ri.threshold_levels(lw, lh, qp, bd, iqt) if not nm.endswith("!"))
            assert sorted(int(b.sum()) for b in blk[qps == qp]) == want
        _launch_and_compare(decs[(0, iqt)], blk, lw, lh, qps, bd, iqt, (0, 0), "thresholds")


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("lw,lh", ri.CLASSES, ids=ALL_IDS)
def test_gpu_residual_beyond_the_defined_range(decs, lw, lh, bd):
    """Blocks that drive the 32-bit intermediate as far as s16 levels can (every level +-32767, the terms adding at one output), and blocks on either side of the final
    clip, against the oracle's s64 arithmetic.  This is the kernel's own promise - the split hi * 2^15 + lo is exact for intermediates below 2^28 - and NOT a reference
    pin: on these blocks the reference's 32-bit second stage overflows (tests/test_oracle_extremes.py leaves them out, by the oracle's it_s2_undef)."""
    g = ri.itdq_group(lw, lh)
    n = max(18, 2 * g + 1)
    qps = ri.walk_qps(n, bd, start=lw + lh)
    blk = ri.dense_signed(lw, lh, qps, bd, 0, (0, 0), sub="beyond")
    ol.census_reset()
    _launch_and_compare(decs[(0, 0)], blk, lw, lh, qps, bd, 0, (0, 0), "beyond")
    cen = ol.census()
    # beyond the reference's range wherever the class can get there at all - the largest column sums of |tm| of its two dimensions times 32768 reach 2^31: from 4x8 on,
    # not the four classes of up to 4x4 with 2x8 and 8x2 - and still below the 2^27 that no intermediate reaches
    reach = int(np.abs(ri.matrix(0, lh)).sum(0).max()) * 32768 * int(np.abs(ri.matrix(0, lw)).sum(0).max()) >= 1 << 31
    assert (cen["it_s2_undef"] > 0) == reach and cen["it_s1_mag"][3:].sum() == 0, (reach, int(cen["it_s2_undef"]), cen["it_s1_mag"].tolist())


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("stride", ["twice_the_width", "128"])
@pytest.mark.parametrize("lw,lh", [(5, 5), (6, 6), (3, 4), (4, 6)], ids=["32x32", "64x64", "8x16", "16x64"])
def test_gpu_residual_strided_blocks(decs, lw, lh, stride, bd):
    """blocks that keep a row stride of twice their width and of 128 samples (a 64x64 sub-block of a CU of 128 keeps the CU's stride; for 64x64 the two are one): the
    columns between the blocks' rows are filled with a pattern and must come back untouched"""
    g = ri.itdq_group(lw, lh)
    n, w, h, ls = 2 * g + 1, 1 << lw, 1 << lh, lw + 1 if stride == "twice_the_width" else 7
    qps = ri.walk_qps(n, bd, start=3)
    for iqt in (0, 1):
        blk = np.concatenate([ri.blocks(k, lw, lh, qps[i::4], bd, iqt, (0, 0), start=i, sub="defined") for i, k in enumerate(ri.GENERATORS)])
        qq = np.concatenate([qps[i::4] for i in range(4)])
        exp = ri.oracle_blocks(blk, lw, lh, qq, bd, iqt)
        buf = ((np.arange(n * (h << ls), dtype=np.int64) * 2654435761 >> 7) & 0xFFFF).astype(np.uint16).view(np.int16).reshape(n, h, 1 << ls).copy()
        want = buf.copy()
        buf[:, :, :w] = blk
        want[:, :, :w] = exp
        got = decs[(0, iqt)].test_itdq(buf.reshape(-1), lw, lh, qq, bd, log2s=ls).reshape(buf.shape)
        assert np.array_equal(got[:, :, w:], want[:, :, w:]), "samples outside the blocks' columns changed"
        assert np.array_equal(got[:, :, :w], want[:, :, :w]), (iqt, np.argwhere(got[:, :, :w] != want[:, :, :w])[:4].tolist())


def test_gpu_residual_shim_refuses_what_the_builder_refuses(decs):
    """DST-VII / DCT-VIII outside 4 .. 32 or mixed with DCT-II, and a stride below the width"""
    from xevd_amd.decoder import XgpuError
    z = np.zeros(64 * 64, np.int16)
    for lw, lh, tr_v, tr_h, ls in [(6, 3, 1, 1, None), (3, 1, 2, 1, None), (3, 3, 1, 0, None), (3, 3, 0, 2, None), (3, 3, 3, 1, None), (4, 4, 0, 0, 3), (2, 3, 0, 0, 3)]:
        with pytest.raises(XgpuError):
            decs[(0, 1)].test_itdq(z[:1 << ((ls or lw) + lh)], lw, lh, [30], 10, tr_v=tr_v, tr_h=tr_h, log2s=ls)


@pytest.mark.parametrize("lw,lh", [(4, 4), (6, 2), (2, 6), (5, 5), (3, 3)], ids=["16x16", "64x4", "4x64", "32x32", "8x8"])
def test_gpu_residual_mixed_items_over_many_workgroups(decs, lw, lh):
    """mixed_item over 4096 work items in one launch - more than the device holds at once, so the later workgroups start on LDS that dense items filled: a column pair a TB
    did not write must read as zero whatever lies there (the `own` mask of stage 2), at 10 bit under both instantiations"""
    g = ri.itdq_group(lw, lh)
    n = 4096 * g + 1
    qps = ri.walk_qps(n, 10, start=1)
    base = {iqt: ri.mixed_item(lw, lh, qps[:64 * g], 10, iqt) for iqt in (0, 1)}
    for iqt in (0, 1):
        blk = np.concatenate([base[iqt]] * 64 + [base[iqt][:1]])
        qq = np.concatenate([qps[:64 * g]] * 64 + [qps[:1]])
        exp = np.concatenate([ri.oracle_blocks(base[iqt], lw, lh, qps[:64 * g], 10, iqt)] * 64 + [ri.oracle_blocks(base[iqt][:1], lw, lh, qps[:1], 10, iqt)])
        got = decs[(0, iqt)].test_itdq(blk.reshape(-1), lw, lh, qq, 10).reshape(blk.shape)
        bad = np.nonzero((got != exp).reshape(n, -1).any(1))[0]
        assert bad.size == 0, (iqt, "first differing block", int(bad[0]), "of", n, "item kind", (int(bad[0]) // g) % 4)


def test_gpu_dequantiser_hold_at_shift_13(decs):
    """The 32-bit dequantiser of the even classes holds a level to 2^23 >> (qp / 6) and relies on everything beyond being clipped anyway, "for every shift <= 13 (bit depths
    to 16)" (itdq_body.h).  Up to 12 bit the shift is at most 9 and a level of half that bound is clipped already, so no input of the other tests can tell a smaller bound
    from the right one.  At a bit depth of 16 the 64x64 class has the shift of 13: levels between half the bound and the first that clips dequantise to values inside s16,
    and a hold below the bound changes them.  Against the oracle's s64 dequantiser; the kernel's own promise, not a reference pin (no profile has 16 bit)."""
    lw = lh = 6
    blocks, qps = [], []
    for qp in range(48, 96, 6):                               # qp % 6 == 0: the multiplier is 40 << (qp / 6), the smallest, which leaves the widest band below the clip
        cmax = (1 << 23) >> (qp // 6)
        mul, shift, offset = ri.dq_params(lw, lh, qp, 16, 1)
        assert shift == 13
        first_clip = ((32768 << shift) - offset - 1) // mul + 1
        assert cmax // 2 < first_clip - 1 <= cmax
        for lev in (cmax // 2 + 1, (cmax // 2 + first_clip) // 2, first_clip - 1, first_clip, cmax - 1, cmax):
            for sg in (1, -1):
                if abs(lev) <= 32767:
                    b = np.zeros((64, 64), np.int16)
                    b[(len(blocks) * 5) % 64, (len(blocks) * 3) % 64] = sg * lev
                    blocks.append(b)
                    qps.append(qp)
    assert len(blocks) >= 24
    blk, qps = np.stack(blocks), np.asarray(qps, np.uint8)
    for iqt in (0, 1):
        exp = ri.oracle_blocks(blk, lw, lh, qps, 16, iqt)
        got = decs[(0, iqt)].test_itdq(blk.reshape(-1), lw, lh, qps, 16).reshape(blk.shape)
        bad = np.nonzero((got != exp).reshape(len(qps), -1).any(1))[0]
        assert bad.size == 0, (iqt, "first differing block", int(bad[0]), "qp", int(qps[bad[0]]), "level", int(blk[bad[0]].sum()))
