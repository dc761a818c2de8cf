"""The pair form of the residual pass (itdq_dispatch_pair in xevd_amd/csrc/itdq_body.h: inside the data-flow intra launch of an IQT sequence a residual workgroup takes two
adjacent entries of the item list and runs them as one double-width item), against the oracle.

Block level, through xgpu_test_itdq_pairs (the pair form on ceil(items / 2) workgroups): every class with 1, G - 1, G, G + 1, 2G - 1, 2G, 2G + 1 and 3G + 1 blocks - a lone
entry, a pair whose second item is partial, a full pair, an odd entry behind a full pair - on residual_inputs.mixed_item, started so that an all-dense item shares its
workgroup with a near-empty one (one item's sparsity masks must neither enable nor suppress work of the other), every block its own QP; 8 and 10 bit, DCT-II on all 36
classes, the four DST-VII / DCT-VIII pairs on 4 .. 32.
The sequential path, through xgpu_test_itdq_pairs_mixed: launches in which the two entries of every workgroup differ in class, or in the transform pair; the residual arena
is poisoned first and compared whole, so an entry left out or done with the other entry's geometry shows.
Picture level: small pictures through cases.run_gpu(resid=True, ahead=True) - the pass inside the previous picture's data-flow intra launch, with the launch's
item-count threshold for the pair form at 1 and at its default.
Bar: bit-exact."""
import functools

import numpy as np
import pytest

import cases
import residual_inputs as ri
import test_gpu_residual_items as items
from xevd_amd import abi

pytestmark = pytest.mark.gpu

POISON = 0x5A5A
BDS = (8, 10)
ALL_IDS = [f"{1 << a}x{1 << b}" for a, b in ri.CLASSES]
ATS_IDS = [f"{1 << a}x{1 << b}" for a, b in ri.ATS_CLASSES]


@pytest.fixture(scope="module")
def dec():
    from xevd_amd.decoder import XgpuDecoder
    d = XgpuDecoder(64, 64, 8, admvp=0, iqt=1, max_pics=2)
    yield d
    d.close()


def counts(g):
    """block counts of a class with G TBs per item: a lone entry (full or not), a pair with a partial second item, a full pair, an odd entry behind a full pair"""
    return sorted({m for m in (1, g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1, 3 * g + 1) if m >= 1})


@functools.lru_cache(maxsize=None)
def pair_blocks(lw, lh, bd, tr):
    """3G + 1 blocks of mixed_item started at its all-dense item, so that the items of the first workgroup are (all dense, near-empty) and those of the second (all zero but
    one block, dense and single alternating); every block its own QP, so the two items of a pair never share one.  -> (blocks, qps, the oracle's residuals), computed once"""
    g = ri.itdq_group(lw, lh)
    n = 3 * g + 1
    qps = ri.walk_qps(n, bd, start=lw + 2 * lh)
    blk = ri.mixed_item(lw, lh, qps, bd, 1, tr, start=g)
    exp = ri.oracle_blocks(blk, lw, lh, qps, bd, 1, tr)
    for a in (blk, qps, exp):
        a.setflags(write=False)
    return blk, qps, exp


def _run_counts(dec, lw, lh, bd, tr):
    g = ri.itdq_group(lw, lh)
    blk, qps, exp = pair_blocks(lw, lh, bd, tr)
    if g > 1:
        dense, sparse = (blk[:g] != 0).reshape(g, -1).sum(1), (blk[g:2 * g] != 0).reshape(g, -1).sum(1)
        assert dense.sum() > sparse.sum(), "the first workgroup pairs a dense item with a near-empty one"
    for m in counts(g):
        got = dec.test_itdq_pairs(blk[:m].reshape(-1), lw, lh, qps[:m], bd, tr_v=tr[0], tr_h=tr[1]).reshape(blk[:m].shape)
        bad = np.nonzero((got != exp[:m]).reshape(m, -1).any(1))[0]
        assert bad.size == 0, (lw, lh, bd, tr, "blocks", m, "first differing block", int(bad[0]), "item", int(bad[0]) // g, "qp", int(qps[bad[0]]),
                               got[bad[0]].ravel()[:6], exp[bad[0]].ravel()[:6])


@pytest.mark.parametrize("lw,lh", ri.CLASSES, ids=ALL_IDS)
def test_gpu_pairs_every_class(dec, lw, lh):
    """DCT-II, 8 and 10 bit: the eight block counts of the class through the pair form"""
    for bd in BDS:
        _run_counts(dec, lw, lh, bd, (0, 0))


@pytest.mark.parametrize("lw,lh", ri.ATS_CLASSES, ids=ATS_IDS)
def test_gpu_pairs_every_class_ats(dec, lw, lh):
    """the four pairs of DST-VII / DCT-VIII on 4 .. 32, 8 and 10 bit"""
    for bd in BDS:
        for tr in ri.ATS_PAIRS:
            _run_counts(dec, lw, lh, bd, tr)


# ------------------------------------------------------------------------------------------------ the sequential path
def _mixed(dec, groups, bd):
    """groups: (n_blocks, lw, lh, tr, log2s) -> the launch through xgpu_test_itdq_pairs_mixed against the oracle, the whole arena compared: what no block covers (the gap
    up to a group's start at a multiple of 64 samples, the columns beyond a strided block's width) must still hold the poison"""
    rows, qp_all, bufs, wants = [], [], [], []
    total = 0
    for gi, (n, lw, lh, tr, ls) in enumerate(groups):
        w, h = 1 << lw, 1 << lh
        qps = ri.walk_qps(n, bd, start=3 * gi + 1)
        blk = ri.mixed_item(lw, lh, qps, bd, 1, tr, start=ri.itdq_group(lw, lh) + gi)
        exp = ri.oracle_blocks(blk, lw, lh, qps, bd, 1, tr)
        pad = (-total) % 64
        buf = np.full((n, h, 1 << ls), 0x1234, np.int16)      # (the columns between a strided block's rows: coefficients nobody may read as such)
        want = np.full((n, h, 1 << ls), POISON, np.int16)
        buf[:, :, :w] = blk
        want[:, :, :w] = exp
        bufs += [np.zeros(pad, np.int16), buf.reshape(-1)]
        wants += [np.full(pad, POISON, np.int16), want.reshape(-1)]
        total += pad + buf.size
        rows.append((n, lw, lh, tr[0], tr[1], ls))
        qp_all.append(qps)
    got = dec.test_itdq_pairs_mixed(np.concatenate(bufs), rows, np.concatenate(qp_all), bd)
    want = np.concatenate(wants)
    bad = np.nonzero(got != want)[0]
    if bad.size:
        starts = np.cumsum([0] + [len(b) for b in bufs])
        part = int(np.searchsorted(starts, bad[0], side="right") - 1)
        raise AssertionError(("first differing sample", int(bad[0]), "group", part // 2, groups[part // 2] if part % 2 else "gap", got[bad[:4]], want[bad[:4]]))


def test_gpu_pairs_entries_of_two_classes(dec):
    """a lone 8x8 block, then G + 1 blocks of every class: entry 0 is alone in its class, every class has a full item at an odd place of the list and a one-block item
    at the even place behind it, so EVERY workgroup holds two entries of different classes and runs the single form twice (LDS forms, register forms and one of each);
    the last one-block item has no partner.  32x32 keeps a row stride of 128 samples and 8x16 one of twice its width.  10 bit, and 8 bit on a shorter list."""
    stride = {(5, 5): 7, (3, 4): 4}
    groups = [(1, 3, 3, (0, 0), 3)] + [(ri.itdq_group(lw, lh) + 1, lw, lh, (0, 0), stride.get((lw, lh), lw)) for lw, lh in ri.CLASSES]
    _mixed(dec, groups, 10)
    short = [(1, 2, 2, (0, 0), 2)] + [(ri.itdq_group(lw, lh) + 1, lw, lh, (0, 0), lw) for lw, lh in [(1, 1), (4, 4), (2, 2), (6, 6), (3, 1), (5, 3), (3, 3)]]
    _mixed(dec, short, 8)


@pytest.mark.parametrize("lw,lh", [(2, 2), (3, 3), (4, 5), (5, 2)], ids=["4x4", "8x8", "16x32", "32x4"])
def test_gpu_pairs_entries_of_two_transform_pairs(dec, lw, lh):
    """one class, a lone DCT-II block and then G + 1 blocks of each transform pair in turn: every workgroup holds two entries of the same class whose (tr_v, tr_h) differ -
    the one thing the pair form may not share - and runs them one after the other"""
    g = ri.itdq_group(lw, lh)
    trs = [(0, 0), (1, 1), (1, 2), (0, 0), (2, 1), (2, 2), (1, 1)]
    _mixed(dec, [(1, lw, lh, (0, 0), lw)] + [(g + 1, lw, lh, tr, lw) for tr in trs], 10)


# ------------------------------------------------------------------------------------------------ picture level
def _class_items(b):
    """TBs per class of a batch without ATS and without CUs above 64 (luma TB = the CU, chroma TBs half its size): -> {(lw, lh): TBs}"""
    out = {}
    for lw, lh, cbf in zip(b["log2w"].tolist(), b["log2h"].tolist(), b["cbf"].tolist()):
        if cbf & 1:
            out[(lw, lh)] = out.get((lw, lh), 0) + 1
        for bit in (2, 4):
            if cbf & bit:
                out[(lw - 1, lh - 1)] = out.get((lw - 1, lh - 1), 0) + 1
    return out


PICTURES = list(items.FORMS) + [
    # a second IQT picture, CTU 64, no ATS: long runs of one class, so most workgroups take the pair form
    ("pairs_main_10b", 208, 120, 10, 1, 1, (2, 2), 0.5, {"addb": 1, "alf": 1, "inter_frac": 0.5, "split_prob": 0.5, "coded_frac": 0.9}, 2),
    # at most 128 x 128: some class has at most G TBs, i.e. one item - an odd count inside the list
    ("pairs_main_small", 120, 72, 10, 1, 1, (1, 1), 0.4, {"inter_frac": 0.5, "split_prob": 0.45, "coded_frac": 0.9}, 3),
]


@pytest.fixture(scope="module")
def picture_refs():
    out = {}
    for spec in PICTURES:
        cs = cases.build_case(*spec[:9], seed=spec[9])
        ref, _, _, resid = cases.run_cpu("oracle", cs)
        out[spec[0]] = (cs, ref, resid)
    return out


@pytest.mark.parametrize("pair_min", ["1", None], ids=["two_items_per_workgroup", "default_threshold"])
@pytest.mark.parametrize("name", [s[0] for s in PICTURES])
def test_gpu_pairs_pictures(picture_refs, name, pair_min, monkeypatch):
    """the picture's residual pass queued with the previous picture's kernels (inside its data-flow intra launch): residual arena and all planes.  The launch gives a
    residual workgroup two items only from XEVD_HIP_ITDQ_PAIR_MIN items on (default 4096: an 8K picture; read when a context opens) - with 1 these small pictures take
    the pair form where the sequence has IQT, without it the same instantiation runs one entry per workgroup"""
    if pair_min is None:
        monkeypatch.delenv("XEVD_HIP_ITDQ_PAIR_MIN", raising=False)
    else:
        monkeypatch.setenv("XEVD_HIP_ITDQ_PAIR_MIN", pair_min)
    cs, ref, resid = picture_refs[name]
    b = cs["batch"]
    assert (b["pred_mode"] == abi.MODE_INTRA).sum() >= 32, "the picture needs intra CUs for a data-flow launch"
    if name == "items_main_10b":
        assert (b["log2w"] == 7).any() and (b["log2h"] == 7).any(), "a CU above 64: its 64x64 sub-blocks keep the CU's stride"
    if name == "pairs_main_small":
        assert cs["w"] <= 128 and cs["h"] <= 128
        tbs = _class_items(b)
        assert any(1 <= n <= ri.itdq_group(*c) for c, n in tbs.items() if min(c) >= 1), ("a class of one item", tbs)
    out, got = cases.run_gpu(cs, resid=True, ahead=True)
    bad = np.nonzero(got[:len(resid)] != resid)[0]
    assert bad.size == 0, ("residual arena", bad[:4], got[bad[:4]], resid[bad[:4]])
    for c in range(3):
        assert np.array_equal(out[c], ref.bufs[c]), f"{name} plane {c}: {np.argwhere(out[c] != ref.bufs[c])[:4]}"
