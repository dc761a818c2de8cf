"""Inputs for the residual pass (dequantisation + the two transform stages) that sit on the range arguments of xevd_amd/csrc/itdq_body.h: blocks of one size class for the
block-level tests (tests/test_gpu_residual_items.py on the GPU, tests/test_oracle_extremes.py against the reference) and, through `fill_tb`, the TBs of the picture cases
of extreme_inputs.RESIDUAL_CASES.

The arithmetic is restated here in exact integers (`model`) for ONE purpose: choosing magnitudes by search, so that a block lands on the wanted side of a clip.  No
expected value comes from it - those are the oracle's and the reference's - and that the blocks land where they were aimed is asserted through the oracle's census
(it_* counters).

Transform codes are the kernel's: 0 DCT-II, 1 DST-VII, 2 DCT-VIII (TR_* of xgpu_internal.h); the oracle's orc_itdq_ats takes 0 DST-VII, 1 DCT-VIII, i.e. code - 1."""
import ctypes as C
import functools

import numpy as np

import oracle_lib as ol

SCALE = {0: (40, 45, 51, 57, 64, 71), 1: (40, 45, 51, 57, 64, 72)}      # xevd_tbl_dq_scale_b / xevd_tbl_dq_scale
CLASSES = [(a, b) for a in range(1, 7) for b in range(1, 7)]
ATS_CLASSES = [(a, b) for a in range(2, 6) for b in range(2, 6)]
ATS_PAIRS = [(1, 1), (1, 2), (2, 1), (2, 2)]
GENERATORS = ("single", "dense_signed", "thresholds", "mixed_item")


def itdq_group(lw, lh):
    """TBs per 256-thread work item of a size class (itdq_group in xevd_amd/csrc/itdq_body.h)"""
    w, h = 1 << lw, 1 << lh
    return 256 // max(w * (h // 16 if h > 16 else 1), h * (w // 16 if w > 16 else 1))


def qp_top(bd):
    return 51 + 6 * (bd - 8)


def dq_params(lw, lh, qp, bd, iqt):
    """-> (mul, shift, offset) of xevd_dquant for the class: clip16((level * mul + offset) >> shift)"""
    odd = (lw + lh) & 1
    shift = bd - 9 + ((lw + lh) >> 1) + 8 * odd
    return (SCALE[iqt][qp % 6] << (qp // 6)) * (181 if odd else 1), shift, (1 << (shift - 1)) if shift else 0


def dequant(level, lw, lh, qp, bd, iqt):
    mul, shift, offset = dq_params(lw, lh, qp, bd, iqt)
    return np.clip((np.asarray(level, np.int64) * mul + offset) >> shift, -32768, 32767)


@functools.lru_cache(maxsize=None)
def matrix(tr, log2n):
    """M[k][n] (coefficient k -> output n) of one stage, int64: xevd_tbl_tm* / xevd_tbl_tr* as the oracle builds them (both pinned to the reference's tables), the 4-point
    ATS kernels in their matrix form"""
    orc = ol.oracle()
    n = 1 << log2n
    if tr == 0:
        return np.ctypeslib.as_array(orc.orc_tm(log2n), (n, n)).astype(np.int64)
    m = np.ctypeslib.as_array(orc.orc_ats_tm(2 - tr, log2n), (n, n)).astype(np.int64)      # the oracle's table index: DCT8 = 0, DST7 = 1
    if n == 4:
        a, b, c, d = (int(v) for v in m[0])
        if tr == 1:
            m = np.array([[a, b, c, b + a], [c, c, 0, -c], [a + b, -a, -c, b], [b, -(b + a), c, -a]], np.int64)
        else:
            m = np.array([[d + c, b, c, d], [b, 0, -b, -b], [c, -b, -d, d + c], [d, -b, d + c, -c]], np.int64)
    return m


def model(coef, lw, lh, qp, bd, iqt, tr=(0, 0)):
    """the two stages on one block (H x W levels) in exact integers -> the values BEFORE each clip and the reference-undefined sum:
    {'s1': stage-1 results before the s16 clip (s16 intermediate) or the 32-bit intermediates, 's2': results before the final clip, 'undef': the largest
    sum_k |tm[k][n]| * |t[k]| of the second stage}"""
    mv, mh = matrix(tr[0], lh), matrix(tr[1], lw)
    s16_mid = bool(iqt) or tr != (0, 0)
    d = dequant(coef, lw, lh, qp, bd, iqt)
    t = mv.T @ d                                            # t[n][j]: output row n of column j
    if s16_mid:
        s1 = (t + 64) >> 7
        t = np.clip(s1, -32768, 32767)
        sh = 20 - bd
    else:
        s1 = t
        sh = 27 - bd
    s2 = (t @ mh + (1 << (sh - 1))) >> sh
    return {"s1": s1, "s2": s2, "undef": int((np.abs(t) @ np.abs(mh)).max())}


def signed_block(lw, lh, tr, n0, m0, level):
    """every position +-level with the signs of column n0 of the vertical matrix times column m0 of the horizontal one: all terms add at output (n0, m0)"""
    sv = np.where(matrix(tr[0], lh)[:, n0] < 0, -1, 1)
    sh = np.where(matrix(tr[1], lw)[:, m0] < 0, -1, 1)
    return np.outer(sv, sh).astype(np.int64) * int(level)


def _first_level(pred):
    """the smallest level in 1 .. 32767 for which pred holds (pred is monotone in the level: every term of the focused sum grows with it), or None"""
    if not pred(32767):
        return None
    lo, hi = 0, 32767                                       # pred(lo) false (level 0: an empty block), pred(hi) true
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    return hi


# targets of dense_signed.  s16 intermediate (IQT, ATS): each side of the stage-1 clip and of the final clip; 32-bit intermediate: each side of the final clip,
# `defined` - the largest level that keeps every second-stage sum where the reference's 32-bit products are defined -, `defined_col` - the same with the levels in
# column 0 alone (each second-stage sum then has one term, so the intermediate itself may pass 2^24: a dense row of them may not) - and `beyond` - the s16 maximum
TARGETS_S16 = ("s1_hi", "s1_lo", "s2_hi", "s2_lo")
TARGETS_S32 = ("s2_hi", "s2_lo", "defined", "defined_col", "beyond")


@functools.lru_cache(maxsize=None)
def dense_levels(lw, lh, qp, bd, iqt, tr, n0, m0, target):
    """-> the signed levels (at most two: the last one on the near side of the target and the first on the far side) for a signed_block at (n0, m0)"""
    sign = -1 if target.endswith("_lo") else 1

    def run(level, sg=None):
        blk = signed_block(lw, lh, tr, n0, m0, (sign if sg is None else sg) * level)
        if target == "defined_col":
            blk[:, 1:] = 0
        return model(blk, lw, lh, qp, bd, iqt, tr)
    if target == "beyond":
        return (32767, -32767)
    if target.startswith("defined"):
        out = []
        for sg in (1, -1):      # (the dequantiser rounds towards minus infinity: the two signs differ by one)
            first = _first_level(lambda v: run(v, sg)["undef"] >= 1 << 31)
            out += [sg * 32767] if first is None else ([sg * (first - 1)] if first > 1 else [])
        return tuple(out)
    key = target[:2]
    if sign > 0:
        first = _first_level(lambda v: run(v)[key].max() > 32767)
    else:
        first = _first_level(lambda v: run(v)[key].min() < -32768)
    if first is None:
        return (sign * 32767,)                                # the clip is out of reach for this class and QP: the largest block there is
    return tuple(sign * v for v in (first - 1, first) if v > 0)


def dense_signed(lw, lh, qps, bd, iqt, tr=(0, 0), sub=None, start=0):
    """one block per QP, the target and the focus (n0, m0) walking with the block index; sub: 'defined' / 'beyond' restrict the 32-bit intermediate to that sub-kind
    (and to the final-clip targets that stay defined resp. to all of them)"""
    w, h = 1 << lw, 1 << lh
    s16_mid = bool(iqt) or tr != (0, 0)
    targets = TARGETS_S16 if s16_mid else (("defined", "defined_col") if sub == "defined" else ("beyond", "s2_hi", "s2_lo") if sub == "beyond" else TARGETS_S32)
    out = np.zeros((len(qps), h, w), np.int16)
    for b, qp in enumerate(qps):
        k = b + start
        n0, m0 = (k * 5) % h, (k * 3) % w
        if k % 3 == 0:                                        # the column of each matrix whose absolute sum is largest: the furthest any output can be driven
            n0, m0 = int(np.abs(matrix(tr[0], lh)).sum(0).argmax()), int(np.abs(matrix(tr[1], lw)).sum(0).argmax())
        target = targets[k % len(targets)]
        lev = dense_levels(lw, lh, int(qp), bd, iqt, tr, n0, m0, target)
        if not lev and target == "defined":                   # at this QP a block of +-1 throughout is beyond the rule already: one column is not
            target = "defined_col"
            lev = dense_levels(lw, lh, int(qp), bd, iqt, tr, n0, m0, target)
        out[b] = signed_block(lw, lh, tr, n0, m0, lev[(k // len(targets)) % len(lev)] if lev else 1)
        if target == "defined_col":
            out[b, :, 1:] = 0
        if not lev:
            out[b, 1:, :] = 0                                 # (nor a column: one level)
    return out


def mid_level(lw, lh, qp, bd, iqt):
    """a level that dequantises to about a quarter of the s16 range"""
    mul, shift, _ = dq_params(lw, lh, qp, bd, iqt)
    return int(min(max((8192 << shift) // mul, 2), 32767))


def single_positions(lw, lh):
    """every position of a block of at most 256 samples; above, one position per (row pair, column pair), its place inside the pair walking"""
    w, h = 1 << lw, 1 << lh
    if w * h <= 256:
        return [(y, x) for y in range(h) for x in range(w)]
    return [(2 * rp + ((rp + cp) & 1), 2 * cp + ((rp + cp) >> 1 & 1)) for rp in range(h // 2) for cp in range(w // 2)]


def single(lw, lh, qps, bd, iqt, tr=(0, 0), start=0, at=None):
    """one level per block: block k holds it at position k of single_positions (positions 32 .. 63 of a 64-point dimension among them; `at`: at that (y, x)), magnitude
    and sign walking over +-1, +-(mid-range), +-32767 with the round"""
    w, h = 1 << lw, 1 << lh
    pos = single_positions(lw, lh)
    out = np.zeros((len(qps), h, w), np.int16)
    for b, qp in enumerate(qps):
        k = b + start
        y, x = pos[k % len(pos)] if at is None else at
        m = (k + k // len(pos)) % 6
        mag = (1, mid_level(lw, lh, int(qp), bd, iqt), 32767)[m % 3]
        out[b, y, x] = -mag if m >= 3 else mag
    return out


def threshold_levels(lw, lh, qp, bd, iqt):
    """-> [(name, level)] in exact integers; a name ending in '!' is a level beyond s16 (not representable: skipped by the callers, listed so that they can tell)"""
    mul, shift, offset = dq_params(lw, lh, qp, bd, iqt)
    hi = ((32768 << shift) - offset - 1) // mul               # the largest level with (level * mul + offset) >> shift <= 32767
    lo = -(((32768 << shift) + offset) // mul)                # the smallest with ... >= -32768
    z_pos = ((1 << shift) - offset - 1) // mul                # the largest with ... == 0
    z_neg = -(offset // mul)                                  # the smallest (negative or zero) with ... == 0
    cmax = (1 << 23) >> (qp // 6)
    lv = [("hi_in", hi), ("hi_clip", hi + 1), ("lo_in", lo), ("lo_clip", lo - 1), ("zero_pos", z_pos), ("nonzero_pos", z_pos + 1), ("zero_neg", z_neg), ("nonzero_neg", z_neg - 1)]
    for d in (-1, 0, 1):
        lv += [(f"cmax{d:+d}", cmax + d), (f"-cmax{d:+d}", -(cmax + d))]
    return [(n if -32768 <= v <= 32767 else n + "!", v) for n, v in lv if v != 0]


def thresholds(lw, lh, qps, bd, iqt, tr=(0, 0), start=0):
    """one level per block from threshold_levels of the block's QP, walking; the position walks over DC, the middle and the last position"""
    w, h = 1 << lw, 1 << lh
    spots = [(0, 0), (h // 2, w // 2 - 1), (h - 1, w - 1)]
    out = np.zeros((len(qps), h, w), np.int16)
    for b, qp in enumerate(qps):
        k = b + start
        lv = [v for n, v in threshold_levels(lw, lh, int(qp), bd, iqt) if not n.endswith("!")]
        y, x = spots[(k // max(len(lv), 1)) % 3]
        out[b, y, x] = lv[k % len(lv)] if lv else 1
    return out


def thresholds_all(lw, lh, bd, iqt, qp_list):
    """every representable threshold level of every QP of qp_list, one block each -> (blocks, qps)"""
    blocks, qps = [], []
    w, h = 1 << lw, 1 << lh
    spots = [(0, 0), (h // 2, w // 2 - 1), (h - 1, w - 1)]
    for qp in qp_list:
        for i, (n, v) in enumerate(threshold_levels(lw, lh, qp, bd, iqt)):
            if n.endswith("!"):
                continue
            b = np.zeros((h, w), np.int16)
            b[spots[(i + qp) % 3]] = v
            blocks.append(b)
            qps.append(qp)
    return np.stack(blocks), np.asarray(qps, np.uint8)


def mixed_item(lw, lh, qps, bd, iqt, tr=(0, 0), start=0):
    """Work items of G blocks in a cycle of four: dense_signed and single blocks alternating - the single level of every other one in a (row pair, column pair) that no
    neighbour leaves empty, of the rest in the last pairs, where for the sparse neighbours of the next kind nothing lies; all dense; all near-empty (one, three or six
    levels each, in pairs that differ from block to block); all zero but one block.  What a wave's union of masks lets a TB read beyond its own mask, and what an earlier workgroup left
    in LDS, must not reach the result."""
    w, h = 1 << lw, 1 << lh
    g = itdq_group(lw, lh)
    sub = None if (iqt or tr != (0, 0)) else "defined"
    out = np.zeros((len(qps), h, w), np.int16)
    for b, qp in enumerate(qps):
        k = b + start
        item, p = (k // g) % 4, k % g
        one = np.zeros((h, w), np.int16)
        if item == 0 and p % 2 == 0 or item == 1:
            out[b] = dense_signed(lw, lh, [qp], bd, iqt, tr, sub=sub, start=k)[0]
            continue
        if item == 0:
            y, x = (h - 1, w - 1) if p % 4 == 1 else ((k * 2) % h, (k * 6) % w)
        elif item == 2:
            y, x = (2 * p + k // g) % h, (2 * (g - p) + 1) % w
            for e in range((0, 2, 5)[p % 3]):                 # every third block one level, the others three and six, each in a row pair and a column pair of its own
                one[(y + 2 * e + 2) % h, (x + 2 * e + 2) % w] = (e + 2) * (-1) ** e
        elif p == (k // (4 * g)) % g:
            y, x = h - 1 - (k // g) % h, (k // g) % w
        else:
            continue
        one[y, x] = (3, -mid_level(lw, lh, int(qp), bd, iqt), 32767, -1)[k % 4]
        out[b] = one
    return out


def blocks(kind, lw, lh, qps, bd, iqt, tr=(0, 0), start=0, sub=None):
    if kind == "single":
        return single(lw, lh, qps, bd, iqt, tr, start)
    if kind == "dense_signed":
        return dense_signed(lw, lh, qps, bd, iqt, tr, sub, start)
    if kind == "thresholds":
        return thresholds(lw, lh, qps, bd, iqt, tr, start)
    if kind == "mixed_item":
        return mixed_item(lw, lh, qps, bd, iqt, tr, start)
    raise ValueError(kind)


def walk_qps(n, bd, start=0):
    """n QPs walking over 0 .. 51 + 6 (bd - 8) in steps coprime to the range"""
    top = qp_top(bd) + 1
    return ((np.arange(n, dtype=np.int64) + start) * 7 + 3) % top


def n_blocks_for(kind, lw, lh):
    """how many blocks let the generator walk through its whole cycle once"""
    g = itdq_group(lw, lh)
    if kind == "single":
        return len(single_positions(lw, lh))
    if kind == "dense_signed":
        return 24
    if kind == "thresholds":
        return 3 * 14
    return 8 * g + 1 if g > 1 else 9


def oracle_blocks(coef, lw, lh, qps, bd, iqt, tr=(0, 0)):
    """coef: (n, H, W) or flat -> the oracle's residuals, same shape (orc_itdq / orc_itdq_ats block by block; bumps the census)"""
    orc = ol.oracle()
    n = 1 << (lw + lh)
    out = np.ascontiguousarray(coef, np.int16).copy()
    flat = out.reshape(-1)
    for i, qp in enumerate(qps):
        p = C.c_void_p(flat.ctypes.data + 2 * i * n)
        if tr == (0, 0):
            orc.orc_itdq(p, lw, lh, int(qp), bd, iqt)
        else:
            orc.orc_itdq_ats(p, lw, lh, int(qp), bd, iqt, tr[0] - 1, tr[1] - 1)
    return out


# ---- picture level: the levels of one TB of a batch (extreme_inputs.set_residual)
def fill_tb(kind, k, lw, lh, qp, bd, iqt, tr, sub):
    """the levels (H x W) of TB number k of a picture, of the block kind `kind`"""
    return blocks(kind, lw, lh, [qp], bd, iqt, tr, start=k, sub=sub)[0]
