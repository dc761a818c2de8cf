"""Adversarial inputs for the picture-level cases (test side only; xevd_amd/synth.py and its draw order stay untouched).

synth.gen_picture keeps every sample in roughly 10 % .. 90 % of the range and cases.build_case draws mild QPs, vectors and ALF
coefficients, so the kernels' packed 16-bit arithmetic, clamps and table tops are never at their limits.  This module makes
  * picture content that sits on the rails or walks through the deblocking thresholds (`content`),
  * batch modifiers: per-CU QP over 0..51, vectors on and around the xevd_mv_clip thresholds, whole-sample vectors on the 8x8 grid,
  * ALF parameters at the largest magnitudes the reference's alf_recon_coef can leave (`alf_params`),
and `apply` puts them into a case that cases.build_case has built (tools={"extreme": {...}}).  What each of them is FOR is asserted
through the oracle's census (oracle_lib.census) in tests/test_oracle_extremes.py.
"""
import numpy as np

import oracle_lib as ol
from xevd_amd.abi import MODE_INTRA

# ALPHA_TABLE / BETA_TABLE of the ADDB filter (the oracle's k_addb_alpha / k_addb_beta, pinned against src_main/xevdm_df.c by
# tests/test_oracle_vs_ref.py); used here only to pick step heights, never to compute an expected value
ALPHA = [0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255]
BETA = [0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18]

CONTENT_KINDS = ("noise", "checker1", "checker2", "checker4", "rows", "cols", "flat0", "flatmax", "rails_dither", "ladder", "gratings",
                 "halves_x", "halves_y")


def _plane(kind, rng, pw, ph, bd, chroma):
    maxv = (1 << bd) - 1
    sc = bd - 8
    yy, xx = np.mgrid[0:ph, 0:pw]
    if kind == "noise":                 # full-range uniform noise
        return rng.integers(0, maxv + 1, (ph, pw))
    if kind.startswith("checker"):      # 0 / max checkerboard of period 1, 2 or 4 samples: the worst case of the 8-tap overshoot
        p = int(kind[7:])
        return (((xx // p) + (yy // p)) & 1) * maxv
    if kind == "rows":
        return (yy & 1) * maxv + 0 * xx
    if kind == "cols":
        return (xx & 1) * maxv + 0 * yy
    if kind == "flat0":
        return np.zeros((ph, pw), np.int64)
    if kind == "flatmax":
        return np.full((ph, pw), maxv, np.int64)
    if kind == "halves_x":              # left half 0, right half max (with halves_y in the other list: every saturated pair of a bi-average)
        return (xx >= pw // 2) * maxv
    if kind == "halves_y":
        return (yy >= ph // 2) * maxv
    if kind == "rails_dither":          # 8x8 blocks at 0 or at max with a dither smaller than the largest beta: the filters stay ON at the rails
        blk = rng.integers(0, 2, ((ph + 7) // 8, (pw + 7) // 8))
        base = np.kron(blk, np.ones((8, 8), np.int64))[:ph, :pw]
        d = rng.integers(0, (12 << sc) + 1, (ph, pw))
        return np.where(base == 1, maxv - d, d)
    if kind == "ladder":
        # A checkerboard of flat blocks (8x8 luma, 4x4 chroma: the deblocking grid) whose steps walk through the thresholds of addb_line_luma / _chroma -
        # alpha(index), (alpha >> 2) + 2, beta(index), each - 1 / + 0 / + 1, scaled by the bit depth - on bases at 0, mid-range and max, plus a ripple of
        # up to beta inside some blocks so the p1 - p0 / p2 - p0 tests fall on both sides as well
        n = 4 if chroma else 8
        heights = []
        for idx in range(16, 52):
            for v in (ALPHA[idx] << sc, ((ALPHA[idx] << sc) >> 2) + 2, BETA[idx] << sc):
                heights += [max(v - 1, 0), v, v + 1]
        heights = np.array(sorted(set(heights)), np.int64)
        bi, bj = yy // n, xx // n
        k = bi * ((pw + n - 1) // n) + bj
        step = heights[(k * 7) % len(heights)] * ((bi + bj) & 1)
        where = (k // 3) % 3                    # base near 0, mid, near max (the step then goes downwards)
        v = np.where(where == 0, step, np.where(where == 1, (maxv + 1) // 2 + step // 2, maxv - step))
        amp = np.array([0, 1, 2 << sc, 5 << sc, 17 << sc])[(k // 5) % 5]
        ripple = rng.integers(0, 1 << 30, (ph, pw)) % (amp + 1)
        return np.clip(np.where(where == 2, v - ripple, v + ripple), 0, maxv)
    if kind == "gratings":
        # 16x16 cells (8x8 chroma) of oriented gratings: direction 0 / 90 / +-45 degrees with weak and strong dominance (a second, weaker grating across the first)
        # x an amplitude ladder from flat to rail-to-rail: the direction x activity grid of the ALF classifier (alf_derive_classification_blk)
        n = 8 if chroma else 16
        ci, cj = yy // n, xx // n
        k = ci * ((pw + n - 1) // n) + cj
        d = k % 4
        period = np.array([2, 3, 4, 6])[(k // 4) % 4]
        mix = np.array([0.0, 0.15, 0.35, 0.6, 1.0])[(k // 16) % 5]         # share of the crossing grating: 0 = one clean direction ... 1 = none dominant
        amp = np.array([0.0, 0.002, 0.004, 0.008, 0.015, 0.03, 0.06, 0.12, 0.25, 0.5])[(k // 80 + k) % 10]
        ph1 = np.stack([xx, yy, xx + yy, xx - yy])
        ph2 = np.stack([yy, xx, xx - yy, xx + yy])
        a = np.take_along_axis(ph1, d[None], 0)[0]
        b = np.take_along_axis(ph2, d[None], 0)[0]
        g = np.sin(2 * np.pi * a / period) + mix * np.sin(2 * np.pi * b / period)
        base = np.array([0.5, 0.5, 0.04, 0.96])[(k // 7) % 4]
        return np.clip(np.round((base + amp * g) * maxv), 0, maxv)
    raise ValueError(kind)


def content(kind, seed, w, h, bd):
    """-> [Y, U, V] int16 planes (4:2:0, active area) of content `kind`, seeded"""
    rng = np.random.default_rng(seed)
    return [_plane(kind, rng, pw, ph, bd, c > 0).astype(np.int16) for c, (pw, ph) in enumerate(((w, h), (w // 2, h // 2), (w // 2, h // 2)))]


def alf_params(kind, seed, n_ctu, enable=(1, 1, 1), ctb="on", across_tiles=0):
    """ALF parameters in the form alf_recon_coef leaves them (src_main/xevdm_alf.c:700-794).  Its asserts are the legal range: every side tap in
    [-512, 511] (:751, :786), the centre tap = 512 - 2 * sum(side taps) in [-1024, 1023] (:761-763, :788-790), so the side taps sum to -255 .. 768.
      extreme   six taps at +511 and six at -512 per class in a class-dependent arrangement (sum -6, centre 524); chroma three and three (centre 518)
      single    one tap per class (another one every class, either sign) at +511 (centre -510) or -255 (centre 1022), the others 0
      smooth    the largest all-positive low-pass: every side tap +64 (sum 768, centre -1024): luma; chroma +128 each
    ctb: 'on' / 'off' / 'checker' CTB flags."""
    rng = np.random.default_rng(seed)
    luma = np.zeros((25, 13), np.int64)
    chroma = np.zeros(7, np.int64)
    if kind == "extreme":
        for c in range(25):
            luma[c, :12] = np.where(rng.permutation(12) < 6, 511, -512)
        chroma[:6] = np.where(rng.permutation(6) < 3, 511, -512)
    elif kind == "single":
        for c in range(25):
            luma[c, (c * 5) % 12] = 511 if c & 1 else -255
        chroma[int(seed) % 6] = -255 if seed & 1 else 511
    elif kind == "smooth":
        luma[:, :12] = 64
        chroma[:6] = 128
    else:
        raise ValueError(kind)
    luma[:, 12] = 512 - 2 * luma[:, :12].sum(1)
    chroma[6] = 512 - 2 * chroma[:6].sum()
    assert luma[:, :12].min() >= -512 and luma[:, :12].max() <= 511 and luma[:, 12].min() >= -1024 and luma[:, 12].max() <= 1023
    assert -1024 <= chroma[6] <= 1023
    flag = {"on": np.ones(n_ctu, np.uint8), "off": np.zeros(n_ctu, np.uint8), "checker": (np.arange(n_ctu) & 1).astype(np.uint8)}[ctb]
    return {"enable": tuple(enable), "luma_coef": luma.astype(np.int16), "chroma_coef": chroma.astype(np.int16), "ctb_flag": flag, "across_tiles": across_tiles}


def set_qp_areas(batch, w, bd, chroma_tbl):
    """Per-CU luma QP over the full 0..51: all CUs that start in the same 16x16 area share one QP (so the edges inside it see exactly that QP - also 0 and 51, which an average of two
    random QPs hardly ever gives), neighbouring areas differ; chroma through the table like synth.gen_frame.  The levels of a coded CU were capped for the QP it
    was drawn with: where the QP rises they are scaled down by the ratio of the two quantiser steps (towards zero), so the residuals stay in the range they had."""
    nx = (w + 15) // 16
    area = (batch["y"].astype(np.int64) >> 4) * nx + (batch["x"].astype(np.int64) >> 4)
    qp_y = (area * 37 + 51) % 52
    qp_c = np.asarray(chroma_tbl, np.int64)[qp_y]
    boff = 6 * (bd - 8)
    old_y = batch["qp"][:, 0].astype(np.int64) - boff
    end = np.append(batch["coef_off"][1:].astype(np.int64), batch["n_coef"])
    size = end - batch["coef_off"].astype(np.int64)
    scale = np.repeat(np.minimum(1.0, 2.0 ** ((old_y - qp_y) / 6.0)), size)
    if batch["n_coef"]:
        batch["coef"][:batch["n_coef"]] = np.trunc(batch["coef"][:batch["n_coef"]] * scale).astype(np.int16)
    batch["qp"] = np.stack([qp_y + boff, qp_c + boff, qp_c + boff], 1).astype(np.uint8)


def set_mv_grid8(batch, seed, w, h):
    """Whole-sample vectors that are multiples of 8 samples and keep the block inside the picture: the reference content arrives on the deblocking grid unfiltered"""
    rng = np.random.default_rng(seed)
    n = len(batch["x"])
    x, y = batch["x"].astype(np.int64), batch["y"].astype(np.int64)
    cw, ch = 1 << batch["log2w"].astype(np.int64), 1 << batch["log2h"].astype(np.int64)
    for lst in range(2):
        dx = rng.integers(-3, 4, n) * 8
        dy = rng.integers(-3, 4, n) * 8
        dx = np.clip(x + dx, 0, np.maximum(w - cw, 0)) // 8 * 8 - x
        dy = np.clip(y + dy, 0, np.maximum(h - ch, 0)) // 8 * 8 - y
        used = batch["refi"][:, lst] >= 0
        batch["mv"][:, lst, 0] = np.where(used, dx * 4, 0)
        batch["mv"][:, lst, 1] = np.where(used, dy * 4, 0)


def set_mv_small(batch, seed, span=9):
    """Vectors of a few quarter samples in all sixteen phases (the block stays where the content is)"""
    rng = np.random.default_rng(seed)
    n = len(batch["x"])
    for lst in range(2):
        v = rng.integers(-span, span + 1, (n, 2))
        batch["mv"][:, lst, :] = np.where((batch["refi"][:, lst] >= 0)[:, None], v, 0)


def set_mv_thresholds(batch, w, h):
    """Vectors exactly on, one quarter sample inside and one outside each threshold of xevd_mv_clip (src_base/xevd_mc.c:435-467: block start below -128 samples,
    block end beyond picture size - 1 + 128 samples, all in quarter samples) and at the s16 limits, for every inter CU in turn; the CUs in the picture's corners
    and on its edges come first in the cycle so each of them gets its own side's thresholds."""
    x, y = batch["x"].astype(np.int64) * 4, batch["y"].astype(np.int64) * 4
    cw, ch = 4 << batch["log2w"].astype(np.int64), 4 << batch["log2h"].astype(np.int64)
    lo_x, lo_y = -512 - x, -512 - y                                       # x + mv == min_x
    hi_x, hi_y = ((w - 1 + 128) << 2) - x - cw + 4, ((h - 1 + 128) << 2) - y - ch + 4     # x + mv + w - 4 == max_x
    inter = np.nonzero((batch["pred_mode"] != MODE_INTRA) & (batch["pred_mode"] != 6))[0]
    aff = batch.get("affine")
    k = 0
    for i in inter:
        if aff is not None and aff[i]:
            continue
        on_l, on_r, on_t, on_b = x[i] == 0, x[i] + cw[i] >= 4 * w, y[i] == 0, y[i] + ch[i] >= 4 * h
        d = (k % 3) - 1
        side = (k // 3) % 6
        vx, vy = int(batch["mv"][i, 0, 0]) % 16, int(batch["mv"][i, 0, 1]) % 16      # a small in-range vector for the other component
        if on_l and not (k & 8):
            side = 0
        elif on_r and not (k & 8):
            side = 1
        if side == 0:
            vx = lo_x[i] + d
        elif side == 1:
            vx = hi_x[i] + d
        elif side == 2:
            vy = lo_y[i] + d
        elif side == 3:
            vy = hi_y[i] + d
        elif side == 4:
            vx, vy = (-32768, 32767) if d < 0 else ((32767, -32768) if d > 0 else (-32768, -32768))
        else:
            vx, vy = (hi_x[i] + d, lo_y[i] - d) if (on_t or on_r) else (lo_x[i] - d, hi_y[i] + d)     # two thresholds at once (corners)
        if on_t and (k & 8):
            vy = lo_y[i] + d
        if on_b and (k & 8):
            vy = hi_y[i] + d
        v = np.clip([vx, vy], -32768, 32767)
        for lst in range(2):
            if batch["refi"][i, lst] >= 0:
                batch["mv"][i, lst] = v if lst == 0 else np.clip([v[0] + d, v[1] - d], -32768, 32767)
        k += 1


def set_dense_levels(batch, level=24, every=2):
    """Every `every`-th coded CU of at most 32x32 gets ALL its coefficients at +level (the top of the stress level range, |level| <= 24).  Every DCT basis
    function is positive at sample 0, so with a high QP the dequantised block saturates at 32767 (the s16 clip of the dequantiser), the first transform stage
    saturates its s16 clip and the residual in the block's corner reaches 32767 at 10 and 12 bit: prediction + residual then exceeds s16 and WRAPS
    (xevd_recon's s16 sum, src_base/xevd_recon.c:39,60) to a negative value that clips to 0, where a saturating sum would give the maximum.  Meant for IQT
    sequences: the Baseline transform's second stage multiplies in 32-bit int and is undefined on such blocks (tests/test_oracle_vs_ref.py, test_itdq_all_sizes)."""
    end = np.append(batch["coef_off"][1:].astype(np.int64), batch["n_coef"])
    ok = np.nonzero((batch["cbf"] != 0) & (batch["log2w"] <= 5) & (batch["log2h"] <= 5))[0][::every]
    for i in ok:
        batch["coef"][int(batch["coef_off"][i]):int(end[i])] = level


PER_CU = ("x", "y", "log2w", "log2h", "pred_mode", "refi", "mv", "qp", "cbf", "coef_off", "ipm", "ats", "ats_inter", "affine", "affine_mv", "dmvr", "tree", "cbf_sub")


def set_tiles(case, col_bd, row_bd, across):
    """Give a CTU-64 case a tile grid (xgpu_tile_grid: borders in CTUs): the CUs are re-ordered tile by tile - tiles in raster order, CTUs in raster order inside a
    tile, as include/xevd_hip.h asks of a batch with tiles -, ctu_cu_start follows that order, and batch and ALF parameters both carry the grid."""
    assert case["log2_ctu"] == 6
    b = case["batch"]
    w_ctu, h_ctu = (case["w"] + 63) // 64, (case["h"] + 63) // 64
    assert col_bd[0] == 0 and col_bd[-1] == w_ctu and row_bd[0] == 0 and row_bd[-1] == h_ctu
    cx, cy = b["x"].astype(np.int64) >> 6, b["y"].astype(np.int64) >> 6
    tile = (np.searchsorted(row_bd, cy, "right") - 1) * (len(col_bd) - 1) + np.searchsorted(col_bd, cx, "right") - 1
    perm = np.argsort(tile, kind="stable")
    n = len(cx)
    for k in PER_CU:
        if b.get(k) is not None:
            b[k] = np.ascontiguousarray(np.asarray(b[k])[perm])
            assert len(b[k]) == n
    ctu = (cy * w_ctu + cx)[perm]
    first = np.concatenate([[0], np.nonzero(np.diff(ctu))[0] + 1, [n]])
    assert len(first) == w_ctu * h_ctu + 1, "every CTU holds a CU"
    b["ctu_cu_start"] = first.astype(np.uint32)
    grid = {"col_bd": list(col_bd), "row_bd": list(row_bd), "across": int(across)}
    b["tiles"] = grid
    if case.get("alf_params") is not None:
        case["alf_params"]["tiles"] = grid
        case["alf_params"]["across_tiles"] = int(across)


def apply(case, spec, seed=0):
    """spec: {'content': kind | [kind per reference picture], 'start': kind, 'qp': 'areas', 'mv': 'grid8' | 'small' | 'thresholds',
              'alf': (kind, ctb), 'levels': 'dense', 'tiles': (col_bd, row_bd, across) }"""
    w, h, bd = case["w"], case["h"], case["bd"]
    base = 7919 * (seed + 1)
    kinds = spec.get("content")
    if kinds is not None:
        done = {}
        for n, (key, pic) in enumerate(sorted(case["refs"].items())):
            if id(pic) in done:
                continue
            kind = kinds if isinstance(kinds, str) else kinds[n % len(kinds)]
            new = ol.Picture(w, h, pic.poc, content(kind, base + n, w, h, bd))
            new.pad_numpy()
            done[id(pic)] = new
        case["refs"] = {key: done[id(pic)] for key, pic in case["refs"].items()}
    if spec.get("start") is not None:
        case["start"] = content(spec["start"], base + 100, w, h, bd)
    b = case["batch"]
    if spec.get("qp") == "areas":
        from xevd_amd import synth
        set_qp_areas(b, w, bd, synth.DEFAULT_CHROMA_QP_BASE)
    if spec.get("mv") == "grid8":
        set_mv_grid8(b, base + 200, w, h)
    elif spec.get("mv") == "small":
        set_mv_small(b, base + 200)
    elif spec.get("mv") == "thresholds":
        set_mv_thresholds(b, w, h)
    if spec.get("levels") == "dense":
        set_dense_levels(b)
    if spec.get("alf") is not None and case.get("alf_params") is not None:
        kind, ctb = spec["alf"]
        old = case["alf_params"]
        case["alf_params"] = alf_params(kind, base + 300, len(old["ctb_flag"]), enable=old["enable"], ctb=ctb, across_tiles=old["across_tiles"])
    if spec.get("tiles") is not None:
        set_tiles(case, *spec["tiles"])
    return case


# ---- the extreme cases: cases.build_case arguments (name, w, h, bd, admvp, iqt, n_refs, bi_frac, tools) + the census requirements they exist for
# (tests/test_oracle_extremes.py: REQUIRE).  Residuals: "amp": 40.0 is the level range of test_gpu_parity's stress_levels cases, the range on which the
# reference's normative C path is compared.
_ADDB = {"addb": 1, "inter_frac": 0.7, "qp_range": (0, 51), "coded_frac": 0.5, "split_prob": 0.6}
_X_LADDER = {"content": ["ladder", "noise", "rails_dither", "ladder"], "qp": "areas", "mv": "grid8"}
EXTREME_CASES = [
    # ADDB: QP 0..51 x slice offsets; step ladder / full-range noise / rails; with ALF behind the filter (k_addb_alf) and without (k_addb)
    ("x_addb_ladder_10b", 264, 200, 10, 1, 1, (2, 2), 0.5, dict(_ADDB, alf=1, split_prob=0.85, extreme=dict(_X_LADDER, alf=("extreme", "on"))), ("addb_idx_luma", "addb_chroma_rows", "addb_branches", "addb_out_clip")),
    ("x_addb_ladder_m12_p12_10b", 264, 200, 10, 1, 1, (2, 2), 0.5, dict(_ADDB, alpha_off=-12, beta_off=12, extreme=_X_LADDER), ("addb_idx_top", "addb_branches", "addb_out_clip")),
    ("x_addb_noise_p12_m12_8b", 200, 136, 8, 1, 1, (2, 2), 0.5, dict(_ADDB, alf=1, alpha_off=12, beta_off=-12, extreme=dict(_X_LADDER, content=["noise", "rails_dither"])), ("addb_idx_top", "addb_chroma_top_rows", "addb_branches")),
    ("x_addb_ladder_p6_m6_8b", 264, 200, 8, 1, 0, (2, 2), 0.5, dict(_ADDB, alpha_off=6, beta_off=-6, extreme=_X_LADDER), ("addb_out_clip",)),
    ("x_addb_ladder_m12_p12_12b", 264, 200, 12, 1, 1, (2, 2), 0.5, dict(_ADDB, alf=1, alpha_off=-12, beta_off=12, extreme=dict(_X_LADDER, alf=("single", "checker"))), ("addb_idx_top", "addb_branches", "addb_lost12")),
    ("x_addb_noise_12b", 264, 200, 12, 1, 1, (2, 2), 0.5, dict(_ADDB, split_prob=0.85, extreme=dict(_X_LADDER, content=["rails_dither", "noise"])), ("addb_idx_luma", "addb_out_clip", "addb_lost12")),
    ("x_addb_ladder_m6_p6_ctu128_10b", 264, 200, 10, 1, 1, (1, 1), 0.5, dict(_ADDB, alf=1, log2_ctu=7, alpha_off=-6, beta_off=6, btt_frac=0.5, extreme=dict(_X_LADDER, alf=("smooth", "on"))), ("addb_idx_top",)),
    ("x_addb_halves_12b", 200, 136, 12, 1, 1, (1, 1), 1.0, dict(_ADDB, inter_frac=1.0, coded_frac=0.3, alpha_off=6, beta_off=6, extreme={"content": ["halves_x", "halves_y"], "mv": "small"}), ("addb_lost12",)),
    # ALF: coefficient magnitudes at the legal limit x gratings (the classifier's direction x activity grid) / noise / checker; CTU 64 and 128; flag kinds
    ("x_alf_gratings_10b", 264, 200, 10, 1, 1, (1, 1), 0.3, {"alf": 1, "addb": 1, "inter_frac": 1.0, "coded_frac": 0.0, "extreme": {"content": "gratings", "mv": "grid8", "alf": ("extreme", "on")}}, ("alf_classes", "alf_clip")),
    ("x_alf_gratings_8b_ctu128", 264, 200, 8, 1, 1, (1, 0), 0.0, {"alf": 1, "no_deblock": 1, "log2_ctu": 7, "inter_frac": 1.0, "coded_frac": 0.0, "extreme": {"content": "gratings", "mv": "grid8", "alf": ("single", "on")}}, ("alf_classes", "alf_clip")),
    ("x_alf_gratings_12b", 264, 200, 12, 1, 1, (1, 1), 0.3, {"alf": 1, "addb": 1, "inter_frac": 1.0, "coded_frac": 0.0, "extreme": {"content": "gratings", "mv": "grid8", "alf": ("extreme", "checker")}}, ("alf_classes", "alf_clip")),
    ("x_alf_noise_smooth_10b", 200, 136, 10, 1, 1, (1, 1), 0.3, {"alf": 1, "addb": 1, "inter_frac": 0.8, "extreme": {"content": "noise", "mv": "small", "alf": ("smooth", "on")}}, ("alf_clip",)),
    ("x_alf_checker_luma_only_8b", 136, 136, 8, 1, 1, (1, 0), 0.0, {"alf": 1, "alf_enable": (1, 0, 0), "no_deblock": 1, "inter_frac": 1.0, "extreme": {"content": "checker2", "mv": "small", "alf": ("extreme", "on")}}, ()),
    ("x_alf_checker_chroma_only_10b", 136, 136, 10, 1, 1, (1, 0), 0.0, {"alf": 1, "alf_enable": (0, 1, 1), "addb": 1, "inter_frac": 1.0, "extreme": {"content": "checker1", "mv": "small", "alf": ("extreme", "on")}}, ()),
    ("x_alf_noise_flags_off_12b", 136, 72, 12, 1, 1, (1, 0), 0.0, {"alf": 1, "addb": 1, "inter_frac": 1.0, "extreme": {"content": "noise", "mv": "small", "alf": ("extreme", "off")}}, ()),
    # interpolation: 0 / max checkerboards and stripes in all phases (the overshoot of the 8-tap / 4-tap filters, both rails of the final clip), bi-averages of rails
    ("x_mc_checker1_main_b_10b", 200, 136, 10, 1, 1, (2, 2), 0.5, {"addb": 1, "alf": 1, "inter_frac": 1.0, "split_prob": 0.2, "extreme": {"content": ["checker1", "checker2", "rows", "cols"], "mv": "small"}}, ("mc_clip",)),
    ("x_mc_checker2_base_b_8b", 200, 136, 8, 0, 0, (2, 2), 0.5, {"inter_frac": 1.0, "split_prob": 0.8, "extreme": {"content": ["checker2", "checker1", "checker4"], "mv": "small"}}, ("mc_clip",)),
    ("x_mc_checker4_main_p_12b", 200, 136, 12, 1, 1, (2, 0), 0.0, {"addb": 1, "inter_frac": 1.0, "extreme": {"content": ["checker4", "checker1"], "mv": "small"}}, ("mc_clip",)),
    ("x_mc_noise_base_p_12b", 136, 72, 12, 0, 0, (1, 0), 0.0, {"inter_frac": 1.0, "extreme": {"content": "noise"}}, ("mc_clip",)),
    ("x_bi_rails_10b", 200, 136, 10, 1, 1, (1, 1), 1.0, {"addb": 1, "inter_frac": 1.0, "coded_frac": 0.3, "extreme": {"content": ["halves_x", "halves_y"], "mv": "small"}}, ("mc_bi_rails",)),
    ("x_bi_flat_8b", 136, 72, 8, 0, 0, (2, 2), 0.7, {"inter_frac": 1.0, "extreme": {"content": ["flat0", "flatmax", "flatmax", "flat0"]}}, ("mc_bi_rails",)),
    # vectors on / around the xevd_mv_clip thresholds and at the s16 limits
    ("x_mv_thresholds_8b", 136, 72, 8, 0, 0, (1, 1), 0.4, {"inter_frac": 1.0, "split_prob": 0.7, "extreme": {"content": "noise", "mv": "thresholds"}}, ("mv_clip",)),
    ("x_mv_thresholds_main_10b", 200, 136, 10, 1, 1, (2, 2), 0.5, {"addb": 1, "inter_frac": 1.0, "extreme": {"content": ["noise", "checker2"], "mv": "thresholds"}}, ("mv_clip",)),
    # residuals that drive the reconstruction into both rails; x_recon_wrap_*: and the 16-bit sum over its top (set_dense_levels; IQT sequences, 10 and 12 bit - at 8 bit
    # the second stage's shift of 12 keeps a block of at most 32x32 coefficients below 32767 - 255, and 64-point blocks carry coefficients in their first 32
    # positions only, see synth.gen_frame)
    ("x_recon_wrap_10b", 136, 136, 10, 1, 1, (1, 1), 0.4, {"addb": 1, "alf": 1, "amp": 40.0, "qp_range": (40, 51), "coded_frac": 0.9, "split_prob": 0.35, "extreme": {"content": "noise", "levels": "dense"}}, ("recon_wrap", "recon_rails")),
    ("x_recon_wrap_12b", 136, 136, 12, 1, 1, (1, 1), 0.4, {"addb": 1, "amp": 40.0, "qp_range": (40, 51), "coded_frac": 0.9, "split_prob": 0.35, "extreme": {"content": "noise", "levels": "dense"}}, ("recon_wrap", "recon_rails")),
    ("x_recon_rails_10b", 200, 136, 10, 1, 1, (2, 2), 0.5, {"addb": 1, "alf": 1, "amp": 40.0, "coded_frac": 0.9, "extreme": {"content": ["noise", "rails_dither"], "mv": "small"}}, ("recon_rails",)),
    ("x_recon_rails_base_8b", 136, 72, 8, 0, 0, (1, 1), 0.4, {"amp": 40.0, "coded_frac": 0.9, "extreme": {"content": "rails_dither"}}, ("recon_rails",)),
    ("x_recon_rails_12b", 136, 136, 12, 1, 1, (1, 1), 0.4, {"addb": 1, "amp": 40.0, "qp_range": (40, 51), "coded_frac": 0.9, "extreme": {"content": "noise"}}, ("recon_rails",)),
    # intra prediction from neighbours at the rails (all-intra, EIPD, + HTDF + IBC), DMVR and affine / EIF on saturated windows
    ("x_intra_eipd_rails_8b", 200, 136, 8, 1, 1, (1, 0), 0.0, {"inter_frac": 0.0, "eipd": 1, "addb": 1, "amp": 40.0, "coded_frac": 0.9, "btt_frac": 0.5}, ("recon_rails",)),
    ("x_intra_eipd_htdf_ibc_10b", 200, 136, 10, 1, 1, (1, 0), 0.0, {"inter_frac": 0.0, "eipd": 1, "addb": 1, "alf": 1, "htdf_qp": 30, "ibc_frac": 0.3, "amp": 40.0, "coded_frac": 0.9, "extreme": {"alf": ("extreme", "on")}}, ("recon_rails",)),
    ("x_intra_base_rails_12b", 136, 120, 12, 0, 0, (1, 0), 0.0, {"inter_frac": 0.0, "amp": 40.0, "coded_frac": 0.9}, ("recon_rails",)),
    ("x_dmvr_checker_10b", 200, 136, 10, 1, 1, (2, 2), 0.9, {"addb": 1, "inter_frac": 1.0, "dmvr_frac": 0.9, "split_prob": 0.3, "oob_frac": 0.0, "extreme": {"content": ["checker2", "noise", "checker4", "rails_dither"]}}, ()),
    ("x_dmvr_noise_8b", 200, 136, 8, 1, 1, (2, 2), 0.9, {"addb": 1, "alf": 1, "inter_frac": 1.0, "dmvr_frac": 0.9, "split_prob": 0.3, "oob_frac": 0.0, "extreme": {"content": "noise"}}, ()),
    ("x_affine_checker_10b", 200, 136, 10, 1, 1, (2, 2), 0.5, {"addb": 1, "inter_frac": 1.0, "affine_frac": 0.9, "split_prob": 0.3, "extreme": {"content": ["checker1", "noise", "checker2"]}}, ()),
    ("x_affine_noise_12b", 200, 136, 12, 1, 1, (1, 1), 0.5, {"addb": 1, "alf": 1, "inter_frac": 1.0, "affine_frac": 0.9, "split_prob": 0.3, "extreme": {"content": "noise"}}, ()),
]

# ---- tile grids inside interior filter areas: pictures of at least 264x264, ADDB + ALF, CTU 64, uneven 2x2 and 3x2 grids - the CTU-aligned tile
# borders cross the 64x64 areas k_addb_alf filters through its interior path -, loop_filter_across_tiles 0 and 1, rail-to-rail content so that a border edge filtered
# by mistake changes samples.  The reference harness drives the deblocking functions without a tile map, so these are held to the oracle only; the oracle's tile handling
# is pinned by the tiled golden streams the reference decoder produced (stream_main_tiles_*, test_stream.py).
_TILES = {"addb": 1, "alf": 1, "inter_frac": 0.8, "qp_range": (30, 51), "coded_frac": 0.5, "split_prob": 0.6}
TILE_CASES = [
    ("xt_2x2_noise_8b", 328, 264, 8, 1, 1, (2, 2), 0.5, dict(_TILES, alpha_off=6, beta_off=6, extreme={"content": ["noise", "rails_dither"], "mv": "small", "alf": ("extreme", "on"), "tiles": ([0, 2, 6], [0, 3, 5], 0)})),
    ("xt_2x2_noise_8b_across", 328, 264, 8, 1, 1, (2, 2), 0.5, dict(_TILES, alpha_off=6, beta_off=6, extreme={"content": ["noise", "rails_dither"], "mv": "small", "alf": ("extreme", "on"), "tiles": ([0, 2, 6], [0, 3, 5], 1)})),
    ("xt_3x2_ladder_10b", 328, 264, 10, 1, 1, (2, 2), 0.5, dict(_TILES, alpha_off=-6, beta_off=12, extreme={"content": ["ladder", "checker2", "noise"], "qp": "areas", "mv": "grid8", "alf": ("single", "checker"), "tiles": ([0, 1, 4, 6], [0, 1, 5], 0)})),
    ("xt_3x2_ladder_10b_across", 328, 264, 10, 1, 1, (2, 2), 0.5, dict(_TILES, alpha_off=-6, beta_off=12, extreme={"content": ["ladder", "checker2", "noise"], "qp": "areas", "mv": "grid8", "alf": ("single", "checker"), "tiles": ([0, 1, 4, 6], [0, 1, 5], 1)})),
    ("xt_3x2_rails_12b", 264, 264, 12, 1, 1, (1, 1), 0.5, dict(_TILES, extreme={"content": "rails_dither", "mv": "small", "alf": ("smooth", "on"), "tiles": ([0, 2, 3, 5], [0, 2, 5], 0)})),
]
