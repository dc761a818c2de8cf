"""The extreme cases (tests/extreme_inputs.py: rail-to-rail content, QP 0..51 x slice offsets, vectors on the MV-clip thresholds, ALF coefficients at their legal
limits, every branch of the DMVR search, of the affine model, of the Hadamard-domain filter and of intra block copy) through the CPU oracle and the REAL reference (oracle/_ref), plus the census: every case asserts that the oracle took the branches it exists for.

The comparison is the one of test_picture_level_oracle_equals_reference: residual arena, pre-deblock planes, maps, final padded planes, against the reference's
normative C path (simd=0) only - its SIMD kernels are known to diverge on out-of-range input (the level-cap comment in synth.gen_frame) and the
residual cases here use the stress level range ("amp": 40).  tests/test_gpu_extremes.py then holds the HIP backend to the oracle on the same cases.

REQUIRE is a condition, not a measurement: it is written out below and was met by choosing inputs on the CPU.  Buckets left out, with the reason:
  * addb_lost[1], addb_lost[2] (c1 / c0 losing bits to the u8 cast): unreachable.  CLIP_TAB's largest entry is 25, so at 12 bit c1 = 25 << 3 = 200,
    luma c0 = 200 + (2 << 3) = 216 and chroma c0 = 26 << 3 = 208 all fit 8 bits; only beta (BETA_TABLE >= 16, i.e. indexB >= 46, << 4) wraps.  Asserted to be 0.
  * mc_stage1_wrap (first-stage sum of the 2-D interpolation not fitting its s16 store): unreachable.  The taps of every phase sum to at most 112 in
    magnitude (Main, phase 8) and the stage-1 shift is bd - 8, so |sum >> shift| <= 112 * 255 = 28560 < 32768 at every bit depth.  Asserted to be 0.
The wrapping 16-bit reconstruction sum is reached at 10 and 12 bit (x_recon_wrap_*: dense blocks of level 24 at high QP saturate the dequantiser and the first
transform stage); at 8 bit it stays with the block-level tests (see the comment at the cases).

DMVR (xi.DMVR_CASES: planted displacements - dmvr_pair -, mirrored / zero vectors, vectors on the clip thresholds, partitions with every sub-block shape).  The census
over these cases together, as test_dmvr_cases_together_reach_every_branch prints it (refined sub-blocks, or events):
  shapes 8x8 / 8x16 / 16x8 / 16x16 (w x h)           247 / 436 / 577 / 453      (8 bit 62 / 89 / 243 / 175, 10 bit 114 / 253 / 174 / 203, 12 bit 71 / 94 / 160 / 75)
  flagged CUs with references not POC-symmetric      25
  search ended: early / centre in round 0 / cost 0 after round 0's move / centre in round 1 / moved twice     223 / 178 / 29 / 659 / 624
  winner below, above, right, left, diagonal         round 0: 200, 221, 211, 223, 457     round 1: 105, 119, 130, 136, 134
  diagonal tried in quadrant ++ / -+ / +- / --       730 / 704 / 719 / 620
  ties right == left / below == above                118 / 108
  sub-sample step -8 .. 8, denominator 0             x: 32 17 24 29 24 35 51 53 256 63 48 41 42 26 19 20 14, 43     y: 23 12 23 30 32 32 46 74 273 72 59 35 24 23 19 13 11, 36
  whole-sample displacement, rows y = -2 .. 2        3 33 40 41 5 / 36 87 132 88 17 / 65 119 401 114 57 / 30 95 108 63 52 / 6 34 43 33 11
  starting vector moved by mv_clip, l / r / t / b    39 / 15 / 34 / 15
  refined vector clipped at its sub-block            38 / 44 / 34 / 36
  refined position from the start window, luma -2 .. 2: 712 1485 2910 1241 504; chroma -1 .. 1: 1632 4174 1046; luma +-3, chroma +-2, further: 0
  regimes copy / vertical / horizontal / 2-D         bilinear 896 220 184 458, luma 1143 478 463 1342, chroma 534 507 484 1901
Buckets asserted to be 0, with the reason:
  * dmvr_not_refined[1] (the identical-motion exit of xevdm_mc's DMVR branch): it asks for poc0 == poc1, the refinement for references on opposite sides of the picture.
  * dmvr_win_off at +-3 luma, +-2 chroma and further (the only offsets for which k_dmvr leaves its packed prediction for the scalar one): the search moves at most
    2 samples = 32 sixteenths, and the sub-sample step of at most 8 exists only when the last round's centre won, i.e. after at most one move: 24.  floor((a + t) / 16) -
    floor(a / 16) is at most 2 for |t| <= 32, and at most 1 with 32 in place of 16.  The clip at the sub-block moves the vector back towards the starting one (which
    passed the same test for the whole CU), never further.  XEVD_HIP_DMVR_SCALAR therefore exists: tests/test_gpu_extremes.py runs the scalar form with it.
dmvr_sub_clip was expected to be unreachable too - a sub-block on a threshold lies wholly in the replicated border, where the costs along that axis are equal - and the
census refuted it: that holds when BOTH lists are on the threshold.  With one list there and the other inside the picture the costs differ along the axis, the search
moves, and the list on the threshold is pushed past it (x_dmvr_thresholds_*: 'dmvr_sub_clip' is a required bucket, and the oracle with a clip that does nothing decodes
those two cases differently).

Affine (xi.AFFINE_CASES: control points solved from target deltas - set_affine -, CTU 128 with every CU shape of 8 .. 128 a side on both paths - affine_partition makes all 25,
none is left out -, and xi.AFFINE_FAR_CASES: 4160 samples along one axis).  The census over the ten cases together, as test_affine_cases_together_reach_every_branch prints it
(936 affine CUs, 1432 list uses):
  CUs on the EIF / the translation path              574 / 362, every shape on both (128x128: 1 / 3); 8 bit 184 / 110, 10 bit 303 / 180, 12 bit 67 / 92
  control points 2 / 3;  list 0 only, list 1 only, both     200 / 736;  298 / 142 / 496
  wx of 0, 1, 2, 3, 4, above 4 (per list)            232 6 5 7 27 1155;  wy 429 9 27 6 55 906
  sub-block width of 4 .. 128                        518 355 30 11 6 16;  height 372 408 66 27 33 30
  EIF applicable / dv[1] < -one / fetched lines      list 0: 594 / 60 / 140, list 1: 461 / 17 / 38;  list 1 not looked at: 122;  sub-block raised to 8: 255 CUs
  memory band exceeded / kept (EIF list uses)        246 (all with three control points) / 607
  window below min_pic / above max_pic / inside      x 60 / 66 / 120, y 83 / 82 / 81;  spreads 128 .. 2272: 245 99 46 63 39
  samples clamped low, high                          x: picture range 11812, 25460, band 73542, 65888;  y: picture range 26662, 16868, band 2561, 2847
  fractions 0 .. 31 all reached (minimum 7364 samples);  negative whole-sample offsets 358407 / 370920;  final clip Y 44406 / 44321, U 12601 / 12644, V 12455 / 12306
  translation vector clipped l / r / t / b           84 / 63 / 77 / 77, with a fraction that the clip removes 18 / 63 / 22 / 77;  moved by clip18 x / y: 33 / 33
  regimes copy / vertical / horizontal / 2-D         luma 150 108 114 207, chroma 81 121 108 269;  luma whole with chroma half x / y: 56 / 75
  map vectors from control point 0 / 1 / 2 / formula 1432 / 1077 / 652 / 22017;  bottom-left of a two-point CU 216;  components moved by clip18 1506;  sub-block = CU 228
  ATS-inter idx 1 .. 4 x pos                         EIF 36 39, 36 46, 11 15, 16 17;  translation 23 30, 21 27, 10 8, 6 13
  cbf 0 .. 7                                         EIF 94 116 11 123 3 95 13 99;  translation 59 61 12 68 12 68 8 94
  the far cases: EIF range moved by clip18           x min 28, max 44 (4160x72);  y min 30, max 28 (136x4160);  in the ten cases above: 0
Asserted to be 0, with the reason:
  * aff_band_vn[0], the memory band exceeded with TWO control points.  Then dv = (-dh[1], dh[0]), and EIF runs only if dh[0] >= -one and max(dh[0], 0) + |dh[1]| <= 102
    (5 x that <= 512).  The 4x4 bounding box (aff_eif_applicable) spans 5 (dh[0] + 512 + |dh[1]|) <= 3070 along x and 5 (|dh[1]| + dh[0] + 512) <= 3070 along y, i.e. at most
    ((3070 + 511) >> 9) + 2 = 8 samples each way: 64 <= 72.  The band is left only by a zoom or shear along x with a small y part, which takes three control points.
  * aff_range_clip18 in pictures of at most 264 samples: min_pic / max_pic stay below 2^17 / 32 = 4096 samples.  Both ends along both axes are reached by AFFINE_FAR_CASES:
    max_pic passes 2^17 - 1 for x < width - cuw - 3969, min_pic passes -2^17 for x > 3968, and for the clip to decide which sample is fetched a vector of more than 4096 samples
    has to end inside the picture (in the replicated border every vector fetches the same values): CUs at x >= 4096, so 4160 is the smallest multiple of 64.
Mutations of the oracle's affine functions, one at a time, and the cases whose comparison with the reference catches them: profiles/affine_census.txt.  Two of the listed ones
change no output and are caught by none: `<` against `<=` (`>` against `>=`) in the two range branches - on equality the re-anchored window IS centre +- spread, since max_pic -
min_pic = (picture + 255 - CU) x 32 is more than any 2 x spread -, and that is also why the min / max of the re-anchored ends never picks the picture's other end.

HTDF and intra block copy (xi.HTDF_CASES, xi.IBC_CASES, xi.HTDF_TILE_CASES: every CU shape as intra and as filter-only inter node in every decoding order - htdf_partition -, the
slice QPs at both ends of every table's range, block vectors placed on purpose - set_ibc_vectors).  The census over them, the buckets asserted empty with their arguments
(check_htdf_empty), 65 mutations of the oracle's filter, availability and copy - all caught - and the oracle's timing against the parent: profiles/htdf_ibc_census.txt.  The output
clip of the filter was expected to be unreachable and is not: both rails at every bit depth.

Intra prediction (xi.INTRA_CASES, xi.INTRA_TILE_CASES: modes assigned on purpose - set_intra_modes - on htdf_partition's shapes, EIPD in right-to-left and left-to-right orders,
the Baseline predictors in both profiles, all-intra and mixed pictures).  The census over them (ip_*), the buckets asserted empty with their arguments (check_intra_empty), 43
mutations of the oracle's predictors and neighbour builders - all caught but the two clips shown to change nothing - and the oracle's timing against the parent:
profiles/intra_census.txt.  The angular predictor's final clip was expected to be unreachable and is; the bilinear one's upper half was not expected and is reached from 10 bit on.

The residual pass (xi.RESIDUAL_CASES: set_residual puts the four block kinds of tests/residual_inputs.py - single levels, blocks whose terms all add at one output aimed at
each side of each clip, the dequantiser's threshold levels, work items mixing dense and near-empty TBs - on every TB of htdf_partition's shapes, with ATS and ATS-inter TUs in
turn and every QP).  Block level: the same generators through the reference's own dequantiser, transform tables and ATS stages on all 36 classes
(test_residual_blocks_oracle_equals_reference); the blocks beyond the range on which the reference's 32-bit second stage is defined are left out, by the oracle's own
it_s2_undef.  The census over the cases (it_*), what is asserted empty or out of reach and why: profiles/residual_census.txt.  No intermediate reaches 2^27, let alone the
2^28 the kernel's split allows; the hold of the 32-bit dequantiser cannot be told from half its value up to 12 bit.

Translational motion compensation (xi.MC_CASES: nine pictures on mc_partition with lists, vectors, flags and TUs assigned in fixed cycles per role of k_inter - set_mv_mc,
set_mc_coding).  Two censuses: the oracle's mc_* (tap rows, regimes, lists, shapes, edges, TUs) and the launch side of tests/mc_launch.py (roles, window alignments, left-out
chunks, lane predicates under wave ballots), which restates the builder's role rule and is held to the builder's arrays in tests/test_builder.py.  Over the cases together every
cell is reached or asserted 0 with its reason (check_mc_together); totals, what the older cases never reached and both mutation tables: profiles/mc_census.txt.  The
identical-motion test "never true" changes no output - equal POCs are one picture, and the average of a prediction with itself is the prediction -; its two halves are caught.

The census (which needs only the oracle) and the generator checks run everywhere; the comparison against the reference carries the `ref` mark and is skipped
where oracle/_ref is not built, like tests/test_oracle_vs_ref.py.
"""
import ctypes as C

import numpy as np
import pytest

import cases
import extreme_inputs as xi
import mc_launch as ml
import oracle_lib as ol
import residual_inputs as ri

# rows of CLIP_TAB (indexA) that hold the same clip values: the classes a chroma index must be seen in
CLIP_ROW_CLASSES = [range(17, 21), range(21, 23), range(23, 27), range(27, 31), range(31, 33), [33], [34], range(35, 37), [37], range(38, 40)] + [[i] for i in range(40, 52)]


def _all(arr, what):
    arr = np.asarray(arr)
    assert (arr > 0).all(), f"{what}: empty buckets at {np.argwhere(arr == 0).tolist()} in {arr.tolist()}"


def _addb_branches(cen, cs):
    for p, plane in enumerate(("luma", "chroma")):
        _all(cen["addb_gate"][p][1:5], f"ADDB {plane} bS 1..4 x [skipped by the alpha-beta gate, filtered]")
        _all(cen["addb_d0"][p], f"ADDB {plane} d0 [inside +-c0, clipped]")
    _all(cen["addb_bs4"], "ADDB luma bS 4 [p, q side] x [weak, strong]")
    _all(cen["addb_apq"], "ADDB luma bS 1..3 (ap, aq) combinations")


def _addb_chroma_rows(cen, cs):
    for cl in CLIP_ROW_CLASSES[:-2]:      # rows 50 and 51 need a slice offset (the chroma QP table ends at 49 for luma QP 51 + offset 1): addb_chroma_top_rows
        assert cen["addb_index_a"][1][list(cl)].sum() > 0, f"no chroma indexA in CLIP_TAB rows {list(cl)}"


def _addb_chroma_top_rows(cen, cs):
    assert cen["addb_index_a"][1][50] > 0 and cen["addb_index_a"][1][51] > 0, cen["addb_index_a"][1][44:].tolist()


def _addb_idx_top(cen, cs):
    for p in range(2):
        assert cen["addb_index_a"][p][51] > 0 and cen["addb_index_b"][p][51] > 0, "index 51 (a negative offset saturates there, a positive one clips)"
    neg_a, neg_b = cs["alpha_off"] < 0, cs["beta_off"] < 0      # get_index takes the offset as u8: with a negative one EVERY index is 51
    if neg_a:
        assert cen["addb_index_a"][0][:51].sum() == 0
    if neg_b:
        assert cen["addb_index_b"][0][:51].sum() == 0


def _recon_rails(cen, cs):
    # both rails, each in at least 0.5 % of the residual-added samples
    assert min(cen["recon_clip"]) * 200 >= cen["recon_coded"] > 0, (cen["recon_clip"].tolist(), cen["recon_coded"])


def dmvr_refined(cs):
    """mask of the CUs the refinement runs on, from the batch and cases.POCS alone: candidates whose references lie at equal distances on either side"""
    b = cs["batch"]
    d0 = cases.CUR_POC - np.asarray(cases.POCS[0])[np.maximum(b["refi"][:, 0], 0)]
    d1 = cases.CUR_POC - np.asarray(cases.POCS[1])[np.maximum(b["refi"][:, 1], 0)]
    return xi.dmvr_candidates(b) & (d0 * d1 < 0) & (np.abs(d0) == np.abs(d1))


def _dmvr_cu128(cen, cs):
    b = cs["batch"]
    shapes = set(zip(b["log2w"][dmvr_refined(cs)].tolist(), b["log2h"][dmvr_refined(cs)].tolist()))
    assert (7, 7) in shapes and ((7, 3) in shapes or (3, 7) in shapes), sorted(shapes)      # 64 sub-blocks (isx / isy up to 28), and a strip of eight


def _dmvr_win_off(cen, cs):
    _all(cen["dmvr_win_off"][0][1:6], "refined position, luma samples from the starting vector's window, -2 .. 2")
    _all(cen["dmvr_win_off"][1][2:5], "refined position, chroma samples from the starting vector's window, -1 .. 1")


# ---- affine: what the cases of xi.AFFINE_CASES are for (per case: the tags below; all of them together: test_affine_cases_together_reach_every_branch)
def _aff_sizes(cen, cs):
    _all(cen["aff_w"][:, [0, 2, 4, 5]], "affine wx / wy of 0, 2, 4, above 4")      # (1 and 3 take a side of 128 and three control points: asked of the cases together)
    _all(cen["aff_sub"][:, :3], "affine sub-block [width, height] of 4, 8, 16")      # (32 takes a delta of 1, 64 and 128 are the whole CU: asked of the cases together)
    _all(cen["aff_shape"].sum((1, 2)), "affine CUs on [the EIF, the translation] path")


def _aff_applic(cen, cs):
    _all(cen["aff_applic"], "EIF applicability per list examined [list 0, list 1] x [applicable, dv[1] < -one, fetched lines]")
    _all([cen["aff_applic_skipped"], cen["aff_lifted"]], "list 1 not examined after list 0 failed; sub-block raised to 8")


def _aff_band(cen, cs):
    _all(cen["aff_band"], "EIF list uses with the memory band [exceeded, kept]")
    _all(cen["aff_range"], "EIF band [x, y] x [below min_pic, above max_pic, inside]")
    _all(cen["aff_spread"], "EIF band spreads 128, 256, 544, 1120, 2272")


def _aff_clip18(cen, cs):
    _all(cen["aff_sub_clip18"], "translation vector moved by clip18 [x, y]")
    _all([cen["aff_mvf_clip18"]], "map vector moved by clip18")


# ---- HTDF and intra block copy: what the cases of xi.HTDF_CASES / xi.IBC_CASES are for (all of them together: test_htdf_cases_together_reach_every_branch, test_ibc_...)
def htdf_table_of(cs, minus8=False):
    """the table a slice QP selects (xevdm_htdf_filter_block: (qp - 16) >> 3 clamped to 0 .. 4), from the case alone"""
    return min(max((int(cs["batch"]["htdf_slice_qp"]) - (8 if minus8 else 0) - 16) >> 3, 0), 4)


def _htdf_pass(cen, cs):
    t = htdf_table_of(cs)
    assert cen["htdf_pass"][t] > 0 and (cen["htdf_thr_edge"][t] > 0).all(), f"table {t}: pass-throughs {cen['htdf_pass'].tolist()}, a == thr - 1 / a == thr {cen['htdf_thr_edge'].tolist()}"


def _htdf_minus8(cen, cs):
    t, t8 = htdf_table_of(cs), htdf_table_of(cs, True)
    assert t8 != t and cen["htdf_table"][0][t] > 0 and cen["htdf_table"][1][t8] > 0 and (cen["htdf_lut"][t8] > 0).all(), f"one picture, two tables ({t}, {t8}): {cen['htdf_table'].tolist()}"
    assert cen["htdf_table"][0].sum() == cen["htdf_table"][0][t] and cen["htdf_table"][1].sum() == cen["htdf_table"][1][t8]


def _htdf_right(cen, cs):
    assert cen["htdf_avail"][3][1] > 0 and cen["htdf_avail"][8][1] > 0 and cen["htdf_src"][2][0] > 0, "a right-to-left order: right and low-right neighbours reconstructed"


def _ibc_parity(cen, cs):
    bv = cen["ibc_bv"]
    _all(bv[:, [0, 2]], "IBC vector components [x, y] x [negative, positive] x [even, odd]")
    _all(bv[:, 1, 0], "IBC vector components of 0 [x, y]")
    assert bv[:, 1, 1].sum() == 0      # (0 is even)


# ---- intra prediction: what the cases of xi.INTRA_CASES are for (all of them together: test_intra_cases_together_reach_every_branch)
def intra_part_counts(cs):
    """the part counts of the case's intra CUs (none of them is filtered: the slice QP of the filter is 0) -> {shape: parts}"""
    b = cs["batch"]
    assert not b.get("htdf_slice_qp")
    parts = xi.intra_parts(b, cs["eipd"])
    sel = b["pred_mode"] == xi.MODE_INTRA
    return {(1 << int(lw), 1 << int(lh)): int(p) for lw, lh, p in zip(b["log2w"][sel], b["log2h"][sel], parts[sel])}


def _ip_modes(cen, cs):
    _all(cen["ip_mode_lr"][:, 1], "every EIPD luma mode with only the left column")
    _all(cen["ip_mode_aspect"], "EIPD luma mode x [wide, square, tall]")
    _all(cen["ip_dm_luma"], "chroma DM resolved to every luma mode")
    _all(cen["ip_cmode_lr"].sum(1), "chroma modes 0 .. 4")


def _ip_right(cen, cs):
    _all(cen["ip_nbr"][0][2][:, 0], "units of the right column read from the picture [luma, chroma]")
    _all(cen["ip_mode_lr"].sum(0), "EIPD CUs with avail_lr 0, 1, 2, 3")
    _all(cen["ip_hor"], "mode 24 from the left column, from the right one, between the two")
    _all(cen["ip_bi_form"], "bilinear: left column, mirrored, both columns")
    _all(cen["ip_bi_corner"][1], "mirrored bilinear on [square, not square: wc_tbl] CUs")
    _all(cen["ip_plan"].sum((1, 2)), "planar [left form, mirrored]")
    _all(cen["ip_dc"].sum(1), "DC over [w + h, w + 2h] samples")
    _all(cen["ip_ang_src"][:, 2], "angular samples of modes [< 12, 13 .. 23, > 24] read from the right column")
    _all([cen["ip_ang_src"][2][0]], "angular samples of modes > 24 read from the row above (only with a right column)")


def _ip_left_only(cen, cs):
    assert cen["ip_nbr"][0][2][:, 0].sum() == 0 and cen["ip_mode_lr"][:, 2:].sum() == 0, "a left-to-right order: no right column (k_intra's EIPD instantiation without the right-hand forms)"
    _all(cen["ip_mode_lr"][:, 1], "every EIPD luma mode with only the left column")
    _all([cen["ip_mode_lr"][:, 0].sum()], "CUs without either column")


def _ip_base(cen, cs):
    _all(cen["ip_base_mode"], "Baseline modes [luma, chroma] x DC, HOR, VER, UL, UR")
    _all([cen["ip_base_c_differs"]], "Baseline CUs whose chroma mode differs")
    _all(cen["ip_nbr"][1][:2], "Baseline builder [up, left] x [luma, chroma] x [available, unavailable later, unavailable first]")
    _all(cen["ip_corner"][[0, 2]], "corner [available, mid]")
    assert cen["ip_shape"][1].sum() == 0 and cen["ip_nbr"][0].sum() == 0


def _ip_parts_eipd(cen, cs):
    parts = intra_part_counts(cs)
    assert parts[(16, 16)] == 1 and parts[(64, 64)] == 16 and set(parts.values()) >= {1, 2, 4, 8, 16}, parts


def _ip_parts_base(cen, cs):
    parts = intra_part_counts(cs)
    assert parts[(64, 64)] == 4 and set(parts.values()) >= {1, 4} and set(parts.values()) & {8, 16}, parts
    if (128, 128) in parts:
        assert parts[(128, 128)] == 16


def _ip_nocoef(cen, cs):
    assert cen["ip_cbf"][0] == cen["ip_cbf"].sum() > 0 and cen["recon_coded"] == 0 and cs["batch"]["n_coef"] == 0, "no CU carries a coefficient: prediction, then the clip"


def _ip_cip(cen, cs):
    _all([cen["ip_unavail"][3]], "neighbour units refused by constrained intra prediction")
    _all(cen["ip_nbr"][0 if cs["eipd"] else 1][:2, :, 1], "units unavailable behind an available one [up, left] x [luma, chroma]")


def _ip_plan_mirror(cen, cs):
    assert cs["bd"] == 12
    _all([cen["ip_plan"][1].sum()], "planar in its mirrored form, at 12 bit")
    _all(cen["ip_plan_clip"], "planar samples clipped [at 0, at max]")


def intra_shapes(cs, right=None):
    """the shapes (log2w - 2, log2h - 2) of the case's intra CUs that have luma, from the batch; right: only those with (True) / without (False) a reconstructed right column"""
    b = cs["batch"]
    tree = b["tree"] if b.get("tree") is not None else np.zeros(len(b["x"]), np.uint8)
    sel = (b["pred_mode"] == xi.MODE_INTRA) & (tree != 2)
    if right is not None:
        sel &= ((xi.intra_avail_lr(b, cs["w"], cs["h"], cs["log2_ctu"]) & 2) != 0) == right
    return set(zip((b["log2w"][sel].astype(int) - 2).tolist(), (b["log2h"][sel].astype(int) - 2).tolist()))


def _ip_side128(cen, cs):
    """four shapes of HTDF_128, one per whole CTU, each predicted - under EIPD each also by the planar predictor, whose mult[5] / shift[5] only a side of 128 reads"""
    big = {sh for sh in intra_shapes(cs) if 5 in sh}
    assert len(big) == 4 and big <= {(int(np.log2(w_)) - 2, int(np.log2(h_)) - 2) for w_, h_ in xi.HTDF_128}, sorted(big)
    for lw, lh in big:
        assert cen["ip_shape"][cs["eipd"]][lw][lh] > 0 and (not cs["eipd"] or cen["ip_plan"][0][lw][lh] > 0), (lw, lh)


def _ip_clips(cen, cs):
    _all(cen["ip_plan_clip"], "planar samples clipped [at 0, at max]")


def mc_launch_census(cs):
    """the launch side of the motion-compensation census (tests/mc_launch.py), once per built case"""
    if "_mc_launch" not in cs:
        cs["_mc_launch"] = ml.census(cs)
    return cs["_mc_launch"]


def _mcr_roles(cen, cs):
    lc = mc_launch_census(cs)
    _all(lc["role"], "k_inter work units in the [region, tile, split] role")
    _all(lc["role_lists"][:, 2], "CUs predicted from two lists in the [region, tile, split] role")
    _all(lc["role_lists"][:, :2].sum(1), "CUs predicted from one list in the [region, tile, split] role")


def _mcr_windows(cen, cs):
    lc = mc_launch_census(cs)
    for r, role in enumerate(("region", "tile")):      # both arrangements of the horizontal pass (odd = mis & 1), and what wanted() leaves out in every whole / fractional combination
        for key, what in (("win_l", "luma"), ("win_c", "chroma")):
            _all(lc[key][r].sum((1, 2)).reshape(4, 2).sum(0), f"{role} role, {what} windows at an [even, odd] alignment")
            _all(lc[key][r].sum((0, 2)), f"{role} role, {what} windows with x [whole, fractional]")
            _all(lc[key][r].sum((0, 1)), f"{role} role, {what} windows with y [whole, fractional]")


def _mcr_lanes(cen, cs):
    lc = mc_launch_census(cs)
    _all(lc["lane_l"].sum(1), "split-role lanes in luma waves of every [H V] (the nine cells [wave][lane]: the cases together)")
    _all(lc["lane_l"].sum(0), "split-role lanes by their own [fx fy]")
    _all(lc["lane_c"].sum(1), "split-role lanes in chroma waves of every [H V]")
    _all(lc["mixed_wave"], "split-role waves with [several CUs, one- and two-list CUs, lanes without a plain inter CU]")


def _mcr_coding(cen, cs):
    _all(cen["mc_cbf"], "plain inter CUs by cbf 0 .. 7")
    _all([cen["mc_skip"]], "skipped CUs")
    if cs["admvp"] and cs["iqt"]:
        _all(cen["mc_tu"][1:], "plain inter CUs by ATS-inter idx 1 .. 4 x pos")
        lc = mc_launch_census(cs)
        _all(lc["role_tu"][:, 1:].sum(2)[lc["role"] > 0], "... every idx in each role the case has")


def _mcr_second_list(cen, cs):
    sl = mc_launch_census(cs)["second_list"]
    _all(np.stack([sl[:, 0, 0] + sl[:, 1, 1], sl[:, 0, 1] + sl[:, 1, 0]], 1), "[region, tile] units whose two lists have [the same, another] luma fy")


def _mcr_clip(cen, cs):
    lc = mc_launch_census(cs)
    _all(cen["mv_clip"], "vectors moved by the MV clip [left, right, top, bottom]")
    _all(lc["role_clip"].sum(1), "... in the [region, tile, split] role")
    _all(cen["mc_edge"][:, 1], "windows wholly over the picture's [left, right, top, bottom] edge")


def _mcr_edges(cen, cs):
    lc = mc_launch_census(cs)
    _all(cen["mc_edge"][:, 0], "windows partly over the picture's [left, right, top, bottom] edge")
    _all(lc["role_edge"].sum(0), "requests over the picture's [left, right, top, bottom] edge")
    _all(lc["role_edge"].sum(1)[lc["role"] > 0], "... in each role the case has")


REQUIRE = {
    # translational motion compensation in k_inter's roles (xi.MC_CASES; what the cases reach together: test_mc_cases_together_reach_every_branch)
    "mcr_roles": _mcr_roles,
    "mcr_windows": _mcr_windows,
    "mcr_lanes": _mcr_lanes,
    "mcr_coding": _mcr_coding,
    "mcr_second_list": _mcr_second_list,
    "mcr_clip": _mcr_clip,
    "mcr_edges": _mcr_edges,
    "mcr_dmvr_fallback": lambda cen, cs: _all([cen["mc_dmvr_fallback"], cen["dmvr_not_refined"][0]], "DMVR-flagged CUs predicted by the translational path, two-list ones on references that are not POC-symmetric"),
    "mcr_identical": lambda cen, cs: _all(cen["mc_lists"], "plain inter CUs using list 0, list 1, both, both collapsed by identical motion on equal POCs"),
    "mcr_big": lambda cen, cs: _all([cen["mc_shape"][5].sum() + cen["mc_shape"][:, 5].sum()], "plain inter CUs with a side of 128"),
    "mcr_ragged": lambda cen, cs: _all(mc_launch_census(cs)["partial_tile_big"], "tiles cut by the picture's [right, bottom] edge inside a CU of at least 32x32"),
    "ip_modes": _ip_modes,
    "ip_right": _ip_right,
    "ip_left_only": _ip_left_only,
    "ip_base": _ip_base,
    "ip_parts_eipd": _ip_parts_eipd,
    "ip_parts_base": _ip_parts_base,
    "ip_nocoef": _ip_nocoef,
    "ip_cip": _ip_cip,
    "ip_clips": _ip_clips,
    # (c = max + 1 takes max x 1025 / 1024 + 1 / 2 >= max + 1 from wc_tbl's 205 for 1 : 4, max x 1026 / 1024 + 1 / 2 from its 114 for 1 : 8: a depth of 10 bit at least)
    "ip_bi_clip": lambda cen, cs: _all(cen["ip_bi_clip"][1:], "bilinear samples clipped at max"),
    "ip_plan_mirror": _ip_plan_mirror,
    "ip_side128": _ip_side128,
    "ip_ibc": lambda cen, cs: _all([cen["ibc_shape"].sum(), cen["ip_shape"].sum()], "IBC CUs and intra CUs in one picture"),
    "htdf_pass": _htdf_pass,
    "htdf_lut": lambda cen, cs: _all(cen["htdf_lut"][htdf_table_of(cs)], f"HTDF look-ups by index 0 .. 15 in table {htdf_table_of(cs)}"),
    "htdf_neg": lambda cen, cs: _all([cen["htdf_idx_neg"], cen["htdf_table"][1][0]], "square intra CUs of 32 / 64 whose QP - 8 gives a negative index, clamped to table 0"),
    "htdf_minus8": _htdf_minus8,
    "htdf_right": _htdf_right,
    "htdf_rails": lambda cen, cs: _all(cen["htdf_out_clip"], "HTDF output clipped [at 0, at max]"),
    "htdf_skips": lambda cen, cs: _all(cen["htdf_skip"][1:5], "CUs not filtered: area < 64, a side of 128, inter with min >= 32, inter without luma cbf"),
    "htdf_cip_mixed": lambda cen, cs: _all(cen["htdf_side_mixed"], "CUs whose [left, upper, right] side mixes neighbours' samples and units constrained intra refused") or _all(cen["htdf_src"], "border samples [side] x [source]"),
    "htdf_qp17": lambda cen, cs: _all(cen["htdf_skip"][:1], "CUs not filtered because the slice QP is 17") or _all([int(cen["htdf_shape"].sum() == 0)], "and none filtered"),
    "ibc_parity": _ibc_parity,
    "ibc_touch": lambda cen, cs: _all(cen["ibc_touch"], "IBC sources that end at the CU's own [left, top] edge"),
    "ibc_spread": lambda cen, cs: _all(cen["ibc_src_cus"], "IBC sources over 1, 2 .. 4, more CUs") or _all(cen["ibc_region"], "IBC sources in CTU rows above, in CTUs to the left, in the own CTU") or _all(cen["ibc_src_kind"], "IBC sources with intra, IBC, filtered, inter samples"),
    "ibc_chain": lambda cen, cs: _all(cen["ibc_src_kind"][1:3], "IBC sources holding IBC / HTDF-filtered samples") or _all(cen["htdf_nbr"][:2, 1], "filtered CUs with an IBC CU on their left / upper side"),
    "ibc_cip": lambda cen, cs: _all(cen["ibc_nbr_of_cintra"], "intra CUs under constrained intra prediction with an IBC CU along their [left, upper] side"),
    "aff_sizes": _aff_sizes,
    "aff_mvf": lambda cen, cs: _all(list(cen["aff_mvf"]) + [cen["aff_mvf_bl_vn2"], cen["aff_mvf_whole_cu"]], "map vectors from control point 0, 1, 2, the formula; bottom-left of two points; whole CU"),
    "aff_applic": _aff_applic,
    "aff_band": _aff_band,
    "aff_eif_clamp": lambda cen, cs: _all(cen["aff_eif_clamp"], "EIF samples clamped [x, y] x [low, high] x [picture range, band]"),
    "aff_eif_rails": lambda cen, cs: _all(cen["aff_eif_clip"], "EIF output clipped [Y, U, V] x [at 0, at max]"),
    "aff_sub_mvclip": lambda cen, cs: _all(cen["aff_sub_mvclip"], "translation vector clipped [left, right, top, bottom]") or _all(cen["aff_sub_mvclip_frac"], "... with a fraction the clip removes"),
    "aff_sub_regime": lambda cen, cs: _all(cen["aff_sub_regime"], "translation [luma, chroma] x [copy, vertical, horizontal, 2-D]") or _all(cen["aff_sub_luma_whole_chroma_half"], "luma whole, chroma half [x, y]"),
    "aff_clip18": _aff_clip18,
    "dmvr_shape": lambda cen, cs: _all(cen["dmvr_shape"], "DMVR sub-blocks of 8x8, 8x16, 16x8, 16x16"),
    "dmvr_cu128": _dmvr_cu128,
    "dmvr_not_refined": lambda cen, cs: _all(cen["dmvr_not_refined"][:1], "flagged bi-predicted CUs whose references are not POC-symmetric"),
    "dmvr_exit": lambda cen, cs: _all(cen["dmvr_exit"], "DMVR search ends [early, centre in round 0, cost 0 after a move, centre in round 1, moved twice]"),
    "dmvr_exit_zero": lambda cen, cs: _all(cen["dmvr_exit"][2:3], "DMVR searches that found cost 0 with their first move"),
    "dmvr_win": lambda cen, cs: _all(cen["dmvr_win"], "DMVR [round] x winner [below, above, right, left, diagonal]"),
    "dmvr_diag": lambda cen, cs: _all(cen["dmvr_diag"], "DMVR diagonal tried in every quadrant"),
    "dmvr_tie": lambda cen, cs: _all(cen["dmvr_tie"], "DMVR ties right == left, below == above"),
    "dmvr_subpel": lambda cen, cs: _all(cen["dmvr_subpel"][:, 1:16], "DMVR sub-sample quotients -7 .. 7 on [x, y]"),
    "dmvr_subpel_ends": lambda cen, cs: _all(cen["dmvr_subpel"][:, [0, 16, 17]], "DMVR sub-sample steps -8, +8, denominator 0 on [x, y]"),
    # the quotients 1, 2 and 4 are where 16 (a - b) EQUALS the divisor the first, second and third compare of the 3-bit division test it against (xi.DMVR_QUOTIENT_STEPS)
    "dmvr_quotients": lambda cen, cs: _all(cen["dmvr_subpel"][:, [8 + 4, 8 + 2, 8 + 1]], "DMVR sub-sample steps 4, 2, 1 on [x, y]"),
    "dmvr_start_clip": lambda cen, cs: _all(cen["dmvr_start_clip"], "starting vectors of refined CUs moved by the MV clip [left, right, top, bottom]"),
    "dmvr_sub_clip": lambda cen, cs: _all(cen["dmvr_sub_clip"], "refined vectors clipped at the sub-block [left, right, top, bottom]"),
    "dmvr_win_off": _dmvr_win_off,
    "dmvr_regime": lambda cen, cs: _all(cen["dmvr_regime"], "DMVR [bilinear, luma, chroma] x [copy, vertical, horizontal, 2-D]"),
    "addb_idx_luma": lambda cen, cs: _all(cen["addb_index_a"][0], "ADDB luma indexA 0..51") or _all(cen["addb_index_b"][0], "ADDB luma indexB 0..51"),
    "addb_idx_top": _addb_idx_top,
    "addb_chroma_rows": _addb_chroma_rows,
    "addb_chroma_top_rows": _addb_chroma_top_rows,
    "addb_branches": _addb_branches,
    "addb_out_clip": lambda cen, cs: _all(cen["addb_out_clip"], "ADDB p0 + d0 / q0 - d0 clipped [luma, chroma] x [at 0, at max]"),
    "addb_lost12": lambda cen, cs: _all(cen["addb_lost"][:1], "12 bit: beta values that lost bits to & 0xFF"),
    "alf_classes": lambda cen, cs: _all(cen["alf_class"], "ALF classes 0..24") or _all(cen["alf_tr"], "ALF transpositions 0..3"),
    "alf_clip": lambda cen, cs: _all(cen["alf_clip"], "ALF output clipped [Y, U, V] x [at 0, at max]"),
    "mc_clip": lambda cen, cs: _all(cen["mc_clip"], "interpolation clipped [Y, U, V] x [at 0, at max]"),
    "mc_bi_rails": lambda cen, cs: _all(cen["mc_bi"], "bi-averaged samples [Y, U, V]") or _all(cen["mc_bi_rails"], "bi-average of 0 + 0, max + max, 0 + max"),
    # The four sides are counted, not compared: WHERE the threshold lies cannot be seen in the picture.  A block moved by the clip starts 128 samples outside the
    # picture, i.e. it lies wholly in the replicated border, where the column (row) one quarter sample further out interpolates to the same values, and the maps
    # keep the unclipped vector.  An off-by-one threshold therefore changes no output of the reference either; what these cases hold is that vectors on, inside
    # and outside each threshold and at +-32767 / -32768 are decoded like the reference decodes them.
    "mv_clip": lambda cen, cs: _all(cen["mv_clip"], "vectors moved by the MV clip [left, right, top, bottom]"),
    "recon_rails": _recon_rails,
    "recon_wrap": lambda cen, cs: _all([cen["recon_wrap"]], "prediction + residual sums that wrapped in s16"),
    # the residual pass (xi.RESIDUAL_CASES; what the cases reach together: test_residual_cases_together_reach_every_branch)
    "it_s32": lambda cen, cs: _all([cen["it_s1_negfrac"], cen["it_s1_mag"][0], cen["it_s1_mag"][1], cen["it_s1_mag"][2]],
                                   "32-bit intermediates: negative with low bits, magnitude below 2^15 / 2^24 / 2^27"),
    "it_high": lambda cen, cs: _all(cen["it_high"], "levels at positions 32 .. 63 [vertical, horizontal]"),
    "it_final_clip": lambda cen, cs: _all(cen["it_s2_clip"][[cs["iqt"]] + [2] * (cs["batch"].get("ats") is not None and cs["bd"] == 12)],
                                          "final clip [low, high] of the sequence's DCT-II arithmetic, and at 12 bit (where an ATS block from 8 wide reaches it, at 10 bit one of 32 only) of ATS"),
    "it_stage1_clip": lambda cen, cs: _all(cen["it_s1_clip"][0] if cs["batch"].get("ats") is None and cs["batch"].get("ats_inter") is None else cen["it_s1_clip"].reshape(-1),
                                           "stage-1 clip [IQT low, high, ATS low, high]"),
    "it_ats_pairs": lambda cen, cs: _all(cen["it_ats_pair"].reshape(-1), "ATS TBs by type pair"),
    "it_ats_inter": lambda cen, cs: _all(cen["it_ats_inter"].sum(2).reshape(-1), "ATS-inter TUs by [idx - 1][pos]"),
    "it_cmax": lambda cen, cs: _all(cen["it_dq_cmax"][0], "levels at 2^23 >> (qp / 6) and one beyond (even classes)"),
    "it_qp_12b": lambda cen, cs: _all(cen["it_qp"][:76], "TBs by QP 0 .. 75"),
    "it_strided": lambda cen, cs: _all([cen["it_strided"].sum()], "sub-blocks that keep their CU's stride"),
}


def run_oracle_with_census(cs):
    ol.census_reset()
    out = cases.run_cpu("oracle", cs)
    return out, ol.census()


def check_census(spec, cs, cen):
    assert cen["addb_lost"][1] == 0 and cen["addb_lost"][2] == 0 and cen["mc_stage1_wrap"] == 0, "a bucket the module docstring calls unreachable was reached"
    assert cen["dmvr_not_refined"][1] == 0 and cen["dmvr_win_off"][0][[0, 6, 7]].sum() == 0 and cen["dmvr_win_off"][1][[0, 1, 5, 6, 7]].sum() == 0, "a DMVR bucket the module docstring calls unreachable was reached"
    assert cen["aff_band_vn"][0] == 0, "an affine bucket the module docstring calls unreachable was reached"
    check_htdf_empty(cen)
    check_intra_empty(cen)
    for tag in spec[9]:
        REQUIRE[tag](cen, cs)


def check_intra_empty(cen):
    """the intra buckets that must stay empty, each with its argument"""
    # The angular predictor's final clip.  Its taps 32 - o, 64 - o, 32 + o, o with 0 <= o < 32 are non-negative and sum to 128, the references are reconstructed samples or
    # the mid value, all in 0 .. max: the sum lies in 0 .. 128 max, and (128 max + 64) >> 7 = max.  A kernel may drop this clip; the census found no sample that needs it.
    assert cen["ip_ang_clip"].sum() == 0, cen["ip_ang_clip"].tolist()
    # The one-column bilinear predictor below 0.  With all references >= 0, v (2wh) = h ((w - k - 1) col + (k + 1) a) + w ((h - j - 1) up + (j + 1) b) + k j (2c - a - b) + wh
    # >= a ((k + 1) h - k j) + b ((j + 1) w - k j) > 0, because c >= 0, j < h and k < w.  (Above max it IS reached: wc_tbl rounds 1/3, 1/5 and 1/9 up, so c exceeds max
    # where a = b = max.)
    assert cen["ip_bi_clip"][0] == 0
    # modes below 12 lean right: they read the row above or the right column, never the left one (ipred_ang_val's first branch)
    assert cen["ip_ang_src"][0][1] == 0
    # The 4096 / (2^k + 1) table beyond k = 5 and wc_tbl at 5: |log2 w - log2 h| is at most 5 for CUs of 4 .. 128 a side, and 5 takes 4x128 or 128x4.  No stream holds one:
    # a binary cut is allowed only where it leaves a ratio of at most 1 : 4 (ALLOW_SPLIT_RATIO: block_ratio <= BLOCK_14, src_main/xevdm_util.h:110, used by
    # xevdm_check_split_mode, xevdm_util.c:1575-1640), and a ternary cut only across the longer side.  The builder does not check ratios - it takes any power-of-two CU of
    # 4 .. 128 a side inside the picture, 4x128 included (tests/test_builder.py, test_builder_takes_a_cu_of_4x128) -, so these entries are dead for streams, not for
    # batches; the partition tables here end at 1 : 16 (4x64, the worst case of the 16-lane kernel's staging) and do not grow for them.  DC over both columns uses
    # log2 (2h), where 5 is 4x64: reached.
    assert cen["ip_dc"][:, 6:].sum() == 0 and cen["ip_dc"][0][5] == 0 and cen["ip_bi_wc"][[0, 5]].sum() == 0
    # the Baseline builder has no right column
    assert cen["ip_nbr"][1][2].sum() == 0


def check_htdf_empty(cen):
    """the HTDF / IBC buckets that must stay empty, each with its argument from the reference's code"""
    # A low corner flag tests the SCU at row ys + scuh + scuw - 1 of the neighbouring column (xevd_get_avail_intra, xevd_util.c:700-703, :737-740), the sample comes from row
    # ys + scuh (xevdm_htdf, xevdm_recon.c:352-368).  Both SCUs lie in ONE column, the read one above the tested one.  In a split tree two SCUs of one column are only ever
    # parted by a horizontal cut (or a quad split), whose upper part is decoded first - SUCO reverses vertical cuts only - and unparted they are one CU: the tested SCU
    # reconstructed implies the read one reconstructed.  So the filter never reads a sample its owner has yet to write, and the plan's "the reference reads what is there" is
    # no race.  (A batch in an order no tree produces could fill this bucket; the builder takes such batches, tests/test_builder.py, and the cases here hold none.)
    assert cen["htdf_stale_corner"].sum() == 0, cen["htdf_stale_corner"].tolist()
    # table 4 after the - 8: (qp - 8 - 16) >> 3 >= 4 takes a slice QP of 56, the syntax ends at 51
    assert cen["htdf_table"][1][4] == 0
    # availability bits 2 and 4 are not written by xevd_get_avail_intra
    assert cen["htdf_avail"][2][1] == 0 and cen["htdf_avail"][4][1] == 0
    # right / low-left / low-right refused by a tile border alone: tiles are decoded in raster order, so the tile to the right and the tiles below are not reconstructed yet,
    # and the low-left SCU of the tile to the left is only looked at when the left neighbour is available, i.e. in the CU's own tile
    assert cen["htdf_tile_refused"][[2, 5, 6]].sum() == 0, cen["htdf_tile_refused"].tolist()
    assert cen["ibc_bv"][:, 1, 1].sum() == 0      # a component of 0 is even


def test_every_requirement_is_carried_by_a_case():
    import glob
    import os
    import golden_io
    assert {os.path.basename(p)[7:-4] for p in glob.glob(os.path.join(golden_io.GOLDEN, "stream_*tiles*.npz"))} == set(TILED_STREAMS_REACHING_INTERIOR_BORDERS)
    tags = {t for spec in xi.EXTREME_CASES for t in spec[9]}
    assert tags == set(REQUIRE), sorted(set(REQUIRE) ^ tags)
    for bd in (8, 10, 12):      # and at every bit depth: interpolation, reconstruction and ALF clips, the top of the ADDB tables
        for tag in ("mc_clip", "recon_rails", "alf_clip", "addb_idx_top" if bd != 8 else "addb_chroma_top_rows"):
            assert any(spec[3] == bd and tag in spec[9] for spec in xi.EXTREME_CASES), (bd, tag)
        assert any(spec[3] == bd and any(t.startswith("dmvr_") for t in spec[9]) for spec in xi.DMVR_CASES), (bd, "a DMVR tag")
        assert any(spec[3] == bd for spec in xi.HTDF_CASES) and any(spec[3] == bd for spec in xi.IBC_CASES), (bd, "an HTDF and an IBC case")


@pytest.mark.parametrize("spec", xi.EXTREME_CASES, ids=[s[0] for s in xi.EXTREME_CASES])
def test_extreme_case_reaches_its_branches(spec):
    cs = cases.build_case(*spec[:9])
    _, cen = run_oracle_with_census(cs)
    check_census(spec, cs, cen)


@pytest.mark.ref
@pytest.mark.parametrize("spec", xi.EXTREME_CASES, ids=[s[0] for s in xi.EXTREME_CASES])
def test_extreme_case_oracle_equals_reference(spec):
    cs = cases.build_case(*spec[:9])
    a, a_pre, ma, ra = cases.run_cpu("oracle", cs)
    b, b_pre, mb, rb = cases.run_cpu("ref", cs, simd=0)
    assert np.array_equal(ra, rb), "residual arena"
    for c in range(3):
        assert np.array_equal(a_pre.active(c), b_pre.active(c)), f"recon plane {c}: {np.argwhere(a_pre.active(c) != b_pre.active(c))[:4]}"
    assert np.array_equal(ma.map_scu & 0x7FFFFFFF, mb.map_scu & 0x7FFFFFFF)
    assert np.array_equal(ma.map_refi, mb.map_refi) and np.array_equal(ma.map_mv, mb.map_mv)
    for c in range(3):
        assert np.array_equal(a.bufs[c], b.bufs[c]), f"final plane {c}: {np.argwhere(a.bufs[c] != b.bufs[c])[:4]}"


def mc_census_together(specs=None):
    """the oracle's mc_* census and the launch census (tests/mc_launch.py) of the motion-compensation cases, summed: -> (oracle side, launch side, [built case])"""
    arith, launch, built = None, None, []
    for spec in (xi.MC_CASES if specs is None else specs):
        cs = cases.build_case(*spec[:9])
        _, cen = run_oracle_with_census(cs)
        lc = mc_launch_census(cs)
        # the two sides agree on which CUs take this path and from which lists: the restatement of "plain", of the clip and of the identical-motion test holds
        assert lc["n_plain"] == cen["mc_shape"].sum() and np.array_equal(lc["lists"], cen["mc_lists"]), (spec[0], lc["n_plain"], lc["lists"].tolist(), cen["mc_lists"].tolist())
        cen = {k: np.asarray(v) for k, v in cen.items() if k.startswith("mc_") or k in ("mv_clip", "dmvr_not_refined")}
        lc = {k: np.asarray(v) for k, v in lc.items()}
        arith = cen if arith is None else {k: arith[k] + cen[k] for k in cen}
        launch = lc if launch is None else {k: launch[k] + lc[k] for k in lc}
        built.append(cs)
    return arith, launch, built


def check_mc_together(a, lc, built):
    """every cell of the two censuses over xi.MC_CASES: reached, or unreachable - asserted 0, with the reason"""
    for tab in range(2):      # every row of k_luma_taps / k_chroma_taps this path can index, in both tables (the Baseline tables hold a filter for each quarter / eighth sample too)
        _all(a["mc_phase"][tab], f"luma quarter-sample phases [fx][fy], {('Baseline', 'Main')[tab]} table")
        _all(a["mc_cphase"][tab], f"chroma eighth-sample phases [fx][fy], {('Baseline', 'Main')[tab]} table")
    _all(a["mc_regime"], "[luma, chroma] x [copy, vertical, horizontal, 2-D]")
    _all(a["mc_luma_whole_chroma_half"], "luma whole, chroma half [x, y]")
    _all(a["mc_lists"], "list 0 only, list 1 only, both, both collapsed by identical motion")
    # The reference index only selects an entry of the picture table (s_ref[index * 2 + list]): cases.POCS gives a case two pictures in list 0 and three in list 1 -
    # index 2 of list 1 is list 0's index 0, the pair with equal POCs.  The entries beyond hold no picture in these cases.
    _all(a["mc_refi"][0][:2], "list 0 indices 0, 1")
    _all(a["mc_refi"][1][:3], "list 1 indices 0, 1, 2")
    assert a["mc_refi"][0][2:].sum() == 0 and a["mc_refi"][1][3:].sum() == 0
    # 4x128 and 128x4: no split tree makes them (a binary cut is allowed up to a ratio of 1 : 4, a ternary one only across the longer side - check_intra_empty has the
    # lines of the reference), and mc_partition has no such shape
    shape_ok = np.ones((6, 6), bool)
    shape_ok[0, 5] = shape_ok[5, 0] = False
    _all(a["mc_shape"][shape_ok], "plain inter CUs of every shape of 4 .. 128 a side")
    assert a["mc_shape"][~shape_ok].sum() == 0
    _all(a["mc_edge"], "luma windows over the picture's [left, right, top, bottom] edge [partly, wholly]")
    _all(a["mc_tu"][1:], "ATS-inter idx 1 .. 4 x pos")
    # a position without an index: ats_inter_info is idx | pos << 4 and idx 0 means no TU - set_mc_coding writes a position only with an index, as the parser does
    assert a["mc_tu"][0][0] > 0 and a["mc_tu"][0][1] == 0
    _all(a["mc_cbf"], "cbf 0 .. 7")
    _all([a["mc_skip"], a["mc_dmvr_fallback"], a["dmvr_not_refined"][0]], "skipped CUs, DMVR-flagged CUs predicted here, two-list ones on references that are not POC-symmetric")
    _all(a["mv_clip"], "vectors moved by the clip")
    # ---- the launch side
    _all(lc["role"], "units by role")
    _all(lc["role_lists"], "[role] x lists")
    # A region (a tile) lies inside one CU only if the CU is at least 64 (32) a side; mc_partition's CUs of 64 and more a side lie on the 64 grid inside the picture, so
    # they are whole regions and leave nothing to the other roles - but for the CUs of 32x32, 32x64 and 64x32 that a ternary cut puts at an offset of 16 into the ragged
    # edge of x_mcr_edges_main_8b_ragged (split role) - and CUs of 32 a side on the 32 grid are whole tiles
    region_ok, tile_ok, split_ok = np.zeros((6, 6), bool), np.zeros((6, 6), bool), shape_ok.copy()
    region_ok[4:, 4:] = True
    tile_ok[3:, 3:] = True
    tile_ok[4:, 4:] = False
    split_ok[3:, 3:] = False
    split_ok[3, 3] = split_ok[3, 4] = split_ok[4, 3] = True
    for r, ok in enumerate((region_ok, tile_ok, split_ok)):
        _all(lc["role_shape"][r][ok], f"CU shapes of role {r}")
        assert lc["role_shape"][r][~ok].sum() == 0, (r, lc["role_shape"][r].tolist())
    _all(lc["win_l"], "[region, tile] x [mis][fx][fy]")
    _all(lc["win_c"], "[region, tile] x [cmis][cfx][cfy]")
    _all(lc["second_list"], "[region, tile] x [list 0 fy][list 1 fy]")
    # a lane that filters in a direction makes the ballot of its wave true: lane & ~wave != 0 cannot be
    ok = np.array([[(lane & ~wave) == 0 for lane in range(4)] for wave in range(4)])
    _all(lc["lane_l"][ok], "split-role lanes [wave][lane], luma")
    _all(lc["lane_c"][ok], "split-role lanes [wave][lane], chroma")
    assert lc["lane_l"][~ok].sum() == 0 and lc["lane_c"][~ok].sum() == 0
    _all(lc["mixed_wave"], "mixed waves")
    _all(lc["partial_tile"], "tiles cut by the picture's [right, bottom] edge")
    _all(lc["partial_tile_big"], "... inside a CU of at least 32x32")
    _all(lc["role_clip"], "[role] x vectors moved by the clip [left, right, top, bottom]")
    _all(lc["role_edge"], "[role] x requests over the picture's [left, right, top, bottom] edge")
    _all(lc["role_tu"][:, 1:], "[role] x ATS-inter idx 1 .. 4 x pos")
    assert (lc["role_tu"][:, 0, 0] > 0).all() and lc["role_tu"][:, 0, 1].sum() == 0      # (as mc_tu[0][1])
    _all(lc["role_cbf"], "[role] x cbf")
    _all(lc["role_skip"], "[role] skipped CUs")
    # the cycles of the region and tile role go on from case to case where the one before stopped (xi.mc_chain_start)
    at = np.zeros(4, np.int64)
    for spec, cs in zip(xi.MC_CASES, built):
        assert tuple(at) == tuple(cs["mc_at"]), (spec[0], at.tolist(), cs["mc_at"])
        at += cs["mc_taken"]
    assert ml.CUR_POC == cases.CUR_POC
    tools = {(spec[3], spec[4], spec[8].get("log2_ctu", 6)) for spec in xi.MC_CASES}
    assert {t[:2] for t in tools} >= {(bd, tab) for bd in (8, 10, 12) for tab in (0, 1)} and {t[1:] for t in tools} == {(tab, ctu) for tab in (0, 1) for ctu in (6, 7)}
    assert {(spec[8].get("addb", 0), spec[8].get("alf", 0)) for spec in xi.MC_CASES} >= {(0, 0), (1, 0), (1, 1)}
    assert all(spec[1] <= 264 and spec[2] <= 264 and spec[9] for spec in xi.MC_CASES)


def test_mc_cases_together_reach_every_branch():
    """the conditions the motion-compensation cases were chosen for, over all of them (profiles/mc_census.txt holds this test's output)"""
    a, lc, built = mc_census_together()
    for k, v in list(a.items()) + list(lc.items()):
        print(k, np.asarray(v).tolist())
    check_mc_together(a, lc, built)


def dmvr_census_together():
    """the census of the DMVR cases, summed: -> (all, {bit depth: ...}, [(case, refined mask)])"""
    total, by_bd, built = None, {}, []
    for spec in xi.DMVR_CASES:
        cs = cases.build_case(*spec[:9])
        _, cen = run_oracle_with_census(cs)
        cen = {k: np.asarray(v) for k, v in cen.items() if k.startswith("dmvr_")}
        total = cen if total is None else {k: total[k] + cen[k] for k in cen}
        by_bd[spec[3]] = cen if spec[3] not in by_bd else {k: by_bd[spec[3]][k] + cen[k] for k in cen}
        built.append((cs, dmvr_refined(cs)))
    return total, by_bd, built


def test_dmvr_cases_together_reach_every_branch():
    """the conditions the DMVR cases were chosen for, over all of them (the table of the module docstring is this test's output)"""
    total, by_bd, built = dmvr_census_together()
    for k, v in total.items():
        print(k, v.tolist())
    for bd in (8, 10, 12):
        print(bd, "bit shapes", by_bd[bd]["dmvr_shape"].tolist())
        assert (by_bd[bd]["dmvr_shape"] >= 16).all(), (bd, by_bd[bd]["dmvr_shape"].tolist())
    for tag in ("dmvr_exit", "dmvr_win", "dmvr_diag", "dmvr_tie", "dmvr_regime", "dmvr_start_clip", "dmvr_sub_clip", "dmvr_subpel", "dmvr_subpel_ends", "dmvr_win_off", "dmvr_not_refined"):
        REQUIRE[tag](total, None)
    _all(total["dmvr_total"], "DMVR whole-sample displacement [y -2 .. 2][x -2 .. 2]")      # (no single case is asked for all 25)
    assert total["dmvr_not_refined"][1] == 0 and total["dmvr_win_off"][0][[0, 6, 7]].sum() == 0 and total["dmvr_win_off"][1][[0, 1, 5, 6, 7]].sum() == 0
    # from the batches: ATS-inter TUs of every index at both positions, with a luma residual, and every cbf combination inside refined CUs; the strips
    ats, cbf, shapes = set(), set(), set()
    for cs, ref in built:
        b = cs["batch"]
        if b.get("ats_inter") is not None:
            ats |= set(b["ats_inter"][ref & ((b["cbf"] & 1) != 0)].tolist())
        cbf |= set(b["cbf"][ref].tolist())
        shapes |= set(zip((1 << b["log2w"][ref].astype(int)).tolist(), (1 << b["log2h"][ref].astype(int)).tolist()))
    assert ats >= {idx | pos << 4 for idx in (1, 2, 3, 4) for pos in (0, 1)}, sorted(ats)
    assert cbf >= set(range(8)), sorted(cbf)
    assert shapes >= {(16, 8), (32, 8), (64, 8), (8, 16), (8, 32), (8, 64), (128, 128)} and shapes & {(128, 8), (8, 128)}, sorted(shapes)
    assert {(spec[3], spec[8].get("addb", 0)) for spec in xi.DMVR_CASES} >= {(8, 0), (8, 1), (10, 1), (12, 0), (12, 1)}      # every depth; the baseline filter reads refined vectors
    assert any(spec[8].get("alf") for spec in xi.DMVR_CASES) and any(spec[8].get("amp") == 40.0 for spec in xi.DMVR_CASES)


@pytest.mark.ref
@pytest.mark.parametrize("spec", xi.DMVR_CASES, ids=[s[0] for s in xi.DMVR_CASES])
def test_dmvr_case_vectors_oracle_equals_reference(spec):
    cs = cases.build_case(*spec[:9])
    a, b = cases.dmvr_mvs("oracle", cs), cases.dmvr_mvs("ref", cs)
    assert len(a) > 0 and a.shape == b.shape and np.array_equal(a, b), f"refined vectors, first differences at sub-blocks {np.argwhere(a != b)[:4, 0].tolist()}"


def affine_census_together():
    """the census of the affine cases, summed: -> (AFFINE_CASES, AFFINE_FAR_CASES, {bit depth: ... of AFFINE_CASES})"""
    def add(a, b):
        return b if a is None else {k: a[k] + b[k] for k in b}
    near, far, by_bd = None, None, {}
    for spec in xi.AFFINE_CASES + xi.AFFINE_FAR_CASES:
        _, cen = run_oracle_with_census(cases.build_case(*spec[:9]))
        cen = {k: np.asarray(v) for k, v in cen.items() if k.startswith("aff_")}
        if spec in xi.AFFINE_FAR_CASES:
            far = add(far, cen)
        else:
            near, by_bd[spec[3]] = add(near, cen), add(by_bd.get(spec[3]), cen)
    return near, far, by_bd


def test_affine_cases_together_reach_every_branch():
    """the conditions the affine cases were chosen for, over all of them (the table of the module docstring is this test's output)"""
    near, far, by_bd = affine_census_together()
    for k, v in near.items():
        print(k, v.tolist())
    print("far cases: aff_range_clip18", far["aff_range_clip18"].tolist(), "aff_band", far["aff_band"].tolist(), "aff_eif_clamp", far["aff_eif_clamp"].tolist())
    _all(near["aff_shape"], "affine CUs on [EIF, translation] x width 8 .. 128 x height 8 .. 128")      # affine_partition makes every shape: none is left out
    _all(near["aff_vn"], "control points 2, 3")
    _all(near["aff_lists"], "list 0 only, list 1 only, both")
    _all(near["aff_w"], "[wx, wy] of 0, 1, 2, 3, 4, above")
    _all(near["aff_sub"], "sub-block [width, height] of 4 .. 128")
    for tag in ("aff_applic", "aff_band", "aff_eif_clamp", "aff_eif_rails", "aff_sub_mvclip", "aff_sub_regime", "aff_clip18", "aff_mvf"):
        REQUIRE[tag](near, None)
    _all(near["aff_eif_frac"], "EIF fractions [x, y] 0 .. 31")
    _all(near["aff_eif_neg"], "EIF samples with a negative whole-sample offset [x, y]")
    _all(near["aff_ats"], "affine CUs by [path] x ATS-inter idx 1 .. 4 x pos")
    _all(near["aff_cbf"], "affine CUs by [path] x cbf 0 .. 7")
    # clip18 of the EIF range takes a picture of more than 4096 samples along the axis (xi.AFFINE_FAR_CASES), in the others it must not happen
    _all(far["aff_range_clip18"], "EIF range moved by clip18 [x, y] x [min, max]")
    _all(far["aff_band"], "the far cases with the band [exceeded, kept]")
    assert near["aff_range_clip18"].sum() == 0
    # the band is never exceeded with two control points (argument in the module docstring)
    assert near["aff_band_vn"][0] == 0 and far["aff_band_vn"][0] == 0 and near["aff_band_vn"][1] == near["aff_band"][0]
    for bd in (8, 10, 12):      # every depth on the EIF path, band kept and exceeded (at 12 bit the row filter shifts by 1, at 8 and 10 by 0), and on the translation path
        print(bd, "bit: CUs on [EIF, translation]", by_bd[bd]["aff_shape"].sum((1, 2)).tolist(), "band", by_bd[bd]["aff_band"].tolist())
        assert (by_bd[bd]["aff_shape"].sum((1, 2)) >= 16).all() and (by_bd[bd]["aff_band"] >= 16).all() and (by_bd[bd]["aff_eif_clip"] > 0).all()
    tools = [spec[8] for spec in xi.AFFINE_CASES]
    assert {(spec[3], spec[8].get("addb", 0)) for spec in xi.AFFINE_CASES} >= {(8, 0), (8, 1), (10, 0), (10, 1), (12, 0), (12, 1)}      # sub-block vectors feed both deblocking filters
    assert any(t.get("alf") for t in tools) and any(t.get("amp") == 40.0 for t in tools)
    assert all(spec[1] <= 264 and spec[2] <= 264 and spec[9] for spec in xi.AFFINE_CASES) and 8 <= len(xi.AFFINE_CASES) <= 10


def htdf_ibc_census_together():
    """the census of the HTDF, the IBC and the tiled HTDF cases, summed: -> (HTDF_CASES, IBC_CASES, HTDF_TILE_CASES, {bit depth: ... of HTDF_CASES})"""
    def add(a, b):
        return b if a is None else {k: a[k] + b[k] for k in b}
    out, by_bd = [None, None, None], {}
    for n, group in enumerate((xi.HTDF_CASES, xi.IBC_CASES, xi.HTDF_TILE_CASES)):
        for spec in group:
            _, cen = run_oracle_with_census(cases.build_case(*spec[:9]))
            cen = {k: np.asarray(v) for k, v in cen.items() if k.startswith(("htdf_", "ibc_"))}
            check_htdf_empty(cen)
            out[n] = add(out[n], cen)
            if n == 0:
                by_bd[spec[3]] = add(by_bd.get(spec[3]), cen)
    return out[0], out[1], out[2], by_bd


HTDF_SLICE_QPS = (18, 23, 24, 31, 32, 39, 40, 47, 48, 51)      # both ends of the filter's range and of every table's


def test_htdf_cases_together_reach_every_branch():
    """the conditions the HTDF cases were chosen for, over all of them (profiles/htdf_ibc_census.txt holds this test's output)"""
    htdf, ibc, tiled, by_bd = htdf_ibc_census_together()
    for k, v in htdf.items():
        if k.startswith("htdf_"):
            print(k, v.tolist())
    print("tiled case: htdf_tile_refused", tiled["htdf_tile_refused"].tolist(), "htdf_skip", tiled["htdf_skip"].tolist(), "; IBC cases: htdf_skip", ibc["htdf_skip"].tolist(), "htdf_nbr", ibc["htdf_nbr"].tolist())
    filterable = np.array([[(4 << a) * (4 << b) >= 64 for b in range(5)] for a in range(5)])
    narrow = np.array([[min(4 << a, 4 << b) < 32 for b in range(5)] for a in range(5)])
    assert ((htdf["htdf_shape"][0] > 0) == filterable).all(), f"intra CUs of every filterable shape, none of 4x4, 4x8, 8x4: {htdf['htdf_shape'][0].tolist()}"
    assert ((htdf["htdf_shape"][1] > 0) == (filterable & narrow)).all(), f"inter CUs of every filterable shape with min < 32, no other: {htdf['htdf_shape'][1].tolist()}"
    # the 4x4-lane form of the kernel (1024 samples and more) on tall, wide and square blocks, intra; the filter-only nodes of 16x32 .. 64x16
    for lw, lh in ((2, 4), (4, 2), (2, 3), (3, 2)):
        assert htdf["htdf_shape"][1][lw][lh] > 0
    _all(htdf["htdf_skip"][1:5], "CUs not filtered: area < 64, a side of 128, inter with min >= 32, inter without luma cbf")
    _all([ibc["htdf_skip"][0], ibc["htdf_skip"][5], tiled["htdf_skip"][6]], "CUs not filtered: QP <= 17 and IBC (the IBC cases), chroma-only tree (the tiled case: the reference harness knows no dual tree)")
    _all(htdf["htdf_table"][0], "filtered CUs by table, plain")
    _all(htdf["htdf_table"][1][:4], "filtered CUs by table after the - 8, tables 0 .. 3")
    _all([htdf["htdf_idx_neg"]], "index negative before the clamp")
    _all(htdf["htdf_avail"][[0, 1, 3, 5, 6, 7, 8]], "availability bits up, left, right, up-left, up-right, low-left, low-right x [clear, set]")
    _all(htdf["htdf_src"], "border samples [left, up, right] x [neighbour, own edge: unavailable, own edge: constrained intra]")
    _all(htdf["htdf_side_mixed"], "CUs whose [left, up, right] side mixes neighbours and refused units")
    _all(tiled["htdf_tile_refused"][[0, 1, 3, 4]], "left, up, up-left, up-right refused by a tile border alone")
    _all(htdf["htdf_lut"], "look-ups [table] x index 0 .. 15")
    _all(htdf["htdf_pass"], "pass-throughs [table]")
    _all(htdf["htdf_thr_edge"], "[table] x [a == thr - 1, a == thr]")
    # the output clip IS reached (rails_dither content, amp 40 residuals): the four shrunken inverse transforms of a sample do leave the range when a neighbour across
    # the window sits on the other rail - the census refuted the guess that their mean cannot
    _all(htdf["htdf_out_clip"], "output samples clipped [at 0, at max]")
    _all(htdf["htdf_nbr"][:, [0, 2, 3, 4]], "filtered CUs by [side] x neighbour kind intra, inter filtered, inter unfiltered, picture edge")
    _all(htdf["htdf_nbr"][[0, 2], 5], "filtered CUs whose [left, right] neighbour is not reconstructed yet")
    # the CU above is decoded before the CU in every order a tree produces (horizontal cuts and quad splits go top first): "there but not available" above is a tile border
    assert htdf["htdf_nbr"][1][5] == 0 and tiled["htdf_nbr"][1][5] > 0 and tiled["htdf_nbr"][1][5] == tiled["htdf_tile_refused"][1]
    _all(ibc["htdf_nbr"][:, 1], "filtered CUs with an IBC CU on their [left, upper, right] side (the IBC cases)")
    check_htdf_empty(htdf)
    for bd in (8, 10, 12):
        print(bd, "bit: filtered CUs [intra, inter]", by_bd[bd]["htdf_shape"].sum((1, 2)).tolist(), "clips", by_bd[bd]["htdf_out_clip"].tolist())
        assert (by_bd[bd]["htdf_shape"].sum((1, 2)) >= 64).all()
    _all([by_bd[8]["htdf_out_clip"].min(), by_bd[10]["htdf_out_clip"].min()], "output clip at both rails at 8 and at 10 bit")
    specs = xi.HTDF_CASES
    assert sorted(s[8]["htdf_qp"] for s in specs) == sorted(HTDF_SLICE_QPS)
    assert all((s[1], s[2], s[8].get("log2_ctu", 6)) in ((264, 264, 7), (264, 200, 6), (200, 136, 6)) and s[8]["extreme"].get("start") for s in specs + xi.IBC_CASES + xi.HTDF_TILE_CASES)
    assert sum(bool(s[8].get("constrained_intra")) for s in specs) == 2 and len(xi.HTDF_TILE_CASES) == 1 and len(specs) == 10
    assert {(bool(s[8].get("addb")), bool(s[8].get("alf"))) for s in specs} >= {(False, False), (True, False), (True, True)}
    assert any(s[8]["extreme"]["htdf_partition"].get("rtl") for s in specs) and any(not s[8]["extreme"]["htdf_partition"].get("rtl") for s in specs)


def intra_census_together():
    """the census of the intra cases and of the tiled one, summed: -> (INTRA_CASES, INTRA_TILE_CASES, {bit depth: ...}, {Baseline / EIPD: ...}, [(spec, case)])"""
    def add(a, b):
        return b if a is None else {k: a[k] + b[k] for k in b}
    out, by_bd, by_profile, built = [None, None], {}, {}, []
    for n, group in enumerate((xi.INTRA_CASES, xi.INTRA_TILE_CASES)):
        for spec in group:
            cs = cases.build_case(*spec[:9])
            _, cen = run_oracle_with_census(cs)
            cen = {k: np.asarray(v) for k, v in cen.items() if k.startswith("ip_")}
            check_intra_empty(cen)
            out[n] = add(out[n], cen)
            if n == 0:
                by_bd[spec[3]], by_profile[cs["eipd"]] = add(by_bd.get(spec[3]), cen), add(by_profile.get(cs["eipd"]), cen)
            built.append((spec, cs))
    return out[0], out[1], by_bd, by_profile, built


# levels of k_intra's dependency plan.  A strand takes a CU of level 2 or more whose only dependency of level 2 or more has no successor yet (xgpu_intra_plan.hip, link_strands), so
# it takes three levels at least; the mixed Baseline pictures, where seven CUs in ten are inter, give 6 and more, the all-intra ones 50 and more (but those of four CTU-sized shapes and an edge, `all128`: 19 and more)
INTRA_MIN_LEVELS, INTRA_MIN_LEVELS_ALL_INTRA = 6, 50


def test_intra_cases_together_reach_every_branch():
    """the conditions the intra cases were chosen for, over all of them (profiles/intra_census.txt holds this test's output)"""
    from test_builder import _build, _lib
    from xevd_amd import abi
    ip, tiled, by_bd, by_profile, built = intra_census_together()
    for k, v in ip.items():
        print(k, v.tolist())
    print("tiled case: ip_unavail", tiled["ip_unavail"].tolist(), "ip_tree", tiled["ip_tree"].tolist(), "ip_mode_lr by lr", tiled["ip_mode_lr"].sum(0).tolist())
    # CUs: every shape of 4 .. 64 a side under both sets of predictors, and sides of 128
    # CUs: under both sets of predictors every shape of 4 .. 64 a side and the nine of HTDF_128 - 128x128, and 128 by 64, 32, 16, 8 both ways -, no other: 128 by 4 has a ratio
    # no stream holds (check_intra_empty) and no partition table either
    every = np.zeros((6, 6), bool)
    every[:5, :5] = True
    for w_, h_ in xi.HTDF_128:
        every[int(np.log2(w_)) - 2, int(np.log2(h_)) - 2] = True
    assert every.sum() == 34 and not every[5, 0] and not every[0, 5]
    for p, name in enumerate(("Baseline", "EIPD")):
        assert ((ip["ip_shape"][p] > 0) == every).all(), f"{name}: intra CUs of every shape of 4 .. 64 a side and of HTDF_128, no other: {ip['ip_shape'][p].tolist()}"
    _all(ip["ip_mode_lr"], "EIPD luma mode 0 .. 32 x avail_lr 0 .. 3")
    _all(ip["ip_mode_aspect"], "EIPD luma mode x [wide, square, tall]")
    _all(ip["ip_cmode_lr"], "EIPD chroma mode 0 .. 4 x avail_lr")
    _all(ip["ip_dm_luma"], "chroma DM resolved to every luma mode")
    _all(ip["ip_base_mode"], "Baseline modes [luma, chroma] x 5")
    _all([ip["ip_base_c_differs"]], "Baseline CUs whose chroma mode differs")
    _all(ip["ip_dc"][0][:5], "DC over one column or none: table index 0 .. 4")
    _all(ip["ip_dc"][1][:6], "DC over both columns: table index 0 .. 5")
    # Planar, bucket by bucket.  Left form: all 34 shapes, the last row and column being mult[5] / shift[5], which only a side of 128 reads.  Mirrored form: exactly the
    # shapes that occur with a reconstructed right column in these batches (avail_lr restated from batch order: intra_shapes), which must hold every shape of up to 32
    # wide and 64 high - all a stream can give, because SUCO reverses the vertical cuts of nodes of at most 64x64 only (xevdm_check_suco_cond) - and may hold CUs of 64
    # wide that htdf_partition's CTU-128 order puts left of a cell decoded before them (the builder takes them: w + h <= 128).  A side of 128 never has one: its right-hand
    # neighbour is the next CTU, or - 64x128 and narrower - a CU of its own CTU, which htdf_partition always runs left to right and the builder would refuse
    # (test_builder_refuses_a_right_neighboured_cu_of_more_than_32_units).
    left_shapes, right_shapes = set(), set()
    for spec, cs in built:
        if spec in xi.INTRA_CASES and cs["eipd"]:
            left_shapes |= intra_shapes(cs, right=False)
            right_shapes |= intra_shapes(cs, right=True)
    in_left, in_right = np.zeros((6, 6), bool), np.zeros((6, 6), bool)
    for sh in left_shapes:
        in_left[sh] = True
    for sh in right_shapes:
        in_right[sh] = True
    assert (in_left == every).all() and in_right[:4, :5].all() and not in_right[5].any() and not in_right[:, 5].any(), (in_left.tolist(), in_right.tolist())
    assert ((ip["ip_plan"][0] > 0) == in_left).all(), f"planar, left form, on every shape [iw][ih] that occurs without a right column - all 34: {ip['ip_plan'][0].tolist()}"
    assert ((ip["ip_plan"][1] > 0) == in_right).all(), f"planar, mirrored, on every shape that occurs with a right column {in_right.tolist()}: {ip['ip_plan'][1].tolist()}"
    _all(ip["ip_plan_clip"], "planar samples clipped [at 0, at max]")
    _all(ip["ip_bi_form"], "bilinear [left, mirrored, both columns]")
    _all(ip["ip_bi_corner"], "one-column bilinear [left, mirrored] x [square, wc_tbl]")
    _all(ip["ip_bi_wc"][1:5], "wc_tbl index 1 .. 4")
    _all(ip["ip_bi_clip"][1:], "bilinear samples clipped at max")
    _all(ip["ip_hor"], "mode 24 by avail_lr 0 / 1, 2, 3")
    src = ip["ip_ang_src"].copy()
    src[0][1] = 1      # (asserted empty in check_intra_empty)
    _all(src, "angular samples by [mode class] x [up, left, right]")
    _all(ip["ip_ang_frac"], "angular fraction o == 0, o != 0")
    _all(ip["ip_ang_clamp"], "angular tap position clamped at -1, at w + h - 1")
    _all(ip["ip_nbr"][0], "EIPD builder [up, left, right] x [luma, chroma] x [available, repeated, nothing before it]")
    _all(ip["ip_nbr"][1][:2], "Baseline builder [up, left] x [luma, chroma] x [available, mid behind an available unit, mid from the first unit]")
    _all(ip["ip_unavail"][[0, 1, 3]], "units unavailable: outside the picture, not reconstructed yet, refused by constrained intra prediction")
    _all([tiled["ip_unavail"][2]], "units unavailable: in another tile (the tiled case)")
    assert ip["ip_unavail"][2] == 0
    _all(ip["ip_corner"], "corner [available, takes up[0], takes mid]")
    _all(tiled["ip_tree"], "CUs by tree 0, luma only, chroma only (the tiled case: the reference harness knows no dual tree)")
    assert ip["ip_tree"][1:].sum() == 0
    _all(ip["ip_cbf"], "intra CUs by cbf 0 .. 7")
    check_intra_empty(ip)
    for bd in (8, 10, 12):
        print(bd, "bit: CUs [Baseline, EIPD]", by_bd[bd]["ip_shape"].sum((1, 2)).tolist(), "planar clips", by_bd[bd]["ip_plan_clip"].tolist(), "mirrored planar", int(by_bd[bd]["ip_plan"][1].sum()))
        assert (by_bd[bd]["ip_shape"].sum((1, 2)) >= 40).all() and by_bd[bd]["ip_plan"][1].sum() > 0 and (by_bd[bd]["ip_plan_clip"] > 0).all()
    # from the batches: the named combinations, the part counts, the depth of the plan
    lib, seen, parts, levels = _lib(), set(), [set(), set()], {}
    for spec, cs in built:
        b = cs["batch"]
        lr = xi.intra_avail_lr(b, cs["w"], cs["h"], cs["log2_ctu"])
        sel = b["pred_mode"] == xi.MODE_INTRA
        if cs["eipd"]:
            seen |= set(zip(b["ipm"][sel, 0].tolist(), (1 << b["log2w"][sel].astype(int)).tolist(), (1 << b["log2h"][sel].astype(int)).tolist(), lr[sel].tolist()))
        if spec in xi.INTRA_CASES:
            parts[cs["eipd"]] |= set(intra_part_counts(cs).items())
        sp = abi.make_seq_params(cs["w"], cs["h"], cs["bd"], log2_ctu=cs["log2_ctu"], iqt=cs["iqt"], admvp=cs["admvp"], addb=cs["addb"], alf=cs["alf"], eipd=cs["eipd"])
        cb, keep = abi.make_cu_batch(b)
        one = _build(lib, sp, cb, 1)
        assert one == _build(lib, sp, cb, 4), spec[0]
        levels[spec[0]] = one[10 + 5]
        assert one[10 + 3] == int(xi.intra_parts(b, cs["eipd"])[sel].sum() + (b["pred_mode"] == 6).sum()), (spec[0], "entries of k_intra's list: the parts of the intra CUs and the copies")
    print("levels of the plan:", levels)
    assert (17, 4, 64, 3) in seen, "mode 17 on a 4x64 CU with both columns"
    assert any(m == 2 and w_ != h_ and l == 2 for m, w_, h_, l in seen), "bilinear with only the right column on a CU that is not square"
    assert {((16, 16), 1), ((64, 64), 16)} <= parts[1] and {p for _, p in parts[1]} == {1, 2, 4, 8, 16}, sorted(parts[1])
    assert {((64, 64), 4), ((128, 128), 16)} <= parts[0] and {p for _, p in parts[0]} == {1, 2, 4, 8, 16}, sorted(parts[0])
    assert min(levels.values()) >= INTRA_MIN_LEVELS, levels
    assert min(levels[s[0]] for s in xi.INTRA_CASES if s[8]["extreme"]["htdf_partition"]["inter_frac"] == 0 and not s[8]["extreme"]["htdf_partition"].get("all128")) >= INTRA_MIN_LEVELS_ALL_INTRA, levels
    specs = xi.INTRA_CASES
    assert {(s[3], bool(s[8].get("eipd"))) for s in specs} >= {(bd, e) for bd in (8, 10, 12) for e in (False, True)}
    assert {s[8].get("log2_ctu", 6) for s in specs if s[8].get("eipd")} == {6, 7} == {s[8].get("log2_ctu", 6) for s in specs if not s[8].get("eipd")}
    assert all(s[1] <= 264 and s[2] <= 264 and not s[8].get("htdf_qp") and s[9] for s in specs) and len(xi.INTRA_TILE_CASES) == 1
    gens = [s[8]["extreme"]["htdf_partition"] for s in specs]
    assert any(g["inter_frac"] == 0 for g in gens) and any(g["inter_frac"] > 0 and s[8].get("constrained_intra") for g, s in zip(gens, specs)) and any(g["inter_frac"] > 0 and not s[8].get("constrained_intra") for g, s in zip(gens, specs))
    assert any(g.get("amp") == 40.0 for g in gens) and sum(g["coded_frac"] == 0 for g in gens) == 1 and any(g.get("rtl") for g in gens) and any(not g.get("rtl") for g in gens)
    assert any("ibc" in s[8]["extreme"] and s[8].get("eipd") for s in specs) and any("ibc" in s[8]["extreme"] and not s[8].get("eipd") for s in specs)


@pytest.mark.parametrize("spec", xi.INTRA_TILE_CASES, ids=[s[0] for s in xi.INTRA_TILE_CASES])
def test_intra_tile_case_reaches_the_tile_and_tree_branches(spec):
    cs = cases.build_case(*spec)
    _, cen = run_oracle_with_census(cs)
    check_intra_tile_census(cen)


def check_intra_tile_census(cen):
    check_intra_empty(cen)
    _all([cen["ip_unavail"][2]], "neighbour units refused because they lie in another tile")
    _all(cen["ip_tree"], "intra CUs by tree 0, luma only, chroma only")
    _all(cen["ip_mode_lr"].sum(0), "EIPD CUs with avail_lr 0, 1, 2, 3")


def intra_surely_level1(cs):
    """mask of the intra CUs that certainly are level 1 of k_intra's plan: no unit of the row above, of the left column or the corner - w + h samples each way - lies in an
    intra CU that comes earlier in the batch (inter CUs are complete before the intra launches).  The plan looks at fewer units for most modes: it may find more."""
    b = cs["batch"]
    ws, hs = (cs["w"] + 3) >> 2, (cs["h"] + 3) >> 2
    intra_at = np.zeros((hs, ws), bool)
    out = np.zeros(len(b["x"]), bool)
    for i in np.nonzero(b["pred_mode"] == xi.MODE_INTRA)[0]:
        xs, ys, wu, hu = int(b["x"][i]) >> 2, int(b["y"][i]) >> 2, (1 << int(b["log2w"][i])) >> 2, (1 << int(b["log2h"][i])) >> 2
        up = ys > 0 and intra_at[ys - 1, max(xs - 1, 0):min(xs + wu + hu, ws)].any()
        le = xs > 0 and intra_at[ys:min(ys + wu + hu, hs), xs - 1].any()
        out[i] = not (up or le)
        intra_at[ys:ys + hu, xs:xs + wu] = True
    return out


# the Baseline cases without copies whose level 1 holds CUs of at most 16 SCUs (the picture of intra CUs only has one level-1 CU, its first, of 128x128: it never takes k_intra_l1)
INTRA_L1_CASES = [s for s in xi.INTRA_CASES if not s[8].get("eipd") and "ibc" not in s[8]["extreme"] and s[8]["extreme"]["htdf_partition"]["inter_frac"] > 0]
# level-1 CUs of at most 16 SCUs whose neighbour arrays are longer than 32 samples: the second staging pass of k_intra_l1's 16-lane body
INTRA_L1_LONG = {"x_ip_base_cip_12b_ctu128": {(32, 8), (64, 4), (32, 4)}, "x_ip_base_mixed_10b": {(4, 64), (64, 4), (4, 32), (32, 4)}}


@pytest.mark.parametrize("spec", INTRA_L1_CASES, ids=[s[0] for s in INTRA_L1_CASES])
def test_intra_l1_case_holds_its_long_shapes(spec):
    """what tests/test_gpu_extremes.py asks of the batches it sends through k_intra_l1, met here on the CPU"""
    cs = cases.build_case(*spec[:9])
    b = cs["batch"]
    small = intra_surely_level1(cs) & (b["log2w"].astype(int) + b["log2h"].astype(int) <= 8)
    shapes = set(zip((1 << b["log2w"][small].astype(int)).tolist(), (1 << b["log2h"][small].astype(int)).tolist()))
    assert small.any() and shapes >= INTRA_L1_LONG[spec[0]] and all(w_ + h_ > 32 for w_, h_ in INTRA_L1_LONG[spec[0]]), sorted(shapes)
    assert set().union(*INTRA_L1_LONG.values()) >= {(32, 8), (64, 4), (4, 64)} and set(INTRA_L1_LONG) == {s[0] for s in INTRA_L1_CASES}
    # ... and the plan agrees: its level 1 (info[4], in list entries) holds at least the CUs this estimate is sure of, none of which is split into parts (at most 16 SCUs), so
    # the launch of level 1 has n_small >= 1 - all that k_intra_l1 asks for with XEVD_HIP_INTRA_SMALL_MIN=1 in a Baseline picture without copies
    from test_builder import _build, _lib
    from xevd_amd import abi
    sp = abi.make_seq_params(cs["w"], cs["h"], cs["bd"], log2_ctu=cs["log2_ctu"], iqt=cs["iqt"], admvp=cs["admvp"], addb=cs["addb"], alf=cs["alf"], eipd=cs["eipd"])
    cb, keep = abi.make_cu_batch(b)
    n_l1 = _build(_lib(), sp, cb, 1)[10 + 4]
    sure = intra_surely_level1(cs)
    assert n_l1 >= int(xi.intra_parts(b, 0)[sure].sum()) >= small.sum() > 0 and not cs["eipd"] and not (b["pred_mode"] == 6).any(), (n_l1, int(sure.sum()), int(small.sum()))


def test_ibc_cases_together_reach_every_branch():
    """the conditions the IBC cases were chosen for, over the three of them (+ the luma-only copies of the tiled case's dual trees)"""
    _, ibc, tiled, _ = htdf_ibc_census_together()
    for k, v in ibc.items():
        if k.startswith("ibc_"):
            print(k, v.tolist())
    print("tiled case: ibc_luma_only", int(tiled["ibc_luma_only"]), "ibc_shape", tiled["ibc_shape"].tolist())
    _all(ibc["ibc_shape"], "IBC CUs of 4 .. 64 x 4 .. 64")
    _all([tiled["ibc_luma_only"]], "IBC CUs in a luma-only tree (the tiled case)")
    REQUIRE["ibc_parity"](ibc, None)
    for tag in ("ibc_touch", "ibc_spread", "ibc_chain", "ibc_cip"):
        REQUIRE[tag](ibc, None)
    _all(ibc["htdf_nbr"][:, 1], "an IBC CU as the left, upper, right neighbour of a filtered CU")
    assert len(xi.IBC_CASES) == 3 and {s[3] for s in xi.IBC_CASES} == {8, 10, 12}


@pytest.mark.parametrize("spec", xi.HTDF_TILE_CASES, ids=[s[0] for s in xi.HTDF_TILE_CASES])
def test_htdf_tile_case_reaches_the_tile_border_branches(spec):
    cs = cases.build_case(*spec)
    _, cen = run_oracle_with_census(cs)
    check_htdf_tile_census(cen)


def check_htdf_tile_census(cen):
    check_htdf_empty(cen)
    _all(cen["htdf_tile_refused"][[0, 1, 3, 4]], "left, up, up-left, up-right refused by a tile border alone")
    _all([cen["htdf_skip"][6], cen["ibc_luma_only"]], "chroma-only CUs left unfiltered; luma-only IBC CUs")
    _all(cen["htdf_shape"][0][[0, 2], [2, 0]], "filtered luma-only CUs of 4x16 and 16x4")


def affine_scu_mask(cs, maps):
    b = cs["batch"]
    mask = np.zeros((maps.h_scu, maps.w_scu), bool)
    for i in np.nonzero(b["affine"])[0]:
        mask[b["y"][i] >> 2:(b["y"][i] >> 2) + ((1 << b["log2h"][i]) >> 2), b["x"][i] >> 2:(b["x"][i] >> 2) + ((1 << b["log2w"][i]) >> 2)] = True
    return mask


@pytest.mark.ref
@pytest.mark.parametrize("spec", xi.AFFINE_CASES + xi.AFFINE_FAR_CASES, ids=[s[0] for s in xi.AFFINE_CASES + xi.AFFINE_FAR_CASES])
def test_affine_case_vectors_oracle_equals_reference(spec):
    """the vectors xevdm_set_affine_mvf leaves in the SCU map for the affine CUs - control points at the corners, the model at the other sub-blocks - and, for the far cases,
    the planes"""
    cs = cases.build_case(*spec[:9])
    a, _, ma, _ = cases.run_cpu("oracle", cs)
    b, _, mb, _ = cases.run_cpu("ref", cs, simd=0)
    mask = affine_scu_mask(cs, ma).ravel()
    assert mask.sum() > 0
    va, vb = ma.map_mv[mask], mb.map_mv[mask]
    assert np.array_equal(va, vb), f"map vectors of affine CUs, first differences at masked SCUs {np.argwhere(va != vb)[:4, 0].tolist()}"
    assert np.array_equal(ma.map_refi[mask], mb.map_refi[mask])
    # and they are sub-block vectors: inside some CU they differ from SCU to SCU
    own = np.zeros((ma.h_scu * ma.w_scu, 2, 2), np.int16)
    bt = cs["batch"]
    for i in np.nonzero(bt["affine"])[0]:
        sel = np.zeros((ma.h_scu, ma.w_scu), bool)
        sel[bt["y"][i] >> 2:(bt["y"][i] >> 2) + ((1 << bt["log2h"][i]) >> 2), bt["x"][i] >> 2:(bt["x"][i] >> 2) + ((1 << bt["log2w"][i]) >> 2)] = True
        own[sel.ravel()] = bt["affine_mv"].reshape(-1, 2, 3, 2)[i][:, 0]
    assert not np.array_equal(own[mask], va)
    for c in range(3):
        assert np.array_equal(a.bufs[c], b.bufs[c]), f"final plane {c}: {np.argwhere(a.bufs[c] != b.bufs[c])[:4]}"


@pytest.mark.parametrize("spec", xi.AFFINE_FAR_CASES, ids=[s[0] for s in xi.AFFINE_FAR_CASES])
def test_affine_far_case_reaches_the_clip18_of_the_eif_range(spec):
    cs = cases.build_case(*spec[:9])
    _, cen = run_oracle_with_census(cs)
    check_far_census(spec, cen)


def check_far_census(spec, cen):
    axis = 0 if spec[1] > spec[2] else 1
    _all(cen["aff_range_clip18"][axis], f"EIF range moved by clip18 along axis {axis} [min, max]")
    _all(cen["aff_band"], "EIF with the band [exceeded, kept]")
    _all(cen["aff_eif_clamp"][axis], f"EIF samples clamped along axis {axis} [low, high] x [picture range, band]")
    assert cen["aff_band_vn"][0] == 0


def check_tile_census(spec, cs, cen):
    """addb_tile_edge: 4-sample segments left alone because they lie on a tile border - [0] all, [1] those inside a 64x64 filter area k_addb_alf takes through its
    interior path (area and 4 samples around it inside the picture)"""
    if cs["batch"]["tiles"]["across"]:
        assert cen["addb_tile_edge"].sum() == 0, "loop_filter_across_tiles = 1 suppresses nothing"
    else:
        assert cen["addb_tile_edge"][1] > 0 and cen["addb_tile_edge"][0] > cen["addb_tile_edge"][1], cen["addb_tile_edge"].tolist()


@pytest.mark.parametrize("spec", xi.TILE_CASES, ids=[s[0] for s in xi.TILE_CASES])
def test_tile_case_has_tile_borders_inside_interior_filter_areas(spec):
    cs = cases.build_case(*spec)
    (a, _, _, _), cen = run_oracle_with_census(cs)
    check_tile_census(spec, cs, cen)
    # and the border matters on this content: the same picture with the flag the other way round differs
    cs["batch"]["tiles"]["across"] ^= 1      # (the ALF parameters share the grid)
    cs["alf_params"]["across_tiles"] ^= 1
    b, _, _, _ = cases.run_cpu("oracle", cs)
    assert any(not np.array_equal(a.bufs[c], b.bufs[c]) for c in range(3))


# which of the committed tiled streams already reach that branch (oracle census over the whole stream: [all, interior]); the GPU suite decodes every one of them
# with the packed filters, tests/test_gpu_extremes.py adds the scalar run for the ones marked here
TILED_STREAMS_REACHING_INTERIOR_BORDERS = {"main_affine_dmvr_tiles_8b": True, "main_btt_tiles_8b": True, "main_dual_tree_tiles_8b": True, "main_every_tool_tiles_8b": True,
                                           "main_tiles_3x2_all_tools_10b": True, "main_tiles_explicit_10b": True,
                                           "main_suco_tiles_dbk_8b": False, "main_tiles_2x2_dbk_8b": False,      # no ADDB: the baseline filter
                                           "main_tiles_across_dmvr_8b": False}                                   # loop_filter_across_tiles = 1


@pytest.mark.parametrize("name", sorted(TILED_STREAMS_REACHING_INTERIOR_BORDERS))
def test_which_tiled_golden_streams_reach_the_tile_border_branch(name):
    import os
    import golden_io
    import stream_util as su
    data = np.load(os.path.join(golden_io.GOLDEN, f"stream_{name}.npz"))["bytes"].tobytes()
    ol.census_reset()
    su.decode_oracle(data)
    cen = ol.census()
    print(name, "addb_tile_edge [all, interior] =", cen["addb_tile_edge"].tolist())
    assert (cen["addb_tile_edge"][1] > 0) == TILED_STREAMS_REACHING_INTERIOR_BORDERS[name], cen["addb_tile_edge"].tolist()


def test_alf_extreme_coefficients_are_at_the_legal_limit():
    """what alf_recon_coef asserts (src_main/xevdm_alf.c:751, :763, :786, :790): side taps in [-512, 511], centre in [-1024, 1023], unity gain"""
    for kind in ("extreme", "single", "smooth"):
        ap = xi.alf_params(kind, 3, 6)
        for f in list(ap["luma_coef"].astype(int)) + [ap["chroma_coef"].astype(int)]:
            assert 2 * f[:-1].sum() + f[-1] == 512 and f[:-1].min() >= -512 and f[:-1].max() <= 511 and -1024 <= f[-1] <= 1023
    assert np.abs(xi.alf_params("extreme", 3, 6)["luma_coef"][:, :12]).min() >= 511
    assert xi.alf_params("smooth", 3, 6)["luma_coef"][0, 12] == -1024 and xi.alf_params("single", 3, 6)["luma_coef"][0, 12] == 1022


# ------------------------------------------------------------------------------------------------ the residual pass
_CEN = ol.OrcCensus()


def _undef_count():
    """the oracle's count of second-stage sums the reference leaves undefined, without converting the whole census"""
    ol.oracle().orc_census_get(C.byref(_CEN))
    return int(_CEN.it_s2_undef)


def _clip_counts():
    """the oracle's dequantiser clips [below, above], both parities, without converting the whole census"""
    ol.oracle().orc_census_get(C.byref(_CEN))
    return np.array([_CEN.it_dq_clip[0][0] + _CEN.it_dq_clip[1][0], _CEN.it_dq_clip[0][1] + _CEN.it_dq_clip[1][1]], np.int64)


def ref_blocks(coef, lw, lh, qps, bd, iqt, tr=(0, 0)):
    """the reference's own dequantiser and transforms on blocks of one class, through its function tables (xevd_tbl_itxb, xevdm_tbl_itx) and its ATS stage functions"""
    lib = ol.ref()
    lib.xevd_dquant.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_uint8]
    w, h, n = 1 << lw, 1 << lh, 1 << (lw + lh)
    f_itxb = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int)
    f_itx = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int)
    f_ats = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int)
    if tr != (0, 0):
        lib.xevdm_init_multi_tbl()
        stage = [f_ats((f"xevdm_itrans_ats_intra_{'DST7' if t == 1 else 'DCT8'}_B{1 << l}", lib)) for t, l in ((tr[0], lh), (tr[1], lw))]
    elif iqt:
        itx = (C.c_void_p * 6).in_dll(lib, "xevdm_tbl_itx")
        stage = [f_itx(itx[lh - 1]), f_itx(itx[lw - 1])]
    else:
        itxb = (C.c_void_p * 6).in_dll(lib, "xevd_tbl_itxb")
        stage = [f_itxb(itxb[lh - 1]), f_itxb(itxb[lw - 1])]
    out = np.ascontiguousarray(coef, np.int16).copy()
    flat = out.reshape(-1)
    t16, t32 = np.zeros(n, np.int16), np.zeros(n, np.int32)
    for i, qp in enumerate(qps):
        p = C.c_void_p(flat.ctypes.data + 2 * i * n)
        shift = bd - 9 + ((lw + lh) >> 1) + 8 * ((lw + lh) & 1)
        lib.xevd_dquant(p, lw, lh, ri.SCALE[iqt][int(qp) % 6] << (int(qp) // 6), (1 << (shift - 1)) if shift else 0, shift)
        if tr != (0, 0):
            stage[0](p, t16.ctypes.data_as(C.c_void_p), 7, w, 0, 0)
            stage[1](t16.ctypes.data_as(C.c_void_p), p, 20 - bd, h, 0, 0)
        elif iqt:
            stage[0](p, t16.ctypes.data_as(C.c_void_p), 7, w)
            stage[1](t16.ctypes.data_as(C.c_void_p), p, 20 - bd, h)
        else:
            stage[0](p, t32.ctypes.data_as(C.c_void_p), 0, w, 0)
            stage[1](t32.ctypes.data_as(C.c_void_p), p, 27 - bd, h, 1)
    return out


def _pin_blocks(kind, lw, lh, bd, iqt, tr, tally=None):
    """one generator on one class: the oracle equals the reference on every block the reference is defined on, and the oracle's counter of undefined sums is non-zero on
    exactly the blocks that residual_inputs' model puts beyond 2^31.  -> (blocks pinned, blocks left out).
    thresholds: per QP the dequantiser's clip counters move exactly where a level that clips fits s16 (threshold_levels skips the others); `tally` counts the
    (class, QP, side) triples of either kind"""
    if kind == "thresholds":      # every representable threshold level of every QP
        blk, qps = ri.thresholds_all(lw, lh, bd, iqt, range(ri.qp_top(bd) + 1))
        n = len(qps)
    else:
        n = ri.n_blocks_for(kind, lw, lh)
        qps = ri.walk_qps(n, bd, start=lw + 2 * lh)
        blk = ri.blocks(kind, lw, lh, qps, bd, iqt, tr)
    s32 = not iqt and tr == (0, 0)
    undef = np.zeros(n, bool)
    got = np.zeros_like(blk)
    clipped = np.zeros((n, 2), bool)
    for i in range(n):
        before, clips = _undef_count(), _clip_counts()
        got[i] = ri.oracle_blocks(blk[i:i + 1], lw, lh, qps[i:i + 1], bd, iqt, tr)[0]
        undef[i] = _undef_count() != before
        clipped[i] = _clip_counts() != clips
    if kind == "thresholds":
        for qp in range(ri.qp_top(bd) + 1):
            names = {nm for nm, _ in ri.threshold_levels(lw, lh, qp, bd, iqt)}
            assert {"lo_clip", "lo_clip!"} & names and {"hi_clip", "hi_clip!"} & names
            for side, nm in enumerate(("lo_clip", "hi_clip")):
                reach = nm in names      # (else it is there as nm + "!": beyond s16, not fed)
                assert clipped[np.asarray(qps) == qp, side].any() == reach, (lw, lh, bd, iqt, "qp", qp, nm, "reachable" if reach else "out of reach", "and the clip counter disagrees")
                if tally is not None:
                    tally["reach" if reach else "unreach"] += 1
    if s32:
        model_says = np.array([ri.model(blk[i].astype(np.int64), lw, lh, int(qps[i]), bd, iqt, tr)["undef"] >= 1 << 31 for i in range(n)])
        assert np.array_equal(undef, model_says), (kind, lw, lh, bd, "the oracle's undefined blocks are not the ones aimed beyond 2^31", np.nonzero(undef != model_says)[0][:4])
    else:
        assert not undef.any()
    keep = np.nonzero(~undef)[0]      # a condition, not a measurement: every pinned block has the counter at 0
    exp = ref_blocks(blk[keep], lw, lh, qps[keep], bd, iqt, tr)
    bad = np.nonzero((exp != got[keep]).reshape(len(keep), -1).any(1))[0]
    assert bad.size == 0, (kind, lw, lh, bd, iqt, tr, "first differing block", int(keep[bad[0]]), "qp", int(qps[keep[bad[0]]]))
    return len(keep), int(undef.sum())


@pytest.mark.ref
@pytest.mark.parametrize("lw", range(1, 7))
@pytest.mark.parametrize("iqt", [0, 1])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_residual_blocks_oracle_equals_reference(bd, iqt, lw):
    """every block generator of residual_inputs on every class (this width, all heights) through the reference's own dequantiser and transform tables, both scale tables
    (iqt picks the table), and through its ATS stage functions for the four type pairs on 4 .. 32: orc_itdq / orc_itdq_ats bit-exact.  Blocks aimed beyond the range on
    which the reference's 32-bit second stage is defined are left out, and they are exactly the blocks on which the oracle's it_s2_undef moves."""
    ol.census_reset()
    pinned = left_out = 0
    tally = {"reach": 0, "unreach": 0}
    for lh in range(1, 7):
        for kind in ri.GENERATORS:
            a, b = _pin_blocks(kind, lw, lh, bd, iqt, (0, 0), tally)
            pinned, left_out = pinned + a, left_out + b
            if 2 <= lw <= 5 and 2 <= lh <= 5:
                for tr in ri.ATS_PAIRS:
                    a, b = _pin_blocks(kind, lw, lh, bd, iqt, tr)
                    pinned, left_out = pinned + a, left_out + b
    cen = ol.census()
    print("pinned", pinned, "left out", left_out, "it_s1_mag", cen["it_s1_mag"].tolist(), "it_s2_clip", cen["it_s2_clip"].tolist(), "it_s1_clip", cen["it_s1_clip"].tolist())
    assert (left_out > 0) == (not iqt), "the 32-bit intermediate has blocks beyond the defined range, the s16 one none"
    _all(cen["it_dq_clip"].reshape(-1), "dequantiser clips [even, odd] x [below, above]")
    # ... per (class, QP) the clip counters moved exactly where the first level that clips fits s16 (_pin_blocks).  Both kinds occur: every class has QPs at which levels
    # clip, and a (class, QP) at which none does exists where even 32767 stays inside at QP 0 - never at 8 bit, from 32x32 (the odd classes: 16x32) on at 10 bit, from 8x8 at 12 bit
    none_clips = any((32767 * ri.dq_params(lw, lh, 0, bd, iqt)[0] + ri.dq_params(lw, lh, 0, bd, iqt)[2]) >> ri.dq_params(lw, lh, 0, bd, iqt)[1] <= 32767 for lh in range(1, 7))
    assert tally["reach"] > 0 and (tally["unreach"] > 0) == none_clips, (tally, none_clips)
    assert bd > 8 or not none_clips
    print("thresholds: (class, QP, side) with a level that clips", tally["reach"], "without", tally["unreach"])
    # thresholds that no s16 level reaches are skipped by the generator, and both kinds occur.  A non-zero level dequantises to 0 where the smallest multiplier,
    # 40 (times 181 for an odd class) at QP 0, stays below half the divisor 2^shift: classes from 32x32 at 10 bit and from 8x8 at 12 bit, the odd ones from 32x64 at 10
    # bit and 8x16 at 12 bit, none at 8 bit.  The levels around 2^23 >> (qp / 6) fit s16 from QP 54 on, 10 and 12 bit; at 8 bit the bound is 32768 from QP 48 on, which
    # -32768 meets and nothing passes.
    for parity in range(2):
        reach = any(40 * (181 if parity else 1) < 1 << (bd - 9 + ((lw + lh) >> 1) + 8 * parity - 1) for lh in range(1, 7) if (lw + lh) & 1 == parity and bd - 9 + ((lw + lh) >> 1) >= 1)
        assert (cen["it_dq_zero"][parity] > 0) == reach, ("levels that dequantise to 0", parity, reach, cen["it_dq_zero"].tolist())
    assert (cen["it_dq_cmax"][:, 0] > 0).all() and ((cen["it_dq_cmax"][:, 1] > 0) == (bd > 8)).all(), cen["it_dq_cmax"].tolist()
    if 2 <= lw <= 5:
        _all(cen["it_s1_clip"][1], "ATS stage-1 clip")
    # The final clip is within reach where the largest second-stage sum passes 32767 after its shift: the column sum of |tm| of this width times the largest
    # intermediate - 32768 for the s16 one (shift 20 - bd), the largest first-stage sum over all heights, 3707 * 32768, for the 32-bit one (shift 27 - bd).  Both
    # kinds must occur over the widths and bit depths (2 wide at 8 bit is out of reach, 64 wide at 12 bit is not): asserted bucket by bucket, reachable or empty.
    colsum = int(np.abs(ri.matrix(0, lw)).sum(0).max())
    if iqt:
        _all(cen["it_s1_clip"][0], "IQT stage-1 clip")
        reach = (32768 * colsum + (1 << (19 - bd))) >> (20 - bd) > 32767
        assert (cen["it_s2_clip"][1] > 0).all() == reach and (cen["it_s2_clip"][1].sum() > 0) == reach, ("IQT final clip", reach, cen["it_s2_clip"][1].tolist())
    else:
        reach = (3707 * 32768 * colsum + (1 << (26 - bd))) >> (27 - bd) > 32767
        assert (cen["it_s2_clip"][0] > 0).all() == reach and (cen["it_s2_clip"][0].sum() > 0) == reach, ("final clip of the 32-bit intermediate", reach, cen["it_s2_clip"][0].tolist())
        _all([cen["it_s1_negfrac"]], "negative intermediates with low bits")
    # no intermediate of the 32-bit path reaches 2^27: the largest column sum of |xevd_tbl_tm64| is 3707, times 32768 = 121 470 976 < 134 217 728 - the kernel's
    # "|acc| < 2^28" (itdq_body.h) has a factor of two to spare
    assert int(np.abs(ri.matrix(0, 6)).sum(0).max()) * 32768 < 1 << 27 and cen["it_s1_mag"][3:].sum() == 0
    if lw == 6:
        assert (cen["it_single"] > 0).all(), "64x64: a single level in every (row pair, column pair)"
        _all(cen["it_high"], "levels at positions 32 .. 63")


def residual_reachable(built):
    """[kind][log2w - 1][log2h - 1] a TB can have, from the geometry of the CUs in these batches alone: a luma TB is the CU up to 64 a side (above: 64), a chroma TB half of
    it; ATS takes intra CUs of at most 32 a side; an ATS-inter TU is a half or a quarter of an inter CU of 8 .. 64 a side along one axis (a half needs 8, a quarter 16:
    xevdm_check_ats_inter_info_coded)"""
    reach = np.zeros((3, 6, 6), bool)
    for spec, cs in built:
        b = cs["batch"]
        for lw, lh in {(int(a), int(c)) for a, c in zip(b["log2w"], b["log2h"])}:
            tw, th = min(lw, 6), min(lh, 6)
            reach[0, tw - 1, th - 1] = reach[0, tw - 2, th - 2] = True
            if lw <= 5 and lh <= 5 and b.get("ats") is not None:
                reach[1, lw - 1, lh - 1] = True
            if lw <= 6 and lh <= 6 and b.get("ats_inter") is not None:
                for uw, uh in [(lw - 1, lh)] * (lw >= 3) + [(lw - 2, lh)] * (lw >= 4) + [(lw, lh - 1)] * (lh >= 3) + [(lw, lh - 2)] * (lh >= 4):
                    reach[2, uw - 1, uh - 1] = reach[2, uw - 2, uh - 2] = True
    return reach


def residual_census_together():
    def add(a, b):
        return b if a is None else {k: a[k] + b[k] for k in b}
    total, by_bd, built = None, {}, []
    for spec in xi.RESIDUAL_CASES:
        cs = cases.build_case(*spec[:9])
        _, cen = run_oracle_with_census(cs)
        cen = {k: np.asarray(v) for k, v in cen.items() if k.startswith("it_")}
        assert cen["it_s2_undef"] == 0 and cen["it_undef_tb"] == 0, (spec[0], "a picture case holds a block the reference is undefined on")
        total, by_bd[spec[3]] = add(total, cen), add(by_bd.get(spec[3]), cen)
        built.append((spec, cs))
    return total, by_bd, built


def check_residual_together(it, by_bd, built):
    reach = residual_reachable(built)
    # what geometry rules out: no class holds a 2 with a 64 (chroma ends at 32, luma starts at 4), ATS neither 2 nor 64, an ATS-inter TU no 64x64
    assert not reach[:, 0, 5].any() and not reach[:, 5, 0].any() and not reach[1, 0].any() and not reach[1, :, 5].any() and not reach[2, 5, 5]
    assert reach[0].sum() == 34 and reach[1].sum() == 16 and reach[2].sum() == 33, reach.sum((1, 2)).tolist()
    assert ((it["it_tb"] > 0) == reach).all(), f"TBs of every reachable [kind][class], no other: {np.argwhere((it['it_tb'] > 0) != reach).tolist()}"
    _all(it["it_plane"][0], "DCT-II TBs by plane")
    _all(it["it_plane"][2], "ATS-inter TUs by plane")
    assert it["it_plane"][1][0] > 0 and it["it_plane"][1][1:].sum() == 0, "ATS-intra is luma only"
    _all(it["it_ats_shape"], "every ATS type pair at every size of 4 .. 32, square and not")
    _all(it["it_ats_inter"], "ATS-inter TUs by [idx - 1][pos][with the ATS transforms / DCT-II (a CU side of 64)]")
    _all(it["it_strided"], "64x64 (chroma 32x32) sub-blocks that keep their CU's stride, by index")
    for bd, cen in by_bd.items():
        top = 51 + 6 * (bd - 8)
        _all(cen["it_qp"][:top + 1], f"{bd} bit: TBs at every QP of 0 .. {top}")
        assert cen["it_qp"][top + 1:].sum() == 0
        assert (cen["it_dq_cmax"] > 0).all() == (bd > 8), (bd, "levels at 2^23 >> (qp / 6) and one beyond, even and odd classes: from QP 54 on", cen["it_dq_cmax"].tolist())
    _all(it["it_dq_clip"], "dequantiser clips [even, odd] x [below, above]")
    _all(it["it_dq_zero"], "non-zero levels that dequantise to 0")
    _all(it["it_high"], "levels at positions 32 .. 63 [vertical, horizontal]")
    _all(it["it_s1_clip"], "stage-1 clips [IQT, ATS] x [low, high]")
    _all([it["it_s1_negfrac"]], "negative 32-bit intermediates with non-zero low bits")
    # the buckets the `defined` rule allows: with one term per second-stage sum (a coefficient column alone) the intermediate may reach 2^31 / 64 = 2^25, so the bucket
    # 2^24 .. 2^27 is reached; nothing reaches 2^27 at all (test_residual_blocks_oracle_equals_reference)
    _all(it["it_s1_mag"][:3], "32-bit intermediates below 2^15 / 2^24 / 2^27")
    assert it["it_s1_mag"][3:].sum() == 0
    _all(it["it_s2_clip"], "final clips [32-bit, IQT, ATS] x [low, high]")
    _all(it["it_nz_pairs"], "TBs by non-zero [row, column] pairs: 0 / 1 / 2 .. 4 / 5 or more / all")
    for d in range(2):
        for k in range(3):
            _all(it["it_single_dim"][d][k][:8 << k], f"single levels in every {'row' if d == 0 else 'column'} pair of the {16 << k}-point dimension")
            assert it["it_single_dim"][d][k][8 << k:].sum() == 0


def test_residual_cases_together_reach_every_branch():
    """the conditions the residual cases were chosen for, over all of them (profiles/residual_census.txt holds this test's output)"""
    it, by_bd, built = residual_census_together()
    for k, v in it.items():
        print(k, v.tolist())
    check_residual_together(it, by_bd, built)
    # a case without the Hadamard filter and with enough intra CUs for a data-flow intra launch (the residual pass rides in it when queued ahead), and one with the filter
    assert any(not cs["batch"].get("htdf_slice_qp") and (cs["batch"]["pred_mode"] == 0).sum() >= 32 for _, cs in built)
    assert any(cs["batch"].get("htdf_slice_qp") for _, cs in built)
