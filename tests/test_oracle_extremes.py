"""The extreme cases (tests/extreme_inputs.py: rail-to-rail content, QP 0..51 x slice offsets, vectors on the MV-clip thresholds, ALF coefficients at their legal
limits) through the CPU oracle and the REAL reference (oracle/_ref), plus the census: every case asserts that the oracle took the branches it exists for.

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

The census (which needs only the oracle) and the generator checks run everywhere; the comparison against the reference carries the `ref` mark and is skipped
where oracle/_ref is not built, like tests/test_oracle_vs_ref.py.
"""
import numpy as np
import pytest

import cases
import extreme_inputs as xi
import oracle_lib as ol

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


REQUIRE = {
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
}


def run_oracle_with_census(cs):
    ol.census_reset()
    out = cases.run_cpu("oracle", cs)
    return out, ol.census()


def check_census(spec, cs, cen):
    assert cen["addb_lost"][1] == 0 and cen["addb_lost"][2] == 0 and cen["mc_stage1_wrap"] == 0, "a bucket the module docstring calls unreachable was reached"
    for tag in spec[9]:
        REQUIRE[tag](cen, cs)


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
