"""GPU suite, ends of the ranges (run with -m gpu on an MI355X): the HIP backend against the CPU oracle on the extreme cases of tests/extreme_inputs.py -
samples on the rails, 0 / max checkerboards through every interpolation phase, QP 0..51 x ADDB slice offsets -12..12 (packed and scalar line filters),
ALF coefficients at their legal limits on gratings / noise / checkerboards, vectors on the MV-clip thresholds, every branch of the DMVR search (planted
displacements, vectors on the thresholds, all sub-block shapes; also its refined vectors, and the scalar form of its prediction), every branch of the affine model
(control points solved from target deltas: sub-block sizes, EIF applicability, the memory band and its clamps, the clip thresholds of the translation path, control points at
the s16 limits, vectors of more than 4096 samples; also the stored sub-block vectors), every branch of the Hadamard-domain filter (xi.HTDF_CASES: every CU shape as intra and as
filter-only inter node in every decoding order, right to left included, the slice QPs at the ends of every table's range, constrained intra prediction with sides that mix, an
uneven tile grid with local dual trees; also with the residual pass ahead - without the ride-along launch - and twice on one decoder) and of intra block copy (xi.IBC_CASES: vectors of
every parity and sign, sources over many CUs, inside filtered CUs and inside other copies), every intra predictor under every launch form (xi.INTRA_CASES: both neighbour-staging
schemes, the right-column forms, 1 to 16 parts per CU; also with the residual pass riding in the data-flow launch - k_intra_itdq, each value of EIPD, of copies and of IQT at least once -, through k_intra_l1's
16-lane body, twice on one decoder, and inside a tile grid with local dual trees), every branch of the residual pass (xi.RESIDUAL_CASES: levels aimed at each side of the
dequantiser's clips, of the first stage's s16 clip and of the final clip, single levels in every row and column pair up to position 63, work items that mix dense and
near-empty TBs, ATS on intra CUs and in ATS-inter TUs with and without IQT, every QP, sub-blocks that keep their CU's stride; also riding in the data-flow intra launch -
k_intra_itdq's own copy of the body and tables - and twice on one decoder), every role, window alignment and regime of k_inter's translational path (xi.MC_CASES: whole-region
CUs, CUs of one or two tiles and CUs down to 4x4 with lists, vectors, flags and TUs in fixed cycles per role, between different noise references over a start picture unlike
both - a chunk left out of a window by mistake reads samples that are wrong; also the SCU maps, the residual pass ahead, twice on one decoder and behind a picture of other
content) - all three padded planes and the residual arena, bit-exact.  tests/test_oracle_extremes.py pins the oracle to the reference on the same cases and seeds; the census assertions (that the inputs
reach the branches they are for) are repeated here because this file needs only the oracle, which always ships."""
import numpy as np
import pytest

import cases
import extreme_inputs as xi
import oracle_lib as ol
from test_oracle_extremes import TILED_STREAMS_REACHING_INTERIOR_BORDERS, check_census, check_htdf_tile_census, check_intra_tile_census, check_tile_census, run_oracle_with_census
from test_oracle_extremes import INTRA_L1_CASES, INTRA_L1_LONG, intra_surely_level1
from test_oracle_extremes import check_residual_together, residual_census_together

pytestmark = pytest.mark.gpu


def _same(out, ref, what):
    for c in range(3):
        assert np.array_equal(out[c], ref.bufs[c]), f"{what} plane {c}: first differences at (row, col) {np.argwhere(out[c] != ref.bufs[c])[:4].tolist()}"


def _check(cs, what, resid=False, **kw):
    ref, _, _, rr = cases.run_cpu("oracle", cs)
    if resid:
        out, res = cases.run_gpu(cs, resid=True, **kw)
        assert np.array_equal(res[:len(rr)], rr), f"{what}: residual arena, first differences at {np.argwhere(res[:len(rr)] != rr)[:4].ravel().tolist()}"
    else:
        out = cases.run_gpu(cs, **kw)
    _same(out, ref, what)


@pytest.mark.parametrize("spec", xi.EXTREME_CASES, ids=[s[0] for s in xi.EXTREME_CASES])
def test_gpu_extreme_case(spec):
    cs = cases.build_case(*spec[:9])
    (ref, _, _, rr), cen = run_oracle_with_census(cs)
    check_census(spec, cs, cen)
    out, res = cases.run_gpu(cs, resid=True)
    assert np.array_equal(res[:len(rr)], rr), f"residual arena, first differences at {np.argwhere(res[:len(rr)] != rr)[:4].ravel().tolist()}"
    _same(out, ref, spec[0])


_SCALAR = [s for s in xi.EXTREME_CASES if s[8].get("addb") and s[3] <= 10]


@pytest.mark.parametrize("spec", _SCALAR, ids=[s[0] for s in _SCALAR])
def test_gpu_extreme_case_scalar_deblocking(spec, monkeypatch):
    """the scalar ADDB line filters (XEVD_HIP_ADDB_SCALAR is read when a context opens) where the packed ones run by default: <= 10 bit"""
    monkeypatch.setenv("XEVD_HIP_ADDB_SCALAR", "1")
    _check(cases.build_case(*spec[:9]), spec[0] + " (scalar ADDB)")


@pytest.mark.parametrize("name", ["x_addb_ladder_10b", "x_alf_gratings_12b", "x_mc_checker2_base_b_8b", "x_mv_thresholds_main_10b", "x_recon_rails_10b",
                                  "x_intra_eipd_htdf_ibc_10b", "x_dmvr_checker_10b", "x_affine_checker_10b"])
def test_gpu_extreme_case_residual_pass_ahead(name):
    """once per family with the residual pass queued inside the previous picture's launch (xgpu_batch_recon_ahead)"""
    spec = next(s for s in xi.EXTREME_CASES if s[0] == name)
    _check(cases.build_case(*spec[:9]), name + " (ahead)", ahead=True)


# ---- DMVR: the cases of xi.DMVR_CASES (every branch of the search, test_dmvr_cases_together_reach_every_branch) - planes and residual arena in test_gpu_extreme_case above
def _check_dmvr(cs, what, **kw):
    """planes and refined vectors: the vectors tell a failure of the search from one of the refined prediction"""
    ref, _, _, _ = cases.run_cpu("oracle", cs)
    want = cases.dmvr_mvs("oracle", cs)
    out, mvs = cases.run_gpu(cs, dmvr=True, **kw)
    got = np.asarray(mvs).reshape(-1, 2, 2)
    assert len(want) > 0 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), f"{what}: refined vectors, first differences at sub-blocks {sorted(set(np.argwhere(got != want)[:, 0].tolist()))[:4]}"
    _same(out, ref, what)


@pytest.mark.parametrize("spec", xi.DMVR_CASES, ids=[s[0] for s in xi.DMVR_CASES])
def test_gpu_dmvr_case_vectors(spec):
    _check_dmvr(cases.build_case(*spec[:9]), spec[0])


@pytest.mark.parametrize("spec", xi.DMVR_CASES, ids=[s[0] for s in xi.DMVR_CASES])
def test_gpu_dmvr_case_residual_pass_ahead(spec):
    _check_dmvr(cases.build_case(*spec[:9]), spec[0] + " (ahead)", ahead=True)


_DMVR_SCALAR = xi.DMVR_CASES + [s for s in xi.EXTREME_CASES if s[0] in ("x_dmvr_checker_10b", "x_dmvr_noise_8b")]


@pytest.mark.parametrize("spec", _DMVR_SCALAR, ids=[s[0] for s in _DMVR_SCALAR])
def test_gpu_extreme_case_scalar_dmvr(spec, monkeypatch):
    """k_dmvr's scalar form of the refined prediction (XEVD_HIP_DMVR_SCALAR is read when a context opens).  Valid input never reaches it - the refined position lies at most
    2 luma / 1 chroma samples from the starting vector's window (tests/test_oracle_extremes.py), the packed form covers 3 / 2 -, so it runs here or nowhere."""
    monkeypatch.setenv("XEVD_HIP_DMVR_SCALAR", "1")
    _check_dmvr(cases.build_case(*spec[:9]), spec[0] + " (scalar DMVR)")


@pytest.mark.parametrize("name", ["x_dmvr_thresholds_10b", "x_dmvr_thresholds_8b_noaddb"])
def test_gpu_dmvr_case_stored_vectors(name):
    """the vectors the picture keeps (side-information export) against the oracle's map: the unrefined ones under ADDB, the refined ones - the baseline filter reads them - without
    (the export hands out torch tensors: whichever test of a run needs torch first pays for its import)"""
    import side_info_ref as sr
    from test_gpu_side_info import decode, open_decoder, start
    spec = next(s for s in xi.DMVR_CASES if s[0] == name)
    cs = cases.build_case(*spec[:9])
    _, _, maps, _ = cases.run_cpu("oracle", cs, pad=False)
    want = sr.blocks_from_maps(maps, maps.map_scu, cs["batch"], {k: p.poc for k, p in cs["refs"].items()}, cases.CUR_POC)
    with open_decoder(cs) as dec:
        slots, cur, hb = start(dec, cs)
        decode(dec, cs, slots, cur, hb)
        got = dec.frame_side_info(cur).cpu().numpy()
    for p in range(4):
        assert np.array_equal(got[p], want[p]), f"{name}: vector plane {p}, first differences at 4x4 units {np.argwhere(got[p] != want[p])[:4].tolist()}"
    # and the case tells the two apart: the oracle's map differs from the batch's own vectors exactly when the filter is the baseline one
    b = cs["batch"]
    own = np.zeros((maps.h_scu, maps.w_scu, 4), np.int16)
    for i in range(len(b["x"])):
        own[b["y"][i] >> 2:(b["y"][i] >> 2) + ((1 << b["log2h"][i]) >> 2), b["x"][i] >> 2:(b["x"][i] >> 2) + ((1 << b["log2w"][i]) >> 2)] = b["mv"][i].reshape(4)
    assert np.array_equal(maps.map_mv.reshape(maps.h_scu, maps.w_scu, 4), own) == bool(cs["addb"])


# ---- affine: the cases of xi.AFFINE_CASES (every branch of the model, test_affine_cases_together_reach_every_branch) - planes, residual arena and census in test_gpu_extreme_case
# above, those with ADDB at up to 10 bit also in test_gpu_extreme_case_scalar_deblocking (the sub-block vectors feed the boundary strengths)
@pytest.mark.parametrize("spec", xi.AFFINE_CASES, ids=[s[0] for s in xi.AFFINE_CASES])
def test_gpu_affine_case_residual_pass_ahead(spec):
    _check(cases.build_case(*spec[:9]), spec[0] + " (ahead)", ahead=True)


@pytest.mark.parametrize("name", ["x_aff_sizes_10b", "x_aff_sizes_8b_noaddb", "x_aff_limits_8b", "x_aff_limits_10b_noaddb"])
def test_gpu_affine_case_stored_vectors(name):
    """the vectors the picture keeps (side-information export) against the oracle's map: every sub-block size, control points at the s16 limits (map vectors moved by
    clip18), two-point CUs whose bottom-left sub-block takes the formula; under ADDB and under the baseline filter.  A failure here and not in the planes is one of
    aff_store_mvf, not of the prediction."""
    import side_info_ref as sr
    from test_gpu_side_info import decode, open_decoder, start
    spec = next(s for s in xi.AFFINE_CASES if s[0] == name)
    cs = cases.build_case(*spec[:9])
    (_, _, maps, _), cen = run_oracle_with_census(cs)
    assert cen["aff_mvf_bl_vn2"] > 0 and (cen["aff_mvf"] > 0).all() and ((cen["aff_mvf_clip18"] > 0) == ("limits" in name)) and (("sizes" not in name) or (cen["aff_sub"][:, :3] > 0).all())
    want = sr.blocks_from_maps(maps, maps.map_scu, cs["batch"], {k: p.poc for k, p in cs["refs"].items()}, cases.CUR_POC)
    with open_decoder(cs) as dec:
        slots, cur, hb = start(dec, cs)
        decode(dec, cs, slots, cur, hb)
        got = dec.frame_side_info(cur).cpu().numpy()
    for p in range(4):
        assert np.array_equal(got[p], want[p]), f"{name}: vector plane {p}, first differences at 4x4 units {np.argwhere(got[p] != want[p])[:4].tolist()}"


@pytest.mark.parametrize("spec", xi.AFFINE_FAR_CASES, ids=[s[0] for s in xi.AFFINE_FAR_CASES])
def test_gpu_affine_far_vectors(spec):
    """clip18 of the EIF range: a picture of 4160 samples along one axis, vectors of more than 4096 samples that end inside it (the wide one: 65 CTUs a row)"""
    from test_oracle_extremes import check_far_census
    cs = cases.build_case(*spec[:9])
    (ref, _, _, rr), cen = run_oracle_with_census(cs)
    check_far_census(spec, cen)
    out, res = cases.run_gpu(cs, resid=True)
    assert np.array_equal(res[:len(rr)], rr), "residual arena"
    _same(out, ref, spec[0])


# ---- HTDF and intra block copy: the cases of xi.HTDF_CASES / xi.IBC_CASES (every branch of the filter and of the copy, test_htdf_cases_together_reach_every_branch,
# test_ibc_cases_together_reach_every_branch) - planes, residual arena and census in test_gpu_extreme_case above, those with ADDB at up to 10 bit also in
# test_gpu_extreme_case_scalar_deblocking
@pytest.mark.parametrize("spec", xi.HTDF_CASES + xi.IBC_CASES, ids=[s[0] for s in xi.HTDF_CASES + xi.IBC_CASES])
def test_gpu_htdf_ibc_case_residual_pass_ahead(spec):
    """with HTDF nodes in the batch the residual pass of the next picture does not ride along in the data-flow launch: the other way of queueing it"""
    _check(cases.build_case(*spec[:9]), spec[0] + " (ahead)", resid=True, ahead=True)


@pytest.mark.parametrize("name", ["x_htdf_qp32_cip_10b_ctu128", "x_ibc_chain_cip_12b"])
def test_gpu_htdf_case_decoded_twice_on_one_decoder(name):
    """one batch decoded twice into one picture of one decoder, the start picture uploaded again in between (as cases.run_gpu(ahead=True) does): the done flags and the
    epoch of the data-flow launch are reused, and both pictures must be the oracle's"""
    from xevd_amd.decoder import XgpuDecoder
    spec = next(s for s in xi.EXTREME_CASES if s[0] == name)
    cs = cases.build_case(*spec[:9])
    ref, _, _, _ = cases.run_cpu("oracle", cs)
    with XgpuDecoder(cs["w"], cs["h"], cs["bd"], log2_ctu=cs["log2_ctu"], iqt=cs["iqt"], admvp=cs["admvp"], addb=cs["addb"], alf=cs["alf"], eipd=cs["eipd"], max_pics=8) as dec:
        slots, by_obj = {}, {}
        for key, pic in cs["refs"].items():
            if id(pic) not in by_obj:
                by_obj[id(pic)] = dec.pic_alloc()
                dec.pic_upload_padded(by_obj[id(pic)], pic.bufs)
            slots[key] = (by_obj[id(pic)], pic.poc)
        cur = dec.pic_alloc()
        hb = dec.batch_create(cs["batch"])
        outs = []
        for _ in range(2):
            dec.pic_upload_padded(cur, cases._start_picture(cs).bufs)
            dec.decode_picture(cur, cases.CUR_POC, slots, hb, deblock=not cs.get("no_deblock"), pad=True, qp_u_offset=cases.QP_OFFSETS[0], qp_v_offset=cases.QP_OFFSETS[1],
                               alpha_off=cs["alpha_off"], beta_off=cs["beta_off"], alf=cs.get("alf_params"))
            dec.sync()
            outs.append([np.array(p, copy=True) for p in dec.pic_download_padded(cur)])
    _same(outs[0], ref, name + " (first decode)")
    _same(outs[1], ref, name + " (second decode)")


@pytest.mark.parametrize("spec", xi.HTDF_TILE_CASES, ids=[s[0] for s in xi.HTDF_TILE_CASES])
def test_gpu_htdf_tile_case(spec):
    """HTDF, IBC and local dual trees inside an uneven tile grid: neighbours and sources across a tile border are not available.  Against the oracle only (the reference
    harness has no tile map)."""
    cs = cases.build_case(*spec)
    (ref, _, _, rr), cen = run_oracle_with_census(cs)
    check_htdf_tile_census(cen)
    out, res = cases.run_gpu(cs, resid=True)
    assert np.array_equal(res[:len(rr)], rr), "residual arena"
    _same(out, ref, spec[0])
    _same(cases.run_gpu(cs, ahead=True), ref, spec[0] + " (ahead)")


# ---- intra prediction: the cases of xi.INTRA_CASES (every predictor, both neighbour-staging schemes, the right-column forms; test_intra_cases_together_reach_every_branch) -
# planes, residual arena and census in test_gpu_extreme_case above (k_intra<DEP, EIPD, IBC, HTDF> behind a plain level-1 launch), those with ADDB at up to 10 bit also in
# test_gpu_extreme_case_scalar_deblocking.  Here the launch forms that run does not take.
@pytest.mark.parametrize("spec", xi.INTRA_CASES, ids=[s[0] for s in xi.INTRA_CASES])
def test_gpu_intra_case_residual_pass_ahead(spec):
    """the next picture's residual pass rides in the data-flow intra launch (k_intra_itdq; no case here has HTDF nodes): tests/test_builder.py holds which of its
    instantiations the cases take - each value of EIPD, of copies and of IQT at least once, five of the ten.  (The case without coefficients has no pass to ride along: it takes the plain launch twice.)"""
    _check(cases.build_case(*spec[:9]), spec[0] + " (ahead)", resid=True, ahead=True)


@pytest.mark.parametrize("spec", INTRA_L1_CASES, ids=[s[0] for s in INTRA_L1_CASES])
def test_gpu_intra_case_sixteen_lanes_per_cu(spec, monkeypatch):
    """k_intra_l1 (XEVD_HIP_INTRA_SMALL_MIN is read when a context opens): the level-1 CUs of at most 16 SCUs of the mixed Baseline cases, 16 lanes each: every such intra CU among inter
    neighbours, 32x8, 64x4 and 4x64 among them (tests/test_oracle_extremes.py: INTRA_L1_LONG)"""
    monkeypatch.setenv("XEVD_HIP_INTRA_SMALL_MIN", "1")
    cs = cases.build_case(*spec[:9])
    b = cs["batch"]
    small = intra_surely_level1(cs) & (b["log2w"].astype(int) + b["log2h"].astype(int) <= 8)
    shapes = set(zip((1 << b["log2w"][small].astype(int)).tolist(), (1 << b["log2h"][small].astype(int)).tolist()))
    assert small.any() and shapes >= INTRA_L1_LONG[spec[0]], sorted(shapes)
    _check(cs, spec[0] + " (k_intra_l1)", resid=True)


@pytest.mark.parametrize("name", ["x_ip_eipd_rtl_12b_ctu128", "x_ip_base_mixed_10b"])
def test_gpu_intra_case_decoded_twice_on_one_decoder(name):
    """as test_gpu_htdf_case_decoded_twice_on_one_decoder, without the filter: an EIPD picture in a right-to-left order and a Baseline one - done flags and epoch reused"""
    test_gpu_htdf_case_decoded_twice_on_one_decoder(name)


@pytest.mark.parametrize("spec", xi.INTRA_TILE_CASES, ids=[s[0] for s in xi.INTRA_TILE_CASES])
def test_gpu_intra_tile_case(spec):
    """intra prediction inside an uneven tile grid with local dual trees: units across a tile border are not available; luma-only and chroma-only CUs.  Against the oracle
    only (the reference harness has neither a tile map nor dual trees)."""
    cs = cases.build_case(*spec)
    (ref, _, _, rr), cen = run_oracle_with_census(cs)
    check_intra_tile_census(cen)
    out, res = cases.run_gpu(cs, resid=True)
    assert np.array_equal(res[:len(rr)], rr), "residual arena"
    _same(out, ref, spec[0])
    _same(cases.run_gpu(cs, ahead=True), ref, spec[0] + " (ahead)")


# ---- the residual pass: the cases of xi.RESIDUAL_CASES (every branch of the dequantiser and of both transform stages, test_residual_cases_together_reach_every_branch) - planes,
# residual arena and the tags' census in test_gpu_extreme_case above, those with ADDB also in test_gpu_extreme_case_scalar_deblocking.  Here the other copy of the body and
# its tables, and the census of the cases together.
@pytest.mark.parametrize("spec", xi.RESIDUAL_CASES, ids=[s[0] for s in xi.RESIDUAL_CASES])
def test_gpu_residual_case_residual_pass_ahead(spec):
    """queued with the previous picture's kernels the residual pass rides in the data-flow intra launch: k_intra_itdq's instantiation of itdq_body.h with that translation
    unit's own constant tables (the case with HTDF nodes takes the side stream instead).  Residual arena and planes."""
    _check(cases.build_case(*spec[:9]), spec[0] + " (ahead)", resid=True, ahead=True)


@pytest.mark.parametrize("name", ["x_res_ats_intra_10b", "x_res_ctu128_noiqt_12b"])
def test_gpu_residual_case_decoded_twice_on_one_decoder(name):
    """as test_gpu_htdf_case_decoded_twice_on_one_decoder: the second decode's residual pass runs on workgroups whose LDS the first one filled"""
    test_gpu_htdf_case_decoded_twice_on_one_decoder(name)


def test_gpu_residual_cases_reach_every_branch():
    """the census assertions of tests/test_oracle_extremes.py over the residual cases together, repeated where only the oracle is needed"""
    it, by_bd, built = residual_census_together()
    check_residual_together(it, by_bd, built)


# ---- translational motion compensation: the cases of xi.MC_CASES (every role, window alignment and regime of k_inter, test_mc_cases_together_reach_every_branch; the launch
# side of their census is tests/mc_launch.py) - planes, residual arena and the tags' census under the default launch in test_gpu_extreme_case above, those with ADDB also in
# test_gpu_extreme_case_scalar_deblocking.  Here the SCU maps, the other way of queueing the residual pass, and what a second picture finds in LDS and in the owner map.
def _mc_expected(cs):
    """the oracle's picture, residual arena and SCU maps (as the side-information export shows them) of a case"""
    import side_info_ref as sr
    ref, _, maps, rr = cases.run_cpu("oracle", cs)
    return ref, rr, sr.blocks_from_maps(maps, maps.map_scu, cs["batch"], {k: p.poc for k, p in cs["refs"].items()}, cases.CUR_POC)


def _mc_picture(dec, cur):
    """what a decode left in picture `cur`: (SCU maps through the side-information export, padded planes)"""
    got = dec.frame_side_info(cur).cpu().numpy()
    return got, [np.array(p, copy=True) for p in dec.pic_download_padded(cur)]


def _mc_same_maps(got, want, what):
    from test_gpu_side_info import PLANE_NAMES
    for p in range(len(PLANE_NAMES)):
        assert np.array_equal(got[p], want[p]), f"{what}: map plane {PLANE_NAMES[p]}, first differences at 4x4 units {np.argwhere(got[p] != want[p])[:4].tolist()}"


@pytest.mark.parametrize("spec", xi.MC_CASES, ids=[s[0] for s in xi.MC_CASES])
def test_gpu_mc_case_scu_maps(spec):
    """what k_inter's map update leaves per SCU - vectors (the unclipped ones), reference POC distances, mode with the skip flag, QP, luma cbf inside the ATS-inter TU only, CU
    edges - through the side-information export, against the oracle's maps; and the planes of that decode"""
    from test_gpu_side_info import decode, open_decoder, start
    cs = cases.build_case(*spec[:9])
    ref, _, want = _mc_expected(cs)
    with open_decoder(cs) as dec:
        slots, cur, hb = start(dec, cs)
        decode(dec, cs, slots, cur, hb)
        got, out = _mc_picture(dec, cur)
    _mc_same_maps(got, want, spec[0])
    _same(out, ref, spec[0])


@pytest.mark.parametrize("spec", xi.MC_CASES, ids=[s[0] for s in xi.MC_CASES])
def test_gpu_mc_case_residual_pass_ahead(spec):
    """the residual pass queued with the previous picture's kernels (xgpu_batch_recon_ahead; what cases.run_gpu(ahead=True) does, the decoder left open): k_inter then finds
    the whole residual arena written before it starts.  Planes, residual arena and SCU maps of the picture whose pass ran ahead, and of the one in front of it."""
    from test_gpu_side_info import decode, open_decoder, start
    cs = cases.build_case(*spec[:9])
    ref, rr, want = _mc_expected(cs)
    with open_decoder(cs) as dec:
        slots, cur, hb = start(dec, cs)
        hb2 = dec.batch_create(cs["batch"])
        dec.decode_picture(cur, cases.CUR_POC, slots, hb, deblock=not cs.get("no_deblock"), pad=True, qp_u_offset=cases.QP_OFFSETS[0], qp_v_offset=cases.QP_OFFSETS[1],
                           alpha_off=cs.get("alpha_off", 0), beta_off=cs.get("beta_off", 0), alf=cs.get("alf_params"), next_batch=hb2)
        dec.sync()
        got0, out0 = _mc_picture(dec, cur)
        dec.pic_upload_padded(cur, cases._start_picture(cs).bufs)
        decode(dec, cs, slots, cur, hb2)
        dec.sync()
        got, out = _mc_picture(dec, cur)
        res = dec.batch_resid(hb2, cs["batch"]["n_coef"])
    _mc_same_maps(got0, want, spec[0] + " (the picture in front)")
    _same(out0, ref, spec[0] + " (the picture in front)")
    assert np.array_equal(res[:len(rr)], rr), f"{spec[0]} (ahead): residual arena, first differences at {np.argwhere(res[:len(rr)] != rr)[:4].ravel().tolist()}"
    _mc_same_maps(got, want, spec[0] + " (ahead)")
    _same(out, ref, spec[0] + " (ahead)")


@pytest.mark.parametrize("name", ["x_mcr_walk_main_10b", "x_mcr_thresholds_base_12b"])
def test_gpu_mc_case_decoded_twice_on_one_decoder(name):
    """one batch decoded twice into one picture of one decoder, the start picture uploaded again in between: the second decode's workgroups find the first one's windows in LDS
    (what a chunk left out by mistake would read), the batch's owner map and items in place, and the picture's SCU maps filled - k_inter leaves the vector words of
    DMVR-refined CUs to k_dmvr.  Planes and SCU maps after each decode."""
    from test_gpu_side_info import decode, open_decoder, start
    spec = next(s for s in xi.MC_CASES if s[0] == name)
    cs = cases.build_case(*spec[:9])
    ref, _, want = _mc_expected(cs)
    seen = []
    with open_decoder(cs) as dec:
        slots, cur, hb = start(dec, cs)
        for _ in range(2):
            dec.pic_upload_padded(cur, cases._start_picture(cs).bufs)
            decode(dec, cs, slots, cur, hb)
            dec.sync()
            seen.append(_mc_picture(dec, cur))
    for (got, out), what in zip(seen, ("first decode", "second decode")):
        _mc_same_maps(got, want, f"{name} ({what})")
        _same(out, ref, f"{name} ({what})")


@pytest.mark.parametrize("name", ["x_mcr_walk_main_8b_aligned", "x_mcr_walk_main_10b"])
def test_gpu_mc_case_after_a_picture_of_other_content(name):
    """a case decoded behind another picture of the same sequence (the same case drawn with another seed: other references, other vectors, other flags and TUs, its cycles
    elsewhere) on one decoder, into the same picture slot, whose SCU maps that picture has just filled: planes and maps bit-identical to decoding it first, and the oracle's.
    Both cases have all three roles; the second one has DMVR-flagged CUs, of whose map records k_inter writes a part only."""
    from test_gpu_side_info import decode, open_decoder, start, upload_refs
    spec = next(s for s in xi.MC_CASES if s[0] == name)
    cs, other = cases.build_case(*spec[:9]), cases.build_case(*spec[:9], seed=1)
    assert not np.array_equal(cs["batch"]["mv"], other["batch"]["mv"]) and not np.array_equal(cs["refs"][(0, 0)].bufs[0], other["refs"][(0, 0)].bufs[0])
    ref, _, want = _mc_expected(cs)
    ref_other, _, want_other = _mc_expected(other)
    assert any(not np.array_equal(want[p], want_other[p]) for p in range(4)), "the two pictures' maps differ"
    with open_decoder(cs) as dec:
        slots, cur, hb = start(dec, cs)
        decode(dec, cs, slots, cur, hb)
        dec.sync()
        first_maps, first = _mc_picture(dec, cur)
    with open_decoder(cs) as dec:
        slots = upload_refs(dec, other)
        cur = dec.pic_alloc()
        hb_other, hb = dec.batch_create(other["batch"]), dec.batch_create(cs["batch"])
        dec.pic_upload_padded(cur, cases._start_picture(other).bufs)
        decode(dec, other, slots, cur, hb_other)
        dec.sync()
        before_maps, before = _mc_picture(dec, cur)
        by_obj = {}
        for key, pic in cs["refs"].items():      # the same slots, the other pictures
            if id(pic) not in by_obj:
                by_obj[id(pic)] = slots[key][0]
                dec.pic_upload_padded(slots[key][0], pic.bufs)
            slots[key] = (by_obj[id(pic)], pic.poc)
        dec.pic_upload_padded(cur, cases._start_picture(cs).bufs)
        decode(dec, cs, slots, cur, hb)
        dec.sync()
        second_maps, second = _mc_picture(dec, cur)
    _mc_same_maps(before_maps, want_other, name + " (the picture before)")
    _same(before, ref_other, name + " (the picture before)")
    for c in range(3):
        assert np.array_equal(second[c], first[c]), f"plane {c}: decoded second differs from decoded first at {np.argwhere(second[c] != first[c])[:4].tolist()}"
    assert np.array_equal(second_maps, first_maps), f"SCU maps: decoded second differs from decoded first in planes {sorted(set(np.argwhere(second_maps != first_maps)[:, 0].tolist()))}"
    _mc_same_maps(second_maps, want, name + " (decoded second)")
    _same(second, ref, name + " (decoded second)")


def test_gpu_mc_cases_reach_every_branch():
    """the census assertions of tests/test_oracle_extremes.py over the motion-compensation cases together, repeated where only the oracle is needed"""
    from test_oracle_extremes import check_mc_together, mc_census_together
    check_mc_together(*mc_census_together())


# content kind x bit depth x partition depth per coding family.  split_prob low / high: k_inter's region and tile roles / its split role see the saturated windows
FAMILIES = {
    "base_pb": (0, 0, (2, 2), 0.4, {"inter_frac": 1.0}),
    "main_b_addb_alf": (1, 1, (2, 2), 0.5, {"addb": 1, "alf": 1, "inter_frac": 1.0}),
    "main_dmvr": (1, 1, (2, 2), 0.9, {"addb": 1, "inter_frac": 1.0, "dmvr_frac": 0.9, "oob_frac": 0.0}),
    "main_affine_eif": (1, 1, (2, 2), 0.5, {"addb": 1, "alf": 1, "inter_frac": 1.0, "affine_frac": 0.9}),
}
CONTENT = ("noise", "checker1", "checker2", "checker4", "rows", "cols", "flat0", "flatmax", "rails_dither", "ladder", "gratings")


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_gpu_content_kinds(family, bd):
    admvp, iqt, n_refs, bi, tools = FAMILIES[family]
    ol.census_reset()
    for n, kind in enumerate(CONTENT):
        for split in ((0.15, 0.85) if kind in ("noise", "checker1", "rails_dither") else ((0.15, 0.85)[(n + bd // 2) & 1],)):
            t = dict(tools, split_prob=split, amp=40.0 if n & 1 else 2.0, extreme={"content": [kind, "noise" if n % 3 == 0 else kind], "mv": None if family == "main_affine_eif" else "small"})
            cs = cases.build_case(f"xm_{family}_{kind}", 136, 72, bd, admvp, iqt, n_refs, bi, t, seed=n)
            _check(cs, f"{family} {kind} {bd} bit split {split}")
    cen = ol.census()      # over the whole sweep: saturated windows went through the interpolation and the reconstruction at both rails
    assert (cen["mc_clip"] > 0).all() and (cen["recon_clip"] > 0).all() and (cen["mc_bi_rails"] > 0).all(), (cen["mc_clip"].tolist(), cen["recon_clip"].tolist())


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("tools", [{"eipd": 1, "addb": 1}, {"eipd": 1, "addb": 1, "alf": 1, "htdf_qp": 27}, {"eipd": 1, "addb": 1, "htdf_qp": 40, "ibc_frac": 0.4}, {}],
                         ids=["eipd", "eipd_htdf_alf", "eipd_htdf_ibc", "base_modes"])
def test_gpu_all_intra_at_the_rails(tools, bd):
    """all-intra pictures whose residuals drive the reconstruction - the neighbours of the next CU - into both rails.  (What the current picture holds beforehand
    plays no part: every sample is written by a CU and unavailable neighbours come from the availability map.)"""
    ol.census_reset()
    for split in (0.2, 0.8):
        t = dict(tools, inter_frac=0.0, amp=40.0, coded_frac=0.9, split_prob=split, btt_frac=0.5 if tools else 0.0)
        if tools.get("alf"):
            t["extreme"] = {"alf": ("extreme", "on")}
        cs = cases.build_case("xm_intra", 136, 72, bd, 1 if tools else 0, 1 if tools else 0, (1, 0), 0.0, t, seed=int(split * 10))
        _check(cs, f"all-intra {sorted(tools)} {bd} bit split {split}", resid=True)
    cen = ol.census()
    assert min(cen["recon_clip"]) * 200 >= cen["recon_coded"] > 0, (cen["recon_clip"].tolist(), cen["recon_coded"])      # each rail in >= 0.5 % of the coded samples


# 5 of the 25 pairs of {-12, -6, 0, 6, 12}^2, a choice: every value occurs for alpha and for beta, with both signs against each other
OFFSETS = [(-12, 12), (-6, -6), (0, 0), (6, -12), (12, 6)]
# XEVD_HIP_ADDB_SCALAR selects the line filters of k_addb_alf only (k_addb alone has one form), and above 10 bit the scalar form is the default: only the
# combinations that differ exist
ADDB_SWEEP = [(bd, alf, 0) for bd in (8, 10, 12) for alf in (0, 1)] + [(bd, 1, 1) for bd in (8, 10)]


@pytest.mark.parametrize("bd,alf,scalar", ADDB_SWEEP, ids=[f"{bd}b-{'k_addb_alf' if alf else 'k_addb'}-{'scalar' if sc else 'default'}" for bd, alf, sc in ADDB_SWEEP])
def test_gpu_addb_offsets_qp_sweep(bd, alf, scalar, monkeypatch):
    """QP 0..51 per CU x slice offsets on the step ladder and on full-range noise, 136x136 (an interior filter tile exists), ALF fused behind the filter or not"""
    if scalar:
        monkeypatch.setenv("XEVD_HIP_ADDB_SCALAR", "1")
    ol.census_reset()
    for n, (ao, bo) in enumerate(OFFSETS):
        for content in (["ladder", "rails_dither"], ["noise", "ladder"]):
            t = {"addb": 1, "alf": alf, "inter_frac": 0.7, "qp_range": (0, 51), "coded_frac": 0.5, "split_prob": 0.7, "alpha_off": ao, "beta_off": bo,
                 "extreme": {"content": content, "qp": "areas", "mv": "grid8", "alf": ("extreme", "on")}}
            cs = cases.build_case("xm_addb", 136, 136, bd, 1, 1, (2, 2), 0.5, t, seed=n)
            _check(cs, f"ADDB offsets ({ao}, {bo}) {bd} bit {content[0]} alf {alf} scalar {scalar}")
    cen = ol.census()      # over the sweep: the top of both tables on both planes, every bS filtered and skipped, strong and weak, all (ap, aq), the beta wrap at 12 bit
    assert (cen["addb_index_a"][:, 51] > 0).all() and (cen["addb_index_b"][:, 51] > 0).all() and (cen["addb_index_a"][0, 46:] > 0).all()
    assert (cen["addb_gate"][:, 1:5] > 0).all() and (cen["addb_bs4"] > 0).all() and (cen["addb_apq"] > 0).all() and (cen["addb_d0"] > 0).all(), cen["addb_gate"].tolist()
    assert (cen["addb_lost"][0] > 0) == (bd == 12)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("content", ["gratings", "noise", "checker2"])
def test_gpu_alf_parameter_kinds(content, bd):
    """coefficient kinds x CTB flag kinds x enables, CTU 64 and 128"""
    kinds = [("extreme", "on", (1, 1, 1)), ("extreme", "checker", (1, 1, 1)), ("single", "on", (1, 1, 1)), ("smooth", "on", (1, 1, 1)), ("single", "off", (1, 1, 1)),
             ("extreme", "on", (1, 0, 0)), ("single", "checker", (0, 1, 1))]
    ol.census_reset()
    for n, (kind, ctb, enable) in enumerate(kinds):
        for log2_ctu in ((6, 7) if n < 3 else ((6, 7)[n & 1],)):
            t = {"alf": 1, "addb": n & 1, "no_deblock": 1 - (n & 1), "alf_enable": enable, "inter_frac": 1.0, "coded_frac": 0.2, "log2_ctu": log2_ctu, "split_prob": 0.4,
                 "extreme": {"content": content, "mv": "grid8" if content == "gratings" else "small", "alf": (kind, ctb)}}
            cs = cases.build_case("xm_alf", 264, 136, bd, 1, 1, (1, 1), 0.3, t, seed=n)
            _check(cs, f"ALF {kind} flags {ctb} enable {enable} CTU {1 << log2_ctu} {content} {bd} bit")
    cen = ol.census()
    assert (cen["alf_clip"] > 0).all() and (cen["alf_tr"] > 0).all(), cen["alf_clip"].tolist()
    if content == "gratings":
        assert (cen["alf_class"] > 0).all(), cen["alf_class"].tolist()


def test_gpu_mv_thresholds_wide_picture():
    """the MV-clip thresholds at a width of 2112 (33 regions a row: the magic-division strip maps)"""
    t = {"addb": 1, "inter_frac": 1.0, "split_prob": 0.6, "extreme": {"content": ["noise", "checker2"], "mv": "thresholds"}}
    cs = cases.build_case("xm_mv_wide", 2112, 72, 8, 1, 1, (1, 1), 0.4, t)
    (ref, _, _, _), cen = run_oracle_with_census(cs)
    assert (cen["mv_clip"] > 0).all(), cen["mv_clip"].tolist()
    _same(cases.run_gpu(cs), ref, "2112x72 MV thresholds")


def test_gpu_rail_to_rail_1080p():
    """one full-size rail-to-rail picture (k_inter's region role on saturated windows, every filter tile of k_addb_alf on 0 / max checkerboards and noise)"""
    t = {"addb": 1, "alf": 1, "inter_frac": 1.0, "split_prob": 0.3, "extreme": {"content": ["checker1", "noise", "checker2", "rails_dither"], "mv": "small", "alf": ("extreme", "on")}}
    cs = cases.build_case("xm_1080p", 1920, 1080, 10, 1, 1, (2, 2), 0.5, t)
    (ref, _, _, _), cen = run_oracle_with_census(cs)
    assert (cen["mc_clip"] > 0).all() and (cen["alf_clip"] > 0).all(), (cen["mc_clip"].tolist(), cen["alf_clip"].tolist())
    _same(cases.run_gpu(cs), ref, "1920x1080 rail to rail")


@pytest.mark.parametrize("scalar", [0, 1], ids=["packed", "scalar"])
@pytest.mark.parametrize("spec", xi.TILE_CASES, ids=[s[0] for s in xi.TILE_CASES])
def test_gpu_tile_borders_inside_interior_filter_tiles(spec, scalar, monkeypatch):
    """uneven 2x2 / 3x2 tile grids whose CTU-aligned borders cross interior 64x64 filter tiles of k_addb_alf (the tile-border branch of
    addb_edge_strength_rt), loop_filter_across_tiles 0 and 1, packed and scalar line filters (at 12 bit both runs take the scalar ones), rail-to-rail content"""
    if scalar:
        monkeypatch.setenv("XEVD_HIP_ADDB_SCALAR", "1")
    cs = cases.build_case(*spec)
    (ref, _, _, rr), cen = run_oracle_with_census(cs)
    check_tile_census(spec, cs, cen)
    out, res = cases.run_gpu(cs, resid=True)
    assert np.array_equal(res[:len(rr)], rr), "residual arena"
    _same(out, ref, spec[0])
    _same(cases.run_gpu(cs, ahead=True), ref, spec[0] + " (ahead)")


@pytest.mark.parametrize("name", sorted(n for n, hit in TILED_STREAMS_REACHING_INTERIOR_BORDERS.items() if hit))
def test_gpu_tiled_golden_streams_scalar_deblocking(name, monkeypatch):
    """the committed tiled streams that reach the tile-border branch inside interior filter tiles (test_which_tiled_golden_streams_reach_the_tile_border_branch) are
    decoded with the packed filters by the stream tests; here with the scalar ones, against the pictures the reference decoder produced"""
    import os
    import golden_io
    import stream_util as su
    monkeypatch.setenv("XEVD_HIP_ADDB_SCALAR", "1")
    d = np.load(os.path.join(golden_io.GOLDEN, f"stream_{name}.npz"))
    got = su.decode_gpu(d["bytes"].tobytes())
    want = su.decode_oracle(d["bytes"].tobytes())
    assert len(got) == len(want)
    for k, (g, w_) in enumerate(zip(got, want)):
        for c in range(3):
            assert np.array_equal(g[c], w_[c]), f"picture {k} plane {c}: {np.argwhere(np.asarray(g[c]) != w_[c])[:4].tolist()}"
