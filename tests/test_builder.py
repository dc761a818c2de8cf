"""The host batch builder (xgpu_batch_create's host half) without a device: xgpu_test_build_batch builds the staging block of a batch in host memory and returns a digest
per array (CU records, CTU starts, TB records, itdq work items, intra records, dependency lists, affine tiles, control points, DMVR sub-blocks, owner map).
Pinned here: the arrays do not depend on the number of builder threads, and they equal the committed digests (tests/golden/builder_digests.json, written by this
file's --write with the builder whose staging blocks the GPU suite decodes bit-exactly: a refactoring of the builder must reproduce them byte for byte).  Further down the
test side's restatements of what the builder and the oracle decide (affine paths, the filter's skip condition, avail_lr of intra CUs) are held to the oracle's census, and the
restatement of k_inter's roles (tests/mc_launch.py) to the builder's own two arrays (xgpu_test_inter_lists)."""
import ctypes as C
import glob
import json
import os
import sys

import numpy as np
import pytest

import golden_io
from xevd_amd import abi, stream

GOLDEN_FILE = os.path.join(golden_io.GOLDEN, "builder_digests.json")


def _lib():
    lib = abi.load()
    lib.xgpu_test_build_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    lib.xgpu_test_build_batch.restype = C.c_int
    return lib


def _build(lib, sp, cb, threads):
    dg, info, ms = (C.c_uint64 * 13)(), (C.c_int * 8)(), C.c_double()
    rc = lib.xgpu_test_build_batch(C.byref(sp), C.byref(cb), threads, dg, info, C.byref(ms))
    assert rc == 0, rc
    # (the coefficient array is the caller's, sent from where it lies: digest 10 is empty; 11..13: the work lists of the three inter launches)
    h = [f"{int(v):016x}" for v in dg]
    return h[:10] + [int(v) for v in info] + h[11:13]


def picture_digests(lib, name, threads):
    case, _ = golden_io.load_picture_case(name)
    sp = abi.make_seq_params(case["w"], case["h"], case["bd"], log2_ctu=case["log2_ctu"], iqt=case["iqt"], admvp=case["admvp"], addb=case["addb"], alf=case["alf"], eipd=case["eipd"])
    cb, keep = abi.make_cu_batch(case["batch"])
    return _build(lib, sp, cb, threads)


def stream_digests(lib, path, threads):
    data = np.load(path)["bytes"].tobytes()
    out = []

    def consume(params, cbs):
        sp = abi.make_seq_params(params["width"], params["height"], params["bit_depth"], iqt=params["iqt"], admvp=params["admvp"], addb=params["addb"], alf=params["tool_alf"],
                                 eipd=params["eipd"], bit_depth_chroma=params["bit_depth_chroma"])
        out.append(_build(lib, sp, cbs, threads))
    for p in stream.iter_stream(data, consume_batch=consume):
        # streams with tool_dmvr expect the backend's refined vectors / decoded luma before the next picture: there is no backend here - fixed stand-ins (the
        # vectors of later pictures then differ from a real decode, deterministically: the builder's input is still a valid batch)
        if p["n_dmvr_sub"]:
            p["dmvr_feedback"](np.zeros((p["n_dmvr_sub"], 2, 2), np.int16))
        if p["needs_ref_luma"]:
            p["set_ref_luma"](p["poc"], np.full((p["height"] + 288, p["width"] + 288), 1 << (p["bit_depth"] - 1), np.int16), 144)
    return out


STREAMS = sorted(glob.glob(os.path.join(golden_io.GOLDEN, "stream_*.npz")))


@pytest.mark.parametrize("name", golden_io.PICTURE_CASES)
def test_builder_picture_cases(name):
    lib = _lib()
    want = json.load(open(GOLDEN_FILE))["pic_" + name]
    for threads in (1, 3):
        assert picture_digests(lib, name, threads) == want, f"{threads} builder thread(s)"


@pytest.mark.parametrize("path", STREAMS, ids=os.path.basename)
def test_builder_stream_pictures(path):
    lib = _lib()
    want = json.load(open(GOLDEN_FILE))[os.path.basename(path)]
    for threads in (1, 4):
        assert stream_digests(lib, path, threads) == want, f"{threads} builder thread(s)"


LARGE = (("intra1080", 1920, 1080, dict(inter_frac=0.0), {}), ("mix1080", 1920, 1080, dict(inter_frac=0.5, bi_frac=0.3, n_refs=(1, 1)), dict(admvp=1)),
         ("eipd4k", 3840, 2160, dict(inter_frac=0.2, eipd=True), dict(eipd=1)), ("htdf1080", 1920, 1080, dict(inter_frac=0.7, n_refs=(1, 0)), {}))


def large_digests(lib, case, threads):
    from xevd_amd import synth
    name, w, h, kw, spkw = case
    b = synth.gen_frame(np.random.default_rng(11), w, h, 10, coded_frac=0.6, qp_range=(22, 37), **kw)
    if name.startswith("htdf"):
        b["htdf_slice_qp"] = 32
    cb, keep = abi.make_cu_batch(b)
    return _build(lib, abi.make_seq_params(w, h, 10, **spkw), cb, threads)


@pytest.mark.parametrize("case", LARGE, ids=[c[0] for c in LARGE])
def test_builder_large_pictures_on_several_threads(case):
    """pictures with enough CUs and dependency nodes (14 k - 58 k) that every parallel section of the builder really runs on several threads: validation and counting,
    owner map, node construction, record scatter and dependency rewrite - same arrays whatever the thread count, equal to the committed digests"""
    lib = _lib()
    want = json.load(open(GOLDEN_FILE))["large_" + case[0]]
    for threads in (1, 4, 7):
        assert large_digests(lib, case, threads) == want, f"{threads} builder thread(s)"


def test_builder_rejects_invalid_batches_without_a_device():
    """the validation pass of the builder (geometry, reference indices, coefficient extents) answers before anything is allocated - also in the host-only shim"""
    lib = _lib()
    case, _ = golden_io.load_picture_case("base_p_8b")
    sp = abi.make_seq_params(case["w"], case["h"], case["bd"])
    for field, value in (("x", 60000), ("log2w", 9), ("coef_off", 1 << 30)):
        b = dict(case["batch"])
        b[field] = b[field].copy()
        b[field][len(b[field]) // 2] = value
        cb, keep = abi.make_cu_batch(b)
        dg, info, ms = (C.c_uint64 * 13)(), (C.c_int * 8)(), C.c_double()
        assert lib.xgpu_test_build_batch(C.byref(sp), C.byref(cb), 2, dg, info, C.byref(ms)) == -101, field


def test_builder_scratch_survives_refused_batches():
    """the working arrays a caller keeps between pictures after batches that are refused half way: on one calling thread, a picture pass 1 refuses (CU outside the
    picture), the same picture with an intra block copy CU whose source block is the CU itself (pass 1 accepts it, the dependency plan refuses it in its parallel
    mode: 14 244 CUs, three threads), then the unmodified picture - which must come out as the committed digests"""
    from xevd_amd import synth
    lib = _lib()
    name, w, h, kw, spkw = LARGE[0]
    want = json.load(open(GOLDEN_FILE))["large_" + name]
    b = synth.gen_frame(np.random.default_rng(11), w, h, 10, coded_frac=0.6, qp_range=(22, 37), **kw)
    n = len(b["x"])
    sp = abi.make_seq_params(w, h, 10, **spkw)

    def refused(bad):
        cb, keep = abi.make_cu_batch(bad)
        dg, info, ms = (C.c_uint64 * 13)(), (C.c_int * 8)(), C.c_double()
        return lib.xgpu_test_build_batch(C.byref(sp), C.byref(cb), threads, dg, info, C.byref(ms))
    for threads in (1, 4, 7):
        outside = dict(b)
        outside["x"] = b["x"].copy()
        outside["x"][n // 2] = 60000
        assert refused(outside) == -101, f"{threads} builder thread(s): pass 1"
        ibc = dict(b)
        ibc["pred_mode"], ibc["mv"] = b["pred_mode"].copy(), b["mv"].copy()
        ibc["pred_mode"][3 * n // 4] = abi.MODE_IBC
        ibc["mv"].reshape(n, 4)[3 * n // 4] = 0
        assert refused(ibc) == -101, f"{threads} builder thread(s): plan"
        cb, keep = abi.make_cu_batch(b)
        assert _build(lib, sp, cb, threads) == want, f"{threads} builder thread(s)"


if __name__ == "__main__" and "--write" in sys.argv:
    lib = _lib()
    out = {"pic_" + n: picture_digests(lib, n, 1) for n in golden_io.PICTURE_CASES}
    for p in STREAMS:
        out[os.path.basename(p)] = stream_digests(lib, p, 1)
    for c in LARGE:
        out["large_" + c[0]] = large_digests(lib, c, 1)
    json.dump(out, open(GOLDEN_FILE, "w"), indent=0)
    print(len(out), "entries")


@pytest.mark.parametrize("name", ["base_i_8b", "main_eipd_b_ctu128_constrained_10b", "main_btt_10b", "main_b_ctu128_intra_mix_8b"])
def test_builder_arbitrary_cu_order_inside_ctus(name):
    """The ORDER of a batch carries meaning (a neighbour counts as reconstructed when it comes earlier; with sps_suco_flag also right-hand neighbours): the CUs of every
    CTU in a random order - orders no split tree produces - must build the same arrays on 1 and 4 threads or be refused alike (a right-hand neighbour next to a CU with more
    than 32 units has no place in the record, an intra block copy source may come later), and never crash."""
    lib = _lib()
    case, _ = golden_io.load_picture_case(name)
    b = dict(case["batch"])
    rng = np.random.default_rng(5)
    start = np.asarray(b["ctu_cu_start"])
    perm = np.concatenate([rng.permutation(np.arange(start[k], start[k + 1])) for k in range(len(start) - 1)]).astype(np.int64)
    per_cu = {"x": 1, "y": 1, "log2w": 1, "log2h": 1, "pred_mode": 1, "refi": 2, "mv": 4, "qp": 3, "cbf": 1, "coef_off": 1, "ipm": 2, "ats": 1, "ats_inter": 1, "affine": 1,
              "affine_mv": 12, "dmvr": 1, "tree": 1, "cbf_sub": 1}
    n = len(b["x"])
    for k, width in per_cu.items():
        if b.get(k) is not None and hasattr(b[k], "shape") and b[k].size == n * width:
            b[k] = np.ascontiguousarray(np.asarray(b[k]).reshape(n, -1)[perm].reshape(np.asarray(b[k]).shape))
    sp = abi.make_seq_params(case["w"], case["h"], case["bd"], log2_ctu=case["log2_ctu"], iqt=case["iqt"], admvp=case["admvp"], addb=case["addb"], alf=case["alf"], eipd=case["eipd"])
    cb, keep = abi.make_cu_batch(b)
    out = []
    for threads in (1, 4):
        dg, info, ms = (C.c_uint64 * 13)(), (C.c_int * 8)(), C.c_double()
        rc = lib.xgpu_test_build_batch(C.byref(sp), C.byref(cb), threads, dg, info, C.byref(ms))
        out.append((rc, [int(v) for v in dg][:10] if rc == 0 else None))
    assert out[0] == out[1] and out[0][0] in (0, -101)


def test_builder_several_callers_at_once():
    """pictures built side by side (examples/evc_decode --builders, bench.py's end-to-end leg): four caller threads, each with its own pool of builder threads, inside
    the builder at the same time - every call returns the committed digests of its picture"""
    import threading
    from xevd_amd import synth
    lib = _lib()
    goldens = json.load(open(GOLDEN_FILE))
    jobs = []
    for case in LARGE[:2]:
        name, w, h, kw, spkw = case
        b = synth.gen_frame(np.random.default_rng(11), w, h, 10, coded_frac=0.6, qp_range=(22, 37), **kw)
        cb, keep = abi.make_cu_batch(b)
        jobs.append((goldens["large_" + name], abi.make_seq_params(w, h, 10, **spkw), cb, keep))
    errors = []

    def caller(k):
        try:
            for rep in range(4):
                want, sp, cb, _ = jobs[(k + rep) % len(jobs)]
                if _build(lib, sp, cb, 1 + k % 3) != want:
                    errors.append(f"caller {k}, call {rep}")
        except Exception as e:      # noqa: BLE001 - reported below
            errors.append(f"caller {k}: {e!r}")
    threads = [threading.Thread(target=caller, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_builder_survives_mutated_batches():
    """tests/tools/fuzz_builder.py (a process of its own: a crash must not take the suite along): picture goldens with a few elements of their arrays overwritten -
    out-of-range geometry, modes, reference indices, offsets - are built or refused, nothing else"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "fuzz_builder.py"), "5", "150"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and b"done:" in r.stdout, r.stdout.decode()[-800:]


@pytest.mark.parametrize("name", ["x_aff_sizes_10b", "x_aff_eif_checker_8b_noaddb"])
def test_builder_affine_tile_lists_follow_the_oracle_census(name):
    """The host sorts the affine CUs into the work lists of k_affine_eif and k_affine_sub with the header the kernels derive the path from (affine_model.h).  Held to the
    oracle here: the path of every CU by the test side's restatement of the model (extreme_inputs.aff_path), whose totals per path and CU shape must be the oracle's census;
    then the builder's tile list must be exactly the one that follows from those paths and the CU sizes - the EIF tiles of 16x16 first, then the translation tiles of 32x32,
    CUs in batch order, tiles row by row -, byte for byte (AffItem: CU index, control-point index, tile origin), on one and on three builder threads."""
    import cases
    import extreme_inputs as xi
    import oracle_lib as ol
    spec = next(s for s in xi.AFFINE_CASES if s[0] == name)
    cs = cases.build_case(*spec[:9])
    b = cs["batch"]
    ol.census_reset()
    cases.run_cpu("oracle", cs, deblock=False, pad=False)
    cen = ol.census()
    shape = np.zeros((2, 5, 5), np.int64)
    lists = ([], [])
    affine = np.nonzero(b["affine"])[0]
    for k, i in enumerate(affine):
        lw, lh = int(b["log2w"][i]), int(b["log2h"][i])
        _, _, eif, _ = xi.aff_path(b["affine_mv"].reshape(-1, 2, 3, 2)[i].astype(np.int64), [b["refi"][i, l] >= 0 for l in range(2)], lw, lh, int(b["affine"][i]))
        shape[0 if eif else 1, lw - 3, lh - 3] += 1
        step = 16 if eif else 32
        lists[0 if eif else 1].extend((i, k, tx, ty, 0) for ty in range(0, 1 << lh, step) for tx in range(0, 1 << lw, step))
    assert np.array_equal(shape, cen["aff_shape"]), "paths by the test side's model against the oracle's census"
    assert len(lists[0]) > 0 and len(lists[1]) > 0
    want = np.array(lists[0] + lists[1], dtype=[("cu", "<u4"), ("aff", "<u4"), ("tx", "<u2"), ("ty", "<u2"), ("pad", "<u4")]).tobytes()
    h = 1469598103934665603
    for byte in want:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    lib = _lib()
    sp = abi.make_seq_params(cs["w"], cs["h"], cs["bd"], log2_ctu=cs["log2_ctu"], iqt=cs["iqt"], admvp=cs["admvp"], addb=cs["addb"], alf=cs["alf"], eipd=cs["eipd"])
    cb, keep = abi.make_cu_batch(b)
    for threads in (1, 3):
        got = _build(lib, sp, cb, threads)
        assert got[10 + 7] == len(lists[0]) + len(lists[1]), "number of affine tiles"
        assert got[6] == f"{h:016x}", f"affine tile list, {threads} builder thread(s)"


def _htdf_ibc_specs():
    import extreme_inputs as xi
    return xi.HTDF_CASES + xi.IBC_CASES + xi.HTDF_TILE_CASES


@pytest.mark.parametrize("spec", _htdf_ibc_specs(), ids=[s[0] for s in _htdf_ibc_specs()])
def test_builder_htdf_ibc_nodes_follow_the_oracle_census(spec):
    """The builder accepts every HTDF / IBC case - right-to-left orders, block vectors whose sources must all precede their CU - on 1 and on 4 threads with equal arrays, and
    the length of k_intra's list is what the oracle's census says: the intra CUs, the IBC CUs and the inter CUs the filter runs on (the filter-only nodes).  An intra CU
    that is not filtered goes in as several parts (xgpu_intra_plan.hip, PartRule: one per 64 units of work, at most 16); in these cases those are the CUs with a side of
    128, the chroma-only ones and - at a slice QP of 17 - all of them."""
    import cases
    import extreme_inputs as xi
    import oracle_lib as ol
    from xevd_amd.abi import MODE_INTRA
    cs = cases.build_case(*spec[:9])
    b = cs["batch"]
    ol.census_reset()
    cases.run_cpu("oracle", cs, deblock=False, pad=False)
    cen = ol.census()
    filt = xi.htdf_filtered(b)
    intra, ibc = b["pred_mode"] == MODE_INTRA, b["pred_mode"] == 6
    # the test side's restatement of the skip condition against the census
    assert (filt & intra).sum() == cen["htdf_shape"][0].sum() and (filt & ~intra).sum() == cen["htdf_shape"][1].sum() and ibc.sum() == cen["ibc_shape"].sum()
    area = b["log2w"].astype(np.int64) + b["log2h"].astype(np.int64)
    parts = np.where(filt, 1, np.clip((1 << np.maximum(area - 4, 0)) * (4 if cs["eipd"] else 1) // 64, 1, 16))
    want = int(parts[intra].sum() + cen["ibc_shape"].sum() + cen["htdf_shape"][1].sum())
    lib = _lib()
    sp = abi.make_seq_params(cs["w"], cs["h"], cs["bd"], log2_ctu=cs["log2_ctu"], iqt=cs["iqt"], admvp=cs["admvp"], addb=cs["addb"], alf=cs["alf"], eipd=cs["eipd"])
    cb, keep = abi.make_cu_batch(b)
    one, four = _build(lib, sp, cb, 1), _build(lib, sp, cb, 4)
    assert one == four
    assert one[10 + 3] == want, (one[10:18], want)
    assert cen["ibc_shape"].sum() > 0 or not spec[8]["extreme"].get("ibc")


def _intra_specs():
    import extreme_inputs as xi
    return xi.INTRA_CASES + xi.INTRA_TILE_CASES


@pytest.mark.parametrize("spec", _intra_specs(), ids=[s[0] for s in _intra_specs()])
def test_builder_intra_modes_and_avail_lr_follow_the_oracle_census(spec):
    """extreme_inputs.intra_avail_lr - avail_lr of every CU from batch order and positions, the test side's restatement that set_intra_modes assigns modes with - held to the
    oracle: the CUs by [luma mode][avail_lr] and [chroma mode][avail_lr] (Baseline: by mode) counted from the batch are the oracle's census, bucket by bucket."""
    import cases
    import extreme_inputs as xi
    import oracle_lib as ol
    from xevd_amd.abi import MODE_INTRA
    cs = cases.build_case(*spec[:9])
    b = cs["batch"]
    ol.census_reset()
    cases.run_cpu("oracle", cs, deblock=False, pad=False)
    cen = ol.census()
    lr = xi.intra_avail_lr(b, cs["w"], cs["h"], cs["log2_ctu"])
    tree = b["tree"] if b.get("tree") is not None else np.zeros(len(lr), np.uint8)
    intra = b["pred_mode"] == MODE_INTRA
    luma, chroma = intra & (tree != 2), intra & (tree != 1)
    if cs["eipd"]:
        by_luma, by_chroma = np.zeros((33, 4), np.int64), np.zeros((5, 4), np.int64)
        np.add.at(by_luma, (b["ipm"][luma, 0], lr[luma]), 1)
        np.add.at(by_chroma, (b["ipm"][chroma, 1], lr[chroma]), 1)
        assert np.array_equal(by_luma, cen["ip_mode_lr"]) and np.array_equal(by_chroma, cen["ip_cmode_lr"])
        assert cen["ip_base_mode"].sum() == 0
    else:
        assert np.array_equal(np.bincount(b["ipm"][luma, 0], minlength=5), cen["ip_base_mode"][0]) and np.array_equal(np.bincount(b["ipm"][chroma, 1], minlength=5), cen["ip_base_mode"][1])
        assert cen["ip_mode_lr"].sum() == 0
    assert intra.sum() == cen["ip_shape"].sum() == cen["ip_tree"].sum() and (intra & (tree == 1)).sum() == cen["ip_tree"][1] and (intra & (tree == 2)).sum() == cen["ip_tree"][2]


def test_builder_intra_cases_cover_the_fused_instantiations():
    """k_intra_itdq<EIPD, IBC, IQT> - the data-flow intra launch with the next picture's residual pass riding along (xgpu_launch.hip: a next batch with coefficients, levels
    beyond the first, no HTDF nodes; k_intra.hip launch_intra: EIPD 2 with a reconstructed right column in an EIPD sequence - always with the copy path -, else 1 / 0 by the
    sequence, the copy path by the batch) - is taken by tests/test_gpu_extremes.py's runs of the intra cases with the residual pass ahead.  Which instantiation a case takes
    follows from the batch.  Of the ten (EIPD 0 / 1 x copies x IQT, EIPD 2 x IQT) the cases take the five asserted below: every value of EIPD, EIPD 0 and 1 each with and
    without copies, each transform at least once - IQT 0 only in the Baseline profile, without copies."""
    import cases
    import extreme_inputs as xi
    from xevd_amd.abi import MODE_INTRA
    lib, seen = _lib(), set()
    for spec in xi.INTRA_CASES:
        cs = cases.build_case(*spec[:9])
        b = cs["batch"]
        sp = abi.make_seq_params(cs["w"], cs["h"], cs["bd"], log2_ctu=cs["log2_ctu"], iqt=cs["iqt"], admvp=cs["admvp"], addb=cs["addb"], alf=cs["alf"], eipd=cs["eipd"])
        cb, keep = abi.make_cu_batch(b)
        got = _build(lib, sp, cb, 1)
        n_waves, n_intra, n_l1 = got[10 + 2], got[10 + 3], got[10 + 4]
        assert not b.get("htdf_slice_qp") and n_intra > n_l1 > 0, spec[0]
        if n_waves == 0:      # nothing for a residual pass to do: the plain launch (the case without coefficients)
            assert b["n_coef"] == 0 and spec[0] == "x_ip_eipd_rtl_nocoef_10b"
            continue
        right = bool((xi.intra_avail_lr(b, cs["w"], cs["h"], cs["log2_ctu"])[b["pred_mode"] == MODE_INTRA] & 2).any())
        ibc = bool((b["pred_mode"] == 6).any())
        seen.add((2, True, cs["iqt"]) if right and cs["eipd"] else (cs["eipd"], ibc, cs["iqt"]))
    assert seen >= {(2, True, 1), (1, False, 1), (1, True, 1), (0, False, 0), (0, True, 1)}, sorted(seen)


def test_builder_refuses_a_right_neighboured_cu_of_more_than_32_units():
    """An intra CU whose right-hand neighbour is reconstructed keeps the availability of its right column in the upper half of a 64-bit mask: w + h of at most 128 samples
    (32 units).  The reference never produces more: sps_suco_flag reverses the vertical cuts of nodes of at most 64x64 - xevdm_check_suco_cond: max(cuw, cuh) <= 1 <<
    min(log2 CTU - ..., 6), and a binary or ternary vertical cut only where cuw > cuh - so such a CU is at most 32 wide and 64 high.  A batch that holds a larger one (here
    the CTU of 128 cut into halves of 64x128, the right one first) is in an order no stream has, and the builder refuses it rather than decode it wrongly; the same
    halves left to right, and quarters of 64x64 right to left, are built."""
    from xevd_amd import synth
    lib = _lib()

    def build(xs, ys, lw, lh):
        part = (np.array(xs, np.uint16), np.array(ys, np.uint16), np.array(lw, np.uint8), np.array(lh, np.uint8), np.array([0, len(xs)], np.uint32))
        b = synth.gen_frame(np.random.default_rng(3), 128, 128, 10, log2_ctu=7, inter_frac=0.0, eipd=True, partition=part)
        cb, keep = abi.make_cu_batch(b)
        dg, info, ms = (C.c_uint64 * 13)(), (C.c_int * 8)(), C.c_double()
        return [lib.xgpu_test_build_batch(C.byref(abi.make_seq_params(128, 128, 10, log2_ctu=7, eipd=1)), C.byref(cb), t, dg, info, C.byref(ms)) for t in (1, 3)]
    assert build([64, 0], [0, 0], [6, 6], [7, 7]) == [-101, -101]
    assert build([0, 64], [0, 0], [6, 6], [7, 7]) == [0, 0]
    assert build([64, 0, 64, 0], [0, 0, 64, 64], [6, 6, 6, 6], [6, 6, 6, 6]) == [0, 0]


def test_builder_takes_a_cu_of_4x128():
    """No stream holds a CU of 1 : 32 (a binary cut must leave a ratio of at most 1 : 4, ALLOW_SPLIT_RATIO), but the builder checks sizes and positions, not ratios: a CTU
    of 128 cut into 32 columns of 4x128 is built.  The census buckets only such a CU fills (tests/test_oracle_extremes.py, check_intra_empty) are dead for streams, not for
    batches."""
    from xevd_amd import synth
    lib = _lib()
    n = 32
    part = (np.arange(n, dtype=np.uint16) * 4, np.zeros(n, np.uint16), np.full(n, 2, np.uint8), np.full(n, 7, np.uint8), np.array([0, n], np.uint32))
    for eipd in (0, 1):
        b = synth.gen_frame(np.random.default_rng(3), 128, 128, 10, log2_ctu=7, inter_frac=0.0, eipd=bool(eipd), partition=part)
        cb, keep = abi.make_cu_batch(b)
        assert _build(lib, abi.make_seq_params(128, 128, 10, log2_ctu=7, eipd=eipd), cb, 1)[10 + 3] == n * (2 if eipd else 1)      # (512 samples: two parts under EIPD, one under the Baseline predictors)


def _residual_specs():
    import extreme_inputs as xi
    return xi.RESIDUAL_CASES


@pytest.mark.parametrize("spec", _residual_specs(), ids=[s[0] for s in _residual_specs()])
def test_builder_residual_work_items_follow_the_oracle_census(spec):
    """The builder sorts the TBs by size class and transform pair and cuts each list into work items of itdq_group TBs.  Held to the oracle's per-TB census: the TBs
    through the ATS matrices by pair and shape (it_ats_shape), the others - DCT-II - as the rest of it_tb, give the number of TBs and, summed over class and pair,
    ceil(TBs / itdq_group) work items; and the test side's restatement of the TB walk (extreme_inputs.residual_tbs, which placed the levels) counts the same lists.  On one
    and on four builder threads, with identical digests."""
    import cases
    import extreme_inputs as xi
    import oracle_lib as ol
    import residual_inputs as ri
    cs = cases.build_case(*spec[:9])
    ol.census_reset()
    cases.run_cpu("oracle", cs, deblock=False, pad=False)
    cen = ol.census()
    ats = np.zeros((2, 2, 6, 6), np.int64)
    ats[:, :, 1:5, 1:5] = cen["it_ats_shape"]
    dct2 = cen["it_tb"].sum(0) - ats.sum((0, 1))
    assert (dct2 >= 0).all()
    items = sum(-(-int(n) // ri.itdq_group(lw + 1, lh + 1)) for lists in (dct2[None], ats.reshape(4, 6, 6)) for lst in lists for (lw, lh), n in np.ndenumerate(lst))
    walk = {}
    for (i, k, sb, tw, th, cl, off, tr, qp) in xi.residual_tbs(cs["batch"]):
        walk[(tw, th, tr)] = walk.get((tw, th, tr), 0) + 1
    for (tw, th, tr), n in walk.items():
        assert n == (dct2[tw - 1, th - 1] if tr == (0, 0) else ats[tr[0] - 1, tr[1] - 1, tw - 1, th - 1]), ("TBs of a class and pair: the test side's walk against the census", tw, th, tr)
    assert sum(walk.values()) == cen["it_tb"].sum()
    lib = _lib()
    sp = abi.make_seq_params(cs["w"], cs["h"], cs["bd"], log2_ctu=cs["log2_ctu"], iqt=cs["iqt"], admvp=cs["admvp"], addb=cs["addb"], alf=cs["alf"], eipd=cs["eipd"])
    cb, keep = abi.make_cu_batch(cs["batch"])
    one, four = _build(lib, sp, cb, 1), _build(lib, sp, cb, 4)
    assert one[10 + 1] == cen["it_tb"].sum(), "transform blocks"
    assert one[10 + 2] == items, "work items of the residual pass"
    assert one == four, "one and four builder threads"


# ---- k_inter's work arrays themselves (xgpu_test_inter_lists) against the test side's restatement of inter_work_lists (tests/mc_launch.py: roles), which the launch side of the
# motion-compensation census stands on: the motion-compensation cases, a picture with local dual trees in a tile grid (chroma-only CUs are ignored), and a picture of 65 regions
# a row (more than one strip)
def _role_specs():
    import extreme_inputs as xi
    return [s[:9] for s in xi.MC_CASES] + [s[:9] for s in xi.HTDF_TILE_CASES] + [xi.AFFINE_FAR_CASES[0][:9]] + [s[:9] for s in xi.EXTREME_CASES if s[0] in ("x_mc_checker2_base_b_8b", "x_htdf_qp32_cip_10b_ctu128")]


@pytest.mark.parametrize("spec", _role_specs(), ids=[s[0] for s in _role_specs()])
def test_inter_role_restatement_equals_the_builders_arrays(spec):
    import cases
    import mc_launch as ml
    cs = cases.build_case(*spec)
    work, items = ml.roles(cs["batch"], cs["w"], cs["h"])
    assert len(work) == ((cs["w"] + 63) >> 6) * ((cs["h"] + 63) >> 6) and len(items) == 4 * len(work)
    for threads in (1, 4):
        got_work, got_items = ml.builder_lists(cs, threads)
        assert np.array_equal(got_work, work), f"{threads} builder thread(s): roles of regions {np.nonzero(got_work != work)[0][:8].tolist()}"
        assert np.array_equal(got_items, items), f"{threads} builder thread(s): items {np.nonzero(got_items != items)[0][:8].tolist()}"
    # second check: digest 13 of xgpu_test_build_batch is the FNV-1a of the role array as it lies in the staging block
    sp = abi.make_seq_params(cs["w"], cs["h"], cs["bd"], log2_ctu=cs["log2_ctu"], iqt=cs["iqt"], admvp=cs["admvp"], addb=cs["addb"], alf=cs["alf"], eipd=cs["eipd"])
    cb, keep = abi.make_cu_batch(cs["batch"])
    h = 1469598103934665603
    for byte in work.astype("<u4").tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert _build(_lib(), sp, cb, 1)[-1] == f"{h:016x}"
    # and every role the kernel reads an item for has one: a region entry four times the same CU, a tile-role wave a CU, the others none
    for k, kinds in enumerate(work):
        own = items[4 * k:4 * k + 4]
        if kinds == ml.WORK_REGION:
            assert own[0] != ml.NONE and (own == own[0]).all()
        else:
            assert all((own[q] != ml.NONE) == (((int(kinds) >> (2 * q)) & 3) == 1) for q in range(4))


def test_inter_lists_shim_counts_and_refuses_too_little_room():
    """xgpu_test_inter_lists: both arrays NULL asks for the count alone; one alone, or room for fewer regions than the picture has, is an invalid argument and writes nothing"""
    import cases
    import extreme_inputs as xi
    cs = cases.build_case(*xi.MC_CASES[0][:9])
    lib = abi.load()
    sp = abi.make_seq_params(cs["w"], cs["h"], cs["bd"], log2_ctu=cs["log2_ctu"], iqt=cs["iqt"], admvp=cs["admvp"], addb=cs["addb"], alf=cs["alf"], eipd=cs["eipd"])
    cb, keep = abi.make_cu_batch(cs["batch"])
    n = C.c_int(0)
    regions = ((cs["w"] + 63) >> 6) * ((cs["h"] + 63) >> 6)
    assert lib.xgpu_test_inter_lists(C.byref(sp), C.byref(cb), 1, None, None, 0, C.byref(n)) == 0 and n.value == regions
    work, items = (C.c_uint32 * regions)(*([0xA5A5A5A5] * regions)), (C.c_uint32 * (4 * regions))(*([0xA5A5A5A5] * (4 * regions)))
    n.value = 0
    assert lib.xgpu_test_inter_lists(C.byref(sp), C.byref(cb), 1, work, items, regions - 1, C.byref(n)) == -101 and n.value == regions
    assert lib.xgpu_test_inter_lists(C.byref(sp), C.byref(cb), 1, work, None, regions, C.byref(n)) == -101
    assert all(v == 0xA5A5A5A5 for v in work) and all(v == 0xA5A5A5A5 for v in items)
