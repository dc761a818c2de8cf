"""GPU suite of the residual export (xgpu_batch_residual, k_residual.hip): the arena of a batch written out as picture-shaped planes, bit-exact against the
numpy restatement (tests/residual_ref.py) applied to the batch's arrays and the CPU ORACLE's arena - never to the arena the GPU produced."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import cases
import oracle_lib as ol
import residual_ref as rr
from xevd_amd import abi, stream

pytestmark = pytest.mark.gpu
INVALID = -101
NAMES = [s[0] for s in cases.CASES]


def spec_of(name):
    return next(s for s in cases.CASES if s[0] == name)


@functools.lru_cache(maxsize=None)
def built(name):
    """(case, [Y, Cb, Cr] of the restatement over the oracle's arena) - made once per case, read only"""
    case = cases.build_case(*spec_of(name))
    _, _, _, arena = cases.run_cpu("oracle", case, pad=False)
    return case, rr.planes(case["batch"], arena, case["w"], case["h"])


def open_decoder(case):
    from xevd_amd.decoder import XgpuDecoder
    return XgpuDecoder(case["w"], case["h"], case["bd"], log2_ctu=case.get("log2_ctu", 6), iqt=case["iqt"], admvp=case["admvp"],
                       addb=case.get("addb", 0), alf=case.get("alf", 0), eipd=case.get("eipd", 0), max_pics=8)


def start(dec, case, batch=None):
    slots, by_obj = {}, {}
    for key, pic in case["refs"].items():
        if id(pic) not in by_obj:
            by_obj[id(pic)] = dec.pic_alloc()
            dec.pic_upload_padded(by_obj[id(pic)], pic.bufs)
        slots[key] = (by_obj[id(pic)], pic.poc)
    cur = dec.pic_alloc()
    dec.pic_upload_padded(cur, cases._start_picture(case).bufs)
    return slots, cur, dec.batch_create(case["batch"] if batch is None else batch)


def decode(dec, case, slots, cur, hb, next_batch=None, filters=True):
    """cases.run_gpu's picture, the decoder left open"""
    dec.decode_picture(cur, cases.CUR_POC, slots, hb, deblock=filters and not case.get("no_deblock"), pad=True, qp_u_offset=cases.QP_OFFSETS[0],
                       qp_v_offset=cases.QP_OFFSETS[1], alpha_off=case.get("alpha_off", 0), beta_off=case.get("beta_off", 0),
                       alf=case.get("alf_params") if filters else None, next_batch=next_batch)


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    bad = np.argwhere(rr.bits(got) != rr.bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


# ------------------------------------------------------------------------------------------------ 1. YUV420 planes of every case
@pytest.mark.parametrize("name", NAMES)
def test_yuv420_every_case(name):
    case, want = built(name)
    with open_decoder(case) as dec:
        slots, cur, hb = start(dec, case)
        decode(dec, case, slots, cur, hb)
        flat, views = dec.batch_residual(hb)
        got, planes = flat.cpu().numpy(), [v.cpu().numpy() for v in views]
    assert got.dtype == np.int16
    for c in range(3):
        same(planes[c], want[c], f"{name}: plane {c}")
    same(got, rr.yuv420(want), name)


# ------------------------------------------------------------------------------------------------ 2. / 3. / 4. forms, energy, destinations on two pictures
FORM_CASES = ["main_btt_ctu128_8b", "main_atsinter_10b"]      # 264x200 (CUs above 64, a last group of 8 pixels in every row), 200x136


@pytest.fixture(scope="module")
def decoded():
    import torch
    out = {}
    for name in FORM_CASES:
        case, want = built(name)
        dec = open_decoder(case)
        slots, cur, hb = start(dec, case)
        decode(dec, case, slots, cur, hb)
        dec.sync()
        out[name] = {"dec": dec, "cur": cur, "hb": hb, "case": case, "want": want, "slots": slots}
    yield out, torch
    for v in out.values():
        v["dec"].close()


@pytest.mark.parametrize("dt", ["int16", "float16", "float32"])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("name", FORM_CASES)
def test_444_forms(decoded, name, channels_last, dt):
    pics, torch = decoded
    p = pics[name]
    got = p["dec"].batch_residual(p["hb"], kind="444", dtype=getattr(torch, dt), channels_last=channels_last).cpu().numpy()
    same(got, rr.f444(p["want"], p["case"]["bd"], p["case"]["bd"], dtype=np.dtype(dt), interleaved=channels_last), f"{name} {dt}")


@pytest.mark.parametrize("name", FORM_CASES)
def test_energy(decoded, name):
    pics, _ = decoded
    p = pics[name]
    got = p["dec"].batch_residual(p["hb"], kind="energy").cpu().numpy()
    want = rr.energy(p["want"])
    same(got, want, name)
    assert (want != 0).any(axis=(1, 2)).all() and want.max() <= 2 ** 19


def test_energy_against_the_cbf_bit_of_the_side_information(decoded):
    """an independent kernel: where a unit holds luma residual, bit 0 of plane 8 of XGPU_SIDE_BLOCKS (the map's luma cbf) is set.  On the picture with CTU 64:
    for a CU above 64 the map's bit is that of its FIRST 64x64 sub-block (xevd_util.c:1615), which says nothing about the other three"""
    pics, _ = decoded
    p = pics["main_atsinter_10b"]
    energy = p["dec"].batch_residual(p["hb"], kind="energy").cpu().numpy()
    flags = p["dec"].frame_side_info(p["cur"]).cpu().numpy()[8]
    assert (energy[0] != 0).sum() > 100
    assert ((flags & 1) == 1)[energy[0] != 0].all()


ES = {abi.OUT_U16: 2, abi.OUT_F16: 2, abi.OUT_F32: 4}
NP = {abi.OUT_U16: np.int16, abi.OUT_F16: np.float16, abi.OUT_F32: np.float32}


def rows_of(layout, want, pitch):
    """[(first element, row)] of a destination with `pitch` elements between rows"""
    if layout == abi.RESID_YUV420:
        h, w = want[0].shape
        rows = [(y * pitch, want[0][y]) for y in range(h)]
        rows += [(h * pitch + j * (pitch // 2), want[1][j]) for j in range(h // 2)]
        return rows + [(h * pitch + (h // 2) * (pitch // 2) + j * (pitch // 2), want[2][j]) for j in range(h // 2)]
    if layout == abi.RESID_444_INTERLEAVED:
        return [(y * pitch, want[y].reshape(-1)) for y in range(want.shape[0])]
    k, h, _ = want.shape
    return [((c * h + y) * pitch, want[c, y]) for c in range(k) for y in range(h)]


FORMS = [(abi.RESID_YUV420, abi.OUT_U16), (abi.RESID_444_PLANAR, abi.OUT_U16), (abi.RESID_444_PLANAR, abi.OUT_F16), (abi.RESID_444_INTERLEAVED, abi.OUT_F32),
         (abi.RESID_444_INTERLEAVED, abi.OUT_U16), (abi.RESID_ENERGY, abi.OUT_F32)]


# (6, 4, 2, 6): a left crop of 4k + 2 (the pixels of a lane reach into a third unit) and a width that is no multiple of 8 (a row's last group is short)
CROPS = [(2, 6, 4, 2), (0, 0, 0, 0), (6, 4, 2, 6)]
DESTINATIONS = [(layout, dtype, crop) for layout, dtype in FORMS for crop in (CROPS if layout != abi.RESID_ENERGY else CROPS[1:2])]      # ENERGY takes no crop


@pytest.mark.parametrize("layout,dtype,crop", DESTINATIONS)
@pytest.mark.parametrize("name", FORM_CASES)
def test_crops_pitches_and_odd_offsets(decoded, name, layout, dtype, crop):
    """tight and padded rows, aligned and offset by one element (the element-store path): the payload is the restatement's, every other byte of a
    sentinel-filled buffer keeps the sentinel"""
    pics, torch = decoded
    p = pics[name]
    case, planes = p["case"], p["want"]
    if layout == abi.RESID_ENERGY:
        want = rr.energy(planes)
        row = want.shape[2]
    elif layout == abi.RESID_YUV420:
        cl, cr, ct, cb = crop
        h, w = planes[0].shape
        want = [planes[0][ct:h - cb, cl:w - cr], planes[1][ct // 2:(h - cb) // 2, cl // 2:(w - cr) // 2], planes[2][ct // 2:(h - cb) // 2, cl // 2:(w - cr) // 2]]
        row = want[0].shape[1]
    else:
        want = rr.f444(planes, case["bd"], case["bd"], crop, NP[dtype], layout == abi.RESID_444_INTERLEAVED)
        row = want.shape[1] * 3 if layout == abi.RESID_444_INTERLEAVED else want.shape[2]
    es, npdt = ES[dtype], NP[dtype]
    tdt = {np.int16: torch.int16, np.float16: torch.float16, np.float32: torch.float32}[npdt]
    sentinel = 23130 if npdt == np.int16 else 77.0
    lib, ctx = p["dec"].lib, p["dec"].ctx
    for pitch, off in ((row, 0), (row + 6, 0), (row + 6, 1), (row, 1), (row + 8, 8)):
        fmt = abi.make_resid_format(layout, dtype, crop, pitch * es)
        need = lib.xgpu_resid_size(C.byref(fmt), case["w"], case["h"])
        assert need > 0 and need % es == 0
        buf = torch.full((off + need // es + 16,), sentinel, dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        assert lib.xgpu_batch_residual(ctx, p["hb"], C.byref(fmt), C.c_void_p(buf.data_ptr() + off * es), need, None) == 0, lib.xgpu_last_error(ctx)
        p["dec"].sync()
        expect = np.full(buf.shape[0], sentinel, npdt)
        for first, r in rows_of(layout, want, pitch):
            expect[off + first:off + first + len(r)] = r
        assert rows_of(layout, want, pitch)[-1][0] + row // (2 if layout == abi.RESID_YUV420 else 1) == need // es      # the last row ends the format's size
        same(buf.cpu().numpy(), expect, f"{name} layout {layout} dtype {dtype} crop {crop} pitch {pitch} offset {off}")


def test_tensor_arguments(decoded):
    """the Python entry: out= with padded rows, crops through the keyword, refusals of shapes and dtypes"""
    pics, torch = decoded
    p = pics["main_atsinter_10b"]
    dec, hb, case, planes = p["dec"], p["hb"], p["case"], p["want"]
    crop = (2, 6, 4, 2)
    w, h = case["w"] - 8, case["h"] - 6
    flat, (y, cb, cr) = dec.batch_residual(hb, crop=crop)
    assert flat.shape == (w * h * 3 // 2,) and y.shape == (h, w) and cb.shape == cr.shape == (h // 2, w // 2)
    same(flat.cpu().numpy(), rr.yuv420(planes, crop))
    buf = torch.full((3, h, w + 8), -7.0, dtype=torch.float16, device="cuda")
    out = buf[:, :, :w]
    assert dec.batch_residual(hb, kind="444", dtype=torch.float16, crop=crop, out=out) is out
    same(out.cpu().numpy(), rr.f444(planes, case["bd"], case["bd"], crop, np.float16))
    assert bool((buf[:, :, w:] == -7.0).all().item())
    for bad in (dict(kind="energy", crop=crop), dict(kind="yuv420", dtype=torch.float32), dict(kind="444", dtype=torch.uint8), dict(kind="planes"),
                dict(kind="444", crop=(1, 0, 0, 0)), dict(kind="444", out=torch.empty((3, h, w), dtype=torch.int16, device="cuda"))):
        with pytest.raises(ValueError):
            dec.batch_residual(hb, **bad)


# ------------------------------------------------------------------------------------------------ 5. a batch that covers half the picture
def test_partial_coverage():
    """only the CUs of the left half of the CTU columns: the units no CU of the batch covers (owner 0xFFFFFFFF) read 0 over a sentinel-filled destination, the
    covered half is what the whole batch gives"""
    import torch
    case, want = built("main_atsinter_10b")
    b = case["batch"]
    ctu = 1 << case.get("log2_ctu", 6)
    w_ctu, h_ctu = (case["w"] + ctu - 1) // ctu, (case["h"] + ctu - 1) // ctu
    edge = (w_ctu // 2) * ctu
    keep = b["x"].astype(int) < edge
    assert keep.any() and not keep.all() and ((b["x"].astype(int) + (1 << b["log2w"].astype(int)))[keep] <= edge).all()
    n = len(b["x"])
    part = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) and k not in ("coef", "ctu_cu_start") else v) for k, v in b.items()}
    part["ctu_cu_start"] = np.concatenate([[0], np.cumsum(keep)])[np.asarray(b["ctu_cu_start"], np.int64)].astype(np.uint32)
    assert len(part["ctu_cu_start"]) == w_ctu * h_ctu + 1 and part["ctu_cu_start"][-1] == keep.sum()
    expect = [p.copy() for p in want]
    expect[0][:, edge:] = 0
    expect[1][:, edge // 2:] = 0
    expect[2][:, edge // 2:] = 0
    assert all((p[:, :edge >> (c > 0)] != 0).any() for c, p in enumerate(expect))
    with open_decoder(case) as dec:
        slots, cur, hb = start(dec, case, part)
        decode(dec, case, slots, cur, hb, filters=False)
        out = torch.full((case["w"] * case["h"] * 3 // 2,), 23130, dtype=torch.int16, device="cuda")
        flat, _ = dec.batch_residual(hb, out=out)
        assert flat is out
        same(flat.cpu().numpy(), rr.yuv420(expect))
        e = torch.full((3, case["h"] // 4, case["w"] // 4), 77.0, dtype=torch.float32, device="cuda")
        same(dec.batch_residual(hb, kind="energy", out=e).cpu().numpy(), rr.energy(expect))


# ------------------------------------------------------------------------------------------------ 6. local dual trees, the player, the application
def oracle_stream_residuals(data):
    """our parser + the CPU oracle (the loop of test_gpu_side_info.oracle_stream_blocks), keeping every picture's arena:
    -> [(poc, [Y, Cb, Cr], chroma mask of the dual-tree blocks)] in decoding order"""
    o = ol.oracle()
    dpb, out = {}, []
    for p in stream.iter_stream(data):
        w, h, bd = p["width"], p["height"], p["bit_depth"]
        sp = abi.make_seq_params(w, h, bd, iqt=p["iqt"], admvp=p["admvp"], addb=p["addb"], alf=p["tool_alf"], eipd=p["eipd"])
        if p["chroma_qp_tables"] is not None:
            keep_tables = [np.ascontiguousarray(t, np.int8) for t in p["chroma_qp_tables"]]
            for i in range(2):
                sp.chroma_qp_table[i] = keep_tables[i].ctypes.data_as(C.POINTER(C.c_int8))
        b = p["batch"]
        cb, keep = abi.make_cu_batch(b)
        cur = ol.Picture(w, h, p["poc"])
        refs = {(i, l): dpb[poc] for l in range(2) for i, poc in enumerate(p["refs"][l])}
        fr = ol.make_frame(cur, refs, p["qp_u_offset"], p["qp_v_offset"])
        maps = ol.Maps(w, h)
        m = maps.orc()
        arena = np.zeros(max(len(b["coef"]), 1), np.int16)
        assert not p["n_dmvr_sub"]
        o.orc_recon_batch(C.byref(sp), C.byref(fr), C.byref(cb), C.byref(m), arena.ctypes.data_as(C.c_void_p))
        mask = np.zeros((h // 2, w // 2), bool)
        if b.get("tree") is not None:
            for i in np.nonzero(np.asarray(b["tree"]) == 2)[0]:
                x, y, cw, ch = int(b["x"][i]), int(b["y"][i]), 1 << int(b["log2w"][i]), 1 << int(b["log2h"][i])
                mask[y >> 1:(y + ch) >> 1, x >> 1:(x + cw) >> 1] = True
        out.append((p["poc"], rr.planes(b, arena, w, h), mask))
        if p["deblock_on"] and p["addb"]:
            o.orc_deblock_addb(C.byref(sp), C.byref(fr), C.byref(cb), C.byref(m), p["alpha_off"], p["beta_off"])
        elif p["deblock_on"]:
            o.orc_deblock_baseline(C.byref(sp), C.byref(fr), C.byref(cb), C.byref(m))
        if p["alf"] is not None:
            ap, keep_ap = abi.make_alf_params(p["alf"])
            o.orc_alf(C.byref(sp), C.byref(fr.cur), C.byref(ap))
        o.orc_pad(C.byref(sp), C.byref(fr.cur))
        if p["is_idr"]:
            dpb.clear()
        for poc in p["release"]:
            dpb.pop(poc, None)
        if p["is_ref"]:
            dpb[p["poc"]] = cur
    return out


def test_dual_tree_stream_player_and_application():
    import stream_util as su
    from xevd_amd.player import StreamDecoder
    data = su.make_stream(264, 200, 3, seed=11, main=True, btt=(2, 0, 0, 0), admvp=True, dual_tree=True, split_prob=0.7, inter_frac=0.6)
    want = oracle_stream_residuals(data)
    assert len(want) == 3
    assert any(m.any() and (pl[1][m] != 0).any() and (pl[2][m] != 0).any() for _, pl, m in want), "no chroma residual under a dual-tree block"
    got = []
    for p, planes in StreamDecoder(data).pictures(residual={}):
        assert planes is not None and len(planes) == 3      # the yielded tuple keeps its shape
        got.append((p["poc"], p["residual"]))
    assert [poc for poc, _ in got] == [poc for poc, _, _ in want]
    for (poc, (flat, views)), (_, pl, _) in zip(got, want):
        for c in range(3):
            same(views[c].cpu().numpy(), pl[c], f"POC {poc}: plane {c}")
        same(flat.cpu().numpy(), rr.yuv420(pl), f"POC {poc}")
    # the other forms run the chroma pass of their own layout
    forms = [(dict(kind="444", dtype="float16", channels_last=True), lambda pl: rr.f444(pl, 8, 8, dtype=np.float16, interleaved=True)),
             (dict(kind="444"), lambda pl: rr.f444(pl, 8, 8)), (dict(kind="energy"), rr.energy), (dict(crop=(2, 6, 4, 2)), lambda pl: rr.yuv420(pl, (2, 6, 4, 2)))]
    import torch
    for kw, ref in forms:
        kw = {k: (getattr(torch, v) if k == "dtype" else v) for k, v in kw.items()}
        for (p, _), (_, pl, _) in zip(StreamDecoder(data).output_order(residual=kw), sorted(want, key=lambda t: t[0])):
            r = p["residual"]
            same(r[0] if isinstance(r, tuple) else r, ref(pl), f"POC {p['poc']} {kw}")
    # tools/xevd_gpu_app.py --residual: the int16 planes, decoding order, after a text line per picture
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        fin, fres = os.path.join(td, "s.evc"), os.path.join(td, "s.resid")
        with open(fin, "wb") as f:
            f.write(data)
        subprocess.run([sys.executable, os.path.join(root, "tools", "xevd_gpu_app.py"), "-i", fin, "--residual", fres], check=True, timeout=300)
        raw = open(fres, "rb").read()
    assert raw == b"".join(f"{poc} 264 200\n".encode() + rr.yuv420(pl).astype("<i2").tobytes() for poc, pl, _ in want)


# ------------------------------------------------------------------------------------------------ 7. ordering
def test_side_stream_destroy_and_the_next_batch():
    """the residual taken on a stream of the caller's, the batch destroyed at once, the next batch created (it takes the block from the pool) and
    reconstructed, nothing synchronised in between: the first tensor still holds the first batch's residual"""
    import torch
    a_case, a_want = built("main_b_10b")
    b_case, b_want = built("main_addb_10b")      # same size and tools as far as the decoder is concerned, another batch
    assert a_case["w"] == b_case["w"] and a_case["h"] == b_case["h"] and not np.array_equal(a_want[0], b_want[0])
    with open_decoder(b_case) as dec:
        slots, cur, hb_a = start(dec, a_case)
        s = torch.cuda.Stream()
        for _ in range(3):
            decode(dec, a_case, slots, cur, hb_a, filters=False)
            with torch.cuda.stream(s):
                got_a, _ = dec.batch_residual(hb_a)
                got_e = dec.batch_residual(hb_a, kind="energy")
            dec.batch_destroy(hb_a)
            hb_b = dec.batch_create(b_case["batch"])
            decode(dec, b_case, slots, cur, hb_b, filters=False)
            with torch.cuda.stream(s):
                got_b, _ = dec.batch_residual(hb_b, kind="yuv420")
            dec.batch_destroy(hb_b)
            hb_a = dec.batch_create(a_case["batch"])
        s.synchronize()
        dec.sync()
        same(got_a.cpu().numpy(), rr.yuv420(a_want))
        same(got_e.cpu().numpy(), rr.energy(a_want))
        same(got_b.cpu().numpy(), rr.yuv420(b_want))


def test_the_picture_is_the_same_with_and_without_the_export():
    import torch
    case, _ = built("main_btt_10b")
    pics = []
    for export in (False, True):
        with open_decoder(case) as dec:
            slots, cur, hb = start(dec, case)
            if export:
                dec.batch_prepare(hb)
                dec.batch_residual(hb, kind="444", dtype=torch.float32)
            decode(dec, case, slots, cur, hb)
            if export:
                with torch.cuda.stream(torch.cuda.Stream()):
                    dec.batch_residual(hb)
                    dec.batch_residual(hb, kind="energy")
            dec.sync()
            pics.append(dec.pic_download(cur))
    for a, b in zip(*pics):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 8. validity by entry point
def test_valid_after_prepare_and_as_next_of_recon_ahead():
    case, want = built("main_b_ctu128_intra_mix_8b")      # intra CUs with dependencies: the next batch's pass rides in the data-flow launch
    with open_decoder(case) as dec:
        slots, cur, hb = start(dec, case)
        hb2 = dec.batch_create(case["batch"])
        dec.batch_prepare(hb)
        early, _ = dec.batch_residual(hb)                  # after batch_prepare, before batch_recon
        dec.frame_begin(cur, cases.CUR_POC, slots, *cases.QP_OFFSETS, deblock_on=False, alf_on=False)
        dec.batch_recon(hb, next_batch=hb2)
        ahead, _ = dec.batch_residual(hb2)                 # hb2 rode as `next`
        ahead_e = dec.batch_residual(hb2, kind="energy")
        dec.pad()
        dec.frame_end()
        after, _ = dec.batch_residual(hb)
        dec.pic_upload_padded(cur, cases._start_picture(case).bufs)
        decode(dec, case, slots, cur, hb2, filters=False)
        after2, _ = dec.batch_residual(hb2)
        dec.sync()
        ref = rr.yuv420(want)
        for name, t in (("after prepare", early), ("as next", ahead), ("after recon", after), ("after recon of next", after2)):
            same(t.cpu().numpy(), ref, name)
        same(ahead_e.cpu().numpy(), rr.energy(want))


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_queue_nothing_and_the_next_call_works():
    import torch
    case, want = built("main_atsinter_10b")
    w, h = case["w"], case["h"]
    with open_decoder(case) as dec:
        lib, ctx = dec.lib, dec.ctx
        fmt = abi.make_resid_format()
        need = lib.xgpu_resid_size(C.byref(fmt), w, h)
        assert need == w * h * 3
        buf = torch.full((need // 2 + 64,), 0x5A5A, dtype=torch.int16, device="cuda")
        host = np.full(need // 2 + 64, 0x5A5A, np.int16)
        slots, cur, hb = start(dec, case)

        def call(ptr=None, size=None, f=fmt, stream=None, batch=None):
            return lib.xgpu_batch_residual(ctx, hb if batch is None else batch, C.byref(f), C.c_void_p(buf.data_ptr() if ptr is None else ptr),
                                           need if size is None else size, stream)

        def untouched():
            torch.cuda.synchronize()
            return bool((buf == 0x5A5A).all().item()) and bool((host == 0x5A5A).all())

        assert call() == INVALID and b"has not been queued" in lib.xgpu_last_error(ctx)      # a batch never queued
        with pytest.raises(Exception):
            dec.batch_residual(hb)
        decode(dec, case, slots, cur, hb)
        never = dec.batch_create(case["batch"])
        assert call(batch=never) == INVALID and b"has not been queued" in lib.xgpu_last_error(ctx)
        assert call(ptr=host.ctypes.data) == INVALID                                       # host pointer
        assert call(size=need - 2) == INVALID                                              # short buffer
        assert call(ptr=buf.data_ptr() + 1) == INVALID                                     # misaligned pointer
        f32 = abi.make_resid_format(abi.RESID_444_PLANAR, abi.OUT_F32)
        assert call(ptr=buf.data_ptr() + 2, size=10 ** 9, f=f32) == INVALID                # float32 at a 2-byte address
        # a destination the ALLOCATION does not hold, whatever dst_size claims: the check is made against the allocation the pointer lies in
        # (hipMemGetAddressRange), not against the claim.  The format is sized past the device's memory, so that no allocation can hold it: a torch tensor is a
        # piece of a larger segment of torch's caching allocator, and a format that merely outgrows the tensor may still fit that segment and is accepted.
        huge = abi.make_resid_format(abi.RESID_444_PLANAR, abi.OUT_F32, row_pitch=1 << 30)
        assert lib.xgpu_resid_size(C.byref(huge), w, h) == (3 * h - 1) * (1 << 30) + w * 4
        assert call(size=1 << 50, f=huge) == INVALID and b"device memory" in lib.xgpu_last_error(ctx)
        for bad in (abi.make_resid_format(crop=(1, 0, 0, 0)), abi.make_resid_format(crop=(0, 0, 0, 3)), abi.make_resid_format(crop=(100, 100, 0, 0)),
                    abi.make_resid_format(dtype=abi.OUT_F16), abi.make_resid_format(dtype=abi.OUT_F32), abi.make_resid_format(row_pitch=w * 2 - 4),
                    abi.make_resid_format(row_pitch=w * 2 + 2), abi.make_resid_format(abi.RESID_444_PLANAR, abi.OUT_U8),
                    abi.make_resid_format(abi.RESID_444_INTERLEAVED, abi.OUT_BF16), abi.make_resid_format(abi.RESID_444_PLANAR, abi.OUT_F32, row_pitch=w * 4 + 2),
                    abi.make_resid_format(abi.RESID_ENERGY, abi.OUT_F32, crop=(2, 0, 0, 0)), abi.make_resid_format(abi.RESID_ENERGY, abi.OUT_U16),
                    abi.make_resid_format(abi.RESID_ENERGY, abi.OUT_F16), abi.make_resid_format(4, abi.OUT_U16), abi.make_resid_format(-1, abi.OUT_U16)):
            assert call(size=10 ** 9, f=bad) == INVALID and b"invalid format" in lib.xgpu_last_error(ctx)
        assert lib.xgpu_batch_residual(ctx, hb, None, C.c_void_p(buf.data_ptr()), need, None) == INVALID
        assert lib.xgpu_batch_residual(ctx, hb, C.byref(fmt), None, need, None) == INVALID
        assert lib.xgpu_batch_residual(ctx, None, C.byref(fmt), C.c_void_p(buf.data_ptr()), need, None) == INVALID
        assert untouched()
        assert call() == 0                                                                 # ... and the next valid call works
        torch.cuda.synchronize()
        same(buf[:need // 2].cpu().numpy(), rr.yuv420(want))
        assert bool((buf[need // 2:] == 0x5A5A).all().item())
