"""GPU suite of the coding side information (xgpu_frame_side_info, k_side_info.hip): the SCU map of the picture decoded last, read back as nine int16
planes per 4x4 unit and as dense motion fields, bit-exact against the numpy restatement (tests/side_info_ref.py) fed with the CPU oracle's maps - the
first direct test of the map on the GPU (refi, vectors, affine sub-block vectors, DMVR under both filters, IBC block vectors)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import cases
import golden_io
import oracle_lib as ol
import side_info_ref as sr
from xevd_amd import abi, stream

pytestmark = pytest.mark.gpu
INVALID = -101


def open_decoder(case):
    from xevd_amd.decoder import XgpuDecoder
    return XgpuDecoder(case["w"], case["h"], case["bd"], log2_ctu=case.get("log2_ctu", 6), iqt=case["iqt"], admvp=case["admvp"],
                       addb=case.get("addb", 0), alf=case.get("alf", 0), eipd=case.get("eipd", 0), max_pics=8)


def upload_refs(dec, case):
    slots, by_obj = {}, {}
    for key, pic in case["refs"].items():
        if id(pic) not in by_obj:
            by_obj[id(pic)] = dec.pic_alloc()
            dec.pic_upload_padded(by_obj[id(pic)], pic.bufs)
        slots[key] = (by_obj[id(pic)], pic.poc)
    return slots


def decode(dec, case, slots, cur, hb):
    """cases.run_gpu's picture, the decoder left open"""
    dec.decode_picture(cur, cases.CUR_POC, slots, hb, deblock=not case.get("no_deblock"), pad=True, qp_u_offset=cases.QP_OFFSETS[0], qp_v_offset=cases.QP_OFFSETS[1],
                       alpha_off=case.get("alpha_off", 0), beta_off=case.get("beta_off", 0), alf=case.get("alf_params"))


def start(dec, case):
    slots = upload_refs(dec, case)
    cur = dec.pic_alloc()
    dec.pic_upload_padded(cur, cases._start_picture(case).bufs)
    return slots, cur, dec.batch_create(case["batch"])


def expected_blocks(case, map_scu=None):
    """the restatement over the oracle's map_refi / map_mv / map_ats and `map_scu` (None: the oracle's own)"""
    _, _, maps, _ = cases.run_cpu("oracle", case, pad=False)
    refs = {k: p.poc for k, p in case["refs"].items()}
    return sr.blocks_from_maps(maps, maps.map_scu if map_scu is None else map_scu, case["batch"], refs, cases.CUR_POC), maps, sr.refp_poc_table(refs)


PLANE_NAMES = ["mv0x", "mv0y", "mv1x", "mv1y", "dpoc0", "dpoc1", "mode", "qp", "flags"]


# ------------------------------------------------------------------------------------------------ BLOCKS, every picture golden
@pytest.mark.parametrize("name", golden_io.PICTURE_CASES)
def test_blocks_every_picture_golden(name):
    case, exp = golden_io.load_picture_case(name)
    want, maps, _ = expected_blocks(case, exp["map_scu"])
    with open_decoder(case) as dec:
        slots, cur, hb = start(dec, case)
        decode(dec, case, slots, cur, hb)
        got = dec.frame_side_info(cur).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.int16
    for p in range(9):
        bad = np.argwhere(got[p] != want[p])
        assert len(bad) == 0, f"{name}: plane {p} ({PLANE_NAMES[p]}) differs at {len(bad)} units, first (row, col) {bad[0].tolist()}: {got[p][tuple(bad[0])]} != {want[p][tuple(bad[0])]}"


# ------------------------------------------------------------------------------------------------ FLOW on a B picture with unequal POC distances
FLOW_CASE = "main_b_10b"      # references at POC 4, 0 / 12, 16 around POC 8: distances -4, -8, +4, +8


@pytest.fixture(scope="module")
def flow_picture():
    import torch
    case, exp = golden_io.load_picture_case(FLOW_CASE)
    _, maps, table = expected_blocks(case, exp["map_scu"])
    dec = open_decoder(case)
    slots, cur, hb = start(dec, case)
    decode(dec, case, slots, cur, hb)
    dec.sync()
    yield {"dec": dec, "cur": cur, "maps": maps, "table": table, "case": case, "torch": torch, "slots": slots, "hb": hb}
    dec.close()


def want_flow(fp, np_dtype, **kw):
    m = fp["maps"]
    return sr.flow(m.map_refi, m.map_mv, fp["table"], cases.CUR_POC, m.w_scu, m.h_scu, dtype=np_dtype, **kw)


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.argwhere(sr.bits(got) != sr.bits(want))
    assert len(bad) == 0, f"{len(bad)} elements differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("per_poc", [False, True])
@pytest.mark.parametrize("lists", ["both", 0, 1])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dt", ["float16", "float32"])
def test_flow_forms(flow_picture, dt, channels_last, lists, per_poc):
    fp = flow_picture
    torch = fp["torch"]
    got = fp["dec"].frame_side_info(fp["cur"], kind="flow", dtype=getattr(torch, dt), channels_last=channels_last, lists=lists, per_poc=per_poc).cpu().numpy()
    same_bits(got, want_flow(fp, np.dtype(dt), lists={"both": 3, 0: 1, 1: 2}[lists], per_poc=per_poc, interleaved=channels_last))
    assert np.isfinite(got.astype(np.float32)).all()


def test_flow_has_motion_in_both_lists(flow_picture):
    """the comparison above is not one of zeros: both lists carry vectors, at more than one POC distance"""
    fp = flow_picture
    m = fp["maps"]
    b = sr.blocks(m.map_scu, m.map_refi, m.map_mv, m.map_ats, np.zeros(m.w_scu * m.h_scu, np.uint8), fp["table"], cases.CUR_POC, m.w_scu, m.h_scu)
    assert len(set(np.unique(b[4]).tolist()) - {0}) >= 2 and len(set(np.unique(b[5]).tolist()) - {0}) >= 2
    assert (b[0] != 0).any() and (b[3] != 0).any()


@pytest.mark.parametrize("crop", [(4, 8, 8, 4), (2, 6, 2, 10), (6, 2, 6, 2), (0, 2, 2, 0), (16, 0, 0, 30)])
@pytest.mark.parametrize("channels_last", [False, True])
def test_flow_crops(flow_picture, crop, channels_last):
    fp = flow_picture
    torch = fp["torch"]
    for dt in ("float16", "float32"):
        got = fp["dec"].frame_side_info(fp["cur"], kind="flow", dtype=getattr(torch, dt), channels_last=channels_last, per_poc=True, crop=crop).cpu().numpy()
        same_bits(got, want_flow(fp, np.dtype(dt), lists=3, per_poc=True, crop=crop, interleaved=channels_last))


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dt", ["float16", "float32"])
def test_flow_padded_rows_and_odd_offset(flow_picture, dt, channels_last):
    """rows padded by the caller (row_pitch), and a destination at an odd element offset - the element-store path - give the values of the aligned one;
    the padding keeps its sentinel"""
    fp = flow_picture
    torch, dec = fp["torch"], fp["dec"]
    tdt = getattr(torch, dt)
    crop = (2, 4, 0, 2)
    w, h = fp["case"]["w"] - 6, fp["case"]["h"] - 2
    want = want_flow(fp, np.dtype(dt), lists=3, crop=crop, interleaved=channels_last)
    row = 4 * w if channels_last else w
    for pitch, off in ((row + 24, 0), (row + 3, 1), (row, 3)):
        rows = h if channels_last else 4 * h
        buf = torch.full((rows * pitch + off + 8,), 77.0, dtype=tdt, device="cuda")
        view = buf[off:off + rows * pitch].view(rows, pitch)[:, :row]
        out = view.view(h, w, 4) if channels_last else view.view(4, h, w)
        assert dec.frame_side_info(fp["cur"], kind="flow", dtype=tdt, channels_last=channels_last, crop=crop, out=out) is out
        same_bits(out.cpu().numpy(), want)
        full = buf.cpu().numpy()
        pad = np.ones(full.shape, bool)
        idx = off + (np.arange(rows)[:, None] * pitch + np.arange(row)[None, :])
        pad[idx.ravel()] = False
        assert (full[pad] == 77.0).all()


def test_blocks_padded_rows_and_odd_offset(flow_picture):
    fp = flow_picture
    torch, dec = fp["torch"], fp["dec"]
    hs, ws = fp["maps"].h_scu, fp["maps"].w_scu
    want = dec.frame_side_info(fp["cur"]).cpu().numpy()
    for pitch, off in ((ws + 6, 0), (ws + 1, 1), (ws, 5), (ws + 8, 8)):
        buf = torch.full((9 * hs * pitch + off + 8,), -12345, dtype=torch.int16, device="cuda")
        out = buf[off:off + 9 * hs * pitch].view(9, hs, pitch)[:, :, :ws]
        assert dec.frame_side_info(fp["cur"], out=out) is out
        assert np.array_equal(out.cpu().numpy(), want)
        full = buf.cpu().numpy()
        pad = np.ones(full.shape, bool)
        pad[(off + (np.arange(9 * hs)[:, None] * pitch + np.arange(ws)[None, :])).ravel()] = False
        assert (full[pad] == -12345).all()


# ------------------------------------------------------------------------------------------------ the reader disturbs nothing
def test_picture_output_is_the_same_before_and_after(flow_picture):
    fp = flow_picture
    dec, cur = fp["dec"], fp["cur"]
    before = dec.pic_output(cur)
    padded = dec.pic_download_padded(cur)
    dec.frame_side_info(cur)
    dec.frame_side_info(cur, kind="flow", per_poc=True, crop=(2, 0, 2, 0))
    dec.sync()
    assert np.array_equal(dec.pic_output(cur), before)
    for a, b in zip(dec.pic_download_padded(cur), padded):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ ordering against the next picture
def test_export_on_a_side_stream_is_ordered_against_the_next_picture():
    """picture A decoded and exported on a stream of the caller's, picture B (other motion) decoded at once, nothing synchronised in between: A's tensors
    hold A's map, B's hold B's"""
    import torch
    a_case, a_exp = golden_io.load_picture_case(FLOW_CASE)
    b_case = dict(a_case)
    other = cases.build_case("side_info_other_motion", a_case["w"], a_case["h"], a_case["bd"], a_case["admvp"], a_case["iqt"], (2, 2), 0.5, seed=7)
    b_case["batch"] = other["batch"]
    want_a, maps_a, table = expected_blocks(a_case, a_exp["map_scu"])
    want_b, maps_b, _ = expected_blocks(b_case)
    assert not np.array_equal(want_a[:4], want_b[:4])
    flow_a = sr.flow(maps_a.map_refi, maps_a.map_mv, table, cases.CUR_POC, maps_a.w_scu, maps_a.h_scu, lists=3, per_poc=True, dtype=np.float32)
    with open_decoder(a_case) as dec:
        slots, cur_a, hb_a = start(dec, a_case)
        cur_b = dec.pic_alloc()
        dec.pic_upload_padded(cur_b, cases._start_picture(b_case).bufs)
        hb_b = dec.batch_create(b_case["batch"])
        s = torch.cuda.Stream()
        for _ in range(3):      # three rounds: the map is rewritten by B, then by A again
            decode(dec, a_case, slots, cur_a, hb_a)
            with torch.cuda.stream(s):
                got_a = dec.frame_side_info(cur_a)
                got_fa = dec.frame_side_info(cur_a, kind="flow", dtype=torch.float32, per_poc=True)
            decode(dec, b_case, slots, cur_b, hb_b)
            with torch.cuda.stream(s):
                got_b = dec.frame_side_info(cur_b)
        s.synchronize()
        dec.sync()
        assert np.array_equal(got_a.cpu().numpy(), want_a)
        same_bits(got_fa.cpu().numpy(), flow_a)
        assert np.array_equal(got_b.cpu().numpy(), want_b)


# ------------------------------------------------------------------------------------------------ refusals launch nothing
def test_refusals_launch_nothing_and_the_next_call_works():
    import torch
    case, exp = golden_io.load_picture_case(FLOW_CASE)
    want, _, _ = expected_blocks(case, exp["map_scu"])
    hs, ws = want.shape[1:]
    with open_decoder(case) as dec:
        lib, ctx = dec.lib, dec.ctx
        fmt = abi.make_side_format()
        need = lib.xgpu_side_info_size(C.byref(fmt), case["w"], case["h"])
        assert need == 9 * hs * ws * 2
        buf = torch.full((need // 2 + 64,), 0x5A5A, dtype=torch.int16, device="cuda")
        host = np.full(need // 2 + 64, 0x5A5A, np.int16)

        def call(pic, ptr=None, size=None, f=fmt, stream=None):
            return lib.xgpu_frame_side_info(ctx, pic, C.byref(f), C.c_void_p(buf.data_ptr() if ptr is None else ptr), need if size is None else size, stream)

        def untouched():
            torch.cuda.synchronize()
            return bool((buf == 0x5A5A).all().item()) and bool((host == 0x5A5A).all())

        slots, cur, hb = start(dec, case)
        assert call(cur) == INVALID and b"no picture yet" in lib.xgpu_last_error(ctx)      # before the first picture
        dec.frame_begin(cur, cases.CUR_POC, slots, *cases.QP_OFFSETS, deblock_on=not case.get("no_deblock"), alf_on=case.get("alf_params") is not None,
                        alpha_off=case.get("alpha_off", 0), beta_off=case.get("beta_off", 0))
        assert call(cur) == INVALID and b"a frame is open" in lib.xgpu_last_error(ctx)      # inside an open frame
        dec.batch_recon(hb)
        if not case.get("no_deblock"):
            dec.deblock()
        if case.get("alf_params") is not None:
            dec.alf(case["alf_params"])
        dec.pad()
        assert call(cur) == INVALID
        dec.frame_end()
        other = slots[(0, 0)][0]
        assert other != cur and call(other) == INVALID and b"another slot" in lib.xgpu_last_error(ctx)      # wrong slot
        assert call(99) == INVALID and call(-1) == INVALID
        assert call(cur, ptr=host.ctypes.data) == INVALID                                    # host pointer
        assert call(cur, size=need - 2) == INVALID                                           # short buffer
        assert call(cur, ptr=buf.data_ptr() + 1) == INVALID                                  # misaligned pointer
        ff = abi.make_side_format(abi.SIDE_FLOW_PLANAR, abi.OUT_F32, lists=1)
        assert call(cur, ptr=buf.data_ptr() + 2, size=10 ** 9, f=ff) == INVALID              # float32 at a 2-byte address
        for bad in (abi.make_side_format(crop=(2, 0, 0, 0)), abi.make_side_format(dtype=abi.OUT_F16), abi.make_side_format(abi.SIDE_FLOW_PLANAR, abi.OUT_U16),
                    abi.make_side_format(abi.SIDE_FLOW_PLANAR, abi.OUT_F16, lists=0), abi.make_side_format(abi.SIDE_FLOW_PLANAR, abi.OUT_F16, crop=(1, 0, 0, 0)),
                    abi.make_side_format(row_pitch=ws * 2 - 2)):
            assert call(cur, size=10 ** 9, f=bad) == INVALID
        assert lib.xgpu_frame_side_info(ctx, cur, None, C.c_void_p(buf.data_ptr()), need, None) == INVALID
        assert lib.xgpu_frame_side_info(ctx, cur, C.byref(fmt), None, need, None) == INVALID
        assert untouched()
        assert call(cur) == 0                                                                # ... and the next valid call works
        torch.cuda.synchronize()
        assert np.array_equal(buf[:need // 2].cpu().numpy().reshape(9, hs, ws), want)
        assert bool((buf[need // 2:] == 0x5A5A).all().item())
        # a frame that did not run the filters it announced ends with an error and records nothing
        dec.frame_begin(cur, cases.CUR_POC, slots, deblock_on=False, alf_on=True)
        dec.batch_recon(hb)
        assert lib.xgpu_frame_end(ctx) == -105
        assert call(cur) == INVALID and b"no picture yet" in lib.xgpu_last_error(ctx)
        with pytest.raises(Exception):
            dec.frame_side_info(cur)


# ------------------------------------------------------------------------------------------------ the player and the application
def oracle_stream_blocks(data):
    """our parser + the CPU oracle (as stream_util.decode_oracle runs them), keeping every picture's maps: -> [(poc, BLOCKS planes)] in decoding order"""
    o = ol.oracle()
    dpb, out = {}, []
    for p in stream.iter_stream(data):
        w, h, bd = p["width"], p["height"], p["bit_depth"]
        sp = abi.make_seq_params(w, h, bd, iqt=p["iqt"], admvp=p["admvp"], addb=p["addb"], alf=p["tool_alf"], eipd=p["eipd"])
        if p["chroma_qp_tables"] is not None:
            keep_tables = [np.ascontiguousarray(t, np.int8) for t in p["chroma_qp_tables"]]
            for i in range(2):
                sp.chroma_qp_table[i] = keep_tables[i].ctypes.data_as(C.POINTER(C.c_int8))
        cb, keep = abi.make_cu_batch(p["batch"])
        cur = ol.Picture(w, h, p["poc"])
        refs = {(i, l): dpb[poc] for l in range(2) for i, poc in enumerate(p["refs"][l])}
        fr = ol.make_frame(cur, refs, p["qp_u_offset"], p["qp_v_offset"])
        maps = ol.Maps(w, h)
        m = maps.orc()
        if p["n_dmvr_sub"]:
            dmv = np.zeros((p["n_dmvr_sub"], 2, 2), np.int16)
            o.orc_recon_batch_ex(C.byref(sp), C.byref(fr), C.byref(cb), C.byref(m), None, dmv.ctypes.data)
            p["dmvr_feedback"](dmv)
        else:
            o.orc_recon_batch(C.byref(sp), C.byref(fr), C.byref(cb), C.byref(m), None)
        out.append((p["poc"], sr.blocks_from_maps(maps, maps.map_scu, p["batch"], {k: pic.poc for k, pic in refs.items()}, p["poc"])))
        if p["deblock_on"] and p["addb"]:
            o.orc_deblock_addb(C.byref(sp), C.byref(fr), C.byref(cb), C.byref(m), p["alpha_off"], p["beta_off"])
        elif p["deblock_on"]:
            o.orc_deblock_baseline(C.byref(sp), C.byref(fr), C.byref(cb), C.byref(m))
        if p["alf"] is not None:
            ap, keep_ap = abi.make_alf_params(p["alf"])
            o.orc_alf(C.byref(sp), C.byref(fr.cur), C.byref(ap))
        o.orc_pad(C.byref(sp), C.byref(fr.cur))
        if p["needs_ref_luma"]:
            p["set_ref_luma"](p["poc"], cur.bufs[0], abi.PAD_L)
        if p["is_idr"]:
            dpb.clear()
        for poc in p["release"]:
            dpb.pop(poc, None)
        if p["is_ref"]:
            dpb[p["poc"]] = cur
    return out


@pytest.mark.parametrize("name", ["stream_hier_b_gop4.npz", "stream_main_dmvr_b_8b.npz"])
def test_player_side_info_and_application(name):
    from xevd_amd.player import StreamDecoder
    data = np.load(os.path.join(golden_io.GOLDEN, name))["bytes"].tobytes()
    want = oracle_stream_blocks(data)
    assert any((b[5] != 0).any() for _, b in want), "the stream has no B picture"
    got = []
    for p, planes in StreamDecoder(data).pictures(side={}):
        assert planes is not None and len(planes) == 3      # the yielded tuple keeps its shape
        got.append((p["poc"], p["side_info"]))
    assert [poc for poc, _ in got] == [poc for poc, _ in want]
    for (poc, t), (_, b) in zip(got, want):
        g = t.cpu().numpy()
        for k in range(9):
            assert np.array_equal(g[k], b[k]), f"POC {poc}: plane {k} ({PLANE_NAMES[k]})"
    # the flow of the player, with its defaults
    flows = [p["side_info"] for p, _ in StreamDecoder(data).pictures(download=False, side=dict(kind="flow", per_poc=True))]
    for f, (_, b) in zip(flows, want):
        same_bits(f.cpu().numpy(), sr.flow_from_blocks(b, b[4:6].astype(np.int64), lists=3, per_poc=True, dtype=np.float16))
    # tools/xevd_gpu_app.py --side-info: those planes, decoding order, after a text line per picture
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        fin, fside = os.path.join(td, "s.evc"), os.path.join(td, "s.side")
        with open(fin, "wb") as f:
            f.write(data)
        subprocess.run([sys.executable, os.path.join(root, "tools", "xevd_gpu_app.py"), "-i", fin, "--side-info", fside], check=True, timeout=300)
        raw = open(fside, "rb").read()
    expect = b"".join(f"{poc} {b.shape[1]} {b.shape[2]}\n".encode() + b.astype("<i2").tobytes() for poc, b in want)
    assert raw == expect
