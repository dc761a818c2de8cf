"""CPU suite of the coding side information (xgpu_frame_side_info): the host-only size function, the numpy restatement of the contract
(tests/side_info_ref.py) on hand-made records, and the restatement's reading of the map bits against the golden map_scu the reference wrote."""
import ctypes as C

import numpy as np
import pytest

import cases
import golden_io
import side_info_ref as sr
from xevd_amd import abi


def size(w, h, **kw):
    return abi.load().xgpu_side_info_size(C.byref(abi.make_side_format(**kw)), w, h)


# ------------------------------------------------------------------------------------------------ xgpu_side_info_size
def test_size_blocks():
    w, h = 200, 136
    ws, hs = w // 4, h // 4
    assert size(w, h) == 9 * hs * ws * 2
    assert size(w, h, row_pitch=128) == (9 * hs - 1) * 128 + ws * 2
    assert size(w, h, row_pitch=ws * 2) == 9 * hs * ws * 2
    assert size(7680, 4320) == 9 * 1080 * 1920 * 2


@pytest.mark.parametrize("dtype,es", [(abi.OUT_F16, 2), (abi.OUT_F32, 4)])
@pytest.mark.parametrize("lists,ch", [(1, 2), (2, 2), (3, 4)])
def test_size_flow(dtype, es, lists, ch):
    w, h = 200, 136
    assert size(w, h, layout=abi.SIDE_FLOW_PLANAR, dtype=dtype, lists=lists) == ch * h * w * es
    assert size(w, h, layout=abi.SIDE_FLOW_INTERLEAVED, dtype=dtype, lists=lists) == ch * h * w * es
    crop = (2, 6, 4, 10)
    cw, chh = w - 8, h - 14
    assert size(w, h, layout=abi.SIDE_FLOW_PLANAR, dtype=dtype, lists=lists, crop=crop) == ch * chh * cw * es
    assert size(w, h, layout=abi.SIDE_FLOW_PLANAR, dtype=dtype, lists=lists, crop=crop, row_pitch=1024) == (ch * chh - 1) * 1024 + cw * es
    assert size(w, h, layout=abi.SIDE_FLOW_INTERLEAVED, dtype=dtype, lists=lists, crop=crop, row_pitch=4096) == (chh - 1) * 4096 + ch * cw * es
    assert size(w, h, layout=abi.SIDE_FLOW_PLANAR, dtype=dtype, lists=lists, per_poc=True) == ch * h * w * es


def test_size_refusals():
    w, h = 200, 136
    flow = dict(layout=abi.SIDE_FLOW_PLANAR, dtype=abi.OUT_F16)
    assert size(w, h, **flow) > 0
    assert size(w, h, crop=(1, 0, 0, 0), **flow) == 0                        # odd crop
    assert size(w, h, crop=(0, 0, 0, 3), **flow) == 0
    assert size(w, h, crop=(-2, 0, 0, 0), **flow) == 0
    assert size(w, h, crop=(100, 100, 0, 0), **flow) == 0                    # nothing left
    assert size(w, h, crop=(2, 0, 0, 0)) == 0                                # crop on BLOCKS
    assert size(w, h, crop=(0, 0, 0, 4)) == 0
    for dt in (abi.OUT_F16, abi.OUT_F32, abi.OUT_BF16, abi.OUT_U8):
        assert size(w, h, dtype=dt) == 0                                     # BLOCKS is int16
    for dt in (abi.OUT_U8, abi.OUT_U16, abi.OUT_BF16, 7, -1):
        assert size(w, h, layout=abi.SIDE_FLOW_PLANAR, dtype=dt) == 0        # FLOW is F16 / F32
    for lists in (0, 4, -1):
        assert size(w, h, lists=lists, **flow) == 0
    assert size(w, h, per_poc=2, **flow) == 0
    assert size(w, h, layout=3, dtype=abi.OUT_F16) == 0
    assert size(w, h, row_pitch=w * 2 - 2, **flow) == 0                      # pitch below a row
    assert size(w, h, row_pitch=w * 2, **flow) > 0
    assert size(w, h, row_pitch=w // 4 * 2 - 2) == 0
    assert size(w, h, row_pitch=w * 4 + 2, layout=abi.SIDE_FLOW_PLANAR, dtype=abi.OUT_F32) == 0      # not a multiple of the element size
    assert size(w, h, row_pitch=w // 4 * 2 + 1) == 0
    for bad in ((204, 136), (200, 132), (0, 136), (200, -8), (202, 136)):    # sizes that are not multiples of 8
        assert size(*bad) == 0 and size(*bad, **flow) == 0
    assert abi.load().xgpu_side_info_size(None, w, h) == 0


# ------------------------------------------------------------------------------------------------ the restatement on hand-made records
def scu_word(intra=0, qp=30, skip=0, cbf=0, ibc=0, cod=1):
    return (intra << 15) | (qp << 16) | (skip << 23) | (cbf << 24) | (ibc << 26) | (cod << 31)


# refs: list 0 = POCs 4, 0, 7; list 1 = POCs 12, 16; the picture is POC 8 -> distances -4, -8, -1 / +4, +8
REFS = {(0, 0): 4, (1, 0): 0, (2, 0): 7, (0, 1): 12, (1, 1): 16}
POC = 8
# (map_scu, refi, mv [2][2], ats_inter, edge bits) of eight units in one row
HAND = [
    (scu_word(intra=1, qp=22, cbf=1), (-1, -1), ((0, 0), (0, 0)), 0, 3),                   # intra
    (scu_word(qp=35), (0, -1), ((5, -7), (99, 99)), 0, 1),                                 # inter, list 0 only: list 1's vector is not read
    (scu_word(qp=36, cbf=1), (-1, 1), ((3, 3), (-2051, 2050)), 0x11, 2),                   # inter, list 1 only, above 512 samples, ats_inter
    (scu_word(qp=37, skip=1), (1, 0), ((-9, 1), (2, -3)), 0, 0),                           # skip, both lists
    (scu_word(qp=38, ibc=1, cbf=1), (-1, -1), ((-16, -4), (0, 0)), 0, 3),                  # IBC: block vector in list 0, no reference
    (scu_word(qp=0), (2, 1), ((32767, -32768), (1, -1)), 0, 0),                            # the ends of the int16 range; distance -1
    (scu_word(qp=127, skip=1, cbf=1), (2, -1), ((0, 0), (0, 0)), 3, 1),                    # zero vector over a negative distance: -0.0 with per_poc
    (scu_word(qp=51), (1, 1), ((2053, -4101), (7, 10)), 0, 2),                             # F16 rounds 513.25 and -1025.25; 10 / 4 / 8 does not divide exactly
]


def hand_maps():
    scu = np.array([r[0] for r in HAND], np.uint32)
    refi = np.array([r[1] for r in HAND], np.int8)
    mv = np.array([r[2] for r in HAND], np.int16)
    ats = np.array([r[3] for r in HAND], np.uint8)
    edges = np.array([r[4] for r in HAND], np.uint8)
    return scu, refi, mv, ats, edges


def test_restatement_blocks_by_hand():
    scu, refi, mv, ats, edges = hand_maps()
    b = sr.blocks(scu, refi, mv, ats, edges, sr.refp_poc_table(REFS), POC, 8, 1)
    assert b.shape == (9, 1, 8) and b.dtype == np.int16
    b = b[:, 0]
    assert b[0].tolist() == [0, 5, 3, -9, -16, 32767, 0, 2053] and b[1].tolist() == [0, -7, 3, 1, -4, -32768, 0, -4101]
    assert b[2].tolist() == [0, 99, -2051, 2, 0, 1, 0, 7] and b[3].tolist() == [0, 99, 2050, -3, 0, -1, 0, 10]      # the record as it is
    assert b[4].tolist() == [0, -4, 0, -8, 0, -1, -1, -8]
    assert b[5].tolist() == [0, 0, 8, 4, 0, 8, 0, 8]
    assert b[6].tolist() == [0, 1, 1, 2, 6, 1, 2, 1]
    assert b[7].tolist() == [22, 35, 36, 37, 38, 0, 127, 51]
    assert b[8].tolist() == [1 | 2 | 4, 2, 1 | 4 | 8, 0, 1 | 2 | 4, 0, 1 | 2 | 8, 4]


def test_restatement_poc_saturation():
    scu, refi, mv, ats, edges = hand_maps()
    refs = dict(REFS)
    refs[(0, 0)], refs[(0, 1)] = -100000, 50000
    b = sr.blocks(scu, refi, mv, ats, edges, sr.refp_poc_table(refs), POC, 8, 1)[:, 0]
    assert b[4, 1] == -32768 and b[5, 3] == 32767
    # the flow divides by the unsaturated distance
    f = sr.flow(refi, mv, sr.refp_poc_table(refs), POC, 8, 1, lists=1, per_poc=True)
    assert f[0, 0, 4] == np.float32(5 * 0.25) / np.float32(-100008)


def test_restatement_flow_by_hand():
    scu, refi, mv, ats, edges = hand_maps()
    t = sr.refp_poc_table(REFS)
    f = sr.flow(refi, mv, t, POC, 8, 1, lists=3)
    assert f.shape == (4, 4, 32) and f.dtype == np.float32
    col = f[:, 0, ::4]                                                      # one pixel per unit
    assert col[0].tolist() == [0, 1.25, 0, -2.25, 0, 8191.75, 0, 513.25]
    assert col[1].tolist() == [0, -1.75, 0, 0.25, 0, -8192, 0, -1025.25]
    assert col[2].tolist() == [0, 0, -512.75, 0.5, 0, 0.25, 0, 1.75]        # unused lists, intra and IBC: +0.0
    assert col[3].tolist() == [0, 0, 512.5, -0.75, 0, -0.25, 0, 2.5]
    assert (np.signbit(f) == (f < 0)).all()                                 # no -0.0 without per_poc
    for r in range(4):
        for k in range(4):
            assert np.array_equal(f[:, r, k::4], f[:, 0, ::4])              # a unit's 16 pixels carry its value
    assert np.array_equal(sr.flow(refi, mv, t, POC, 8, 1, lists=1), f[:2]) and np.array_equal(sr.flow(refi, mv, t, POC, 8, 1, lists=2), f[2:])
    assert np.array_equal(sr.flow(refi, mv, t, POC, 8, 1, lists=3, interleaved=True), f.transpose(1, 2, 0))
    # F16: round to nearest even above 512 samples (spacing 0.5 in [512, 1024), 1 in [1024, 2048))
    h = sr.flow(refi, mv, t, POC, 8, 1, lists=3, dtype=np.float16)
    assert h.dtype == np.float16
    assert float(h[0, 0, 28]) == 513.0 and float(h[1, 0, 28]) == -1025.0 and float(h[2, 0, 8]) == -513.0 and float(h[3, 0, 8]) == 512.5
    assert float(h[0, 0, 20]) == 8192.0
    # per_poc: one float32 division by the distance
    p = sr.flow(refi, mv, t, POC, 8, 1, lists=3, per_poc=True)
    pc = p[:, 0, ::4]
    assert pc[0, 1] == np.float32(1.25) / np.float32(-4) and pc[2, 7] == np.float32(1.75) / np.float32(8)
    assert pc[3, 7] == np.float32(2.5) / np.float32(8) and pc[0, 7] == np.float32(513.25) / np.float32(-8)
    assert pc[0, 5] == np.float32(-8191.75) and pc[1, 3] == np.float32(0.25) / np.float32(-8)
    third = sr.flow(np.array([[0, -1]], np.int8), np.array([[[1, 0], [0, 0]]], np.int16), sr.refp_poc_table({(0, 0): 11}), POC, 1, 1, lists=1, per_poc=True)
    assert third[0, 0, 0] == np.float32(0.25) / np.float32(3) and float(third[0, 0, 0]) != 0.25 / 3      # does not divide exactly: rounded once, in float32
    assert pc[0, 6] == 0 and np.signbit(pc[0, 6]) and not np.signbit(pc[2, 6])      # 0 / -1 = -0.0; the unused list stays +0.0
    assert not np.signbit(pc[:, 0]).any() and not np.signbit(pc[:, 4]).any()      # intra, IBC: +0.0
    # crops: a multiple of 4 and not
    for crop in ((4, 8, 0, 0), (2, 6, 2, 0), (6, 2, 0, 2)):
        g = sr.flow(refi, mv, t, POC, 8, 1, lists=3, crop=crop)
        assert g.shape == (4, 4 - crop[2] - crop[3], 32 - crop[0] - crop[1])
        assert np.array_equal(g, f[:, crop[2]:4 - crop[3], crop[0]:32 - crop[1]])
    # the flow from the planes is the flow from the maps
    b = sr.blocks(scu, refi, mv, ats, edges, t, POC, 8, 1)
    for per_poc in (False, True):
        for dt in (np.float32, np.float16):
            a1 = sr.flow(refi, mv, t, POC, 8, 1, lists=3, per_poc=per_poc, dtype=dt, crop=(2, 2, 0, 2))
            a2 = sr.flow_from_blocks(b, b[4:6].astype(np.int64), lists=3, per_poc=per_poc, dtype=dt, crop=(2, 2, 0, 2))
            assert np.array_equal(sr.bits(a1), sr.bits(a2))


def test_restatement_edges():
    # a 128 x 32 CU has a transform border at x = 64; a chroma-only CU of a dual tree leaves the map alone
    batch = {"x": np.array([0, 128, 128, 128]), "y": np.array([0, 0, 0, 16]), "log2w": np.array([7, 4, 4, 4]), "log2h": np.array([5, 4, 4, 4]),
             "tree": np.array([0, 1, 2, 1])}
    e = sr.edge_bits(batch, 36, 8)
    assert (e[:, 0] & 1).all() and (e[:, 16] & 1).all() and not (e[:, 1:16] & 1).any() and not (e[:, 17:32] & 1).any()
    assert (e[0, :32] & 2).all() and not (e[1:, :32] & 2).any()
    assert (e[0, 32:36] == [3, 2, 2, 2]).all() and (e[4, 32:36] == [3, 2, 2, 2]).all() and (e[1:4, 32] == 1).all() and (e[1:4, 33:36] == 0).all()


# ------------------------------------------------------------------------------------------------ the bit reading against the reference's map_scu
@pytest.mark.parametrize("name", golden_io.PICTURE_CASES)
def test_restatement_reads_the_reference_map(name):
    """planes 6, 7 and bit 0 of plane 8, made from the ORACLE's maps, equal what the same bits of the golden map_scu - written by the reference
    (tests/golden/make_golden.py) - give: mode from MCU_GET_IF / MCU_GET_IBC / MCU_GET_SF, QP from MCU_GET_QP, luma cbf from MCU_GET_CBFL"""
    case, exp = golden_io.load_picture_case(name)
    _, _, maps, _ = cases.run_cpu("oracle", case, pad=False)
    refs = {k: p.poc for k, p in case["refs"].items()}
    b = sr.blocks_from_maps(maps, maps.map_scu, case["batch"], refs, cases.CUR_POC)
    g = exp["map_scu"].astype(np.uint32).reshape(maps.h_scu, maps.w_scu)
    mode = np.full(g.shape, sr.MODE_INTER, np.int16)
    mode[((g >> 23) & 1) == 1] = sr.MODE_SKIP
    mode[((g >> 26) & 1) == 1] = sr.MODE_IBC
    mode[((g >> 15) & 1) == 1] = sr.MODE_INTRA
    assert np.array_equal(b[6], mode)
    assert np.array_equal(b[7], ((g >> 16) & 0x7F).astype(np.int16))
    assert np.array_equal(b[8] & 1, ((g >> 24) & 1).astype(np.int16))
    # and the planes hang together: a unit without a reference has no distance, an intra unit no vector
    assert (b[4][maps.map_refi.reshape(g.shape + (2,))[:, :, 0] < 0] == 0).all() and (b[5][maps.map_refi.reshape(g.shape + (2,))[:, :, 1] < 0] == 0).all()
    assert (b[0:4, b[6] == sr.MODE_INTRA] == 0).all() and (b[4:6, (b[6] == sr.MODE_INTRA) | (b[6] == sr.MODE_IBC)] == 0).all()
    batch = case["batch"]
    modes_in = set(int(m) for m in np.unique(batch["pred_mode"]))
    assert set(int(m) for m in np.unique(b[6])) <= {1 if m == 3 else m for m in modes_in}
