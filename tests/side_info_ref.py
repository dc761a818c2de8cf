"""The contract of xgpu_frame_side_info (include/xevd_hip.h) restated in numpy: from the reference's maps (map_scu, map_refi,
map_mv, map_ats_inter), the CU-edge bits and the frame parameters (refp_poc, poc) to the nine BLOCKS planes, and from those to every FLOW form - float32
step by step, astype(float16) for F16.  Test infrastructure only."""
import numpy as np

MAX_REFS = 17
MODE_INTRA, MODE_INTER, MODE_SKIP, MODE_IBC = 0, 1, 2, 6


def refp_poc_table(refs):
    """{(idx, list): poc} -> [MAX_REFS][2] int64 (entries past a list: unused)"""
    t = np.zeros((MAX_REFS, 2), np.int64)
    for (i, l), poc in refs.items():
        t[i, l] = poc
    return t


def edge_bits(batch, w_scu, h_scu):
    """the two edge bits of every unit from the batch's CU rectangles by the rule of k_inter.hip: a unit's left (top) edge is a CU border or a 64-sample
    transform border inside a wider (taller) CU - ((x - cu_x) & 63) == 0.  Chroma-only CUs of a local dual tree (tree == 2) leave the map alone.
    -> uint8 [h_scu, w_scu], bit 0 left, bit 1 top"""
    e = np.zeros((h_scu, w_scu), np.uint8)
    tree = batch.get("tree")
    for i in range(len(batch["x"])):
        if tree is not None and tree[i] == 2:
            continue
        x, y, w, h = int(batch["x"][i]), int(batch["y"][i]), 1 << int(batch["log2w"][i]), 1 << int(batch["log2h"][i])
        xs = np.arange(x, x + w, 4)
        ys = np.arange(y, y + h, 4)
        le = (((xs - x) & 63) == 0).astype(np.uint8)
        te = (((ys - y) & 63) == 0).astype(np.uint8)
        e[y >> 2:(y + h) >> 2, x >> 2:(x + w) >> 2] = le[None, :] | (te[:, None] << 1)
    return e


def dpoc_planes(map_refi, refp_poc, poc):
    """unsaturated refp_poc[refi][list] - poc per unit and list, 0 where refi < 0 -> int64 [2][...]"""
    refi = np.asarray(map_refi).astype(np.int64)
    t = np.asarray(refp_poc, np.int64)
    out = []
    for l in range(2):
        r = refi[..., l]
        out.append(np.where(r >= 0, t[np.clip(r, 0, MAX_REFS - 1), l] - int(poc), 0))
    return np.stack(out)


def blocks(map_scu, map_refi, map_mv, map_ats, edges, refp_poc, poc, w_scu, h_scu):
    """-> int16 [9, h_scu, w_scu]"""
    scu = np.asarray(map_scu, np.uint32).reshape(h_scu, w_scu)
    refi = np.asarray(map_refi, np.int8).reshape(h_scu, w_scu, 2)
    mv = np.asarray(map_mv, np.int16).reshape(h_scu, w_scu, 2, 2)
    ats = np.asarray(map_ats).reshape(h_scu, w_scu)
    edges = np.asarray(edges, np.uint8).reshape(h_scu, w_scu)
    out = np.zeros((9, h_scu, w_scu), np.int16)
    out[0], out[1], out[2], out[3] = mv[:, :, 0, 0], mv[:, :, 0, 1], mv[:, :, 1, 0], mv[:, :, 1, 1]
    d = dpoc_planes(refi, refp_poc, poc)
    out[4], out[5] = np.clip(d[0], -32768, 32767), np.clip(d[1], -32768, 32767)
    intra, ibc, skip = (scu >> 15) & 1, (scu >> 26) & 1, (scu >> 23) & 1
    out[6] = np.where(intra == 1, MODE_INTRA, np.where(ibc == 1, MODE_IBC, np.where(skip == 1, MODE_SKIP, MODE_INTER)))
    out[7] = (scu >> 16) & 0x7F
    out[8] = ((scu >> 24) & 1) | ((edges & 1) << 1) | (((edges >> 1) & 1) << 2) | ((ats != 0).astype(np.uint32) << 3)
    return out


def blocks_from_maps(maps, map_scu, batch, refs, poc):
    """the BLOCKS planes of a picture from the oracle's maps (tests/oracle_lib.Maps after a run), the map_scu to read the bits from, the batch (edges) and
    {(idx, list): poc} of the references"""
    return blocks(map_scu, maps.map_refi, maps.map_mv, maps.map_ats, edge_bits(batch, maps.w_scu, maps.h_scu), refp_poc_table(refs), poc, maps.w_scu, maps.h_scu)


def flow(map_refi, map_mv, refp_poc, poc, w_scu, h_scu, lists=3, per_poc=False, crop=(0, 0, 0, 0), dtype=np.float32, interleaved=False):
    """the dense motion field: [C, H, W] (interleaved: [H, W, C]) of `dtype`, from the map's refi and vectors"""
    refi = np.asarray(map_refi, np.int8).reshape(h_scu, w_scu, 2)
    mv = np.asarray(map_mv, np.int16).reshape(h_scu, w_scu, 2, 2)
    d = dpoc_planes(refi, refp_poc, poc)
    chans = []
    for l in ([0], [1], [0, 1])[lists - 1]:
        used = refi[:, :, l] >= 0
        for k in range(2):
            v = mv[:, :, l, k].astype(np.float32) * np.float32(0.25)
            if per_poc:
                with np.errstate(divide="ignore", invalid="ignore"):
                    v = v / np.where(used, d[l], 1).astype(np.float32)      # one float32 division
            chans.append(np.where(used, v, np.float32(0.0)).astype(np.float32))
    unit = np.stack(chans)                                                   # [C, h_scu, w_scu]
    cl, cr, ct, cb = crop
    h, w = 4 * h_scu - ct - cb, 4 * w_scu - cl - cr
    uy = (np.arange(h) + ct) >> 2
    ux = (np.arange(w) + cl) >> 2
    out = unit[:, uy][:, :, ux].astype(dtype)
    return np.ascontiguousarray(out.transpose(1, 2, 0)) if interleaved else out


def flow_from_blocks(b, dpoc, lists=3, per_poc=False, crop=(0, 0, 0, 0), dtype=np.float32, interleaved=False):
    """the same from the nine planes; dpoc: the UNSATURATED distances [2, h_scu, w_scu] (planes 4 / 5 where nothing saturates).  A list is in use where its
    distance is not 0."""
    h_scu, w_scu = b.shape[1:]
    chans = []
    for l in ([0], [1], [0, 1])[lists - 1]:
        used = dpoc[l] != 0
        for k in range(2):
            v = b[2 * l + k].astype(np.float32) * np.float32(0.25)
            if per_poc:
                v = v / np.where(used, dpoc[l], 1).astype(np.float32)
            chans.append(np.where(used, v, np.float32(0.0)).astype(np.float32))
    unit = np.stack(chans)
    cl, cr, ct, cb = crop
    h, w = 4 * h_scu - ct - cb, 4 * w_scu - cl - cr
    out = unit[:, (np.arange(h) + ct) >> 2][:, :, (np.arange(w) + cl) >> 2].astype(dtype)
    return np.ascontiguousarray(out.transpose(1, 2, 0)) if interleaved else out


def bits(a):
    """the bit patterns of a float array (so that +0.0 and -0.0 compare unequal)"""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
