"""The launch side of the translational motion-compensation census: which of k_inter's own branches a batch reaches (xevd_amd/csrc/k_inter.hip; needs no GPU).

The oracle's census (mc_* of oracle/xevd_oracle.h) counts the arithmetic the reference has as well: tap rows, regimes, lists.  The kernel's branches are not the reference's:
it gives every 64x64 region of the picture one of three roles, fetches the windows of two of them in 16-byte aligned chunks of which a whole-sample component leaves some
out, and predicates single lanes of the third.  This module restates
  * the rule of inter_work_lists (xgpu_builder.hip) from the batch - `roles`: a 32x32 tile belongs to a CU if it lies wholly inside the CU and wholly inside the picture,
    a region if all four tiles belong to one CU, chroma-only tree CUs are ignored - and is held to the arrays the device is given (xgpu_test_inter_lists: `builder_lists`,
    tests/test_builder.py) at 1 and 4 builder threads;
  * the kernel's address arithmetic - `mvt` from the clip, px = 4 * window origin + mvt, mis = ((px >> 2) - 3) & 7, cmis = ((px >> 3) - 1) & 7, fx / fy / cfx / cfy from the
    UNCLIPPED vector - and which chunks `wanted()` asks for,
and counts (`census`).  Units: in the region and tile roles a work unit is one region / one tile and one list it is predicted from (after the identical-motion test); in the
split role a CU (with at least one lane in a split-role tile) and one list, or - lane_l, lane_c - a lane and one list.  Arrays per CU (role_lists, role_shape, role_tu,
role_cbf, role_skip) count a CU once per role it has a part in: a CU of 64x64 that ends in the ragged last columns of the picture has a tile-role part and split-role parts.
  role[3]                     units by role: 0 region, 1 tile, 2 split
  role_lists[3][4]            CUs using list 0 only / list 1 only / both / both collapsed to one by identical motion on equal POCs
  role_shape[3][6][6]         CUs by [log2w - 2][log2h - 2]
  win_l[2][8][2][2]           region / tile units by [mis][fx][fy];  win_c[2][8][2][2] by [cmis][cfx][cfy]
  second_list[2][2][2]        region / tile units with two lists by [list 0 fy][list 1 fy] (luma): list 1's window lands in the block whose left-out rows still hold list 0's
  lane_l[4][4], lane_c[4][4]  split-role lanes by [wave: H * 2 + V from the ballot over the lanes that run the list][lane: fx * 2 + fy]; a lane that filters makes its wave
                              filter, so only the nine cells with lane & ~wave == 0 exist
  mixed_wave[3]               split-role tiles holding lanes of more than one CU / of CUs predicted from one and from two lists / lanes that run no plain inter CU at all
                              (intra, IBC, affine or refined neighbours, outside the picture)
  partial_tile[2]             split-role tiles with a plain inter lane that the picture's right / bottom edge cuts;  partial_tile_big[2]: ... with lanes of a CU of at least 32x32 - a tile that CU
                              covers wholly as far as the picture goes, split-role only because the picture ends
  role_clip[3][4]             units whose vector the MV clip moved: left / right / top / bottom threshold
  role_edge[3][4]             units whose luma request reaches over the picture's left / right / top / bottom edge.  Region and tile role: the chunks asked for, so from the
                              first chunk's start - up to 7 samples left of the window - to the last chunk's end; split role: the CU's window
  role_tu[3][5][2], role_cbf[3][8], role_skip[3]
"""
import ctypes as C

import numpy as np

from xevd_amd import abi
from xevd_amd.abi import MODE_INTRA

WORK_REGION = 0x100      # XGPU_WORK_REGION
STRIP = 16               # XGPU_INTER_STRIP
NONE = 0xFFFFFFFF
CUR_POC = 8              # cases.CUR_POC (not imported: cases imports extreme_inputs)


def _tree(b):
    return b["tree"] if b.get("tree") is not None else np.zeros(len(b["x"]), np.uint8)


def region_order(w, h):
    """the 64x64 regions in the kernel's order: vertical strips STRIP regions wide, row by row inside a strip -> [(rx, ry)]"""
    rx_n, ry_n = (w + 63) >> 6, (h + 63) >> 6
    return [(rx, ry) for s0 in range(0, rx_n, STRIP) for ry in range(ry_n) for rx in range(s0, min(s0 + STRIP, rx_n))]


def roles(b, w, h):
    """inter_work_lists restated -> (work [n_regions], items [n_regions * 4]) as uint32"""
    tiles_x, tiles_y, full_x, full_y = (w + 31) >> 5, (h + 31) >> 5, w >> 5, h >> 5
    tcu = np.full((tiles_y, tiles_x), NONE, np.int64)
    tany = np.zeros((tiles_y, tiles_x), bool)
    tree = _tree(b)
    for i in range(len(b["x"])):
        if tree[i] == 2:
            continue
        x0, y0 = int(b["x"][i]), int(b["y"][i])
        x1, y1 = x0 + (1 << int(b["log2w"][i])), y0 + (1 << int(b["log2h"][i]))
        for ty in range(y0 >> 5, ((y1 - 1) >> 5) + 1):
            for tx in range(x0 >> 5, ((x1 - 1) >> 5) + 1):
                if tx < full_x and ty < full_y and (tx << 5) >= x0 and (tx << 5) + 32 <= x1 and (ty << 5) >= y0 and (ty << 5) + 32 <= y1:
                    tcu[ty, tx] = i
                else:
                    tany[ty, tx] = True
    work, items = [], []
    for rx, ry in region_order(w, h):
        tx, ty = 2 * rx, 2 * ry
        quad = [(tx + (q & 1), ty + (q >> 1)) for q in range(4)]
        own = [int(tcu[uy, ux]) if ux < tiles_x and uy < tiles_y else NONE for ux, uy in quad]
        if own[0] != NONE and own.count(own[0]) == 4:
            work.append(WORK_REGION)
            items += own
            continue
        kinds = 0
        for q, (ux, uy) in enumerate(quad):
            if own[q] != NONE:
                kinds |= 1 << (2 * q)
            elif ux < tiles_x and uy < tiles_y and tany[uy, ux]:
                kinds |= 2 << (2 * q)
        work.append(kinds)
        items += own
    return np.array(work, np.uint32), np.array(items, np.uint32)


def builder_lists(case, threads=1):
    """the same two arrays as the host builder leaves them for the device (xgpu_test_inter_lists: no device, no HIP call)"""
    lib = abi.load()
    sp = abi.make_seq_params(case["w"], case["h"], case["bd"], log2_ctu=case.get("log2_ctu", 6), iqt=case["iqt"], admvp=case["admvp"], addb=case.get("addb", 0),
                             alf=case.get("alf", 0), eipd=case.get("eipd", 0))
    cb, keep = abi.make_cu_batch(case["batch"])
    n = C.c_int(0)
    cap = ((case["w"] + 63) >> 6) * ((case["h"] + 63) >> 6)
    work, items = (C.c_uint32 * cap)(), (C.c_uint32 * (4 * cap))()
    rc = lib.xgpu_test_inter_lists(C.byref(sp), C.byref(cb), threads, work, items, cap, C.byref(n))
    assert rc == 0 and n.value == cap, (rc, n.value, cap)
    return np.ctypeslib.as_array(work).copy(), np.ctypeslib.as_array(items).copy()


def plain_cus(case):
    """per CU: (plain, mvs, mvt, use, kind) - `plain`: predicted by k_inter's translational path (inter, not IBC, not affine, not a DMVR candidate on POC-symmetric
    references); mvs: the vectors as coded; mvt: after the clip of xevd_mv_clip, as the kernel forms it (the s16 cast included); use[l]: list l is predicted from, after the
    identical-motion test; kind: the mc_lists bucket"""
    b, w, h = case["batch"], case["w"], case["h"]
    n = len(b["x"])
    poc = {k: p.poc for k, p in case["refs"].items()}
    aff, dm, tree = b.get("affine"), b.get("dmvr"), _tree(b)
    out = []
    for i in range(n):
        pm = int(b["pred_mode"][i])
        r = [int(b["refi"][i, 0]), int(b["refi"][i, 1])]
        cw, ch = 1 << int(b["log2w"][i]), 1 << int(b["log2h"][i])
        plain = pm != MODE_INTRA and pm != 6 and tree[i] != 2 and not (aff is not None and aff[i])
        mvs = [[int(b["mv"][i, l, 0]), int(b["mv"][i, l, 1])] for l in range(2)]
        qx, qy = int(b["x"][i]) << 2, int(b["y"][i]) << 2
        mvt, moved = [], []
        for l in range(2):
            mx, my = mvs[l]
            mv_ = [False] * 4
            if qx + mvs[l][0] < -512:
                mx, mv_[0] = -512 - qx, True
            if qy + mvs[l][1] < -512:
                my, mv_[2] = -512 - qy, True
            if qx + mvs[l][0] + 4 * cw - 4 > (w - 1 + 128) << 2:
                mx, mv_[1] = ((w - 1 + 128) << 2) - qx - 4 * cw + 4, True
            if qy + mvs[l][1] + 4 * ch - 4 > (h - 1 + 128) << 2:
                my, mv_[3] = ((h - 1 + 128) << 2) - qy - 4 * ch + 4, True
            mvt.append([((mx + 32768) & 0xFFFF) - 32768, ((my + 32768) & 0xFFFF) - 32768])
            moved.append(mv_)
        use = [r[0] >= 0, r[1] >= 0]
        kind = 2 if use[0] and use[1] else (0 if use[0] else 1)
        if plain and use[0] and use[1]:
            p0, p1 = poc[(r[0], 0)], poc[(r[1], 1)]
            if p0 == p1 and mvt[0] == mvt[1]:
                use[1], kind = False, 3
            if dm is not None and dm[i] and cw >= 8 and ch >= 8 and (CUR_POC - p0) * (CUR_POC - p1) < 0 and abs(CUR_POC - p0) == abs(CUR_POC - p1):
                plain = False
        if not (use[0] or use[1]):
            plain = False
        out.append((plain, mvs, mvt, use, kind, moved))
    return out


def _aligned_reach(px, py, fx, fy, size, w, h):
    """what request_luma asks for, against the picture: chunks k with 8 k + 8 > s0 and 8 k < s1 of rows that start at sample ((px >> 2) - 3) & ~7"""
    X, Y = px >> 2, py >> 2
    base, mis = (X - 3) & ~7, (X - 3) & 7
    s0, s1 = (mis, mis + size + 7) if fx else (mis + 3, mis + 3 + size)
    first, last = base + 8 * (s0 // 8), base + 8 * ((s1 + 7) // 8) - 1
    top, bottom = (Y - 3, Y + size + 3) if fy else (Y, Y + size - 1)
    return [first < 0, last >= w, top < 0, bottom >= h]


def census(case, work=None, items=None):
    b, w, h = case["batch"], case["w"], case["h"]
    if work is None:
        work, items = roles(b, w, h)
    cus = plain_cus(case)
    ws, hs = (w + 3) >> 2, (h + 3) >> 2
    owner = np.full((hs, ws), -1, np.int64)
    tree = _tree(b)
    for i in range(len(b["x"])):
        if tree[i] != 2:
            owner[int(b["y"][i]) >> 2:(int(b["y"][i]) + (1 << int(b["log2h"][i]))) >> 2, int(b["x"][i]) >> 2:(int(b["x"][i]) + (1 << int(b["log2w"][i]))) >> 2] = i
    z = lambda *s: np.zeros(s, np.int64)
    cen = {"role": z(3), "role_lists": z(3, 4), "role_shape": z(3, 6, 6), "win_l": z(2, 8, 2, 2), "win_c": z(2, 8, 2, 2), "second_list": z(2, 2, 2), "lane_l": z(4, 4),
           "lane_c": z(4, 4), "mixed_wave": z(3), "partial_tile": z(2), "partial_tile_big": z(2), "role_clip": z(3, 4), "role_edge": z(3, 4), "role_tu": z(3, 5, 2),
           "role_cbf": z(3, 8), "role_skip": z(3), "n_plain": 0, "lists": z(4)}
    in_role = [set(), set(), set()]
    for k, (rx, ry) in enumerate(region_order(w, h)):
        units = []
        if work[k] == WORK_REGION:
            units.append((0, int(items[4 * k]), rx << 6, ry << 6, 64))
        else:
            for q in range(4):
                kind = (int(work[k]) >> (2 * q)) & 3
                tx0, ty0 = (rx << 6) + ((q & 1) << 5), (ry << 6) + ((q >> 1) << 5)
                if kind == 1:
                    units.append((1, int(items[4 * k + q]), tx0, ty0, 32))
                elif kind == 2:
                    _split_tile(cen, b, cus, owner, tx0, ty0, w, h, in_role[2])
        for role, i, wx, wy, size in units:
            plain, mvs, mvt, use, kind, moved = cus[i]
            if not plain:
                continue
            in_role[role].add(i)
            fys = []
            for l in range(2):
                if not use[l]:
                    continue
                px, py = (wx << 2) + mvt[l][0], (wy << 2) + mvt[l][1]
                fx, fy, cfx, cfy = int(mvs[l][0] & 3 != 0), int(mvs[l][1] & 3 != 0), int(mvs[l][0] & 7 != 0), int(mvs[l][1] & 7 != 0)
                cen["role"][role] += 1
                cen["win_l"][role][((px >> 2) - 3) & 7][fx][fy] += 1
                cen["win_c"][role][((px >> 3) - 1) & 7][cfx][cfy] += 1
                cen["role_clip"][role] += moved[l]
                cen["role_edge"][role] += _aligned_reach(px, py, fx, fy, size, w, h)
                fys.append(fy)
            if len(fys) == 2:
                cen["second_list"][role][fys[0]][fys[1]] += 1
    ai_all = b.get("ats_inter")
    for role in range(3):
        for i in in_role[role]:
            plain, mvs, mvt, use, kind, moved = cus[i]
            ai = int(ai_all[i]) if ai_all is not None else 0
            cen["role_lists"][role][kind] += 1
            cen["role_shape"][role][int(b["log2w"][i]) - 2][int(b["log2h"][i]) - 2] += 1
            cen["role_tu"][role][ai & 15][(ai >> 4) & 1] += 1
            cen["role_cbf"][role][int(b["cbf"][i]) & 7] += 1
            cen["role_skip"][role] += int(b["pred_mode"][i]) == 2
            if role == 2:      # the split role's units: the CU and a list
                X0, Y0, cw, ch = int(b["x"][i]), int(b["y"][i]), 1 << int(b["log2w"][i]), 1 << int(b["log2h"][i])
                for l in range(2):
                    if not use[l]:
                        continue
                    X, Y = ((X0 << 2) + mvt[l][0]) >> 2, ((Y0 << 2) + mvt[l][1]) >> 2
                    fx, fy = mvs[l][0] & 3 != 0, mvs[l][1] & 3 != 0
                    cen["role"][2] += 1
                    cen["role_clip"][2] += moved[l]
                    cen["role_edge"][2] += [X - (3 if fx else 0) < 0, X + cw - 1 + (4 if fx else 0) >= w, Y - (3 if fy else 0) < 0, Y + ch - 1 + (4 if fy else 0) >= h]
    for i, (plain, mvs, mvt, use, kind, moved) in enumerate(cus):
        if plain:
            cen["n_plain"] += 1
            cen["lists"][kind] += 1
            assert any(i in s for s in in_role), f"plain inter CU {i} has no part in any role"
    return cen


def _split_tile(cen, b, cus, owner, tx0, ty0, w, h, seen):
    """one split-role tile = one wave, a lane per SCU: the ballots per list over the lanes that run it, the lanes by what they filter themselves"""
    lanes = []
    for ly in range(8):
        for lx in range(8):
            sx, sy = (tx0 >> 2) + lx, (ty0 >> 2) + ly
            i = int(owner[sy, sx]) if sx < owner.shape[1] and sy < owner.shape[0] else -1
            lanes.append(i if i >= 0 and cus[i][0] else -1)
    on = [i for i in lanes if i >= 0]
    if not on:      # nothing of a plain inter CU in it: k_inter predicts nothing here
        return
    big = any(b["log2w"][i] >= 5 and b["log2h"][i] >= 5 for i in on)
    cen["partial_tile"] += [int(tx0 + 32 > w), int(ty0 + 32 > h)]
    cen["partial_tile_big"] += [int(tx0 + 32 > w and big), int(ty0 + 32 > h and big)]
    seen.update(on)
    cen["mixed_wave"] += [len(set(on)) > 1, len({int(cus[i][3][0]) + int(cus[i][3][1]) for i in on}) > 1, len(on) < 64]
    for l in range(2):
        run = [i for i in on if cus[i][3][l]]
        if not run:
            continue
        f = [(int(cus[i][1][l][0] & 3 != 0), int(cus[i][1][l][1] & 3 != 0), int(cus[i][1][l][0] & 7 != 0), int(cus[i][1][l][1] & 7 != 0)) for i in run]
        wave_l = 2 * max(v[0] for v in f) + max(v[1] for v in f)
        wave_c = 2 * max(v[2] for v in f) + max(v[3] for v in f)
        for v in f:
            cen["lane_l"][wave_l][2 * v[0] + v[1]] += 1
            cen["lane_c"][wave_c][2 * v[2] + v[3]] += 1
