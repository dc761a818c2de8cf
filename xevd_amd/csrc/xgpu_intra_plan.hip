// xgpu_intra_plan.hip - the dependency plan of the order-dependent CUs of a batch (intra, IBC, HTDF): availability masks, dependency lists, levels, strands and
// parts -> the sorted record list of k_intra.hip.  Plain C++ (no kernel in this file); called by the batch builder (xgpu_builder.hip) with its caller's scratch object.
#include <chrono>
#include "xgpu_host.h"

// Intra CUs: availability masks, dependency lists and levels.  An SCU map of "CU index in decode order" stands in for the
// reference's COD flags: a neighbouring SCU is reconstructed at CU i's turn iff its CU index is below i (xevd_recon_unit
// sets COD CU by CU, xevd.c:744-754; xevd_get_avail_intra, xevd_util.c:689-745; single tile/slice).  The list is sorted by
// level (1 + the highest level among the intra CUs read), which is a topological order: every dependency sits earlier.
namespace {
const uint32_t NONE = 0xFFFFFFFFu;
// what the nodes of one picture are built from
struct NodeCtx {
    const xgpu_ctx *c; const xgpu_cu_batch *b;
    const uint32_t *owner, *luma_owner;      // SCU -> CU index: the caller's final map (parallel mode) or the one painted in step with the loop; constrained_tree: the luma CUs apart
    const int *level;                // by CU index; all zero while the parallel mode builds its nodes (the levels are assigned afterwards)
    const uint8_t *ctu_tile;         // tile of every CTU; NULL: one tile
    int ws, hs, ctu_sh; bool fast, constrained, constrained_tree;
    // tiles: a neighbour in another tile is not available (map_tidx[curr] == map_tidx[neighbour] in xevd_get_avail_intra, xevd_get_nbr_b, xevdm_get_nbr)
    int tile_of(int sx, int sy) const { return ctu_tile ? ctu_tile[(size_t)(sy >> ctu_sh) * c->w_ctu + (sx >> ctu_sh)] : 0; }
    int tree_of(int j) const { return b->tree ? b->tree[j] : 0; }      // local dual tree: 1 luma-only, 2 chroma-only CU
    uint32_t own(int sx, int sy) const { return owner[(size_t)sy * ws + sx]; }
};
// one CU on its way into the list: its record (a slot of the final list in the parallel mode, a temporary in the sequential one) and the list its dependencies go to
struct Node {
    IntraRec &r; std::vector<uint32_t> &deps; PlanOut &fl;
    const int i, xs, ys, my_tile, hidx;
    int lv; uint32_t last;           // the highest level among the CUs read (sequential mode); the dependency appended last (a neighbour over several SCUs is searched for once)
};
// append dependency j unless it is already in this record's list
inline void add_dep(Node &nd, uint32_t j) { if (std::find(nd.deps.begin() + nd.r.dep_first, nd.deps.end(), j) == nd.deps.end()) nd.deps.push_back(j); }
inline void add_dep_once(const NodeCtx &x, Node &nd, uint32_t j) { if (j != nd.last && plan_is_node(x.b, j)) { add_dep(nd, j); nd.last = j; } }

// the border samples the filter reads (xevdm_htdf, xevdm_recon.c:299-385) with the availability of xevd_get_avail_intra (xevd_util.c:689-745):
// "reconstructed" = earlier in decoding order
inline void add_htdf(const NodeCtx &x, Node &nd)
{
    const xgpu_cu_batch *b = x.b;
    const int i = nd.i, xs = nd.xs, ys = nd.ys, ws = x.ws, hs = x.hs, scuw = (1 << b->log2w[i]) >> 2, scuh = (1 << b->log2h[i]) >> 2;
    auto cod = [&](int sx, int sy) -> bool { return x.own(sx, sy) < (uint32_t)i && x.tile_of(sx, sy) == nd.my_tile; };
    auto dep = [&](int sx, int sy) {
        const uint32_t j = x.own(sx, sy);
        if (j >= (uint32_t)i) return;                       // not reconstructed yet: the reference reads what is there, so do we
        if (plan_is_node(b, j)) add_dep(nd, j);
        nd.lv = std::max(nd.lv, x.level[j]);
    };
    uint32_t av = 0;
    if (xs > 0 && cod(xs - 1, ys)) {
        av |= 1u << 1;
        if (ys + scuh + scuw - 1 < hs && cod(xs - 1, ys + scuh + scuw - 1)) av |= 1u << 7;
    }
    if (ys > 0) {
        if (x.tile_of(xs, ys - 1) == nd.my_tile) av |= 1u << 0;
        if (xs > 0 && cod(xs - 1, ys - 1)) av |= 1u << 5;
        if (xs + scuw < ws && cod(xs + scuw, ys - 1)) av |= 1u << 6;
    }
    if (xs + scuw < ws && cod(xs + scuw, ys)) {
        av |= 1u << 3;
        if (ys + scuh + scuw - 1 < hs && cod(xs + scuw, ys + scuh + scuw - 1)) av |= 1u << 8;
    }
    if (av & 2u)  for (int k = 0; k < scuh; k++) dep(xs - 1, ys + k);
    if (av & 1u)  for (int k = 0; k < scuw; k++) dep(xs + k, ys - 1);
    if (av & 8u)  for (int k = 0; k < scuh; k++) dep(xs + scuw, ys + k);
    if (av & 32u) dep(xs - 1, ys - 1);
    if (av & 64u) dep(xs + scuw, ys - 1);
    if ((av & 128u) && ys + scuh < hs) dep(xs - 1, ys + scuh);
    if ((av & 256u) && ys + scuh < hs) dep(xs + scuw, ys + scuh);
    nd.r.flags |= 4u | (av << 8) | ((uint32_t)nd.hidx << 20) | ((b->pred_mode[i] == XGPU_MODE_INTRA && x.constrained) ? 16u : 0u);
    nd.fl.htdf = true; nd.fl.ibc = true;                      // (ibc: the instantiation with the extra node kinds)
}
// an inter CU that is only here for its filter: k_inter / k_affine have reconstructed it, the node filters it in place
inline bool node_filter_only(const NodeCtx &x, Node &nd) { nd.r.cbf = 0; nd.r.ipm[0] = nd.r.ipm[1] = 0; nd.r.flags = 8u; add_htdf(x, nd); return true; }
// intra block copy: the CU waits for the intra / IBC CUs under its source block - the luma block at the vector plus, for an odd
// vector, the sample column / row before it that the halved chroma vector reaches; all of it must precede the CU in decoding order
inline bool node_ibc(const NodeCtx &x, Node &nd)
{
    const xgpu_cu_batch *b = x.b;
    const int i = nd.i, bvx = b->mv[i * 4], bvy = b->mv[i * 4 + 1], w = 1 << b->log2w[i], h = 1 << b->log2h[i];
    const int x0 = b->x[i] + (bvx & ~1), x1 = b->x[i] + bvx + w - 1, y0 = b->y[i] + (bvy & ~1), y1 = b->y[i] + bvy + h - 1;
    nd.r.ipm[0] = nd.r.ipm[1] = 0;
    nd.r.flags = 2u | (x.tree_of(i) == 1 ? 64u : 0u); nd.r.le = (uint64_t)(uint16_t)bvx | ((uint64_t)(uint16_t)bvy << 16);
    for (int sy = y0 >> 2; sy <= y1 >> 2; sy++)
        for (int sx = x0 >> 2; sx <= x1 >> 2; sx++) {
            const uint32_t j = x.own(sx, sy);
            if (j >= (uint32_t)i) return false;
            add_dep_once(x, nd, j);
            nd.lv = std::max(nd.lv, x.level[j]);
        }
    nd.fl.ibc = true;
    return true;
}
inline bool node_intra(const NodeCtx &x, Node &nd)
{
    const xgpu_cu_batch *b = x.b;
    IntraRec &r = nd.r;
    const int i = nd.i, xs = nd.xs, ys = nd.ys, ws = x.ws, hs = x.hs;
    const int wu = (1 << b->log2w[i]) >> 2, hu = (1 << b->log2h[i]) >> 2, units = wu + hu;
    const bool eipd = x.c->sp.tool_eipd != 0;
    // which neighbour units the CU's predictors actually read (xevd_ipred.c:96-164,587-622): only those create a dependency;
    // the others are still fetched by the kernel (availability is about COD flags, not about use) but their values are ignored
    bool need_ul = false;
    int need_up = 0, need_le = 0;                                                      // number of leading units read on each side
    if (eipd) { need_up = need_le = units; need_ul = true; }                           // EIPD modes: planar / bilinear / angular read both whole sides
    else for (int k = 0; k < 2; k++) {
        const int m = r.ipm[k];
        if (m == 0) { need_up = std::max(need_up, wu); need_le = std::max(need_le, hu); }
        else if (m == 1) need_le = std::max(need_le, hu);
        else if (m == 2) need_up = std::max(need_up, wu);
        else if (m == 3) { need_up = std::max(need_up, wu); need_le = std::max(need_le, hu); need_ul = true; }
        else { need_up = units; need_le = units; }
    }
    if (x.tree_of(i) == 1) r.flags |= 64u;              // luma only: the chroma samples stay as they are
    if (x.tree_of(i) == 2) {
        // chroma only: after the luma CUs of its block (the CUs that read this block later wait for this one CU)
        r.flags |= 32u;
        for (int sy = ys; sy < ys + hu; sy++) for (int sx = xs; sx < xs + wu; sx++) {
            const uint32_t j = x.own(sx, sy);
            if (j >= (uint32_t)i) continue;
            add_dep_once(x, nd, j);
            nd.lv = std::max(nd.lv, x.level[j]);
        }
    }
    bool used = true;
    uint32_t last_used = NONE;                                                         // the neighbour CU the unit before this one was looked up for
    auto ok = [&](int sx, int sy) -> bool {
        const uint32_t j = x.own(sx, sy);
        if (j >= (uint32_t)i || x.tile_of(sx, sy) != nd.my_tile) return false;         // not reconstructed yet (or nothing there), or in another tile
        if (x.constrained) {                                                           // constrained_intra_pred: intra neighbours only
            const uint32_t jl = x.constrained_tree ? x.luma_owner[(size_t)sy * ws + sx] : j;
            if (b->pred_mode[jl < (uint32_t)i ? jl : j] != XGPU_MODE_INTRA) return false;
        }
        if (!used) return true;
        if (j != last_used) {                                                          // (a wide neighbour covers several units: looked at once)
            last_used = j;
            add_dep_once(x, nd, j);                                                       // inter CUs are complete before the intra kernel starts
            if (!x.fast) nd.lv = std::max(nd.lv, x.level[j]);                          // (parallel mode: the levels are assigned afterwards)
        }
        return true;
    };
    used = need_ul;
    if (xs > 0 && ys > 0 && ok(xs - 1, ys - 1)) r.flags |= 1u;
    for (int k = 0; k < units; k++) {
        used = k < need_up;
        if (ys > 0 && xs + k < ws && ok(xs + k, ys - 1)) r.up |= 1ull << k;
    }
    for (int k = 0; k < units; k++) {
        used = k < need_le;
        if (xs > 0 && ys + k < hs && ok(xs - 1, ys + k)) r.le |= 1ull << k;
    }
    // sps_suco_flag: a split coded right to left leaves the CU with its RIGHT neighbours reconstructed.  avail_lr (xevd_check_nev_avail, xevd_util.c:1156-1174: the
    // SCU left of / right of the CU's first row is reconstructed, whatever its mode) goes into flag bits 23 / 24; the units of the right column the predictors may
    // read (xevdm_get_nbr :123-147) into the upper half of `up`: such a CU lies in a node of at most 64x64 that was split vertically, so its masks are short
    const uint32_t jl = xs > 0 ? x.own(xs - 1, ys) : NONE, jr = xs + wu < ws ? x.own(xs + wu, ys) : NONE;
    if (jr < (uint32_t)i && x.tile_of(xs + wu, ys) == nd.my_tile) {
        if (units > 32) return false;
        r.flags |= 1u << 24;
        nd.fl.right = true;
        if (jl < (uint32_t)i && x.tile_of(xs - 1, ys) == nd.my_tile) r.flags |= 1u << 23;      // (only matters next to bit 24: LR_11 against LR_01)
        uint32_t ri = 0;
        for (int k = 0; k < units; k++) {
            used = eipd;                                    // (the Baseline predictors never read the right column; HTDF lists its own dependencies)
            if (ys + k < hs && ok(xs + wu, ys + k)) ri |= 1u << k;
        }
        r.up |= (uint64_t)ri << 32;
    }
    if (nd.hidx >= 0) add_htdf(x, nd);
    return true;
}
// CU i, which is a node -> its record r and its dependencies (CU indices) appended to deps; lv_out = its level when the levels of its dependencies are known
// (sequential mode).  false: an invalid batch
inline bool make_node(const NodeCtx &x, const int i, IntraRec &r, std::vector<uint32_t> &deps, PlanOut &fl, int &lv_out)
{
    const xgpu_cu_batch *b = x.b;
    memset(&r, 0, sizeof(r));
    r.cu = (uint32_t)i; r.dep_first = (uint32_t)deps.size();
    r.x = b->x[i]; r.y = b->y[i]; r.log2w = b->log2w[i]; r.log2h = b->log2h[i]; r.cbf = b->cbf[i] & 7;
    if (b->ipm) { r.ipm[0] = b->ipm[i * 2]; r.ipm[1] = b->ipm[i * 2 + 1]; }  r.coef_off = b->coef_off[i];
    const int xs = b->x[i] >> 2, ys = b->y[i] >> 2;
    Node nd = { r, deps, fl, i, xs, ys, x.tile_of(xs, ys), plan_htdf_idx(b, (uint32_t)i), 0, NONE };
    const bool ok = b->pred_mode[i] == XGPU_MODE_INTRA ? node_intra(x, nd) : b->pred_mode[i] == XGPU_MODE_IBC ? node_ibc(x, nd) : node_filter_only(x, nd);
    r.dep_count = (uint32_t)deps.size() - r.dep_first;
    lv_out = nd.lv + 1;
    return ok;
}
// Parts (k_intra.hip): a wave takes 64 units (EIPD: rows of four luma samples + a chroma pair) or 64 SCUs (Baseline predictors) of its CU per step, a 64x64 CU is 16 (4) steps
// of one wave - on the critical path of every chain through it, and the level-1 launch is as long as its largest CUs take.  Such a CU goes into the list as several entries,
// one per step (at most 16), each with its own done flag: every part stages the neighbours and derives the plan itself and reconstructs its share; whoever reads the CU waits
// for all parts.  Not for HTDF / IBC nodes (the filter stage works on the whole block).  XEVD_HIP_NO_PARTS=1: A/B measurements.
struct PartRule {
    bool off, eipd;
    int operator()(const IntraRec &r) const { return off || (r.flags & (2u | 4u | 8u)) ? 1 : std::max(1, std::min((1 << (r.log2w + r.log2h - 4)) * (eipd ? 4 : 1) / 64, 16)); }
};
// Strands (k_intra.hip): a CU of level 2 and up whose dependency list holds exactly ONE CU of level 2 and up (the others are level-1 CUs, complete before the
// data-flow launch) is linked to that CU when it has no successor yet; the wave that reconstructs the parent continues with it.
// At entry: S.recs / S.deps / S.level complete.  Sets S.rec_of_cu (CU index -> record, -1: no node), S.succ (record -> its successor's record) and S.member
// (1: reached through its parent, not through a ticket), all three from scratch.
void link_strands(BuilderScratch &S, int n, const PartRule parts_of)
{
    static const bool no_strands = getenv("XEVD_HIP_NO_STRANDS") != NULL;      // A/B measurements
    const std::vector<IntraRec> &recs = S.recs;
    S.rec_of_cu.assign((size_t)n, -1);
    for (size_t ri = 0; ri < recs.size(); ri++) S.rec_of_cu[recs[ri].cu] = (int32_t)ri;
    S.succ.assign(recs.size(), NONE); S.member.assign(recs.size(), 0);
    for (size_t ri = 0; ri < recs.size(); ri++) {
        const IntraRec &r = recs[ri];
        if (S.level[r.cu] < 2) continue;
        int cnt = 0; uint32_t parent = NONE;
        for (uint32_t d = r.dep_first; d < r.dep_first + r.dep_count; d++) if (S.level[S.deps[d]] >= 2) { cnt++; parent = S.deps[d]; }
        if (cnt != 1 || no_strands) continue;
        const size_t pr = (size_t)S.rec_of_cu[parent];
        if (parts_of(r) > 1 || parts_of(recs[pr]) > 1) continue;
        if (S.succ[pr] == NONE) { S.succ[pr] = (uint32_t)ri; S.member[ri] = 1; }
    }
}
// sort by level (levels are 1-based; every dependency sits on a lower one), the larger CUs of a level first - a 64x64 CU is four rounds of its wave and should
// not be the last thing a launch starts -, decode order otherwise, the strand members behind everything else
inline size_t sort_key(const BuilderScratch &S, size_t ri) { return S.member[ri] ? ((size_t)S.plan.n_levels + 1) * 16 : (size_t)S.level[S.recs[ri].cu] * 16 + (size_t)(14 - (S.recs[ri].log2w + S.recs[ri].log2h)); }      // counting sort: log2w + log2h is 4 .. 14
// -> first[key] = list position of the key's first entry; sizes plan.recs, sets plan.n_level1_small
std::vector<int> sort_counts(BuilderScratch &S, const PartRule parts_of)
{
    const int max_level = S.plan.n_levels;
    std::vector<int> first(((size_t)max_level + 3) * 16, 0); size_t n_entries = 0;
    for (size_t ri = 0; ri < S.recs.size(); ri++) { const int np = parts_of(S.recs[ri]); first[sort_key(S, ri) + 1] += np; n_entries += (size_t)np; }
    for (size_t l = 1; l < first.size(); l++) first[l] += first[l - 1];
    // the level-1 entries of at most 16 SCUs (log2 w + log2 h <= 8: key 16 + 6 and up) end the level's part of the list: k_intra gives them 16 lanes each
    S.plan.n_level1_small = max_level >= 1 ? first[2 * 16] - first[16 + 6] : 0;
    S.plan.recs.resize(n_entries);
    return first;
}
// positions (serial: a running counter per key): S.pos = CU index -> list position of its first part (NONE: no node), from scratch; plan.n_level1, plan.n_heads
void assign_positions(BuilderScratch &S, int n, std::vector<int> &first, const PartRule parts_of)
{
    S.pos.assign((size_t)n, NONE); S.plan.n_level1 = 0; S.plan.n_heads = 0;
    for (size_t ri = 0; ri < S.recs.size(); ri++) {
        const int np = parts_of(S.recs[ri]);
        int &k = first[sort_key(S, ri)];
        S.pos[S.recs[ri].cu] = (uint32_t)k;
        k += np;
        if (S.level[S.recs[ri].cu] == 1) S.plan.n_level1 += np;
        if (!S.member[ri]) S.plan.n_heads += np;
    }
}
// dependency CU indices -> list positions, every part of a CU that has parts.  Level-1 CUs are finished by their own launch before the data-flow launch starts: they drop
// out of the waiting lists; a strand member waits for nobody (its one dependency of the launch is the CU its wave has just finished).  Counted per record first
// (S.nfirst, every element written), so that the records and their lists (plan.recs, plan.deps: every element written) can be written by the builder's threads
template <class Trace> void rewrite_deps(BuilderScratch &S, int nthr, const PartRule parts_of, Trace &&PT)
{
    const size_t n_recs = S.recs.size();
    S.nfirst.resize(n_recs + 1);
    uint32_t *const nf_p = S.nfirst.data();
    const IntraRec *const rc_p = S.recs.data(); const int32_t *const roc_p = S.rec_of_cu.data(); const uint8_t *const mem_p = S.member.data();
    const uint32_t *const dp_p = S.deps.data(), *const pos_p = S.pos.data(), *const succ_p = S.succ.data();
    const uint32_t n_l1 = (uint32_t)S.plan.n_level1;
    const int KS = std::max(1, std::min(nthr, std::max(1, (int)n_recs / 2048)));
    auto range = [&](int k, size_t &a0, size_t &a1) { a0 = n_recs * (size_t)k / KS; a1 = n_recs * (size_t)(k + 1) / KS; };
    S.pool.run(KS, [&](int k) {
        size_t a0, a1; range(k, a0, a1);
        for (size_t ri = a0; ri < a1; ri++) {
            uint32_t c = 0;
            if (!mem_p[ri])
                for (uint32_t d = rc_p[ri].dep_first; d < rc_p[ri].dep_first + rc_p[ri].dep_count; d++) {
                    const uint32_t j = dp_p[d];
                    if (pos_p[j] >= n_l1) c += (uint32_t)parts_of(rc_p[(size_t)roc_p[j]]);
                }
            nf_p[ri + 1] = c;
        }
    });
    nf_p[0] = 0; for (size_t ri = 0; ri < n_recs; ri++) nf_p[ri + 1] += nf_p[ri];
    PT("sort");
    S.plan.deps.resize((size_t)nf_p[n_recs]);                         // (the plan object keeps its capacity between pictures)
    uint32_t *const nd_p = S.plan.deps.data(); IntraRec *const out_p = S.plan.recs.data();
    S.pool.run(KS, [&](int k) {                                       // records and lists (parallel: every record knows where it goes)
        size_t a0, a1; range(k, a0, a1);
        for (size_t ri = a0; ri < a1; ri++) {
            const IntraRec &r = rc_p[ri];
            uint32_t w = nf_p[ri];
            if (!mem_p[ri])
                for (uint32_t d = r.dep_first; d < r.dep_first + r.dep_count; d++) {
                    const uint32_t j = dp_p[d], pj = pos_p[j];
                    if (pj < n_l1) continue;
                    const int npj = parts_of(rc_p[(size_t)roc_p[j]]);
                    for (int q = 0; q < npj; q++) nd_p[w++] = pj + (uint32_t)q;
                }
            const int np = parts_of(r);
            for (int q = 0; q < np; q++) {
                IntraRec &o = out_p[(size_t)pos_p[r.cu] + q];
                o = r; o.pad0 = (uint8_t)q; o.pad1[0] = (uint8_t)np;
                o.dep_first = nf_p[ri]; o.dep_count = nf_p[ri + 1] - nf_p[ri];
                // the device reads the successor's list position where the host kept the CU index
                o.cu = succ_p[ri] == NONE ? NONE : pos_p[rc_p[succ_p[ri]].cu];
            }
        }
    });
}
}      // namespace

// S.nodes (the CUs that are nodes, in decoding order) -> S.plan.  final_owner: the finished SCU -> CU map of the picture.  false: an IBC source block that is not
// reconstructed before its CU, or a right-hand neighbour next to a CU whose masks have no room for it - S stays usable (every vector is re-initialised where it is used)
bool build_intra_plan(xgpu_ctx *c, const xgpu_cu_batch *b, BuilderScratch &S, const uint32_t *final_owner, int nthr)
{
    const int n = b->n_cu, ws = c->w_scu, hs = c->h_scu;
    IntraPlan &plan = S.plan;
    // Batches without local dual trees (everything but BTT + ADMVP streams) take the FINAL SCU -> CU map the caller has already painted (in parallel, for k_inter):
    // "reconstructed before CU i" is then "owner index below i", no painting in step with the loop, and the nodes are independent of each other - built on the
    // builder's threads, levels assigned afterwards.  (At 8K this function was 11 of the builder's 15 ms, whatever the thread count.)
    const bool fast = final_owner != NULL && b->tree == NULL;
    static const bool pt_on = getenv("XEVD_HIP_BUILD_TRACE") != NULL;
    auto pt_t0 = std::chrono::steady_clock::now();
    auto PT = [&](const char *what) { if (pt_on) { const auto t = std::chrono::steady_clock::now(); fprintf(stderr, "    intra plan: %-12s %.2f ms\n", what, std::chrono::duration<double, std::milli>(t - pt_t0).count()); pt_t0 = t; } };
    // constrained intra prediction inside local dual trees: "is the neighbour intra-coded" is a property of the LUMA CU over the SCU (map_scu is written by the
    // luma CUs only) - an IBC luma CU under a chroma-only intra CU is not an intra neighbour.  The luma owners are kept apart from the repainted map for that test.
    const bool constrained_tree = b->constrained_intra_pred != 0 && b->tree != NULL;
    if (!fast) S.owner_own.assign((size_t)ws * hs, NONE);  if (constrained_tree) S.luma_owner.assign((size_t)ws * hs, NONE);      // sequential mode: all unowned, painted CU by CU
    S.level.assign((size_t)n, 0);                              // 0: no node (complete before the intra kernels start), or not assigned yet
    std::vector<uint8_t> ctu_tile;
    if (b->tiles) {
        ctu_tile.assign((size_t)c->w_ctu * c->h_ctu, 0);
        for (int tj = 0; tj < b->tiles->n_rows; tj++) for (int ti = 0; ti < b->tiles->n_cols; ti++)
            for (int cy = b->tiles->row_bd[tj]; cy < b->tiles->row_bd[tj + 1]; cy++)
                for (int cx = b->tiles->col_bd[ti]; cx < b->tiles->col_bd[ti + 1]; cx++) ctu_tile[(size_t)cy * c->w_ctu + cx] = (uint8_t)(tj * b->tiles->n_cols + ti);
    }
    const NodeCtx x = { c, b, fast ? final_owner : S.owner_own.data(), S.luma_owner.data(), S.level.data(), ctu_tile.empty() ? NULL : ctu_tile.data(), ws, hs, c->sp.log2_ctu - 2,
                        fast, b->constrained_intra_pred != 0, constrained_tree };
    std::vector<IntraRec> &recs = S.recs; std::vector<uint32_t> &deps = S.deps; std::vector<int> &level = S.level;      // recs: decode order; dep lists hold CU indices until the rewrite
    int max_level = 0; PT("setup");
    if (!fast) {
        // painted CU by CU as the loop reaches them ("reconstructed before CU i" = painted): inside a local dual tree the node's chroma-only CU follows its
        // luma CUs and covers them again
        auto paint = [&](int i) {
            const int xs = b->x[i] >> 2, ys = b->y[i] >> 2, w = (1 << b->log2w[i]) >> 2, h = (1 << b->log2h[i]) >> 2;
            for (int r = 0; r < h; r++) std::fill_n(S.owner_own.begin() + (size_t)(ys + r) * ws + xs, w, (uint32_t)i);
            if (constrained_tree && b->tree[i] != 2)
                for (int r = 0; r < h; r++) std::fill_n(S.luma_owner.begin() + (size_t)(ys + r) * ws + xs, w, (uint32_t)i);
        };
        PlanOut fl;                            // (its flags only: the sequential mode appends to S.deps directly)
        deps.clear(); recs.clear();
        for (int i = 0; i < n; paint(i), i++) {
            if (!plan_is_node(b, (uint32_t)i)) continue;
            int lv = 0; IntraRec r;
            if (!make_node(x, i, r, deps, fl, lv)) return false;
            recs.push_back(r); level[(size_t)i] = lv; max_level = std::max(max_level, lv);
        }
        plan.has_ibc = fl.ibc; plan.has_htdf = fl.htdf; plan.has_right = fl.right;
    } else {
        // the ranges of S.nodes go to the threads: every entry becomes exactly one record, the threads write their ranges of the final list; the dependency
        // lists are per thread (S.outs: cleared here) and concatenated afterwards (dep_first moved along while the levels are assigned)
        const uint32_t *const nodes = S.nodes.data();
        const int nn = (int)S.nodes.size(), K = std::max(1, std::min(nthr, std::max(1, nn / 2048)));
        if ((int)S.outs.size() < K) S.outs.resize((size_t)K);
        for (PlanOut &o : S.outs) { o.deps.clear(); o.ibc = o.htdf = o.right = o.bad = false; }
        recs.resize((size_t)nn);               // (no re-initialisation of records that are overwritten anyway)
        IntraRec *const recs_p = recs.data(); PlanOut *const outs = S.outs.data();
        S.pool.run(K, [&](int k) {
            PlanOut &o = outs[k];
            int lv = 0;
            const int q0 = (int)((long long)nn * k / K), q1 = (int)((long long)nn * (k + 1) / K);
            o.deps.reserve((size_t)(q1 - q0) * 3);
            for (int q = q0; q < q1 && !o.bad; q++) o.bad = !make_node(x, (int)nodes[q], recs_p[q], o.deps, o, lv);
        });
        PT("nodes");
        size_t nd = 0;
        for (int k = 0; k < K; k++) { const PlanOut &o = outs[k]; if (o.bad) return false; nd += o.deps.size(); plan.has_ibc |= o.ibc; plan.has_htdf |= o.htdf; plan.has_right |= o.right; }
        deps.clear(); deps.reserve(nd);
        // levels, in decoding order: 1 + the highest level among the nodes read (CUs that are no nodes - complete before the intra kernels start - count as level 0)
        for (int k = 0; k < K; k++) {
            const uint32_t base = (uint32_t)deps.size();
            deps.insert(deps.end(), outs[k].deps.begin(), outs[k].deps.end());
            for (int q = (int)((long long)nn * k / K), q1 = (int)((long long)nn * (k + 1) / K); q < q1; q++) {
                IntraRec &r = recs_p[q];
                r.dep_first += base;
                int lv = 0;
                for (uint32_t d = r.dep_first; d < r.dep_first + r.dep_count; d++) lv = std::max(lv, level[deps[d]]);
                level[r.cu] = lv + 1; max_level = std::max(max_level, lv + 1);
            }
        }
    }
    PT("levels"); plan.n_levels = max_level;
    static const bool no_parts = getenv("XEVD_HIP_NO_PARTS") != NULL; const PartRule parts_of = { no_parts, c->sp.tool_eipd != 0 };
    link_strands(S, n, parts_of);
    std::vector<int> first = sort_counts(S, parts_of);
    assign_positions(S, n, first, parts_of);
    rewrite_deps(S, nthr, parts_of, PT);
    return true;
}
