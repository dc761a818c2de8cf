// xgpu_builder.hip - the host batch builder (xgpu_batch_create): validation, CU / TB records, owner map, the work lists of k_inter, the pinned staging block and its
// upload; the dependency plan of the order-dependent CUs (intra, IBC, HTDF) is xgpu_intra_plan.hip.  Plain C++ (no kernel in this file); xgpu_test_build_batch runs
// it without a device.  (xevd_ctu_row_rec_mt's per-CU cu_init + coef_rect_to_series, xevd.c:567-676, become this pass.)
#include <chrono>
#include "xgpu_host.h"
#include "affine_model.h"

namespace {
// The staging block and the device block of a batch: the uploaded arrays at the same offsets in both (one copy sends them), then the device-only regions (residual
// arena, intra done flags + ticket counter, DMVR vectors).  Everything that places, fills, points at or digests an array reads this table.
enum Seg { SEG_CUS, SEG_CTU, SEG_TBS, SEG_WAVES, SEG_INTRA, SEG_DEPS, SEG_AFF, SEG_CPMV, SEG_DMVR, SEG_OWNER, SEG_IITEM, SEG_IWORK, SEG_COEF, SEG_RESID, SEG_DONE, SEG_DMV, SEG_COUNT };
struct StageLayout {
    size_t off[SEG_COUNT], alloc[SEG_COUNT], payload[SEG_COUNT], stage_bytes, d_need;      // alloc: at least min_count elements (no kernel argument points past the block); payload: what the batch fills
    template <class T> T *at(void *base, Seg s) const { return (T *)((uint8_t *)base + off[s]); }
};
struct SegSize { Seg seg; size_t elem, count, min_count; };
template <size_t N> void stage_layout(StageLayout &L, const SegSize (&rows)[N])      // rows: one per segment, in layout order
{
    static_assert(N == SEG_COUNT, "one row per segment");
    size_t o = 0;
    for (const SegSize &r : rows) {
        L.off[r.seg] = o; L.payload[r.seg] = r.elem * r.count; L.alloc[r.seg] = r.elem * std::max(r.count, r.min_count);
        if (r.seg == SEG_COEF) L.stage_bytes = o + L.alloc[r.seg];
        o += (L.alloc[r.seg] + 255) / 256 * 256;
    }
    L.d_need = o;
}
// size class of a TB = (log2w, log2h) x (vertical, horizontal) transform kind; ATS kinds only occur for intra luma TBs
enum { NCLS = 64 * 9 };
inline int ats_inter_of(const xgpu_cu_batch *b, int i) { return (b->ats_inter && b->pred_mode[i] != XGPU_MODE_INTRA && b->pred_mode[i] != XGPU_MODE_IBC) ? b->ats_inter[i] : 0; }
inline int tr_code(const xgpu_cu_batch *b, int i, int k)
{
    if (k != 0) return 0;
    if (const int ai = ats_inter_of(b, i)) {
        // xevdm_get_ats_inter_trs (src_main/xevdm_util.c:3636-3668): DST-VII across the split, DCT-VIII along it for the
        // first part / DST-VII for the last; CUs wider or taller than 32 keep DCT-II
        if (b->log2w[i] > 5 || b->log2h[i] > 5) return 0;
        const int idx = ai & 15, pos = ai >> 4, hor = idx == 2 || idx == 4;
        const int tv = hor ? (pos == 0 ? TR_DCT8 : TR_DST7) : TR_DST7, th = hor ? TR_DST7 : (pos == 0 ? TR_DCT8 : TR_DST7);
        return tv * 3 + th;
    }
    if (!b->ats || !(b->ats[i] & 1) || b->pred_mode[i] != XGPU_MODE_INTRA) return 0;
    const int tv = (b->ats[i] >> 1) & 1 ? TR_DCT8 : TR_DST7, th = (b->ats[i] >> 2) & 1 ? TR_DCT8 : TR_DST7;
    return tv * 3 + th;
}
// The transform blocks of CU i (geometry validated), in the order of the CU's coefficients: f(component, sub-block, class, tw, th, cl, comp_off) with tw / th = the
// TB's log2 size, cl = log2 width of the component block, comp_off = its start behind coef_off[i]; returns the extent of the CU's coefficients.  Pass 1 counts with it what pass 2 fills.
template <class F> inline size_t for_each_tb(const xgpu_cu_batch *b, int i, F &&f)
{
    // luma log2 size of the CU's coefficient block: the CU, or the ATS-inter TU (xevdm_get_tu_size, xevdm_util.c:3585-3608)
    int bw = b->log2w[i], bh = b->log2h[i]; const int idx = ats_inter_of(b, i) & 15;
    if (idx == 1 || idx == 3) bw -= idx == 3 ? 2 : 1;
    if (idx == 2 || idx == 4) bh -= idx == 4 ? 2 : 1;
    // TBs are at most 64 wide/tall: a larger CU is cut into 64x64 (chroma 32x32) sub-blocks (xevd_itdq.c:544-621)
    const int nsx = b->log2w[i] > 6 ? 2 : 1, nsy = b->log2h[i] > 6 ? 2 : 1;
    size_t ext = 0;
    for (int k = 0; k < 3; k++) {
        if (!((b->cbf[i] >> k) & 1)) continue;
        const int cl = k ? bw - 1 : bw, ch = k ? bh - 1 : bh;        // component block of the CU
        const int tw = std::min(bw, 6) - (k ? 1 : 0), th = std::min(bh, 6) - (k ? 1 : 0), cls = tr_code(b, i, k) * 64 + tw * 8 + th;
        for (int sb = 0; sb < 4; sb++) {
            if ((sb & 1) >= nsx || (sb >> 1) >= nsy) continue;
            if (nsx * nsy > 1 && b->cbf_sub && !((b->cbf_sub[i] >> (4 * k + sb)) & 1)) continue;
            f(k, sb, cls, tw, th, cl, (uint32_t)ext);
        }
        ext += (size_t)1 << (cl + ch);
    }
    return ext;
}
// the chroma-only CU that closes the local dual tree of luma-only CU i (b->n_cu: there is none)
inline int closing_chroma_cu(const xgpu_cu_batch *b, int i) { int j = i + 1; while (j < b->n_cu && b->tree[j] != 2) j++; return j; }
// DMVR candidates the backend can refine: flagged, plain inter, two references, at least 8x8 (the POC test happens on the device)
inline bool dmvr_cand(const xgpu_cu_batch *b, int i)
{
    return b->dmvr && b->dmvr[i] && b->pred_mode[i] != XGPU_MODE_INTRA && b->pred_mode[i] != XGPU_MODE_IBC && !(b->affine && b->affine[i]) &&
           b->refi[i * 2] >= 0 && b->refi[i * 2 + 1] >= 0 && b->log2w[i] >= 3 && b->log2h[i] >= 3;
}
// the branch xevdm_affine_mc takes for CU i (EIF when a sub-block would be smaller than 8 samples): the kernels' own code, affine_model.h
inline bool affine_is_eif(const xgpu_cu_batch *b, int i)
{
    const bool use[2] = { b->refi[i * 2] >= 0, b->refi[i * 2 + 1] >= 0 };
    AffModel md[2];
    for (int l = 0; l < 2; l++) md[l] = aff_model(b->affine_mv + (size_t)i * 12 + l * 6, b->log2w[i], b->log2h[i], b->affine[i]);
    int sw, sh; bool mb;
    aff_subblock(md, use, b->log2w[i], b->log2h[i], sw, sh, mb);
    return sw < 8 || sh < 8;
}
// The builder's per-CU passes run on `builder_threads` host threads (xgpu_set_builder_threads; default 1), each over a contiguous range of CUs: pass 1
// validates and counts per range, a prefix over the ranges gives every thread its own start in each output list, pass 2 and the owner map then write
// disjoint parts - the lists come out exactly as the sequential passes build them.
struct Part { int cls[NCLS]; int n_aff, n_eif, n_sub, n_dmvr; std::vector<uint32_t> nodes; };      // nodes: the CUs of the range that enter the dependency plan (intra, IBC, HTDF)
struct Build {      // one call of the builder: what its phases hand to each other
    xgpu_ctx *c; const xgpu_cu_batch *b; BuilderScratch &S; int n, nthr;
    std::vector<Part> parts;
    int cls_count[NCLS], cls_first[NCLS], n_tb, n_waves, n_aff, n_aff_eif, n_aff_sub, n_dmvr;
    template <class F> void run_parts(F fn) { S.pool.run(nthr, [&](int k) { fn(k, (int)((long long)n * k / nthr), (int)((long long)n * (k + 1) / nthr)); }); }      // fn(thread, first CU, one past the last)
    void copy_sliced(void *dst, const void *src, size_t bytes)      // in 64-byte-aligned slices on the builder's threads
    {
        S.pool.run(nthr, [&](int k) { const size_t a0 = bytes * (size_t)k / nthr & ~(size_t)63, a1 = k + 1 == nthr ? bytes : (bytes * (size_t)(k + 1) / nthr & ~(size_t)63);
                                      memcpy((uint8_t *)dst + a0, (const uint8_t *)src + a0, a1 - a0); });
    }
    // pass 1 over the CUs [i0, i1): validate + count TBs per size class, affine tiles, DMVR sub-blocks, plan nodes.  NULL, or the condition that does not hold
#define CUCHK(cond) do { if (!(cond)) return #cond; } while (0)
    const char *validate_and_count(int i0, int i1, Part &P)
    {
        for (int i = i0; i < i1; i++) {
            const int lw = b->log2w[i], lh = b->log2h[i];
            CUCHK(lw >= 2 && lw <= 7 && lh >= 2 && lh <= 7 && lw <= c->sp.log2_ctu && lh <= c->sp.log2_ctu);
            CUCHK(b->x[i] + (1 << lw) <= c->sp.width && b->y[i] + (1 << lh) <= c->sp.height && !(b->x[i] & 3) && !(b->y[i] & 3));
            CUCHK(b->pred_mode[i] <= XGPU_MODE_DIR || b->pred_mode[i] == XGPU_MODE_IBC);
            if (b->tree && b->tree[i]) {      // local dual tree: luma-only intra / IBC CUs, chroma-only intra CUs, only the coefficients of the planes they have
                CUCHK(b->tree[i] <= 2 && (b->pred_mode[i] == XGPU_MODE_INTRA || (b->tree[i] == 1 && b->pred_mode[i] == XGPU_MODE_IBC)));
                CUCHK((b->cbf[i] & (b->tree[i] == 1 ? 6 : 1)) == 0);
                if (b->tree[i] == 1) {        // a luma-only CU lies inside the chroma-only CU that closes its tree (checked here: nothing is allocated yet)
                    const int j = closing_chroma_cu(b, i);
                    CUCHK(j < n && b->x[j] <= b->x[i] && b->y[j] <= b->y[i] && b->x[i] + (1 << lw) <= b->x[j] + (1 << b->log2w[j]) && b->y[i] + (1 << lh) <= b->y[j] + (1 << b->log2h[j]));
                }
            }
            if (b->pred_mode[i] == XGPU_MODE_IBC) {
                // the source block (and the chroma block at the halved vector) inside the active picture; that it is reconstructed before the CU is
                // checked by the dependency plan
                const int bvx = b->mv[i * 4], bvy = b->mv[i * 4 + 1];
                CUCHK(b->x[i] + (bvx & ~1) >= 0 && b->y[i] + (bvy & ~1) >= 0 && b->x[i] + bvx + (1 << lw) <= c->sp.width && b->y[i] + bvy + (1 << lh) <= c->sp.height);
                CUCHK(!(b->affine && b->affine[i]));
            } else if (b->pred_mode[i] != XGPU_MODE_INTRA) CUCHK(b->refi[i * 2] < XGPU_MAX_REFS && b->refi[i * 2 + 1] < XGPU_MAX_REFS);
            CUCHK(b->qp[i * 3] < 96 && b->qp[i * 3 + 1] < 96 && b->qp[i * 3 + 2] < 96);                     // 0..51 + 6 * (bit depth - 8)
            if (const int ai = ats_inter_of(b, i)) {
                // availability as xevdm_check_ats_inter_info_coded (xevdm_util.c:3565-3583): CU <= 64, split dimension >= 8 (>= 16 for quarters)
                const int idx = ai & 15, pos = ai >> 4;
                CUCHK(idx >= 1 && idx <= 4 && pos <= 1 && lw <= 6 && lh <= 6);
                CUCHK(((idx == 1 || idx == 3) ? lw : lh) >= (idx >= 3 ? 4 : 3));
            }
            if (b->affine && b->affine[i]) {
                // affine CUs exist from 8x8 (xevdm_eco.c:1529), with 2 or 3 control points and at least one reference
                CUCHK(b->affine_mv != NULL && (b->affine[i] == 2 || b->affine[i] == 3) && b->pred_mode[i] != XGPU_MODE_INTRA);
                CUCHK(lw >= 3 && lh >= 3 && (b->refi[i * 2] >= 0 || b->refi[i * 2 + 1] >= 0));
                P.n_aff++;
                if (affine_is_eif(b, i)) P.n_eif += ((1 << lw) + 15) / 16 * (((1 << lh) + 15) / 16);
                else                     P.n_sub += ((1 << lw) + 31) / 32 * (((1 << lh) + 31) / 32);
            }
            if (dmvr_cand(b, i)) P.n_dmvr += (lw > 4 ? 1 << (lw - 4) : 1) * (lh > 4 ? 1 << (lh - 4) : 1);
            const char *bad = nullptr;        // ATS exists for 4..32 only (checked before anything is allocated)
            const size_t need = for_each_tb(b, i, [&](int, int, int cls, int tw, int th, int, uint32_t) {
                if (cls < 64 || (tw >= 2 && tw <= 5 && th >= 2 && th <= 5)) P.cls[cls]++;
                else bad = "tr_code(i, k) == 0 || (tw >= 2 && tw <= 5 && th >= 2 && th <= 5)";
            });
            if (bad) return bad;
            CUCHK((size_t)b->coef_off[i] + need <= b->n_coef);
            if (plan_is_node(b, (uint32_t)i)) P.nodes.push_back((uint32_t)i);
        }
        return nullptr;
    }
#undef CUCHK
    // phase 1: validate + count on the threads, then the totals: TBs and work items per class, where each class starts in the TB list
    int pass1()
    {
        parts.resize((size_t)nthr);      // (value-initialised, like this object's own counts: all zero)
        std::vector<const char *> bad((size_t)nthr, nullptr);
        run_parts([&](int k, int i0, int i1) { bad[(size_t)k] = validate_and_count(i0, i1, parts[(size_t)k]); });
        for (const char *m : bad)
            if (m) { snprintf(c->err, sizeof(c->err), "%s: invalid argument: %s", __FILE__, m); return XGPU_ERR_INVALID_ARGUMENT; }
        for (const Part &P : parts) { for (int k = 0; k < NCLS; k++) cls_count[k] += P.cls[k]; n_aff += P.n_aff; n_aff_eif += P.n_eif; n_aff_sub += P.n_sub; n_dmvr += P.n_dmvr; }
        for (int k = 0; k < NCLS; k++) {
            cls_first[k] = n_tb; n_tb += cls_count[k];
            if (cls_count[k]) { const int per = itdq_group_size((k & 63) >> 3, k & 7); n_waves += (cls_count[k] + per - 1) / per; }
        }
        return XGPU_OK;
    }
    // SCU -> CU map of the picture (k_inter's lanes find their CU through it; the dependency plan reads "reconstructed before" off it); SCUs outside the batch -
    // another tile's - stay unowned.  Painted in ordinary memory (short row fills) and copied into the pinned block in one piece further down.  S.own: every SCU written here (by the fill first unless the batch covers the picture)
    void paint_owner_map()
    {
        std::vector<uint32_t> &own = S.own; own.resize((size_t)c->w_scu * c->h_scu);
        size_t covered = 0;
        for (int i = 0; i < n; i++) if (!(b->tree && b->tree[i] == 2)) covered += (size_t)1 << (b->log2w[i] + b->log2h[i] - 4);
        if (covered != own.size()) std::fill(own.begin(), own.end(), 0xFFFFFFFFu);
        uint32_t *const own_p = own.data();
        run_parts([&, own_p](int, int i0, int i1) {           // CUs do not overlap: the ranges paint disjoint SCUs
            for (int i = i0; i < i1; i++) {
                if (b->tree && b->tree[i] == 2) continue;           // the SCU maps of a dual-tree block belong to its luma CUs
                const int ws = (1 << b->log2w[i]) >> 2, hh = (1 << b->log2h[i]) >> 2;
                uint32_t *o = own_p + (size_t)(b->y[i] >> 2) * c->w_scu + (b->x[i] >> 2);
                for (int r = 0; r < hh; r++, o += c->w_scu) std::fill_n(o, ws, (uint32_t)i);
            }
        });
    }
    // Work lists of the three inter launches (k_inter.hip): 64x64 regions inside one CU, 32x32 tiles inside one CU, the other tiles that hold SCUs of the batch.  A tile /
    // region counts as "inside one CU" only when it lies inside the picture as a whole (the kernels' shared-window paths have no partial form).  The CUs mark the tiles
    // (disjoint CUs: disjoint full tiles; `any` is a relaxed flag several CUs of one tile may set), one sequential sweep in the kernels' spatial order - vertical strips
    // XGPU_INTER_STRIP regions wide, row by row inside a strip - emits the lists.
    // S.tile_cu / S.tile_any: reset per tile; S.inter_items ([entry * 4 + tile]: the CU a whole tile lies in, else none) and S.inter_work (per 64x64 region, InterArgs.work): rebuilt
    void inter_work_lists()
    {
        std::vector<uint32_t> &inter_items = S.inter_items, &inter_work = S.inter_work;
        const int tiles_x = (c->sp.width + 31) >> 5, tiles_y = (c->sp.height + 31) >> 5, full_x = c->sp.width >> 5, full_y = c->sp.height >> 5;
        S.tile_cu.assign((size_t)tiles_x * tiles_y, 0xFFFFFFFFu);
        S.tile_any.assign((size_t)tiles_x * tiles_y, 0);
        uint32_t *const tcu = S.tile_cu.data(); uint8_t *const tany = S.tile_any.data();
        run_parts([&, tcu, tany](int, int i0, int i1) {
            for (int i = i0; i < i1; i++) {
                if (b->tree && b->tree[i] == 2) continue;
                const int x0 = b->x[i], y0 = b->y[i], x1 = x0 + (1 << b->log2w[i]), y1 = y0 + (1 << b->log2h[i]);
                for (int ty = y0 >> 5; ty <= (y1 - 1) >> 5; ty++)
                    for (int tx = x0 >> 5; tx <= (x1 - 1) >> 5; tx++) {
                        if (tx < full_x && ty < full_y && (tx << 5) >= x0 && (tx << 5) + 32 <= x1 && (ty << 5) >= y0 && (ty << 5) + 32 <= y1) tcu[(size_t)ty * tiles_x + tx] = (uint32_t)i;
                        else __atomic_store_n(&tany[(size_t)ty * tiles_x + tx], (uint8_t)1, __ATOMIC_RELAXED);
                    }
            }
        });
        inter_items.clear(); inter_work.clear();
        const int regions_x = (c->sp.width + 63) >> 6, regions_y = (c->sp.height + 63) >> 6;
        for (int s0 = 0; s0 < regions_x; s0 += XGPU_INTER_STRIP)
            for (int ry = 0; ry < regions_y; ry++)
                for (int rx = s0; rx < std::min(s0 + XGPU_INTER_STRIP, regions_x); rx++) {
                    const int tx = rx * 2, ty = ry * 2;
                    const bool whole = tx + 1 < tiles_x && ty + 1 < tiles_y;
                    const uint32_t o = tcu[(size_t)ty * tiles_x + tx];
                    if (whole && o != 0xFFFFFFFFu && tcu[(size_t)ty * tiles_x + tx + 1] == o && tcu[(size_t)(ty + 1) * tiles_x + tx] == o && tcu[(size_t)(ty + 1) * tiles_x + tx + 1] == o) {
                        inter_work.push_back(XGPU_WORK_REGION);
                        for (int q = 0; q < 4; q++) inter_items.push_back(o);      // every wave of the region role reads the item of its own tile's place
                        continue;
                    }
                    uint32_t kinds = 0;
                    for (int q = 0; q < 4; q++) {
                        const int ux = tx + (q & 1), uy = ty + (q >> 1);
                        uint32_t oq = 0xFFFFFFFFu;
                        if (ux < tiles_x && uy < tiles_y) {
                            oq = tcu[(size_t)uy * tiles_x + ux];
                            if (oq != 0xFFFFFFFFu) kinds |= 1u << (2 * q);
                            else if (tany[(size_t)uy * tiles_x + ux]) kinds |= 2u << (2 * q);
                        }
                        inter_items.push_back(oq);
                    }
                    inter_work.push_back(kinds);
                }
    }
    // sps_suco_flag: is any CU decoded AFTER its right-hand neighbour?  (All right-hand neighbours of a CU lie in the other part of one vertical split: the first one
    // tells.)  Only the baseline deblocking filter wants to know beforehand - it applies chroma edges 2 samples apart in the order the reference's tree walk reaches
    // them (k_deblock.hip) and takes its left-to-right instantiation otherwise; ADDB is order-free, the intra plan finds its right-hand neighbours itself
    bool probe_order_rl()
    {
        if (c->sp.tool_addb) return false;
        std::atomic<int> found(0); const uint32_t *const own_p = S.own.data();
        run_parts([&, own_p](int, int i0, int i1) {
            for (int i = i0; i < i1 && !found.load(std::memory_order_relaxed); i++) {
                const int xr = b->x[i] + (1 << b->log2w[i]);
                if (xr < c->sp.width && own_p[(size_t)(b->y[i] >> 2) * c->w_scu + (xr >> 2)] < (uint32_t)i) found.store(1, std::memory_order_relaxed);
            }
        });
        return found.load() != 0;
    }
    // the dependency plan: S.nodes = the nodes pass 1 collected per range, in decoding order (rebuilt); S.plan reset, and filled when there are nodes
    bool intra_plan()
    {
        S.nodes.clear(); S.plan.reset();
        for (const Part &P : parts) S.nodes.insert(S.nodes.end(), P.nodes.begin(), P.nodes.end());
        return S.nodes.empty() || build_intra_plan(c, b, S, S.own.data(), nthr);
    }
    // the blocks of the batch: a pooled block that is large enough (the smallest such), else a new one; host-only: the caller's scratch.  coef_pinned: the coefficient
    // arena lies inside a range from xgpu_host_alloc - then it is sent from where it lies (no staging copy of the largest array)
    int acquire_block(xgpu_dbatch *db, const StageLayout &L, bool &coef_pinned)
    {
        int best = -1;
        {
            std::lock_guard<std::mutex> g(c->pool_mu);
            for (const auto &h : c->pinned)
                if ((const uint8_t *)b->coef >= h.p && (const uint8_t *)(b->coef + b->n_coef) <= h.p + h.n) coef_pinned = b->n_coef != 0;
            for (size_t k = 0; k < c->pool.size(); k++)
                if (c->pool[k].d_cap >= L.d_need && c->pool[k].h_cap >= L.stage_bytes && (best < 0 || c->pool[k].d_cap < c->pool[best].d_cap)) best = (int)k;
            if (best >= 0) { db->blk = c->pool[best]; c->pool.erase(c->pool.begin() + best); }
        }
        if (db->host_only) {
            memset(&db->blk, 0, sizeof(db->blk));
            // (kept between calls like a pooled block: a fresh 60 MB malloc per call would time the kernel's page zeroing.  Grown, never cleared: the builder writes what it digests)
            if (S.host_stage.size() < L.stage_bytes) S.host_stage.resize(L.stage_bytes);
            db->blk.h_stage = S.host_stage.data(); db->blk.h_cap = L.stage_bytes;
        } else if (best >= 0) {
            if (hipEventSynchronize(db->blk.uploaded) != hipSuccess) return XGPU_ERR_UNEXPECTED;      // its staging block may still feed an upload
            // ... and its device block the kernels of the batch that had it before: the upload stream waits for them
            if (hipStreamWaitEvent(c->up_stream, db->blk.done, 0) != hipSuccess) return XGPU_ERR_UNEXPECTED;
        } else {
            memset(&db->blk, 0, sizeof(db->blk));
            const size_t d_cap = L.d_need + L.d_need / 4, h_cap = L.stage_bytes + L.stage_bytes / 4;             // headroom: pictures of a stream vary
            if (hipMalloc((void **)&db->blk.d_base, d_cap) != hipSuccess) return XGPU_ERR_OUT_OF_MEMORY;
            if (hipHostMalloc(&db->blk.h_stage, h_cap, hipHostMallocDefault) != hipSuccess) return XGPU_ERR_OUT_OF_MEMORY;
            db->blk.d_cap = d_cap; db->blk.h_cap = h_cap;
            static const bool blocking = getenv("XEVD_HIP_BLOCKING_SYNC") != NULL && atoi(getenv("XEVD_HIP_BLOCKING_SYNC")) != 0;      // see xgpu_open
            if (hipEventCreateWithFlags(&db->blk.uploaded, hipEventDisableTiming | (blocking ? hipEventBlockingSync : 0)) != hipSuccess) return XGPU_ERR_UNEXPECTED;
            if (hipEventCreateWithFlags(&db->blk.done, hipEventDisableTiming) != hipSuccess) return XGPU_ERR_UNEXPECTED;
            if (hipEventCreateWithFlags(&db->blk.itdq_done, hipEventDisableTiming) != hipSuccess) return XGPU_ERR_UNEXPECTED;
        }
        if (db->n_chroma_cus) {
            const size_t nb = sizeof(uint32_t) * (size_t)db->n_chroma_cus;
            if (db->blk.chroma_cap < nb) {      // (a pooled block: hipFree waits for the kernels that read the old list)
                if (db->blk.d_chroma) (void)hipFree(db->blk.d_chroma);
                db->blk.d_chroma = NULL; db->blk.chroma_cap = 0;
                if (hipMalloc((void **)&db->blk.d_chroma, nb + nb / 4) != hipSuccess) return XGPU_ERR_OUT_OF_MEMORY;
                db->blk.chroma_cap = nb + nb / 4;
            }
            db->d_chroma_cus = db->blk.d_chroma;
        }
        return XGPU_OK;
    }
    // pass 2: CU records, affine tiles + control points, DMVR sub-blocks and the TB scatter into class order; every thread starts where the ranges before it end in each list
    void fill_records(const StageLayout &L, void *hs)
    {
        CuRec *const cus = L.at<CuRec>(hs, SEG_CUS); TbRec *const tbs = L.at<TbRec>(hs, SEG_TBS); int16_t *const cpmv = L.at<int16_t>(hs, SEG_CPMV);
        AffItem *const aff_items = L.at<AffItem>(hs, SEG_AFF); DmvrItem *const dmvr_items = L.at<DmvrItem>(hs, SEG_DMVR);
        const int bdoff = 6 * (c->sp.bit_depth_luma - 8);
        run_parts([&](int part, int i0, int i1) {
        int cls_fill[NCLS]; memcpy(cls_fill, cls_first, sizeof(cls_fill));
        int aff_fill = 0, eif_fill = 0, sub_fill = n_aff_eif, dmvr_fill = 0;
        for (int q = 0; q < part; q++) {
            const Part &P = parts[(size_t)q];
            for (int k = 0; k < NCLS; k++) cls_fill[k] += P.cls[k];
            aff_fill += P.n_aff; eif_fill += P.n_eif; sub_fill += P.n_sub; dmvr_fill += P.n_dmvr;
        }
        for (int i = i0; i < i1; i++) {
            CuRec &r = cus[i]; memset(&r, 0, sizeof(r));
            if (b->affine && b->affine[i]) {
                r.affine = b->affine[i];
                memcpy(cpmv + (size_t)aff_fill * 12, b->affine_mv + (size_t)i * 12, sizeof(int16_t) * 12);
                const bool eif = affine_is_eif(b, i);
                const int step = eif ? 16 : 32;
                for (int ty = 0; ty < (1 << b->log2h[i]); ty += step)
                    for (int tx = 0; tx < (1 << b->log2w[i]); tx += step) {
                        AffItem &it = aff_items[eif ? eif_fill++ : sub_fill++];
                        it.cu = (uint32_t)i; it.aff = (uint32_t)aff_fill; it.tx = (uint16_t)tx; it.ty = (uint16_t)ty; it.pad = 0;
                    }
                aff_fill++;
            }
            r.x = b->x[i]; r.y = b->y[i]; r.log2w = b->log2w[i]; r.log2h = b->log2h[i];
            r.pred_mode = b->pred_mode[i]; r.cbf = b->cbf[i] & 7;
            if (b->tree && b->tree[i] == 1) {
                // a luma-only CU: its left / top edge is an edge of the chroma block (the chroma-only CU that follows) only on that block's border
                const int j = closing_chroma_cu(b, i);
                if (b->x[i] != b->x[j]) r.pred_mode |= CU_NOCH_L;          // (containment was validated in pass 1)
                if (b->y[i] != b->y[j]) r.pred_mode |= CU_NOCH_T;
            }
            r.refi[0] = b->refi[i * 2]; r.refi[1] = b->refi[i * 2 + 1];
            r.qp_map = (uint8_t)((b->qp[i * 3] - bdoff) & 0x7F);
            r.map_cbf = (uint8_t)((r.cbf & 1) && (!(r.log2w > 6 || r.log2h > 6) || !b->cbf_sub || (b->cbf_sub[i] & 1)));
            r.coef_off = b->coef_off[i];
            memcpy(r.mv, &b->mv[i * 4], sizeof(r.mv));
            r.qp[0] = b->qp[i * 3]; r.qp[1] = b->qp[i * 3 + 1]; r.qp[2] = b->qp[i * 3 + 2];
            if (b->ipm) { r.ipm[0] = b->ipm[i * 2]; r.ipm[1] = b->ipm[i * 2 + 1]; }
            r.ats_inter = (uint8_t)ats_inter_of(b, i);
            if (dmvr_cand(b, i)) {
                r.dmvr = 1;
                const int dxs = std::min(1 << b->log2w[i], 16), dys = std::min(1 << b->log2h[i], 16);
                for (int sy = 0; sy < (1 << b->log2h[i]); sy += dys)
                    for (int sx = 0; sx < (1 << b->log2w[i]); sx += dxs) {
                        DmvrItem &it = dmvr_items[dmvr_fill++];
                        it.cu = (uint32_t)i; it.sx = (uint8_t)(sx >> 2); it.sy = (uint8_t)(sy >> 2); it.pad = 0;
                    }
            }
            for_each_tb(b, i, [&](int k, int sb, int cls, int tw, int th, int cl, uint32_t comp_off) {
                TbRec &t = tbs[cls_fill[cls]++];
                t.off = r.coef_off + comp_off + ((uint32_t)(sb >> 1) << (th + cl)) + ((uint32_t)(sb & 1) << tw);
                t.log2w = (uint8_t)tw; t.log2h = (uint8_t)th; t.qp = r.qp[k]; t.log2s = (uint8_t)cl;
            });
        }
        });
    }
    // work items of the largest blocks first: an item of 64x64 blocks runs longest (two 64-point passes over 4096 samples), and what is launched last is the tail
    void fill_work_items(TbWave *wv)
    {
        int w = 0;
        for (int sz = 12; sz >= 2; sz--)
        for (int k = 0; k < NCLS; k++) {
            if (!cls_count[k] || ((k & 63) >> 3) + (k & 7) != sz) continue;
            const int per = itdq_group_size((k & 63) >> 3, k & 7);
            for (int f = 0; f < cls_count[k]; f += per) {
                wv[w].first = cls_first[k] + f; wv[w].count = (uint16_t)std::min(per, cls_count[k] - f);
                wv[w].log2w = (uint8_t)((k & 63) >> 3); wv[w].log2h = (uint8_t)(k & 7);
                wv[w].tr_v = (uint8_t)((k >> 6) / 3); wv[w].tr_h = (uint8_t)((k >> 6) % 3); wv[w].pad[0] = wv[w].pad[1] = 0; w++;
            }
        }
    }
    // the inter items with their CU's record (a region- or tile-role wave goes item -> reference windows, no CU-record fetch in between), and the arrays copied as they are
    void fill_items_and_copies(const StageLayout &L, void *hs)
    {
        memcpy(L.at<uint8_t>(hs, SEG_CTU), b->ctu_cu_start, L.payload[SEG_CTU]);
        InterItem *const it = L.at<InterItem>(hs, SEG_IITEM); const CuRec *const cus = L.at<CuRec>(hs, SEG_CUS);
        const uint32_t *const ii = S.inter_items.data(); const size_t n_items = S.inter_items.size();
        S.pool.run(nthr, [&, it, ii](int part) {
            for (size_t k = n_items * (size_t)part / nthr; k < n_items * (size_t)(part + 1) / nthr; k++) {
                if (ii[k] == 0xFFFFFFFFu) memset(&it[k], 0, sizeof(InterItem));
                else { it[k].pos = 0; it[k].cu = ii[k]; it[k].pad[0] = it[k].pad[1] = 0; it[k].rec = cus[ii[k]]; }
            }
        });
        if (L.payload[SEG_IWORK]) memcpy(L.at<uint8_t>(hs, SEG_IWORK), S.inter_work.data(), L.payload[SEG_IWORK]);
        if (L.payload[SEG_COEF]) copy_sliced(L.at<uint8_t>(hs, SEG_COEF), b->coef, L.payload[SEG_COEF]);      // the largest array (45 MB at 8K)
        if (L.payload[SEG_INTRA]) memcpy(L.at<uint8_t>(hs, SEG_INTRA), S.plan.recs.data(), L.payload[SEG_INTRA]);
        if (L.payload[SEG_DEPS]) memcpy(L.at<uint8_t>(hs, SEG_DEPS), S.plan.deps.data(), L.payload[SEG_DEPS]);
    }
    // one copy: the staging block has the device layout (a pinned coefficient arena goes from the caller's buffer).  On the upload stream: the
    // copy overlaps the kernels of the pictures before; xgpu_batch_recon makes the kernel stream wait for `uploaded`
    hipError_t upload(xgpu_dbatch *db, const StageLayout &L, bool coef_pinned)
    {
        uint8_t *const dbase = db->blk.d_base;
        hipError_t e = hipMemcpyAsync(dbase, db->h_stage, coef_pinned ? L.off[SEG_COEF] : L.stage_bytes, hipMemcpyHostToDevice, c->up_stream);
        if (e == hipSuccess && coef_pinned) e = hipMemcpyAsync(dbase + L.off[SEG_COEF], b->coef, sizeof(int16_t) * b->n_coef, hipMemcpyHostToDevice, c->up_stream);
        if (e == hipSuccess && db->n_chroma_cus) e = hipMemcpyAsync(db->d_chroma_cus, db->h_chroma_cus, sizeof(uint32_t) * (size_t)db->n_chroma_cus, hipMemcpyHostToDevice, c->up_stream);
        if (e == hipSuccess) e = hipMemsetAsync(db->d_intra_done, 0, L.alloc[SEG_DONE], c->up_stream);
        if (e == hipSuccess) e = hipMemsetAsync(db->d_resid, 0, L.alloc[SEG_RESID], c->up_stream);
        if (e == hipSuccess) e = hipEventRecord(db->blk.uploaded, c->up_stream);
        return e;
    }
};
void batch_info_fill(const xgpu_dbatch *db, int info[XGPU_BATCH_INFO_COUNT])
{
    info[0] = db->n_cu; info[1] = db->n_tb; info[2] = db->n_waves; info[3] = db->n_intra; info[4] = db->n_intra_l1; info[5] = db->n_levels; info[6] = db->n_dmvr; info[7] = db->n_aff_eif + db->n_aff_sub;
}
// host_only (xgpu_test_build_batch): everything but the device - the staging block is the caller's scratch, nothing is uploaded; *layout receives where the arrays lie
int batch_build(xgpu_ctx *c, const xgpu_cu_batch *b, xgpu_dbatch **out, bool host_only, StageLayout *layout, const BuilderScratch **scratch_out = nullptr)
{
    ARGCHK(c, c != NULL); ARGCHK(c, b != NULL && out != NULL);
    *out = NULL;
    ARGCHK(c, b->n_cu >= 0 && b->n_ctu == c->w_ctu * c->h_ctu);
    ARGCHK(c, b->n_cu == 0 || (b->x && b->y && b->log2w && b->log2h && b->pred_mode && b->refi && b->mv && b->qp && b->cbf && b->coef_off));
    ARGCHK(c, b->ctu_cu_start != NULL && (b->n_coef == 0 || b->coef != NULL));
    ARGCHK(c, b->htdf_slice_qp >= 0 && b->htdf_slice_qp <= 51);
    ARGCHK(c, b->ctu_cu_start[0] == 0 && b->ctu_cu_start[b->n_ctu] == (uint32_t)b->n_cu);      // the kernels index the CU records through it
    for (int k = 0; k < b->n_ctu; k++) ARGCHK(c, b->ctu_cu_start[k] <= b->ctu_cu_start[k + 1]);
    TileMask tmask; ARGCHK(c, tile_mask(c, b->tiles, tmask));
    if (!host_only) HIPCHK(c, hipSetDevice(c->sp.device));
    static const bool bt_on = getenv("XEVD_HIP_BUILD_TRACE") != NULL;      // phase times of the builder on stderr
    auto bt_t0 = std::chrono::steady_clock::now();
    auto BT = [&](const char *what) { if (bt_on) { const auto t = std::chrono::steady_clock::now(); fprintf(stderr, "  batch build: %-14s %.2f ms\n", what, std::chrono::duration<double, std::milli>(t - bt_t0).count()); bt_t0 = t; } };
    static thread_local BuilderScratch scratch;      // the one thread_local of the builder: phases and workers get it by reference (inside a worker the NAME would mean that thread's own, empty object)
    const int n = b->n_cu;
    Build B = { c, b, scratch, n, std::max(1, std::min(c->builder_threads, std::max(1, n / 4096))) };
    BuilderScratch &S = B.S; const IntraPlan &plan = S.plan;
    if (scratch_out) *scratch_out = &scratch;      // (xgpu_test_inter_lists: the calling thread's own object, valid until its next build)
    if (const int rc = B.pass1()) return rc;
    BT("pass 1");
    B.paint_owner_map();
    BT("owner map");
    B.inter_work_lists();
    BT("inter lists");
    const bool order_rl = B.probe_order_rl();
    ARGCHK(c, B.intra_plan());      // false: an IBC source block that is not reconstructed before its CU
    const int n_intra = (int)plan.recs.size(), n_deps = (int)plan.deps.size();
    BT("intra plan");
    xgpu_dbatch *db = new xgpu_dbatch();
    memset(db, 0, sizeof(*db)); db->host_only = host_only ? 1 : 0;
    db->n_cu = n; db->n_ctu = b->n_ctu; db->n_tb = B.n_tb; db->n_waves = B.n_waves; db->n_coef = b->n_coef; db->n_intra = n_intra; db->n_intra_deps = n_deps; db->n_levels = plan.n_levels; db->n_intra_l1 = plan.n_level1; db->n_intra_l1_small = plan.n_level1_small; db->n_intra_heads = plan.n_heads; db->n_aff_eif = B.n_aff_eif; db->n_aff_sub = B.n_aff_sub; db->n_dmvr = B.n_dmvr; db->has_ibc = plan.has_ibc ? 1 : 0; db->has_htdf = plan.has_htdf ? 1 : 0; db->has_right = plan.has_right ? 1 : 0; db->order_rl = order_rl ? 1 : 0;
    db->tile_starts = tmask; db->tiles_across = b->tiles ? (b->tiles->loop_filter_across_tiles ? 1 : 0) : 1; db->n_inter_work = (int)S.inter_work.size();
    const SegSize rows[] = { { SEG_CUS, sizeof(CuRec), (size_t)n, 1 }, { SEG_CTU, sizeof(uint32_t), (size_t)b->n_ctu + 1, 1 }, { SEG_TBS, sizeof(TbRec), (size_t)B.n_tb, 1 }, { SEG_WAVES, sizeof(TbWave), (size_t)B.n_waves, 1 },
        { SEG_INTRA, sizeof(IntraRec), (size_t)n_intra, 1 }, { SEG_DEPS, sizeof(uint32_t), (size_t)n_deps, 1 }, { SEG_AFF, sizeof(AffItem), (size_t)(B.n_aff_eif + B.n_aff_sub), 1 }, { SEG_CPMV, sizeof(int16_t) * 12, (size_t)B.n_aff, 1 },
        { SEG_DMVR, sizeof(DmvrItem), (size_t)B.n_dmvr, 1 }, { SEG_OWNER, sizeof(uint32_t), (size_t)c->w_scu * c->h_scu, 0 }, { SEG_IITEM, sizeof(InterItem), S.inter_items.size(), 1 }, { SEG_IWORK, sizeof(uint32_t), S.inter_work.size(), 1 },
        { SEG_COEF, sizeof(int16_t), b->n_coef, 8 }, { SEG_RESID, sizeof(int16_t), b->n_coef, 8 }, { SEG_DONE, sizeof(uint32_t), (size_t)n_intra + 1, 1 }, { SEG_DMV, sizeof(int16_t) * 4, (size_t)B.n_dmvr, 1 } };
    StageLayout L; stage_layout(L, rows); db->stage_bytes = L.stage_bytes;
    auto fail = [&](int code) { xgpu_batch_destroy(c, db); return code; };
    // local dual trees: the chroma-only CUs that carry chroma coefficients, for xgpu_batch_residual (the owner map names the luma CUs).  Kept by the batch
    // object, not in the staging block
    if (b->tree && !host_only) {
        int nc = 0;
        for (int i = 0; i < n; i++) nc += b->tree[i] == 2 && (b->cbf[i] & 6);
        if (nc) {
            db->h_chroma_cus = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)nc);
            if (!db->h_chroma_cus) return fail(XGPU_ERR_OUT_OF_MEMORY);
            for (int i = 0; i < n; i++) if (b->tree[i] == 2 && (b->cbf[i] & 6)) db->h_chroma_cus[db->n_chroma_cus++] = (uint32_t)i;
        }
    }
    bool coef_pinned = host_only && b->n_coef != 0;      // (the builder alone: the coefficient copy - a plain memcpy, skipped for pinned arenas - stays out of the measurement)
    if (const int rc = B.acquire_block(db, L, coef_pinned)) return fail(rc);
    if (coef_pinned) L.payload[SEG_COEF] = 0;            // nothing of it in the staging block
    BT("block");
    void *const hs = db->h_stage = db->blk.h_stage;
    B.copy_sliced(L.at<uint8_t>(hs, SEG_OWNER), S.own.data(), L.payload[SEG_OWNER]);
    B.fill_records(L, hs);
    B.fill_work_items(L.at<TbWave>(hs, SEG_WAVES));
    B.fill_items_and_copies(L, hs);
    uint8_t *const dbase = db->blk.d_base;
    db->d_cus = L.at<CuRec>(dbase, SEG_CUS); db->d_ctu_start = L.at<uint32_t>(dbase, SEG_CTU); db->d_tbs = L.at<TbRec>(dbase, SEG_TBS);
    db->d_waves = L.at<TbWave>(dbase, SEG_WAVES); db->d_intra = L.at<IntraRec>(dbase, SEG_INTRA); db->d_intra_deps = L.at<uint32_t>(dbase, SEG_DEPS);
    db->d_aff_items = L.at<AffItem>(dbase, SEG_AFF); db->d_cpmv = L.at<int16_t>(dbase, SEG_CPMV);
    db->d_dmvr_items = L.at<DmvrItem>(dbase, SEG_DMVR); db->d_dmvr_mv = L.at<int16_t>(dbase, SEG_DMV); db->d_owner = L.at<uint32_t>(dbase, SEG_OWNER);
    db->d_inter_items = L.at<InterItem>(dbase, SEG_IITEM); db->d_inter_work = L.at<uint32_t>(dbase, SEG_IWORK);
    db->d_coef = L.at<int16_t>(dbase, SEG_COEF); db->d_resid = L.at<int16_t>(dbase, SEG_RESID); db->d_intra_done = L.at<uint32_t>(dbase, SEG_DONE);
    BT("stage filled");
    if (layout) *layout = L;
    if (host_only) { *out = db; return XGPU_OK; }
    const hipError_t e = B.upload(db, L, coef_pinned);
    if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "batch upload: %s", hipGetErrorString(e)); return fail(XGPU_ERR_UNEXPECTED); }
    BT("uploads queued");
    *out = db; return XGPU_OK;
}
}      // namespace
int xgpu_batch_create(xgpu_ctx *c, const xgpu_cu_batch *b, xgpu_dbatch **out) { return batch_build(c, b, out, false, NULL); }

// Test shim (no device, no HIP call): the host batch builder alone on `threads` builder threads -> digest[k] = FNV-1a of array k of the staging block (CU records, CTU
// starts, TB records, work items, intra records, dependency lists, affine tiles, control points, DMVR sub-blocks, owner map, coefficients, inter items, inter work), info
// as xgpu_batch_info, *ms = the builder's wall time.  What the CPU suite uses to pin the builder (goldens of the digests, independence of the thread count).
int xgpu_test_build_batch(const xgpu_seq_params *sp, const xgpu_cu_batch *b, int threads, uint64_t digest[XGPU_TEST_BUILD_DIGESTS], int info[XGPU_BATCH_INFO_COUNT], double *ms)
{
    if (!sp || !b || !digest || threads < 1 || threads > 64) return XGPU_ERR_INVALID_ARGUMENT;
    if (sp->width <= 0 || sp->height <= 0 || (sp->width & 7) || (sp->height & 7) || sp->log2_ctu < 5 || sp->log2_ctu > 7) return XGPU_ERR_INVALID_ARGUMENT;
    xgpu_ctx *c = new xgpu_ctx();
    c->sp = *sp; c->sp.chroma_qp_table[0] = c->sp.chroma_qp_table[1] = NULL;
    c->builder_threads = threads; c->err[0] = 0;
    c->stream = c->up_stream = c->down_stream = c->side_stream = 0;
    ctx_geometry(c);
    xgpu_dbatch *db = NULL;
    StageLayout L;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = batch_build(c, b, &db, true, &L);
    if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc == XGPU_OK) {
        static const Seg order[] = { SEG_CUS, SEG_CTU, SEG_TBS, SEG_WAVES, SEG_INTRA, SEG_DEPS, SEG_AFF, SEG_CPMV, SEG_DMVR, SEG_OWNER, SEG_COEF, SEG_IITEM, SEG_IWORK };
        for (int k = 0; k < XGPU_TEST_BUILD_DIGESTS; k++) {
            uint64_t h = 1469598103934665603ull;
            if (k < (int)(sizeof(order) / sizeof(order[0]))) { const uint8_t *p = L.at<uint8_t>(db->h_stage, order[k]); for (size_t i = 0; i < L.payload[order[k]]; i++) { h ^= p[i]; h *= 1099511628211ull; } }
            digest[k] = h;
        }
        if (info) batch_info_fill(db, info);
        xgpu_batch_destroy(c, db);
    }
    delete c;
    return rc;
}

// Test shim (no device, no HIP call), beside xgpu_test_build_batch: the two arrays inter_work_lists() leaves for k_inter, copied out as they are - work[k]: the roles of
// region k in strip order, items[4 * k + q]: the CU the whole tile q of region k lies in (0xFFFFFFFF: none).  *n_work receives the number of regions; with
// work == items == NULL only the count is returned; one of them alone, or room for fewer than that many regions (cap_work), is an invalid argument (the count is still returned).  tests/mc_launch.py holds its restatement of the role rule to these arrays.
int xgpu_test_inter_lists(const xgpu_seq_params *sp, const xgpu_cu_batch *b, int threads, uint32_t *work, uint32_t *items, int cap_work, int *n_work)
{
    if (!sp || !b || !n_work || threads < 1 || threads > 64 || (work == NULL) != (items == NULL) || cap_work < 0) return XGPU_ERR_INVALID_ARGUMENT;
    if (sp->width <= 0 || sp->height <= 0 || (sp->width & 7) || (sp->height & 7) || sp->log2_ctu < 5 || sp->log2_ctu > 7) return XGPU_ERR_INVALID_ARGUMENT;
    xgpu_ctx *c = new xgpu_ctx();
    c->sp = *sp; c->sp.chroma_qp_table[0] = c->sp.chroma_qp_table[1] = NULL;
    c->builder_threads = threads; c->err[0] = 0;
    c->stream = c->up_stream = c->down_stream = c->side_stream = 0;
    ctx_geometry(c);
    xgpu_dbatch *db = NULL;
    StageLayout L;
    const BuilderScratch *S = nullptr;
    int rc = batch_build(c, b, &db, true, &L, &S);
    if (rc == XGPU_OK) {
        const size_t n = S->inter_work.size();
        *n_work = (int)n;
        if (work) {
            if ((size_t)cap_work < n || S->inter_items.size() != 4 * n) rc = XGPU_ERR_INVALID_ARGUMENT;      // too little room: the count is returned, nothing is written
            else {
                memcpy(work, S->inter_work.data(), n * sizeof(uint32_t));
                memcpy(items, S->inter_items.data(), 4 * n * sizeof(uint32_t));
            }
        }
        xgpu_batch_destroy(c, db);
    }
    delete c;
    return rc;
}

void block_free(BatchBlock &blk)
{
    for (void *p : { (void *)blk.d_base, (void *)blk.d_chroma }) if (p) (void)hipFree(p);
    if (blk.h_stage) (void)hipHostFree(blk.h_stage);
    for (hipEvent_t e : { blk.uploaded, blk.done, blk.itdq_done }) if (e) (void)hipEventDestroy(e);
    memset(&blk, 0, sizeof(blk));
}

void xgpu_batch_destroy(xgpu_ctx *c, xgpu_dbatch *db)
{
    if (!db) return;
    if (db->host_only) { delete db; return; }      // xgpu_test_build_batch: the staging block is the builder's scratch, nothing else was acquired
    if (db->h_chroma_cus) {      // the list's upload reads it: the copy has left the host memory once `uploaded` has happened
        if (db->blk.uploaded) (void)hipEventSynchronize(db->blk.uploaded);
        free(db->h_chroma_cus);
        db->h_chroma_cus = NULL;
    }
    // No synchronisation: kernels still queued on the context's stream keep reading the block; whoever reuses it makes the upload stream wait
    // for the `done` event those kernels signal, and the host waits for `uploaded` before it touches the staging block.
    // The event is recorded here, not behind the batch's kernels: a marker between two kernels of a picture idles the device for ~6 us (profiles/round3_trace_window.txt),
    // and a batch that stays resident (decoded again and again) never needs it.
    if (db->blk.d_base && db->blk.h_stage && db->blk.uploaded && db->blk.done && db->blk.itdq_done && c) {
        if (db->prepared == 1) (void)hipStreamWaitEvent(c->stream, db->blk.itdq_done, 0);      // a residual pass on the side stream that nobody consumed
        if (db->used || db->prepared) (void)hipEventRecord(db->blk.done, c->stream);
        std::lock_guard<std::mutex> g(c->pool_mu); c->pool.push_back(db->blk);
    }
    else {      // a block whose acquisition failed half way
        if (c && c->stream) (void)hipStreamSynchronize(c->stream);
        block_free(db->blk);
    }
    delete db;
}
int xgpu_set_builder_threads(xgpu_ctx *c, int n)
{
    ARGCHK(c, c != NULL); ARGCHK(c, n >= 1 && n <= 64);
    c->builder_threads = n;
    return XGPU_OK;
}
int xgpu_batch_info(xgpu_ctx *c, const xgpu_dbatch *db, int info[XGPU_BATCH_INFO_COUNT])
{
    ARGCHK(c, c != NULL); ARGCHK(c, db != NULL && info != NULL);
    batch_info_fill(db, info);
    return XGPU_OK;
}
int xgpu_batch_wait_upload(xgpu_ctx *c, xgpu_dbatch *db)
{
    ARGCHK(c, c != NULL); ARGCHK(c, db != NULL);
    HIPCHK(c, hipEventSynchronize(db->blk.uploaded));
    return XGPU_OK;
}
