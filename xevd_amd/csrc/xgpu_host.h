// xgpu_host.h - what the host-side translation units of the backend share (xgpu_api.hip: context, pictures, output into host memory; xgpu_output.hip: the outputs
// into device memory; xgpu_builder.hip: the batch builder; xgpu_intra_plan.hip: its dependency plan; xgpu_launch.hip: the per-picture launch sequencing;
// xgpu_shims.hip: the fine-grained test shims).  Private to xevd_amd/csrc.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include "xgpu_internal.h"

#define HIPCHK(c, expr)                                                                                         \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            snprintf((c)->err, sizeof((c)->err), "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return XGPU_ERR_UNEXPECTED;                                                                         \
        }                                                                                                       \
    } while (0)
#define ARGCHK(c, cond)                                                                                         \
    do {                                                                                                        \
        if (!(cond)) {                                                                                          \
            if (c) snprintf((c)->err, sizeof((c)->err), "%s:%d invalid argument: %s", __FILE__, __LINE__, #cond); \
            return XGPU_ERR_INVALID_ARGUMENT;                                                                   \
        }                                                                                                       \
    } while (0)


static inline int align_up(int v, int a) { return (v + a - 1) / a * a; }
// the picture geometry of a context, from c->sp (xgpu_open, and the device-less context of xgpu_test_build_batch)
static inline void ctx_geometry(xgpu_ctx *c)
{
    const int w = c->sp.width, h = c->sp.height, ctu = 1 << c->sp.log2_ctu;
    c->w_scu = w >> 2; c->h_scu = h >> 2; c->w_ctu = (w + ctu - 1) / ctu; c->h_ctu = (h + ctu - 1) / ctu;
    c->s_l = align_up(XGPU_MARGIN_L + w + XGPU_PAD_L, 64); c->s_c = align_up(XGPU_MARGIN_C + (w >> 1) + XGPU_PAD_C, 64);
    c->rows_l = h + 2 * XGPU_PAD_L; c->rows_c = (h >> 1) + 2 * XGPU_PAD_C;
    c->off_u = (size_t)c->s_l * c->rows_l; c->off_v = c->off_u + (size_t)c->s_c * c->rows_c;
    c->pic_elems = c->off_v + (size_t)c->s_c * c->rows_c + 64;   // +64: slack for the 16-byte window over-read of the last row
}
static inline bool valid_pic(const xgpu_ctx *c, int pic) { return pic >= 0 && pic + 1 < (int)c->pics.size() && c->pics[pic + 1].used; }
static inline DevPic &dpic(xgpu_ctx *c, int pic) { return c->pics[pic + 1]; }
// ADDB directly followed by ALF runs as ONE kernel (k_addb_alf)
static inline bool addb_alf_fused(const xgpu_ctx *c) { return c->fp.deblock_on && c->sp.tool_addb && c->fp.alf_on && !c->split_addb_alf; }

// HIP-event kernel timing (xgpu_api.hip)
void time_begin(xgpu_ctx *c, int k, hipEvent_t *a, hipEvent_t *b);
void time_end(xgpu_ctx *c, int k, hipEvent_t a, hipEvent_t b);
#define TIMED(c, k, stmt)                      \
    do {                                       \
        hipEvent_t ta_ = 0, tb_ = 0;           \
        time_begin(c, k, &ta_, &tb_);          \
        stmt;                                  \
        time_end(c, k, ta_, tb_);              \
    } while (0)

// the DRA post-filter's inverse tables of an output call (xgpu_api.hip): what upload_dra refuses, and the upload to c->d_dra on the context's stream
// (hidden: shared by two files of the library, not a name it exports)
__attribute__((visibility("hidden"))) int check_dra(xgpu_ctx *c, const xgpu_dra_luts *dra);
__attribute__((visibility("hidden"))) int upload_dra(xgpu_ctx *c, const xgpu_dra_luts *dra);

// xgpu_tile_grid -> TileMask; false: not a partition of the picture's CTU grid
inline bool tile_mask(const xgpu_ctx *c, const xgpu_tile_grid *g, TileMask &m)
{
    memset(&m, 0, sizeof(m));
    if (!g) return true;
    if (g->n_cols < 1 || g->n_cols > XGPU_MAX_TILE_COLS || g->n_rows < 1 || g->n_rows > XGPU_MAX_TILE_ROWS || c->w_ctu > 256 || c->h_ctu > 256) return false;
    if (g->col_bd[0] != 0 || g->row_bd[0] != 0 || g->col_bd[g->n_cols] != c->w_ctu || g->row_bd[g->n_rows] != c->h_ctu) return false;
    for (int i = 0; i < g->n_cols; i++) if (g->col_bd[i + 1] <= g->col_bd[i]) return false;
    for (int j = 0; j < g->n_rows; j++) if (g->row_bd[j + 1] <= g->row_bd[j]) return false;
    for (int i = 1; i < g->n_cols; i++) m.vb[g->col_bd[i] >> 5] |= 1u << (g->col_bd[i] & 31);
    for (int j = 1; j < g->n_rows; j++) m.hb[g->row_bd[j] >> 5] |= 1u << (g->row_bd[j] & 31);
    return true;
}

// HTDF (xevdm.c:1381-1392 with xevdm_htdf_skip_condition, xevdm_recon.c:270-297): which CUs are filtered right after their reconstruction, and with which of the five
// tables (-1: not filtered).  Such a CU - inter ones included - reads the final samples of the CUs before it and is read by the ones after it: it is a node of the
// dependency graph next to the intra and IBC CUs
static inline int plan_htdf_idx(const xgpu_cu_batch *b, uint32_t j)
{
    const int hqp = b->htdf_slice_qp;
    const bool intra = b->pred_mode[j] == XGPU_MODE_INTRA;
    if (hqp <= 17 || (b->tree && b->tree[j] == 2) || b->pred_mode[j] == XGPU_MODE_IBC || !((b->cbf[j] & 1) || intra)) return -1;
    const int w = 1 << b->log2w[j], h = 1 << b->log2h[j], mn = std::min(w, h), mx = std::max(w, h);
    if (w * h < 64 || mx >= 128 || (!intra && mn >= 32)) return -1;
    const int qp = hqp - ((intra && w == h && mn >= 32) ? 8 : 0);
    return std::min(std::max((qp - 20 + 4) >> 3, 0), 4);
}
static inline bool plan_is_node(const xgpu_cu_batch *b, uint32_t j) { return b->pred_mode[j] == XGPU_MODE_INTRA || b->pred_mode[j] == XGPU_MODE_IBC || plan_htdf_idx(b, j) >= 0; }
// the dependency plan of a batch (xgpu_intra_plan.hip): the records of k_intra.hip's list and their waiting lists (list positions)
struct IntraPlan {
    std::vector<IntraRec> recs; std::vector<uint32_t> deps; bool has_ibc, has_htdf, has_right;
    int n_levels, n_level1, n_level1_small, n_heads;      // n_heads: level-1 CUs + strand heads = the part of the list the launches range over
    void reset() { recs.clear(); deps.clear(); n_levels = n_level1 = n_level1_small = n_heads = 0; has_ibc = has_htdf = has_right = false; }
};
struct PlanOut { std::vector<uint32_t> deps; bool ibc = false, htdf = false, right = false, bad = false; };      // one thread of the plan's parallel mode: its lists, the k_intra instantiations its nodes ask for
// What a caller of the builder keeps between pictures, ONE object per calling thread: the worker threads, and working arrays of 6 - 60 MB at 8K (allocated per call they
// go through mmap / munmap, whose TLB shootdown reaches every thread of the process).  Each is (re)initialised where a phase uses it: a refused batch leaves it usable.
struct BuilderScratch {
    WorkPool pool;
    IntraPlan plan;
    // the builder: SCU -> CU map; per 32x32 tile its one CU / any CU; k_inter's work lists; the plan's nodes in decoding order; the staging block of a host-only build
    std::vector<uint32_t> own, tile_cu, inter_items, inter_work, nodes;
    std::vector<uint8_t>  tile_any, host_stage;
    // the plan: sequential mode's SCU maps; nodes in decoding order + their lists (CU indices); CU -> record, record -> successor, CU -> position, record -> first dependency
    std::vector<uint32_t> owner_own, luma_owner, deps, succ, pos, nfirst;
    std::vector<int> level; std::vector<IntraRec> recs; std::vector<PlanOut> outs; std::vector<int32_t> rec_of_cu; std::vector<uint8_t> member;
};
__attribute__((visibility("hidden"))) bool build_intra_plan(xgpu_ctx *c, const xgpu_cu_batch *b, BuilderScratch &S, const uint32_t *final_owner, int nthr);      // S.nodes -> S.plan; false: an invalid batch
__attribute__((visibility("hidden"))) void block_free(BatchBlock &blk);      // frees what a block holds (xgpu_batch_destroy, xgpu_close)
