// xgpu_internal.h - device-side record formats and the context of the MI355X reconstruction backend.
// Everything here is private to xevd_amd/csrc; the public boundary is include/xevd_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include "../../include/xevd_hip.h"

// ---------------------------------------------------------------------------------------------------------
// Device picture.  16-bit planar 4:2:0 like the reference's XEVD_PIC (src_base/xevd_def.h:630-679), but with a
// geometry chosen for HBM: the first active sample of every row is 256-byte aligned (left margin 192 luma /
// 128 chroma samples >= the reference's 144 / 72 padding) and the row stride is a multiple of 64 samples, so
// that a wave's 128-byte row segments never straddle more cache lines than necessary.
// ---------------------------------------------------------------------------------------------------------
#define XGPU_MARGIN_L 192
#define XGPU_MARGIN_C 128

struct DevPic {
    int16_t *base;        // one allocation: Y, U, V padded planes
    int16_t *y, *u, *v;   // first active sample of each plane
    int      s_l, s_c;    // strides in samples
    int      used;
};

// Per-CU record on the device: 32 bytes, read as two 16-byte loads.  Built on the host from the SoA batch of the
// ABI because every consumer (inter kernel, map update, TB list) needs all fields of a CU together.
struct __attribute__((aligned(16))) CuRec {
    uint16_t x, y;            // luma sample position
    uint8_t  log2w, log2h;
    uint8_t  pred_mode;       // XGPU_MODE_*
    uint8_t  cbf;             // bit c: component c coded
    int8_t   refi[2];
    uint8_t  qp_map;          // core->qp = qp_y - 6*(bd-8): the QP stored in map_scu (xevd_util.c:1626)
    uint8_t  map_cbf;         // luma cbf bit of the SCU map = is_coef_sub[Y_C][0] (xevd_util.c:1615)
    uint32_t coef_off;        // offset of the CU's residual block in the arena (s16 units)
    int16_t  mv[2][2];        // unclipped quarter-pel
    uint8_t  qp[3];           // dequant QPs
    uint8_t  ipm[2];
    uint8_t  ats_inter;       // ats_inter_info of an inter CU (idx | pos << 4), 0 = whole-CU transform
    uint8_t  affine;          // 0, or the number of control points (2 / 3) of an affine CU: predicted by k_affine, not k_inter
    uint8_t  dmvr;            // 1: a DMVR candidate with two references and at least 8x8 samples - predicted by k_dmvr when the picture's POCs allow (else k_inter)
};
static_assert(sizeof(CuRec) == 32, "CuRec must be 32 bytes");

// SCU map record: the reference's map_scu / map_refi / map_mv (xevd_def.h:372-438) fused into one 16-byte
// element so that a deblocking lane fetches a neighbour with one load.
struct __attribute__((aligned(16))) ScuRec {
    uint32_t scu;             // bit 15 intra, 16-22 QP, 23 skip, 24 luma cbf, 31 COD; bits 8/9: left/top CU edge; bits 0-7, 12-14: SCU_RANK
    int8_t   refi[2];
    uint16_t ats_inter;       // mctx->map_ats_inter of the SCU (ADDB: non-zero on either side of an edge -> bS 2)
    int16_t  mv[2][2];
};
static_assert(sizeof(ScuRec) == 16, "ScuRec must be 16 bytes");
#define SCU_EDGE_L (1u << 8)      // the SCU's left edge is a CU boundary  (free bits 7:14 of map_scu)
#define SCU_EDGE_T (1u << 9)      // the SCU's top edge is a CU boundary
#define SCU_NOCH_L (1u << 10)     // ... but not an edge of the chroma block (a luma-only CU inside a local dual tree): the filters leave chroma alone there
#define SCU_NOCH_T (1u << 11)
// bits 0-7 and 12-14: the low 11 bits of the CU's index in the batch = its place in decoding order.  The baseline deblocking filter of the Main library reaches a
// vertical CU edge with the LATER of the two CUs (xevdm_df.c:186-330: left edge when the left neighbour is done, right edge when the right one is), so with
// sps_suco_flag chroma edges 2 samples apart are not always applied left to right; two CUs of one CTU are at most 320 places apart, CTUs follow each other
#define SCU_RANK(idx)  (((uint32_t)(idx) & 0xFFu) | ((((uint32_t)(idx) >> 8) & 7u) << 12))
#define SCU_RANK_OF(m) ((int)(((m) & 0xFFu) | (((m) >> 4) & 0x700u)))
#define CU_NOCH_L 0x40            // CuRec.pred_mode bits 6 / 7 carry the two flags to k_inter's map pass (bits 0-3: XGPU_MODE_*)
#define CU_NOCH_T 0x80

// One coded transform block for the dequant + inverse-transform kernel.
struct TbRec {
    uint32_t off;             // arena offset (s16 units) of the TB's first coefficient
    uint8_t  log2w, log2h, qp;
    uint8_t  log2s;           // log2 of the row stride: = log2w, or log2 of the CU width for a 64x64 sub-block of a larger CU
};
// transform kinds of a work item (wave-uniform): 0 = DCT-II, 1 = DST-VII, 2 = DCT-VIII (ATS, src_main/xevdm_itdq.c:163-421)
#define TR_DCT2 0
#define TR_DST7 1
#define TR_DCT8 2
// One 256-thread work item of the itdq kernel: `count` consecutive TbRecs of one size class.
struct TbWave {
    uint32_t first;
    uint16_t count;
    uint8_t  log2w, log2h;
    uint8_t  tr_v, tr_h;      // TR_* of the vertical (first) and horizontal (second) stage
    uint8_t  pad[2];
};

#define XGPU_WORK_REGION 0x100u
#define XGPU_INTER_STRIP 16       // width, in 64x64 regions, of the vertical strips the inter work lists are ordered in (xgpu_batch_create, k_inter.hip)
// One item of the two uniform work lists: where, which CU, and the CU's record (the kernels need no second fetch to start their window requests)
struct __attribute__((aligned(16))) InterItem { uint32_t pos, cu, pad[2]; CuRec rec; };
static_assert(sizeof(InterItem) == 48, "InterItem must be 48 bytes");
struct RefEntry { const int16_t *y, *u, *v; int poc; int pad; };

// Kernel arguments of the inter reconstruction kernel (passed by value).
struct InterArgs {
    int16_t *cur_y, *cur_u, *cur_v;
    int      s_l, s_c;                 // all pictures of a ctx share the geometry
    int      pic_w, pic_h;
    int      bd_l, bd_c;
    int      admvp;
    // One entry of `work` per 64x64 region of the PICTURE, in vertical strips XGPU_INTER_STRIP regions wide, row by row inside a strip (every XCD takes a contiguous
    // eighth of that order: a compact patch of the picture): XGPU_WORK_REGION = the region lies inside one CU of the batch; else two bits per 32x32 tile of the
    // region (bits 2q.. for tile q = column | row << 1): 0 no SCU of the batch, 1 the tile lies inside one CU, 2 every other tile with SCUs of the batch.
    // items[entry * 4 + q]: the CU (index and record) of tile q where it lies inside one CU (all four the same for a region entry), zero elsewhere.
    const uint32_t  *work;
    const InterItem *items;
    int      n_work;
    int      regions_x, strip_entries, full_entries;      // 16 x regions_y; entries in front of the last, narrower strip
    uint32_t magic_strip, magic_last;                     // floor(2^32 / d) + 1 for d = strip_entries and the last strip's width: n / d = mulhi(n, magic) for n x d < 2^32; magic_last 0 = width 1 (or no last strip)
    const CuRec    *cus;
    const int16_t  *resid;
    ScuRec  *maps;
    int      w_scu;
    const uint32_t *owner;             // [w_scu * h_scu] batch index of the CU covering each SCU (0xFFFFFFFF: none), painted by xgpu_batch_create
    int      n_cu;
    int      cur_poc;                  // POC of the picture being decoded (DMVR's distance test)
    int      dmvr_to_map;              // k_dmvr writes its refined vectors into the map records (DmvrArgs.refined_to_map): k_inter leaves those words alone
    RefEntry refp[XGPU_MAX_REFS][2];
};

// DMVR (k_dmvr.hip): one work item per 16x16 (or smaller) sub-block of a candidate CU
struct DmvrItem { uint32_t cu; uint8_t sx, sy; uint16_t pad; };          // CU record index, sub-block origin inside the CU in 4-sample units
struct DmvrArgs {
    int16_t *cur_y, *cur_u, *cur_v;
    int      s_l, s_c;
    int      pic_w, pic_h;
    int      bd_l, bd_c;
    int      admvp, cur_poc;
    const CuRec    *cus;
    const DmvrItem *items;
    int      n_items;
    const int16_t  *resid;
    int16_t *out_mv;                   // [n_items][2][2] quarter-sample vectors kept for temporal prediction
    ScuRec  *maps;                     // the SCU map the deblocking filter reads, and
    int      w_scu, refined_to_map;    // whether it gets the refined vectors (baseline filter of the Main library) or keeps the unrefined ones (ADDB)
    int      force_scalar;             // XEVD_HIP_DMVR_SCALAR: the refined prediction in its scalar form for every sub-block (the form valid input never reaches)
    RefEntry refp[XGPU_MAX_REFS][2];
};

// Affine CUs (k_affine.hip): one work item per tile of an affine CU - 16x16 luma samples in the EIF branch, 32x32 in the translation branch.
struct AffItem { uint32_t cu, aff; uint16_t tx, ty; uint32_t pad; };      // CU record index, index into the control-point array, tile origin in the CU
static_assert(sizeof(AffItem) == 16, "AffItem must be 16 bytes");
struct AffineArgs {
    int16_t *cur_y, *cur_u, *cur_v;
    int      s_l, s_c;
    int      pic_w, pic_h;
    int      bd_l, bd_c;
    int      admvp;
    const CuRec   *cus;
    const int16_t *cpmv;               // [n_affine][2][3][2] quarter-pel control points
    const AffItem *items;              // the EIF tiles (16x16), then the sub-block-translation tiles (32x32)
    int      n_eif, n_sub;
    const int16_t *resid;
    ScuRec  *maps;
    int      w_scu;
    RefEntry refp[XGPU_MAX_REFS][2];
};

// One intra CU of a picture, in dependency-level order.  Availability = the reference's COD flags at the CU's turn
// (xevd_get_nbr_b, src_base/xevd_ipred.c:47-92): bit k of `up` / `le` = the k-th 4-luma-sample unit of the row above /
// the column to the left (cw/4 + ch/4 units each) comes from the picture, else it is mid grey.
struct __attribute__((aligned(16))) IntraRec {
    uint32_t cu;              // index into the CU records
    uint32_t flags;           // bit 0: the up-left sample is available; bit 1: an intra-block-copy CU (then `le` = block vector x | y << 16, `up` = 0);
                              // bit 2: HTDF runs on the CU, bit 3: and nothing else (an inter CU), bit 4: under constrained intra prediction (the up / le masks
                              // pick the border units), bits 8-16: xevd_get_avail_intra's bits 0-8, bits 20-22: table
                              // bits 23 / 24: avail_lr - the SCU left / right of the CU's first row is reconstructed before it (the right one only where
                              // sps_suco_flag reversed a split); with bit 24 the upper half of `up` is the mask of the RIGHT column's units
    uint64_t up, le;
    uint32_t dep_first, dep_count;   // range of the dependency list: positions (in this list) of the intra CUs it reads from
    uint16_t x, y;            // the CU fields the kernel needs, copied here so that one record fetch starts the work
    uint8_t  log2w, log2h, cbf, pad0;
    uint8_t  ipm[2], pad1[2];
    uint32_t coef_off;
};
static_assert(sizeof(IntraRec) == 48, "IntraRec must be 48 bytes");
struct IntraArgs {
    int16_t *cur_y, *cur_u, *cur_v;
    int      s_l, s_c;
    int      bd_l, bd_c;
    const CuRec    *cus;
    const IntraRec *list;
    const uint32_t *deps;
    const int16_t  *resid;
    uint32_t *done;           // [n_intra] = epoch once the CU's samples are published; [n_intra] (one past) = the ticket counter
    uint32_t  epoch, ticket_base;
    int       n_intra;        // list length (the ticket counter sits at done[n_intra])
    int       first, count;   // the list range this launch covers
    int       n_small;        // level-1 launch: the LAST n_small entries of the range are CUs of at most 16 SCUs (the list is sorted by size inside a level): 16 lanes per CU (k_intra.hip)
};

struct ItdqArgs {
    const int16_t *coef;
    int16_t       *resid;
    const TbRec   *tbs;
    const TbWave  *waves;
    int            n_waves;
    int            bd;
    int            iqt;
};

// Tile borders of a picture as bit masks over CTU columns / rows: bit i set = a tile starts at CTU column (row) i > 0.  All zero for one tile.
struct TileMask {
    uint32_t vb[8], hb[8];             // pictures up to 16384 samples = 256 CTUs of 64
    __host__ __device__ bool col_start(int ctu_x) const { return (vb[ctu_x >> 5] >> (ctu_x & 31)) & 1; }
    __host__ __device__ bool row_start(int ctu_y) const { return (hb[ctu_y >> 5] >> (ctu_y & 31)) & 1; }
    // first CTU column / row of the tile that holds CTU i, and one past its last (n = CTUs per picture row / column)
    __host__ __device__ static int tile_first(const uint32_t *m, int i)
    {
        for (int w = i >> 5; w >= 0; w--) {
            uint32_t v = m[w];
            if (w == (i >> 5)) v &= 0xFFFFFFFFu >> (31 - (i & 31));
            if (v) return (w << 5) + 31 - __builtin_clz(v);
        }
        return 0;
    }
    __host__ __device__ static int tile_end(const uint32_t *m, int i, int n)
    {
        for (int w = (i + 1) >> 5; w < 8; w++) {
            uint32_t v = m[w];
            if (w == ((i + 1) >> 5)) v &= 0xFFFFFFFFu << ((i + 1) & 31);
            if (v) { const int e = (w << 5) + __builtin_ctz(v); return e < n ? e : n; }
        }
        return n;
    }
};

struct DbkArgs {
    int      s_l, s_c;
    int      pic_w, pic_h, w_scu, h_scu;
    int      bd_l, bd_c;
    int      ctu_sh;                   // SCUs per CTU = 1 << ctu_sh
    TileMask no_filter;                // tile borders the filter must leave alone (loop_filter_across_tiles = 0; else all zero)
    const ScuRec *maps;
    uint8_t  st[3][4][64];             // strength by component, edge class, map QP (host-built from xevd_tbl_df_st)
};

#define ADDB_LDS_TABLE_BYTES (52 + 52 + 260 + XGPU_MAX_REFS * 2 + 192)
#define ADDB_LDS_TABLE_DWORDS ((ADDB_LDS_TABLE_BYTES + 3) / 4)
struct AddbArgs {
    int      s_l, s_c;
    int      w_scu, h_scu;
    int      bd_l, bd_c, log2_ctu;
    int      alpha_off, beta_off, qp_u_off, qp_v_off;
    TileMask no_filter;                // as in DbkArgs
    const ScuRec *maps;
    int8_t   chroma_qp[2 * 96];        // [c][qp + 6*(bdc-8)]
    uint8_t  pic_id[XGPU_MAX_REFS * 2];// picture slot of refp[idx][list], 255 = none
    // alpha[52] beta[52] clip[260] pic_id[2 * XGPU_MAX_REFS] chroma_qp[192] in the order and at the offsets of k_addb_alf's LDS copy, as dwords
    uint32_t lds_tables[ADDB_LDS_TABLE_DWORDS];
};

#define ALF_CTB_BITS 8704           // 8192 x 4320 in 64 x 64 CTUs
struct AlfArgs {
    int      s_l, s_c, pic_w, pic_h, bd, log2_ctu, w_ctu, across_tiles;
    TileMask tiles;                    // tile starts: a CTU's windows end at its tile (alf_process_tile)
    uint32_t magic_tiles_x;            // floor(2^32 / tiles per row) + 1, set by launch_alf: tile / tiles_x as a multiplication; 0 = one tile per row
    int      multi_tile;               // 0: one tile - the masks are not looked at
    int      pad;                      // 1: the tiles on the picture border also write the 144 / 72-sample padding of the output picture (no k_pad launch)
    int      enable[3];
    const uint8_t *ctb_flag;           // device, [n_ctu] or null
    int      ctb_in_args;              // 1: the per-CTU luma flags travel in ctb_bits (pictures up to ALF_CTB_BITS CTUs): no H2D copy between the kernels
    uint32_t ctb_bits[ALF_CTB_BITS / 32];
    // The luma filter set as the filter loop wants it: for each of the 25 classes and the 4 transpose indices (xevdm_alf.c:268-273) the thirteen coefficients in the
    // block's orientation, packed in the pairs the v_dot2 / v_mad_i32_i16 forms take - (f3,f2) (f8,f7) (f6,f5) (f10,f9) (f12,f11) (f1,f0) (-,f4), high half first - so a
    // lane fetches its filter with two 16-byte loads at (class * 4 + transpose) (xgpu_alf builds it; round 5 read thirteen s16 from an LDS copy of coef_final through a
    // nibble permutation and packed them with run-time shifts, ~70 instructions per lane of a kernel bound by instruction issue).  Argument blocks above 4 KB launch on
    // this runtime (tools/ubench/kernarg_probe.hip: 8 KB tested)
    uint32_t ctab[25 * 4][8];
    uint32_t cchroma[4];               // the chroma filter: (f3,f2) (f5,f4) (f1,f0) (-,f6)
};

// One device block + one pinned staging block of a batch.  xgpu_batch_destroy returns them to the context's pool instead of freeing:
// hipMalloc / hipFree / hipHostMalloc synchronise the device and serialise across the threads of a process, which capped many-stream
// decoding on one GPU (tools/bench_multistream.py) and cost a stream synchronisation per picture.
struct BatchBlock { uint8_t *d_base; size_t d_cap; void *h_stage; size_t h_cap; hipEvent_t uploaded, done, itdq_done;      // uploaded: the H2D copies have left the host memory; done: the reconstruction kernels have read the block
                    uint32_t *d_chroma; size_t chroma_cap; };      // the chroma-only CUs of a batch with local dual trees (xgpu_dbatch.d_chroma_cus): an allocation of its own, made for the first such batch and grown on demand

struct xgpu_dbatch {
    BatchBlock blk;
    int        n_cu, n_ctu, n_tb, n_waves;
    size_t     n_coef;
    CuRec     *d_cus;
    uint32_t  *d_ctu_start;
    uint32_t  *d_owner;               // SCU -> CU index of the batch, over the whole picture
    InterItem *d_inter_items;                        // k_inter's roles per region of the picture and the CUs of its whole tiles (InterArgs)
    uint32_t  *d_inter_work;
    int        n_inter_work;
    int16_t   *d_coef, *d_resid;
    TbRec     *d_tbs;
    TbWave    *d_waves;
    DmvrItem  *d_dmvr_items;          // sub-blocks of the DMVR candidates
    int16_t   *d_dmvr_mv;             // their vectors after xgpu_batch_recon
    int        n_dmvr;
    AffItem   *d_aff_items;           // tiles of the affine CUs
    int16_t   *d_cpmv;
    int        n_aff_eif, n_aff_sub;
    IntraRec  *d_intra;               // intra CUs sorted by dependency level
    uint32_t  *d_intra_deps;          // dependency lists (positions in d_intra)
    uint32_t  *d_intra_done;          // [n_intra] done epochs + [1] ticket counter
    int        has_ibc, has_htdf;     // the intra list holds intra-block-copy CUs / HTDF nodes
    int        order_rl;              // some CU is decoded after its right-hand neighbour (sps_suco_flag; only looked for when the baseline deblocking filter is the one that runs)
    int        has_right;             // ... CUs whose right-hand neighbours are reconstructed first (sps_suco_flag): the instantiations that know the right reference column
    TileMask   tile_starts;           // of the batch's tile grid (zero: one tile)
    int        tiles_across;          // its loop_filter_across_tiles
    int        n_intra_l1_small;      // of the level-1 entries, the ones with at most 16 SCUs (log2 w + log2 h <= 8): they end the level's part of the list
    int        n_intra, n_levels, n_intra_deps, n_intra_l1, n_intra_heads;      // n_intra_l1: CUs of level 1 (head of the list); n_intra_heads: + the strand heads of the data-flow launch (the strand members follow)
    uint32_t   intra_epoch, intra_tickets;
    void      *h_stage;               // pinned staging block
    int        host_only;             // built by xgpu_test_build_batch: h_stage is the builder's scratch, the block holds nothing to free or pool
    size_t     stage_bytes;
    int        prepared;              // 1: xgpu_batch_prepare has queued the residual pass (k_itdq) on the side stream: `blk.itdq_done` says when it has finished;
                                      // 2: it ran on the main stream with the previous picture (xgpu_batch_recon_ahead)
    int        upload_waited;         // the main stream already waits for blk.uploaded
    int        used;                  // kernels that read the block have been queued (xgpu_batch_recon, or a residual pass ahead)
    // xgpu_batch_residual: the chroma-only CUs (local dual tree, tree == 2) that carry chroma coefficients, by batch index - the owner map names the luma CUs only.
    // Not part of the staging block: the host's copy is freed with the batch, the device's lives in blk.d_chroma and is uploaded in front of blk.uploaded
    uint32_t  *h_chroma_cus, *d_chroma_cus;
    int        n_chroma_cus;
};

// the device block of the scaled output's tap tables, as the host laid it out: per table (0 yl, 1 yc, 2 xl, 3 xc) the byte offsets of first[], count[] and w[], the
// weights' stride, and the widest span of source samples 64 neighbouring destination columns reach (pass 2's LDS need), rounded to whole groups of 8
struct ScaleTabs { size_t off_first[4], off_count[4], off_w[4]; int stride[4]; int capy, capc; };
struct ScaleAxisTab { size_t first, count, w; int stride; };      // one table in a host blob: byte offsets of first[], count[] and the weights (xgpu_scale.hip)
struct Lut3dSlot { uint8_t *d; int n; };      // one 3D LUT of a context (xgpu_lut3d_create): its device block - the shaper, then the cube -, NULL = free
// one dither matrix of a context (xgpu_dither_create): mh rows of mw + 16 ranks - each row followed by its own first 16 entries, so that a run of up to 16 ranks
// from any column is contiguous -, NULL = free
struct DitherSlot { uint16_t *d; int mw, mh, k; };
struct xgpu_ctx {
    xgpu_seq_params sp;
    int8_t          chroma_qp[2][96];  // [c][qp + 6*(bdc-8)]
    hipStream_t     stream;            // kernels
    hipStream_t     up_stream, down_stream;      // batch uploads / output downloads: their own DMA queues, ordered against the kernels by events
    hipStream_t     side_stream;       // xgpu_batch_prepare: the residual pass of the NEXT picture, behind the current picture's k_inter (fills the GPU under the
    hipEvent_t      after_inter;       //   latency-bound dependency kernel); after_inter = the point of the main stream it may start behind
    int             have_after_inter;
    std::mutex      pool_mu;           // xgpu_batch_create / _destroy may run on a builder thread next to the thread that drives the context
    struct HostRange { uint8_t *p; size_t n; };
    std::vector<HostRange> pinned;     // xgpu_host_alloc'ed ranges: batch arrays inside them are sent without a staging copy
    int             w_scu, h_scu, w_ctu, h_ctu;
    int             s_l, s_c, rows_l, rows_c;
    size_t          pic_elems, off_u, off_v;
    std::vector<DevPic> pics;
    ScuRec         *d_maps;
    uint8_t        *d_ctb_flag;       // ALF luma CTB flags of the current picture
    std::vector<BatchBlock> pool;     // blocks of destroyed batches, reused by later ones of the same stream (same HIP stream -> ordered)
    uint8_t        *d_out[2];         // packed output pictures (xgpu_pic_output): two in flight, grown on demand
    uint8_t        *d_md5;            // xgpu_pic_md5: the picture's planes as the signature's message (+ 48 bytes of digest behind it), allocated at the first call
    hipEvent_t      md5_ready;
    size_t          out_caps[2];
    hipEvent_t      out_ready[2], out_done[2];      // conversion kernel finished (kernel stream) / copy to the host finished (download stream)
    int             out_busy[2], out_next;
    int32_t        *d_dra;            // [3][1024] DRA inverse tables of the current output call
    float          *d_cm;             // xgpu_pic_output_device_cm: the tables of cm_tab on the device (lin[4096], tone, encode)
    xgpu_colour_tables_t *cm_tab;     // the host's copy, made for (cm_key, cm_bd); NULL until the first call
    xgpu_colour_transform cm_key;
    int             cm_bd;
    // xgpu_pic_output_device_scaled: the four tap tables on the device (sc_tab; made for sc_key = source size, destination size, filter, chroma_loc - all -1 until
    // the first call) and the intermediate of the vertical pass (sc_mid, sc_mid_cap bytes, grown on demand).  Both are the context's, like d_dra and d_cm: every
    // call that uses them is ordered behind the previous one through the context's stream (odev_ev), whichever stream it runs on.
    uint8_t        *sc_tab;
    size_t          sc_tab_cap;
    int             sc_key[6];
    ScaleTabs       sc_host;          // what sc_tab holds: offsets, strides, pass 2's spans
    uint16_t       *sc_mid;
    size_t          sc_mid_cap;
    unsigned long long *cmp_part;     // xgpu_pic_compare: the workgroups' partial sums of the current call (cmp_part_cap bytes, grown on demand), ordered like sc_mid
    size_t          cmp_part_cap;
    // xgpu_pic_stats: one block of STATS_BLK_BYTES, allocated at the first call and ordered like sc_mid - the accumulation block of the histograms (zeroed on
    // the call's stream before its kernels), the lin table of (stats_lin_tc, stats_lin_bd) (-1: none; uploaded again only when they change) and the workgroups'
    // partial sums of the current call
    uint8_t        *stats_blk;
    int             stats_lin_tc, stats_lin_bd;
    // xgpu_pic_output_device_resampled: the descriptor and the four bicubic tap tables of one picture on the device (rs_blk; made for rs_key = source size,
    // destination size, kernel, antialias, chroma_loc - rs_key[0] = -1 until the first call), with pass 2's spans.  Its intermediate is sc_mid.  Ordered like sc_tab.
    uint8_t        *rs_blk;
    size_t          rs_blk_cap;
    int             rs_key[7], rs_capy, rs_capc;
    uint8_t        *roi_blk;          // xgpu_pic_output_device_rois: the descriptors and tap tables of the current call (its intermediate is sc_mid), ordered like sc_tab;
                                      // xgpu_pic_output_device_warp: the host maps of the current call
    size_t          roi_blk_cap;
    // xgpu_pic_output_device_ladder: the records and the tap tables of all rungs in one device block (lad_blk; lad_host is the host's copy, whose tables were
    // made for lad_key = source size, rung sizes, filter, both sitings - empty until the first call); its intermediate is sc_mid.  Ordered like sc_tab.
    uint8_t        *lad_blk;
    size_t          lad_blk_cap;
    std::vector<int> lad_key;
    std::vector<uint8_t> lad_host;
    std::vector<uint8_t> lad_sent;    // the records lad_blk holds (empty: none): a call whose records equal them uploads nothing
    std::vector<ScaleAxisTab> lad_tabs;      // where lad_host holds the four tables of every rung: luma rows, chroma rows, luma columns, chroma columns
    int             lad_cap;           // what lad_host's horizontal tables ask of LDS per row and plane
    hipEvent_t      odev_ev[2];       // xgpu_pic_output_device on a caller's stream: picture ready on the context stream / the caller's kernel done (created at the first call)
    xgpu_frame_params fp;
    int             have_frame;
    int             side_pic;          // the slot whose xgpu_frame_end came last with no xgpu_frame_begin since: d_maps holds ITS side information (xgpu_frame_side_info); -1: none
    TileMask        no_dbk;            // tile borders the deblocking of the current picture leaves alone (set by xgpu_batch_recon)
    hipEvent_t      fork_ev, join_ev;  // k_dmvr / k_affine on the side stream beside k_inter: where they may start, where the kernel stream takes them back
    int             builder_threads;   // xgpu_set_builder_threads: host threads xgpu_batch_create spreads its per-CU passes over (default 1)
    int             pad_done;          // the padding of the current picture has been written (by k_alf's border tiles): xgpu_pad launches nothing
    int             where;             // 0: the picture being built lives in its DPB slot, 1: in the scratch picture
    int             order_rl;          // a batch of the picture has CUs decoded after their right-hand neighbours (xgpu_dbatch.order_rl): k_dbk's order-aware instantiation
    int             itdq_pair_min;     // data-flow launches that carry a residual pass of at least this many work items (IQT) give a residual workgroup two of them (k_intra_itdq; XEVD_HIP_ITDQ_PAIR_MIN, default 4096)
    int             intra_small_min;   // level-1 launches with at least this many CUs of at most 16 SCUs give those 16 lanes each (k_intra_l1; XEVD_HIP_INTRA_SMALL_MIN, default 2048)
    int             addb_scalar;                       // XEVD_HIP_ADDB_SCALAR: the scalar line filters (the > 10-bit instantiation) at every bit depth - read per context, tests set it
    int             dmvr_scalar;                       // XEVD_HIP_DMVR_SCALAR: k_dmvr's scalar form of the refined prediction for every sub-block - read per context, tests set it
    int             addb_pending, split_addb_alf;      // ADDB + ALF in one kernel: xgpu_deblock left its arguments in addb_args for xgpu_alf
    AddbArgs        addb_args;
    // timing
    int             timing;
    struct Ev { hipEvent_t a, b; int k; };
    std::vector<Ev> ev_pending;
    std::vector<hipEvent_t> ev_pool;
    double          t_ms[XGPU_K_COUNT];
    long long       t_n[XGPU_K_COUNT];
    char            err[256];
    // xgpu_lut3d_create: the context's 3D LUTs by handle; read by the LUT output calls, which end in the context's stream like every output call
    Lut3dSlot       lut3d[XGPU_MAX_LUT3D];
    // xgpu_dither_create: the context's dither matrices by handle, read by the dithered output calls under the same ordering
    DitherSlot      dither[XGPU_MAX_DITHER];
    // the overlaid output calls' device boxes (an OvlBlock written by k_overlay_prepare, read by the call's kernel; grown on demand, ordered like sc_tab)
    uint8_t        *ovl_blk;
    size_t          ovl_blk_cap;
};

// The host threads of a batch builder: workers that stay alive between pictures (a std::thread per phase and picture cost ~0.1 ms each - more than a phase of
// the builder takes).  One pool per CALLING thread (xgpu_batch_create may run on several builder threads of one context at once): a member of the
// builder's BuilderScratch.  run(n, f): f(0) on the caller, f(1) .. f(n - 1) on workers, returns when all are done.
class WorkPool {
public:
    ~WorkPool() { { std::lock_guard<std::mutex> g(mu); stop = true; } cv.notify_all(); for (std::thread &t : th) t.join(); }
    template <class F> void run(int n, F &&f)
    {
        if (n <= 1) { f(0); return; }
        while ((int)th.size() < n - 1) { const int idx = (int)th.size(); th.emplace_back([this, idx]() { worker(idx); }); }
        const std::function<void(int)> fn = [&f](int k) { f(k); };
        { std::lock_guard<std::mutex> g(mu); job = &fn; want = n - 1; left = n - 1; gen++; }
        cv.notify_all();
        f(0);
        std::unique_lock<std::mutex> g(mu);
        done_cv.wait(g, [this]() { return left == 0; });
        job = nullptr;
    }
private:
    void worker(int idx)
    {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)> *fn = nullptr;
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&]() { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
                if (idx < want) fn = job;
            }
            if (!fn) continue;
            (*fn)(idx + 1);
            std::lock_guard<std::mutex> g(mu);
            if (--left == 0) done_cv.notify_one();
        }
    }
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv, done_cv;
    const std::function<void(int)> *job = nullptr;
    int want = 0, left = 0;
    uint64_t gen = 0;
    bool stop = false;
};

// kernel launchers (one per .hip file)
void launch_itdq(xgpu_ctx *c, const ItdqArgs &a, hipStream_t s);
void launch_itdq_pairs(xgpu_ctx *c, const ItdqArgs &a, hipStream_t s);      // IQT only: two entries of the item list per workgroup, as k_intra_itdq's residual side takes them (k_intra.hip)
void launch_inter(xgpu_ctx *c, const InterArgs &a);      // k_inter on the ctx stream
void launch_test_recon(xgpu_ctx *c, const int16_t *coef, const int16_t *pred, int is_coef, int cuw, int cuh, int16_t *rec, int s_rec, int bd);
void launch_test_dbk(xgpu_ctx *c, int16_t *buf, int16_t *buf_v, int st, int st_v, int stride, int bd, int hor, int chroma);
void launch_intra(xgpu_ctx *c, const IntraArgs &a, bool dep, bool ibc, bool htdf, const ItdqArgs *next, bool right = false);      // next != NULL (dep launches): k_intra_itdq
int  intra_chunk(bool with_itdq);                // list positions per ticket of the data-flow launch (= waves per workgroup: 8, with the residual pass riding 4)
void launch_affine(xgpu_ctx *c, const AffineArgs &a, hipStream_t s);
void launch_dmvr(xgpu_ctx *c, const DmvrArgs &a, hipStream_t s);
void launch_dbk(xgpu_ctx *c, const DbkArgs &a, int dir, const DevPic &src, const DevPic &dst, bool order_rl = false);
void upload_transform_tables(const int *tm, const int16_t *ats, hipStream_t s);
int  itdq_group_size(int log2w, int log2h);     // TBs of one size class per 256-thread work item
void launch_addb_fused(xgpu_ctx *c, const AddbArgs &a, const DevPic &src, const DevPic &dst);      // both passes, one read + one write of the picture
void launch_alf(xgpu_ctx *c, const AlfArgs &a, const AddbArgs *deblock, const DevPic &src, const DevPic &dst);      // deblock != NULL: ADDB on SRC first, inside the same kernel
void launch_pad(xgpu_ctx *c, const DevPic &p);
void launch_copy_bw(xgpu_ctx *c, const void *src, void *dst, size_t bytes);
void launch_output(xgpu_ctx *c, const DevPic &pic, const int32_t *d_dra, int out_bd, int crop_l, int crop_r, int crop_t, int crop_b, uint8_t *d_dst, bool raw16 = false,
                   hipStream_t s = nullptr);      // s = NULL: the context's stream
// k_output_rgb.hip, k_output_yuv.hip (k_output_yuv444): the cropped picture as three channels at luma resolution - R'G'B' or Y'CbCr 4:4:4
// (xgpu_pic_output_device).  Everything the kernels need, resolved on the host by xgpu_api.hip.  YUV444 reads no matrix: coef / maxv stay zero,
// shift = B - 8 (the u8 rounding shift), fcoef[0] = fy = float32(1 / yr), fcoef[1] = fc = float32(1 / cr).
struct RgbOutArgs {
    const int16_t *y, *u, *v;       // first sample of the cropped area of every plane
    int      sy, sc;                // plane strides in samples
    int      w, h, cw, ch;          // cropped luma / chroma size
    uint8_t *dst;
    size_t   pitch, plane;          // bytes between rows / between the planes of the planar layout
    int      aligned;               // dst, pitch and plane are multiples of 16 bytes: vector stores
    int      bgr;
    int      coef[5], shift;        // cy, crv, cgu, cgv, cbu and S of the integer outputs
    float    fcoef[5];              // the same for the float outputs (2^D - 1 = 1)
    int      yo, co, maxv;          // luma offset (16 << (B-8) or 0), chroma offset 2^(B-1), 2^D - 1
    int      hc;                    // LINEAR: 1 = chroma horizontally between luma columns (ChromaSampleLocType 1, 3, 5)
    int      ve[2], vo[2];          // LINEAR: vertical quarter weights of rows (i-1, i) for even luma rows, of (i, i+1) for odd ones
    const int32_t *dra;             // [3][1024] DRA inverse tables, or NULL
};
// where a row's 3 x 8 elements go (output_common.h, output_three_sinks): three planes, the three elements of a pixel side by side, with the A element behind
// them, or one 10:10:10:2 word per pixel
enum { OUT_SINK_PLANAR, OUT_SINK_INTERLEAVED, OUT_SINK_RGBA, OUT_SINK_RGB10A2 };
void launch_output_rgb(const RgbOutArgs &a, int layout, int dtype, int upsample, hipStream_t s);
void launch_output_yuv444(const RgbOutArgs &a, int layout, int dtype, int upsample, hipStream_t s);
// k_output_cm.hip: k_output_rgb's arguments (coef / shift / maxv: those of the U16 form, whatever the dtype) and the colour transform's
// The transform's fields are one member, so that the scaled outputs' argument types (below) carry the same thing behind their own fields.
struct CmParams {
    const float *lin, *tone, *enc;  // device tables: linear light per code [n_lin]; g(Y) or NULL (scale instead); the destination curve or NULL (linear output)
    int      n_lin, use_matrix;
    float    m[9], luma[3], scale;  // source -> destination primaries, luminance weights of the source primaries, linear_scale
    float    outmax;                // integer dtypes: 2^D - 1
};
struct CmOutArgs : RgbOutArgs { CmParams cm; };
void launch_output_cm(const CmOutArgs &a, int layout, int dtype, int upsample, hipStream_t s);
// k_output_scaled.hip: the cropped picture resized to dw x dh and converted (xgpu_pic_output_device_scaled).  RgbOutArgs' source, destination
// and conversion fields (w, h, cw, ch: the SOURCE size; pitch / plane: of the dw x dh destination; aligned, hc, ve, vo are not read), then the taps and the two passes'.
// The five files of the two-pass resize outputs (this one, k_output_rois.hip, k_output_resampled.hip, k_output_scaled_cm.hip, k_output_scaled_lin.hip) share the bodies
// of their horizontal kernels, the body of the batch vertical kernel and the launch of the horizontal pass (output_resize.h); the argument types below differ in
// what a body's row and pixel policies read.
struct ScaleTaps { const int32_t *first, *count; const int16_t *w; int stride; };      // one axis of one plane, on the device
struct ScaledOutArgs : RgbOutArgs {
    int      dw, dh;                // destination size
    ScaleTaps yl, yc;               // vertical, luma / chroma rows: w[o * stride + k]
    ScaleTaps xl, xc;               // horizontal, luma / chroma columns, TRANSPOSED: w[k * dw + o] (stride = dw), so that the lanes of a wave read neighbours
    uint16_t *mid;                  // the vertical pass' output, 3 fraction bits: Y [dh][mpy], then Cb and Cr [dh][mpc]
    int      mpy, mpc;              // its row pitches in samples, multiples of 8
    int      smax;                  // 2^B - 1: the clip of every source sample
    int      capy, capc;            // pass 2: samples of a Y / of a Cb or Cr row one wave stages in LDS (multiples of 8)
    int      normalize;
    float    mean[3], inv_std[3];   // by output position (after bgr)
};
void launch_output_scaled(const ScaledOutArgs &a, int layout, int dtype, hipStream_t s);
void launch_scale_vertical(const ScaledOutArgs &a, hipStream_t s);      // its vertical pass alone (k_output_scaled_cm.hip follows it with a horizontal pass of its own)
// x_off: pass 2's groups of 64 destination columns start x_off columns before column 0 (a letterboxed image, whose workgroups are laid over the whole image)
int  scale_build_tables(int ws, int hs, int wd, int hd, int filter, int chroma_loc, std::vector<uint8_t> &blob, ScaleTabs &tb, int x_off = 0);      // xgpu_scale.hip
// k_output_rois.hip: several rectangles of one picture, each resized to dw x dh - stretched, or letterboxed into it - as a batch of images
// (xgpu_pic_output_device_rois).  One record per rectangle, in the context's descriptor block in front of the tap tables it points into.
struct __attribute__((aligned(16))) RoiDesc {
    uint64_t dst;                   // byte offset of the image in the destination
    int      x, y, w, h;            // the rectangle, luma samples from the first sample of the picture minus f->crop (even)
    int      ix, iy, iw, ih;        // the filtered part inside the dw x dh image; every other element is the pad value
    uint32_t mid;                   // first sample of its intermediate: Y [ih][mpy], then Cb and Cr [ih][mpc]
    int      mpy, mpc;
    uint32_t first[4], count[4], wt[4];      // byte offsets in the block of the tables 0 yl, 1 yc, 2 xl, 3 xc (laid out as ScaledOutArgs' are)
    int      stride[4];
    int      skip;                  // the device-box call (k_rois_prepare): 1 = an index at or above the count - pass 2 writes no element of the image
    int      pad_[2];
};
static_assert(sizeof(RoiDesc) == 128, "RoiDesc must be 128 bytes");
// ScaledOutArgs' picture, destination and conversion fields (y, u, v: the picture minus f->crop; dst, pitch, plane: of image 0; capy, capc: the widest of all
// rectangles; mid: the base of all intermediates; w, h, cw, ch and the four taps are not read), then the batch's
struct RoisOutArgs : ScaledOutArgs {
    const uint8_t *blk;             // the descriptor block: n RoiDesc, then the tap tables
    int      n;
    float    padv[3];               // the pad value by output position, before the normalise (integer dtypes: the integer)
};
void launch_output_rois(const RoisOutArgs &a, int layout, int dtype, int max_w, int max_ih, hipStream_t s);
void launch_rois_vertical(const RoisOutArgs &a, int max_w, int max_ih, hipStream_t s);      // its vertical pass alone
// k_output_resampled.hip: the same block and arguments with bicubic tap tables (xgpu_pic_output_device_resampled / _rois_resampled): `mid`
// holds int16 with two fraction bits, and RoiDesc::skip is not read
void launch_output_resampled(const RoisOutArgs &a, int layout, int dtype, int max_w, int max_ih, hipStream_t s);
int  resample_build_tables(int ws, int hs, int wd, int hd, int kernel, int antialias, int chroma_loc, std::vector<uint8_t> &blob, ScaleTabs &tb, int x_off = 0);      // xgpu_scale.hip
// k_output_scaled_cm.hip: the two scaled outputs with the colour transform between the filter and the store (xgpu_pic_output_device_scaled_cm / _rois_cm,
// INTEGRATION.md section 8m).  The vertical passes are k_scale_vertical / k_rois_vertical; the horizontal pass keeps the transform's tables in global memory (L1 / L2) and
// only its spans in dynamic LDS.  coef / shift / maxv: those of the U16 form, whatever the dtype (CmOutArgs' rule).
struct ScaledCmOutArgs : ScaledOutArgs { CmParams cm; };
struct RoisCmOutArgs : RoisOutArgs { CmParams cm; };
void launch_output_scaled_cm(const ScaledCmOutArgs &a, int layout, int dtype, hipStream_t s);
void launch_output_rois_cm(const RoisCmOutArgs &a, int layout, int dtype, int max_w, int max_ih, hipStream_t s);
// k_output_scaled_lin.hip: the same two outputs filtered in linear light (xgpu_pic_output_device_scaled_lin / _rois_lin).  The argument
// types are the colour-managed ones with another intermediate: `mid` is float32, R, G, B planes [rows][mpy] one behind the other (RoiDesc::mid counts floats; mpc,
// capc and the chroma taps are not read); hc / ve / vo are read (the chroma upsampling of the full-size output), as is `upsample`.
void launch_output_scaled_lin(const ScaledCmOutArgs &a, int layout, int dtype, int upsample, hipStream_t s);
void launch_output_rois_lin(const RoisCmOutArgs &a, int layout, int dtype, int upsample, int max_w, int max_ih, hipStream_t s);
// the bytes of a workgroup's LDS one row of the horizontal pass needs at most (capy floats x 3): what one plain launch may request
static const size_t LIN_LDS_LIMIT = 64 * 1024;
// k_output_ladder.hip: n renditions ("rungs") of one picture as 4:2:0 video surfaces, each at its own size (xgpu_pic_output_device_ladder, INTEGRATION.md section
// 8l).  One record per (rung, plane) and pass, in the context's block in front of the tap tables it points into: 3 n records of the vertical pass (plane 0, 1, 2
// of every rung), then the horizontal pass' - per rung Y, Cb, Cr (YUV420P) or Y and the interleaved Cb Cr rows (NV12 / P016: `pair`).
int  scale_build_axis(int n, int s, int h, int N, int S, int H, int filter, bool transposed, int group, std::vector<uint8_t> &blob, ScaleAxisTab &t, int *cap);
struct __attribute__((aligned(16))) LadderDesc {
    uint64_t dst;                   // horizontal: the address of the plane's first element in the rung's destination
    uint64_t pitch;                 // horizontal: bytes between two rows of the plane
    uint32_t mid[2];                // first sample of the plane's intermediate [rows][mp] (horizontal, pair: of Cb's and of Cr's)
    int      mp;                    // its row pitch in samples, a multiple of 8
    int      plane;                 // vertical: the source plane, 0 Y, 1 Cb, 2 Cr
    int      sw;                    // vertical: columns of the source plane
    int      rows, cols;            // destination rows (both passes) and columns (horizontal) of the plane
    int      pair;                  // horizontal: 1 = Cb and Cr of a position side by side
    uint32_t first, count, wt;      // byte offsets in the block of the pass' table: rows (vertical, w[o * stride + k]) or columns (horizontal, transposed)
    int      stride;
};
static_assert(sizeof(LadderDesc) == 64, "LadderDesc must be 64 bytes");
#define LADDER_GROUP 4              // destination positions of one lane of the horizontal pass; a workgroup row is 64 lanes
// ScaledOutArgs' picture fields (y, u, v, sy, sc: the picture minus f->crop; dra, smax; mid: the base of all intermediates), then the call's
struct LadderOutArgs : ScaledOutArgs {
    const uint8_t *blk;             // 3 n vertical records, nh horizontal records, the tap tables
    int      n, nh;
    int      cap;                   // horizontal: the samples of one row of one plane a wave stages in LDS (the widest of all records; a multiple of 8)
    int      cshift, cmaxv, cout8, clsh;      // the depth rule: conv1's shift B - D, 2^D - 1, D == 8; P016's left shift 16 - D
};
// max_sw / max_vrows: the widest source plane and the most destination rows of the vertical records; max_cols / max_rows: of the horizontal ones
void launch_output_ladder(const LadderOutArgs &a, int dtype, int max_sw, int max_vrows, int max_cols, int max_rows, hipStream_t s);
// k_output_rois_dev.hip: the descriptor block of k_output_rois.hip made on the device from boxes in device memory (xgpu_pic_output_device_rois_dev, INTEGRATION.md
// section 8f).  The block: `capacity` RoiDesc, then one slot of tap tables per box at tab + i * slot - table t's first[], count[] and weights at off_first[t],
// off_count[t], off_w[t] inside it -, every size taken from the bounds alone (rois_dev_layout, xgpu_api.hip).
struct RoisPrepArgs {
    uint8_t *blk;
    const void *boxes;              // capacity boxes of box_format
    const int *count;               // live boxes, or NULL: capacity
    xgpu_roi_result *results;       // or NULL
    int      capacity, box_format;
    int      pw, ph, mw, mh;        // the picture minus the crop; the bounds
    int      wd, hd, fit, filter, chroma_loc;
    int      capy, capc;            // what pass 2's LDS holds per row: a wider span makes the box XGPU_ROI_TOO_LARGE
    size_t   image_pitch;
    uint32_t tab, slot;             // bytes: where the slots start in the block, and one slot
    uint32_t off_first[4], off_count[4], off_w[4];
    uint32_t mid_slot;              // samples of the intermediate per box
};
void launch_rois_prepare(const RoisPrepArgs &a, hipStream_t s);
// k_output_warp.hip: n affine maps of one picture, each giving one dw x dh image (xgpu_pic_output_device_warp).  ScaledOutArgs' picture,
// destination and conversion fields (y, u, v, w, h, cw, ch: the picture minus f->crop; dst, pitch, plane: of image 0; the taps, mid and the caps are not read),
// then the batch's
struct WarpOutArgs : ScaledOutArgs {
    const int64_t *maps;            // [n][6] Q16 on the device: the context's block (host maps) or the caller's array (device maps, unchecked)
    int32_t *status;                // device maps: [n] 0 = written, 1 = refused; or NULL
    int      n;
    int      ls;                    // log2 of `samples`
    int      border;                // XGPU_WARP_CLAMP / XGPU_WARP_PAD
    int      sh, sv;                // the chroma grid lies sh / 2, sv / 2 luma samples behind the luma grid (xgpu_scale_taps' siting_half_luma)
    float    padv[3];               // the pad value by output position, before the normalise (integer dtypes: the integer)
    size_t   image_pitch;           // bytes between two images
};
void launch_output_warp(const WarpOutArgs &a, int layout, int dtype, hipStream_t s);
// k_output_remap.hip: n coordinate grids of one picture, each giving one dw x dh image (xgpu_pic_output_device_remap).  ScaledOutArgs'
// fields as WarpOutArgs reads them, then the batch's
struct RemapOutArgs : ScaledOutArgs {
    const uint8_t *grid;            // grid 0 on the device: [gh][gw] nodes of 8 bytes, (x, y) int32 Q16 or float32 luma samples; never read by the host
    size_t   grid_pitch;            // bytes between two grids
    int      gw, gh;                // nodes per row / rows of a grid
    int      k;                     // step_log2: a node every 2^k pixels (0: one per pixel)
    int      f32;                   // 1 = XGPU_GRID_F32
    int      n;
    int      ls;                    // log2 of `samples`
    int      border;                // XGPU_WARP_CLAMP / XGPU_WARP_PAD
    int      sh, sv;                // the chroma siting, as WarpOutArgs'
    float    padv[3];               // the pad value by output position, before the normalise (integer dtypes: the integer)
    size_t   image_pitch;           // bytes between two images
};
void launch_output_remap(const RemapOutArgs &a, int layout, int dtype, hipStream_t s);
void launch_test_scale_taps(int n_plane, int subsampling, int siting, int n_dst, int filter, int32_t *first, int32_t *count, int16_t *w, int w_stride, hipStream_t s);
// k_output_yuv.hip (k_output_semiplanar): NV12 / P016 - xgpu_pic_output's samples, luma rows then rows of interleaved Cb Cr
struct SemiPlanarArgs {
    const int16_t *y, *u, *v;       // first sample of the cropped area of every plane
    int      sy, sc;                // plane strides in samples
    int      w, ch;                 // cropped luma width, chroma rows (= luma rows / 2)
    uint8_t *dst;
    size_t   pitch, chroma_off;     // bytes between rows, byte offset of the chroma plane (luma rows x pitch)
    int      aligned;               // dst, pitch and chroma_off are multiples of 16 bytes: vector stores
    int      shift, out8, maxv;     // conv1's arguments at depth D: B - D, D == 8, 2^D - 1
    int      lsh;                   // P016: 16 - D, the sample in the high bits of the word; NV12: 0
    const int32_t *dra;             // [3][1024] DRA inverse tables, or NULL
};
void launch_output_semiplanar(const SemiPlanarArgs &a, int dtype, hipStream_t s);
// k_output_packed.hip (xgpu_pic_output_device_packed).  k_output_packed_rgb: CmOutArgs (cm is read only with a transform; `plane` is not
// read) and the A element; RGB10A2 runs the U16 instances with coef / shift / maxv (cm.outmax) of D = 10.
struct PackedRgbArgs : CmOutArgs {
    uint32_t alpha;                 // the bits of the A element (float dtypes: the float32 bits of alpha, rounded to the dtype in the kernel); RGB10A2: the 2-bit code
};
void launch_output_packed_rgb(const PackedRgbArgs &a, int layout, int dtype, int upsample, bool cm, hipStream_t s);      // not: RGBA, a float dtype, no transform
// ... which is k_output_rgb's interleaved image at `mid` (rows mid_pitch bytes apart: a multiple of 16 that holds a multiple of 8 pixels) and this copy behind it;
// reads a's w, h, dst, pitch, aligned and alpha
void launch_packed_rgba_from_rgb(const PackedRgbArgs &a, int dtype, const uint8_t *mid, size_t mid_pitch, hipStream_t s);
// k_output_packed_422: RgbOutArgs' source, size, destination, ve / vo and DRA fields (chroma_row reads them; the matrix fields and hc are not read), then
// SemiPlanarArgs' conversion
struct Packed422Args : RgbOutArgs {
    int      cshift, out8, cmax;    // conv1's arguments at depth D: B - D, D == 8, 2^D - 1
    int      lsh;                   // U16: 16 - D, the sample in the high bits of the word; U8: 0
};
void launch_output_packed_422(const Packed422Args &a, int dtype, bool uyvy, int upsample, hipStream_t s);
// k_output_lut3d.hip (xgpu_pic_output_device_lut3d / _packed_lut3d): k_output_rgb's arguments (coef / shift / maxv: those of the U16
// form, whatever the dtype) and the LUT's.  One LUT is one device block: the shaper, then the cube lut3d_shaper_bytes behind it.
struct Lut3dOutArgs : RgbOutArgs {
    const uint16_t *shaper;         // [3][maxv + 1] positions
    const uint2    *cube;           // n^3 records R | G << 16, B: node (r, g, b) at r + n * (g + n * b)
    int      n;                     // nodes per axis, 2 .. 65
    uint32_t dmax;                  // integer dtypes: 2^D - 1 of the store
    uint32_t alpha;                 // the packed layouts' A element (PackedRgbArgs' rule)
};
static inline size_t lut3d_shaper_bytes(int bit_depth) { return (size_t)3 * sizeof(uint16_t) << bit_depth; }      // a multiple of 16
void launch_output_lut3d(const Lut3dOutArgs &a, int layout, int dtype, int upsample, hipStream_t s);
void launch_output_packed_lut3d(const Lut3dOutArgs &a, int layout, int dtype, int upsample, hipStream_t s);
// k_output_dither.hip (xgpu_pic_output_device_dithered / _packed_dithered): the matrix of one call.  Pixel (x, y) of the cropped
// destination has rank tab[((y + py) & mhm) * stride + ((x + px) & mwm) + run] for run 0 .. 15 (DitherSlot's extended rows)
struct DitherArgs {
    const uint16_t *tab;
    int      stride, mwm, mhm;      // ranks per extended row; mw - 1, mh - 1
    int      px, py, k;             // the phase; L = 2^k levels
};
// the three-channel family: PackedRgbArgs (k_output_packed_rgb's, `plane` read by the planar sink) with, for the matrix path, coef / shift / maxv of the store's
// depth D and, with a transform, cm.outmax = 2^D - 1
struct DitherRgbArgs : PackedRgbArgs { DitherArgs di; };
void launch_output_dither_rgb(const DitherRgbArgs &a, int sink, int dtype, int upsample, bool cm, hipStream_t s);
struct DitherSemiArgs : SemiPlanarArgs { DitherArgs di; };
void launch_output_dither_semiplanar(const DitherSemiArgs &a, int dtype, hipStream_t s);
// k_output_overlay.hip (xgpu_pic_output_device_overlaid / _packed_overlaid): the layers of one call.  A layer is the unclipped
// rectangle [x0, x1) x [y0, y1) in cropped destination coordinates; colour / fill: R | G << 8 | B << 16 | A << 24.
struct OvlLayer {
    int      x0, y0, x1, y1;
    int      kind, opacity, thickness;
    uint32_t colour, fill;
    uint32_t pitch;                 // bitmaps: bytes between two rows
    const uint8_t *pix;             // bitmaps: the pixel of (x0, y0)
};
// the device boxes of a call in the context's block, written by k_overlay_prepare: box i is a BOX layer [x0, x1) x [y0, y1) in `colour`; a skipped box is all zeros
struct OvlBox { int x0, y0, x1, y1; uint32_t colour; };
struct OvlBlock { int count, pad_[3]; OvlBox box[XGPU_MAX_OVERLAY_BOXES]; };
struct OvlArgs {
    const OvlBlock *boxes;          // or NULL: no device boxes
    int      n;                     // host layers
    int      maxv;                  // M, the element maximum
    int      box_thickness, box_fill_alpha;
    int      m[9], off[3], s;       // NV12 / P016: the forward matrix, the offsets and S (xgpu_overlay_coeffs)
    OvlLayer layer[XGPU_MAX_OVERLAY_LAYERS];
};
// the three-channel family: PackedRgbArgs as k_output_packed_rgb reads them; the surfaces: SemiPlanarArgs
struct OverlayRgbArgs : PackedRgbArgs { OvlArgs ov; };
struct OverlaySemiArgs : SemiPlanarArgs { OvlArgs ov; };
void launch_output_overlay_rgb(const OverlayRgbArgs &a, int sink, int dtype, int upsample, bool cm, hipStream_t s);
void launch_output_overlay_semiplanar(const OverlaySemiArgs &a, int dtype, hipStream_t s);
struct OvlPrepArgs {
    OvlBlock *blk;
    const void *boxes;              // capacity boxes of box_format
    const int32_t *count, *labels;  // or NULL
    int      capacity, box_format, n_palette;
    int      pw, ph;                // the image: a box that misses it is skipped
    uint32_t palette[16];
};
void launch_overlay_prepare(const OvlPrepArgs &a, hipStream_t s);
// xgpu_overlay.hip: the host side of those calls that needs no device
void   overlay_forward_matrix(double kr, double kb, int full_range, int d, int32_t m[9], int32_t off[3], int *shift);
int    overlay_layers_check(const xgpu_overlay_layer *layers, int n, const xgpu_overlay_boxes *boxes, const char **why);
size_t overlay_layer_bytes(const xgpu_overlay_layer &l);
void   overlay_fill_args(const xgpu_overlay_layer *layers, int n, const xgpu_overlay_boxes *boxes, const OvlBlock *blk, int maxv, OvlArgs &o);
void   overlay_fill_prepare(const xgpu_overlay_boxes *boxes, OvlBlock *blk, int pw, int ph, OvlPrepArgs &p);
// k_side_info.hip: the SCU map of the picture decoded last as nine int16 planes per unit (k_side_blocks) or as a dense motion field (k_side_flow)
struct SideArgs {
    const ScuRec *maps;
    int      w_scu, h_scu;
    uint8_t *dst;
    size_t   pitch, plane;          // bytes between rows / between planes (BLOCKS, FLOW planar)
    int      aligned;               // dst, pitch and plane are multiples of 16 bytes: vector stores
    int      w, h, crop_l, crop_t;  // FLOW: the cropped size and where it starts in the picture
    int      list0, per_poc;        // FLOW: the list of a one-list field; divide by the POC distance
    int      poc;
    int      refp_poc[XGPU_MAX_REFS][2];
};
void launch_side_blocks(const SideArgs &a, hipStream_t s);
void launch_side_flow(const SideArgs &a, bool planar, int dtype, int n_lists, hipStream_t s);
// k_residual.hip: the residual arena of a batch as picture-shaped planes (xgpu_batch_residual)
struct ResidArgs {
    const uint32_t *owner;          // [h_scu * w_scu] CU of the batch over every 4x4 luma unit, 0xFFFFFFFF: none
    const CuRec    *cus;
    const int16_t  *resid;          // the arena: at least 8 samples, 256-byte aligned
    int      w_scu, h_scu;
    uint8_t *dst;
    size_t   pitch, plane;          // bytes between rows / between the planes of 444 planar and ENERGY
    size_t   off_c[2], pitch_c;     // YUV420: byte offsets of the Cb and Cr planes, bytes between their rows
    int      aligned;               // dst, pitch and the plane distances allow the vector stores of every plane
    int      w, h, crop_l, crop_t;  // the cropped size and where it starts in the picture
    float    scale[3];              // float dtypes: 2^-B per component
    const uint32_t *chroma_cus;     // the batch's chroma-only CUs with coded chroma (local dual tree)
    int      n_chroma_cus;
};
void launch_residual(const ResidArgs &a, int layout, int dtype, hipStream_t s);
// k_compare.hip: a picture against a reference in one pass (xgpu_pic_compare)
struct CompareArgs {
    const uint16_t *a[3];           // the picture: first sample of the cropped area of every plane
    int      sa[3];                 // its strides in samples
    const uint8_t *r[3];            // the reference: the same, as bytes
    size_t   pr[3];                 // bytes between its rows
    int      r8;                    // reference elements are bytes (zero-extended), else 16-bit
    int      vec_a[3], vec_r[3];    // the plane's cropped base and pitch allow the vector loads (16 bytes; a byte reference: 8)
    int      w[3], h[3];            // cropped size of every plane
    int      tiles_x[3];            // 64x32 tiles per row of tiles
    int      tile_first[4];         // tiles of plane c: tile_first[c] .. tile_first[c + 1]
    int      ssim, block_map;
    long long c1, c2;               // the SSIM constants at the coding depth
    unsigned long long *part;       // [workgroups][3][CMP_PART_WORDS]: every workgroup's sums per component, reduced into res by k_compare_finish
    xgpu_compare_result *res;
    uint64_t *map;                  // [3][mh][mw]
    int      mw, mh;
};
#define CMP_PART_WORDS 8            // n, sse, n_diff, first_diff, windows, q, max_abs, (unused)
int  compare_workgroups(int tiles);                 // the workgroups launch_compare starts for that many tiles
void launch_compare(const CompareArgs &a, hipStream_t s);
// k_stats.hip: the statistics of one picture (xgpu_pic_stats)
#define STATS_MAX_BINS       4096   // 2^12: the bins of one histogram at most
#define STATS_MAX_WORKGROUPS 1024   // 4 per CU: twice as many were slower with a histogram to flush
#define STATS_PART_WORDS     8      // n, sum, sum_sq, min, max, (unused)
#define STATS_ACC_BYTES      ((size_t)4 * STATS_MAX_BINS * sizeof(uint32_t))      // [3][nbins] and the light histogram
#define STATS_LIN_BYTES      ((size_t)STATS_MAX_BINS * sizeof(float))
#define STATS_PART_BYTES     ((size_t)STATS_MAX_WORKGROUPS * 3 * STATS_PART_WORDS * sizeof(unsigned long long))
#define STATS_BLK_BYTES      (STATS_ACC_BYTES + STATS_LIN_BYTES + STATS_PART_BYTES)
struct StatsArgs {
    const uint16_t *a[3];           // first sample of the cropped area of every plane
    int      sa[3];                 // its strides in samples
    int      vec[3];                // the plane's cropped base and pitch allow the 16-byte loads
    int      w[3], h[3];            // cropped size of every plane
    int      tiles_x[3];            // 64x32 tiles per row of tiles
    int      tile_first[4];         // tiles of plane c: tile_first[c] .. tile_first[c + 1]
    int      bd, hist_bits;         // the coding depth; 0: no histogram
    int      pctl_e4[2];
    int      light;
    RgbOutArgs rgb;                 // light: the U16 planar conversion of xgpu_pic_output_device (dst, pitch, plane, aligned are not read)
    int      upsample;
    uint32_t *acc;                  // the accumulation block: [3][2^hist_bits], then [2^bd] (zero before the launch)
    const float *lin;               // light: [2^bd]
    unsigned long long *part;       // [workgroups][3][STATS_PART_WORDS]
    xgpu_stats_result *res;
    uint32_t *hist;                 // the caller's, laid out like acc
};
void launch_stats(const StatsArgs &a, hipStream_t s);
bool colour_transfer_supported(int tc);      // xgpu_colour.hip: a TransferCharacteristics code point of xgpu_colour_transform's list
void launch_md5(xgpu_ctx *c, hipStream_t s, const uint8_t *d_msg, int w, int h, uint32_t *d_digest);      // k_md5.hip: the three planes packed back to back at d_msg -> d_digest[3][4]
void launch_test_mc(xgpu_ctx *c, const int16_t *plane, int stride, int ref_x, int ref_y, int has_dx, int has_dy,
                    int gmv_x, int gmv_y, int16_t *pred, int w, int h, int bd, int luma);
