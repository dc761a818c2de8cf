/*
 * xevd_hip.h - C ABI of the MI355X (gfx950) per-CU reconstruction backend for an MPEG-5 EVC decoder.
 *
 * This is the drop-in boundary: plain C, plain pointers and sizes, no C++/torch types.  Every entry point
 * replaces one coarse slot of the reference decoder's function table (all citations are relative to the
 * reference tree mpeg5/xevd v0.7.0):
 *
 *   xgpu_open / xgpu_close        <- xevd_platform_init / xevd_platform_deinit  src_base/xevd.c:2074-2163
 *                                    (the `void *pf` "platform specific data" slot, src_base/xevd_def.h:1452-1470)
 *   xgpu_pic_alloc / xgpu_pic_free<- PICBUF_ALLOCATOR.fn_alloc / fn_free         src_base/xevd_def.h:684-705
 *   xgpu_frame_begin              <- slice_init + refp set-up                    src_base/xevd.c:378-405,1871-1903
 *   xgpu_batch_create/_recon      <- body of xevd_ctu_row_rec_mt -> xevd_recon_unit
 *                                                                                 src_base/xevd.c:1470-1526, 678-756
 *                                    (xevd_sub_block_itdq, xevd_mc, xevd_recon_yuv, xevd_set_dec_info)
 *   xgpu_deblock                  <- ctx->fn_deblock (xevd_deblock)              src_base/xevd.c:1116-1243,1909-1976
 *   xgpu_alf                      <- mctx->fn_alf (xevd_alf -> alf_process)      src_main/xevdm.c:2105, xevdm_alf.c:901-1249
 *   xgpu_pad                      <- ctx->fn_picbuf_expand                       src_base/xevd_util.c:365-427
 *   xgpu_pic_download             <- xevd_pull (picture hand-off)                src_base/xevd.c:2042-2071
 *   xgpu_pic_md5                  <- xevd_picbuf_signature / xevd_md5_imgb (picture signature)       src_base/xevd_util.c:985-1002, 1557-1572
 *   xgpu_pic_output               <- xevd_pull + the application's imgb_cpy_codec_to_out (crop fields xevd.c:2058-2069,
 *                                    bit-depth conversions app/xevd_app_util.h:441-552,656-700)
 *   xgpu_pic_output_device        (no counterpart: the picture as YUV or R'G'B' into the caller's device memory)
 *   xgpu_batch_residual           (no counterpart in the library: the prediction residual of a picture - what the reconstruction adds to the prediction - as dense planes)
 *   xgpu_frame_side_info          (no counterpart in the library; FFmpeg's export_mvs is the usual example: motion vectors, modes, QP of the picture decoded last)
 *   xgpu_pic_compare              (no counterpart in the library; ffmpeg's psnr / ssim filters are the usual example: a picture against a reference, exactly)
 *   xgpu_pic_stats                (no counterpart in the library; ffmpeg's signalstats / histogram filters and a player's peak detection are the usual examples)
 *
 * plus fine-grained shims with the reference's per-block function-table signatures
 * (XEVD_MC_L / XEVD_MC_C src_base/xevd_mc.h:47-49, XEVD_ITXB src_base/xevd_def.h:360, fn_recon :1466)
 * so parity tests can drive one block exactly like the reference tables are driven: xgpu_test_*.
 *
 * Conventions (same as the reference's): every function returns XGPU_OK (0) or a negative error code with
 * the numeric values of XEVD_ERR_* (inc/xevd.h:48-77); nothing throws; no global state - one xgpu_ctx per
 * decoder instance, one HIP stream per ctx; a ctx is thread-compatible, not thread-safe.  All sample
 * storage is 16-bit (`pel` = s16, src_base/xevd_port.h:51) also for 8-bit streams.
 */
#ifndef XEVD_HIP_H
#define XEVD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XGPU_OK                    0
#define XGPU_ERR                  (-1)    /* XEVD_ERR                      */
#define XGPU_ERR_INVALID_ARGUMENT (-101)  /* XEVD_ERR_INVALID_ARGUMENT     */
#define XGPU_ERR_OUT_OF_MEMORY    (-102)  /* XEVD_ERR_OUT_OF_MEMORY        */
#define XGPU_ERR_UNSUPPORTED      (-104)  /* XEVD_ERR_UNSUPPORTED          */
#define XGPU_ERR_UNEXPECTED       (-105)  /* XEVD_ERR_UNEXPECTED (HIP errors map here) */

#define XGPU_MAX_REFS   17      /* XEVD_MAX_NUM_REF_PICS, src_base/xevd_def.h */
#define XGPU_PAD_L      144     /* PIC_PAD_SIZE_L = MAX_CU_SIZE + 16, src_base/xevd_def.h:211 */
#define XGPU_PAD_C      72      /* PIC_PAD_SIZE_C, :212 */

/* prediction modes, numeric values of MODE_* in src_base/xevd_def.h:284-287 */
#define XGPU_MODE_INTRA 0
#define XGPU_MODE_INTER 1
#define XGPU_MODE_SKIP  2
#define XGPU_MODE_DIR   3
#define XGPU_MODE_IBC   6      /* intra block copy (Main, sps->ibc_flag): mv[0] = whole-sample block vector into the current picture, refi unused */

typedef struct xgpu_ctx    xgpu_ctx;     /* one decoder instance on one GPU          */
typedef struct xgpu_dbatch xgpu_dbatch;  /* a CU batch resident in HBM               */

/* Sequence-level parameters: the SPS fields that change arithmetic on this path. */
typedef struct xgpu_seq_params {
    int device;               /* HIP device ordinal                                              */
    int width, height;        /* luma picture size in samples (ctx->w, ctx->h); multiples of 8  */
    int bit_depth_luma;       /* sps->bit_depth_luma_minus8 + 8   (8..12)                        */
    int bit_depth_chroma;     /* sps->bit_depth_chroma_minus8 + 8                                */
    int chroma_format_idc;    /* 1 (4:2:0) is implemented                                        */
    int log2_ctu;             /* ctx->log2_max_cuwh: 6 Baseline (xevd.c:249-252), 5..7 Main      */
    int tool_iqt;             /* sps->tool_iqt  : 16-bit two-stage transform + scale table ..72  */
    int tool_admvp;           /* sps->tool_admvp: Main 8-tap luma / 4-tap chroma tables          */
    int tool_addb;            /* sps->tool_addb : ADDB deblocking (else baseline filter)         */
    int tool_alf;             /* sps->tool_alf                                                   */
    int max_pics;             /* picture slots to make available (DPB + current), <= 34          */
    /* chroma QP mapping tables (xevd_qp_chroma_dynamic[0..1][-qpBdOffsetC .. 57], xevd_tbl.c:359-426);
       entry [c][qp + 6*(bit_depth_chroma-8)]; NULL = the sequence default: xevd_tbl_qp_chroma_adjust_base, or
       _main when tool_iqt is on (src_main/xevdm.c:471-479)                                            */
    const int8_t *chroma_qp_table[2];
    int tool_eipd;            /* sps->tool_eipd : 33 luma / 5 chroma intra modes, neighbour padding of xevdm_get_nbr; batch.ipm then
                                 holds core->ipm[0] (IPD_DC 0, PLN 1, BI 2, angular 3..32) and core->ipm[1] (DM 0, BI 1, DC 2, HOR 3, VER 4) */
} xgpu_seq_params;

/* Per-picture parameters: what slice_init / the slice header contribute to this path. */
typedef struct xgpu_frame_params {
    int pic;                               /* destination picture slot                                   */
    int poc;                               /* ctx->poc.poc_val                                           */
    int num_refp[2];                       /* ctx->dpm.num_refp[list]                                    */
    int refp_pic[XGPU_MAX_REFS][2];        /* picture slot of ctx->refp[idx][list].pic                   */
    int refp_poc[XGPU_MAX_REFS][2];        /* ctx->refp[idx][list].pic->poc                              */
    int qp_u_offset, qp_v_offset;          /* sh.qp_u_offset / sh.qp_v_offset (pic_qp_*_offset)          */
    int deblock_alpha_offset, deblock_beta_offset;  /* sh_deblock_alpha/beta_offset (ADDB only)          */
    /* which in-loop filters WILL run on this picture (sh.deblocking_filter_on, sh.alf_on).  The filters work
       out of place between the DPB slot and a private scratch picture; knowing the plan up front lets
       reconstruction start in the buffer from which the last filter lands in the DPB slot without a copy.  */
    int deblock_on, alf_on;
} xgpu_frame_params;

/* Tile grid of a picture: the PPS tile syntax after set_tile_info (src_main/xevdm.c:2162-2330).  Tiles are rectangles of CTUs; a CU
   sees no neighbour in another tile (intra prediction, HTDF border, motion candidates), and the in-loop filters treat tile borders
   as loop_filter_across_tiles says: the deblocking filters leave edges on a tile border alone when it is 0 (xevdm_df.c:142, 233,
   274), the ALF windows end at the tile - mirrored when 0, replicated when 1 (alf_process_tile, xevdm_alf.c:901-1160).            */
#define XGPU_MAX_TILE_COLS 20      /* MAX_NUM_TILES_COL / MAX_NUM_TILES_ROW, src_base/xevd_def.h */
#define XGPU_MAX_TILE_ROWS 22
typedef struct xgpu_tile_grid {
    int n_cols, n_rows;
    int col_bd[XGPU_MAX_TILE_COLS + 1];      /* first CTU column of every tile column; col_bd[n_cols] = CTUs per picture row */
    int row_bd[XGPU_MAX_TILE_ROWS + 1];
    int loop_filter_across_tiles;            /* pps.loop_filter_across_tiles_enabled_flag */
} xgpu_tile_grid;

/* Adaptive loop filter parameters of one picture: what alf_process has after alf_recon_coef
   (src_main/xevdm_alf.c:700-794, 1167-1195) - coefficient reconstruction from the APS stays on the host. */
typedef struct xgpu_alf_params {
    int            enable[3];     /* alf_slice_param.enable_flag[Y, U, V]                                    */
    const int16_t *luma_coef;     /* alf->coef_final: [25 classes][13] 7x7-diamond coefficients              */
    const int16_t *chroma_coef;   /* alf_slice_param.chroma_coef: [7] 5x5-diamond coefficients               */
    const uint8_t *ctb_flag;      /* alf_ctb_flag of the luma plane, [n_ctu] raster; NULL = every CTU on     */
    int            across_tiles;  /* pps.loop_filter_across_tiles_enabled_flag (changes right/bottom borders) */
    const xgpu_tile_grid *tiles;  /* NULL = one tile; else its loop_filter_across_tiles must equal across_tiles */
} xgpu_alf_params;

/*
 * One batch of decoded CUs (one tile or one picture), structure-of-arrays, in decode order, grouped by CTU.
 * The ORDER carries meaning: a neighbouring CU counts as reconstructed before CU i when its index is below i (xevd_get_avail_intra / xevdm_get_nbr / xevd_check_nev_avail read the
 * COD flags the reference sets CU by CU) - left, above, and with sps_suco_flag also right-hand neighbours.  Nothing else tells the backend about split order.
 * It must be the order of a walk over the split tree (any node's parts left to right or right to left): all neighbours along one side of a CU are then decoded before it or all
 * after it, which the reference's deblocking walk relies on (xevdm_df.c:237,280) and the backend's filters take for granted.
 * It is the post-entropy-decode record set of XEVD_CU_DATA (src_base/xevd_def.h:1145-1190) after MV
 * derivation (xevd.c:705-728), flattened per leaf CU.  Coefficients are stored CU-contiguous exactly as
 * coef_rect_to_series produces them (xevd.c:640-676): for a CU, the coded components in the order Y, U, V,
 * each `w*h` (luma) / `(w/2)*(h/2)` (chroma) s16 values, row-major; an un-coded component occupies nothing.
 */
typedef struct xgpu_cu_batch {
    int             n_cu;
    const uint16_t *x, *y;        /* [n_cu] top-left luma sample                                          */
    const uint8_t  *log2w, *log2h;/* [n_cu] 2..6 (7 with Main CTU 128)                                    */
    const uint8_t  *pred_mode;    /* [n_cu] XGPU_MODE_*; SKIP/DIR are inter CUs (MVs already derived)     */
    const int8_t   *refi;         /* [n_cu][2]  reference index per list, <0 = unused                     */
    const int16_t  *mv;           /* [n_cu][2][2] quarter-pel (list, x/y), unclipped                      */
    const uint8_t  *qp;           /* [n_cu][3]  core->qp_y/qp_u/qp_v: dequant QPs incl. 6*(bd-8)          */
    const uint8_t  *cbf;          /* [n_cu]  bit c set = component c has coefficients (is_coef[c])        */
    const uint16_t *cbf_sub;      /* [n_cu] or NULL: for CUs wider/taller than 64, bit (4*c + sb) = nnz_sub[c][sb]
                                     of the 64x64 sub-blocks sb = (j<<1)|i (xevd_itdq.c:544-621); NULL = every
                                     sub-block of a coded component is coded                                */
    const uint8_t  *ipm;          /* [n_cu][2] intra luma / chroma mode of intra CUs (core->ipm[0..1]): IPD_DC_B 0, HOR 1, VER 2,
                                     UL 3, UR 4 (src_base/xevd_def.h:332-342); NULL = DC                      */
    const uint8_t  *ats;          /* [n_cu] or NULL: bit 0 = ats_intra_cu, bit 1 = ats_intra_mode_v, bit 2 = ats_intra_mode_h
                                     (0 = DST-VII, 1 = DCT-VIII; luma TB of intra CUs, xevdm.c:602, xevdm_itdq.c:406-421)   */
    const uint8_t  *ats_inter;    /* [n_cu] or NULL: ats_inter_info of inter CUs = idx | pos << 4 (src_main/xevdm_def.h:232-236):
                                     idx 1/3 = left|right half/quarter-width TU, 2/4 = top|bottom half/quarter-height TU, pos 0 =
                                     first part coded, 1 = last part.  The CU's coefficient blocks then have the TU size
                                     (xevdm_get_tu_size, xevdm_util.c:3585-3608) for all three components          */
    const uint32_t *coef_off;     /* [n_cu]  offset (in s16 units) of the CU's first coefficient          */
    const int16_t  *coef;         /* [n_coef] coefficient arena                                           */
    size_t          n_coef;
    int             n_ctu;
    const uint32_t *ctu_cu_start; /* [n_ctu+1] first CU of every CTU in CTU decode order (raster; with tiles: tile by tile) */
    int             constrained_intra_pred;   /* pps.constrained_intra_pred_flag: intra CUs only predict from intra neighbours
                                                 (xevd_get_nbr_b, src_base/xevd_ipred.c:47,61,77)          */
    /* affine motion (Main, sps->tool_affine; xevdm_affine_mc, src_main/xevdm_mc.c:2606): both NULL = no affine CU in the batch */
    const uint8_t  *affine;       /* [n_cu] or NULL: 0 = translational, 2 / 3 = control points of an inter CU (mcore->affine_flag + 1);
                                     CUs of at least 8x8.  `mv` of such a CU is only stored for a list it does not use          */
    const int16_t  *affine_mv;    /* [n_cu][2][3][2] quarter-pel control-point vectors mcore->affine_mv[list][vertex][x/y]
                                     (top-left, top-right, bottom-left; the third ignored with 2 control points)              */
    const uint8_t  *dmvr;         /* [n_cu] or NULL: 1 = the CU's merge mode allows decoder-side motion vector refinement (sps->tool_dmvr and mcore->dmvr_enable:
                                     a skip CU without MMVD or a direct-mode CU, not affine; src_main/xevdm.c:1272-1288).  The backend applies the
                                     remaining conditions of xevdm_mc (two references at equal POC distances on either side of the picture, at least
                                     8x8, src_main/xevdm_mc.c:1895-1911) and refines per 16x16 sub-block (processDMVR :1647-1829).  The SCU map the
                                     deblocking filter reads keeps the UNREFINED vectors (map_unrefined_mv, xevdm.c:2009-2041); the refined ones
                                     come back through xgpu_batch_dmvr_mvs for the host's temporal motion prediction                              */
    int             htdf_slice_qp;/* 0 = no HTDF.  With sps->tool_htdf: ctx->sh.qp of the picture's slice - the Hadamard-domain filter
                                     (xevdm_htdf, src_main/xevdm_recon.c:153-385) then runs on the luma block of every intra CU and every
                                     inter CU with luma coefficients right after its reconstruction, reading one sample of border from
                                     the CUs reconstructed before it (xevdm.c:1381-1392; a slice QP up to 17 switches it off)          */
    const xgpu_tile_grid *tiles;  /* NULL = one tile.  Else the CUs come tile by tile (tiles in raster order, CTUs in raster order inside a
                                     tile - xevdm_dec_slice, src_main/xevdm.c:2614-2718) and neighbours in another tile are unavailable   */
    const uint8_t  *tree;         /* [n_cu] or NULL: local dual tree of Main streams with sps_btt_flag and tool_admvp (mode constraint eOnlyIntra below a split that
                                     would leave chroma blocks under 16 samples, src_main/xevdm.c:1775-1833): 0 = the CU has luma and chroma, 1 = luma only
                                     (TREE_L: intra or IBC; cbf bits 1-2 clear; writes the SCU maps as usual), 2 = chroma only (TREE_C: the split node's
                                     chroma block, intra, ipm[0] = the luma mode its DM refers to, cbf bit 0 clear; follows its luma CUs in decoding order,
                                     leaves the SCU maps alone; chroma edges are deblocked at ITS border, not at those of the luma CUs inside)          */
} xgpu_cu_batch;

/* ------------------------------------------------------------------ lifetime ---------------------- */
int  xgpu_open(const xgpu_seq_params *sp, xgpu_ctx **out);
void xgpu_close(xgpu_ctx *ctx);
int  xgpu_sync(xgpu_ctx *ctx);                         /* wait for everything enqueued on the ctx stream */
const char *xgpu_last_error(const xgpu_ctx *ctx);
const char *xgpu_version(void);

/* Pinned host memory for the arrays a batch points at (north_star: "batches decoded CUs per tile into pinned SoA buffers"): a coefficient
   arena inside such a range is sent to the device straight from the caller's buffer, everything else through the context's staging
   blocks.  The range must stay untouched until xgpu_batch_wait_upload() of the batch that points into it has returned.            */
int  xgpu_host_alloc(xgpu_ctx *ctx, size_t bytes, void **out);
void xgpu_host_free(xgpu_ctx *ctx, void *p);

/* ------------------------------------------------------------------ pictures ---------------------- */
int  xgpu_pic_alloc(xgpu_ctx *ctx);                    /* -> slot >= 0, or error                          */
int  xgpu_pic_free(xgpu_ctx *ctx, int pic);
/* planes point at the first ACTIVE sample (XEVD_PIC.y/u/v); strides in samples.  Upload does not pad.   */
int  xgpu_pic_upload(xgpu_ctx *ctx, int pic, const int16_t *y, int s_y, const int16_t *u, const int16_t *v, int s_c);
int  xgpu_pic_download(xgpu_ctx *ctx, int pic, int16_t *y, int s_y, int16_t *u, int16_t *v, int s_c);
/* The output side in one call: the active area minus a conformance-window crop (luma samples, even: sps picture_crop_*_offset
   as xevd_pull reports them), converted to out_bit_depth - 8: one byte per sample, (v + round) >> shift clipped to 255;
   below the coding depth: the same rounding shift clipped to the range, 16 bit; above: v << shift; equal: copy - and packed
   as Y, U, V planes back to back without row padding (the bytes imgb_write puts in a .yuv file).  Crop, conversion and
   packing run on the device; `dst` (host, >= xgpu_pic_output_size() bytes) receives one contiguous copy.  Blocking.
   `dra` (NULL = none): the DRA post-filter xevd_pull applies to its copy of the picture when sps->tool_dra and the PPS names a
   DRA parameter set (xevd_apply_filter, src_main/xevdm.c:3305-3349): the inverse-mapping tables of DRA_CONTROL after xevd_init_dra
   (the table construction stays host code), applied before the conversion - Cb and Cr scaled around 512 by a factor looked up
   with the UNMAPPED luma sample at (2y, 2x), then luma through its table (xevdm_dra.c:272-355); 4:2:0 at up to 10 bit. */
typedef struct xgpu_dra_luts {
    const int32_t *luma_inv_scale_lut;         /* [1024]  DRA_CONTROL.luma_inv_scale_lut          */
    const int32_t *chroma_inv_scale_lut[2];    /* [1024]  DRA_CONTROL.int_chroma_inv_scale_lut[c] */
} xgpu_dra_luts;
size_t xgpu_pic_output_size(const xgpu_ctx *ctx, int out_bit_depth, int crop_l, int crop_r, int crop_t, int crop_b);   /* 0: invalid */
int  xgpu_pic_output(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, int out_bit_depth, int crop_l, int crop_r, int crop_t, int crop_b,
                     void *dst, size_t dst_size);
/* The same in two halves, for a decode loop that overlaps the output of picture k with the kernels of picture k+1: _async queues the
   conversion behind the picture's kernels and the copy to `dst` (pinned memory for a truly asynchronous copy) on the context's download
   stream and returns a ticket; _wait blocks until `dst` holds the picture.  At most two outputs are in flight (a third call waits for the
   first); the picture slot may be decoded into again as soon as _async has returned.                                                   */
int  xgpu_pic_output_async(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, int out_bit_depth, int crop_l, int crop_r, int crop_t, int crop_b,
                           void *dst, size_t dst_size, int *ticket);
int  xgpu_pic_output_wait(xgpu_ctx *ctx, int ticket);
/* Output into device memory - for a consumer on the same GPU (a model, a metric), no staging buffer, no copy to the host.  The same crop and DRA as
   xgpu_pic_output, then one of:
     XGPU_OUT_YUV420P          xgpu_pic_output's bytes (k_output unchanged): dtype U8 with out_bit_depth 8, else U16 (out_bit_depth 0 = the coding depth)
     XGPU_OUT_RGB_PLANAR       3 planes of H x W (R, G, B - or B, G, R with bgr), plane k at k * H * row_pitch
     XGPU_OUT_RGB_INTERLEAVED  H rows of W x 3 elements
   RGB: 4:2:0 chroma upsampled on the cropped chroma plane (edge-clamped) - NEAREST c[y>>1][x>>1], or LINEAR with quarter weights placed by
   chroma_loc (H.273 ChromaSampleLocType 0..5), (sum + 8) >> 4 - then Y'CbCr -> R'G'B' with the matrix of `matrix` (H.273 MatrixCoefficients
   1 BT.709, 4 FCC, 5 / 6 BT.601, 7 SMPTE 240M, 9 BT.2020 non-constant luminance; others XGPU_ERR_UNSUPPORTED) and limited / full range.
   Integer outputs (U8: 8 bit, U16: the coding depth) are fixed point: coefficients round(k * (2^D - 1) / range * 2^S), S = 27 - D, channel =
   clip((sum + 2^(S-1)) >> S, 0, 2^D - 1); float outputs evaluate the same formula in float32 with 2^D - 1 = 1, clipped to [0, 1] (F16 / BF16: that
   value rounded to nearest even).
   Video surfaces (k_output_yuv.hip), for an encoder, a display path, another GPU video library, or a model that works on Y'CbCr:
     XGPU_OUT_NV12             H rows of W luma elements, then H/2 rows of W elements Cb0 Cr0 Cb1 Cr1 ..., all rows row_pitch apart, the chroma plane at
                               H * row_pitch.  The samples of YUV420P at the same out_bit_depth, one for one: U8 with out_bit_depth 8, or U16 with
                               out_bit_depth 0 (the coding depth, which must be above 8) or 9..16, value in the low bits
     XGPU_OUT_P016             as NV12, U16 only: word = (sample at depth D) << (16 - D), D = out_bit_depth (0 = the coding depth, else 8..16) -
                               D = 10 is P010, 12 is P012
     XGPU_OUT_YUV444_PLANAR / _INTERLEAVED   Y, Cb, Cr at luma resolution, laid out as the RGB layouts: chroma upsampled as for RGB (upsample,
                               chroma_loc), then U8: the 8-bit rule of xgpu_pic_output; U16: the sample (out_bit_depth 0 or the coding depth); floats:
                               H.273's E'Y = clip((Y - yo) * fy, 0, 1), E'Cb = clip((Cb - 2^(B-1)) * fc, -0.5, 0.5), E'Cr alike, fy = float32(1 / yr),
                               fc = float32(1 / cr) with the offset and excursions of full_range
   These four read neither matrix nor bgr (bgr must be 0); NV12 / P016 read no chroma_loc, upsample or full_range.
   The exact contract: INTEGRATION.md section 8a. */
#define XGPU_OUT_YUV420P          0
#define XGPU_OUT_RGB_PLANAR       1
#define XGPU_OUT_RGB_INTERLEAVED  2
#define XGPU_OUT_NV12             3
#define XGPU_OUT_P016             4
#define XGPU_OUT_YUV444_PLANAR    5
#define XGPU_OUT_YUV444_INTERLEAVED 6
#define XGPU_OUT_U8               0
#define XGPU_OUT_U16              1
#define XGPU_OUT_F16              2
#define XGPU_OUT_BF16             3
#define XGPU_OUT_F32              4
#define XGPU_UPSAMPLE_NEAREST     0
#define XGPU_UPSAMPLE_LINEAR      1
typedef struct xgpu_output_format {
    int layout;                /* XGPU_OUT_YUV420P | _RGB_PLANAR | _RGB_INTERLEAVED | _NV12 | _P016 | _YUV444_PLANAR | _YUV444_INTERLEAVED */
    int bgr;                   /* RGB layouts: channel order B, G, R; every other layout: 0                                          */
    int dtype;                 /* XGPU_OUT_U8 | _U16 | _F16 | _BF16 | _F32 (YUV420P, NV12: U8 / U16 by out_bit_depth; P016: U16)     */
    int out_bit_depth;         /* YUV420P, NV12, P016: as xgpu_pic_output (0 = the coding depth); RGB, YUV444: 0 or the coding depth */
    int matrix, full_range, chroma_loc, upsample;      /* H.273 MatrixCoefficients, video_full_range_flag, ChromaSampleLocType, XGPU_UPSAMPLE_* */
    int crop[4];               /* left, right, top, bottom luma samples - even                                                        */
    size_t row_pitch;          /* bytes between rows of a plane / of the interleaved image; 0 = tight (YUV420P: must be 0)            */
} xgpu_output_format;
/* Host only, no context: the bytes format `f` needs at d_dst for a picture of width x height (the uncropped size) at coding depth bit_depth, the last
   row tight; 0: invalid format or size.  NV12 / P016: (H + H/2 - 1) * pitch + W * es; RGB / YUV444 planar: (3H - 1) * pitch + W * es, interleaved:
   (H - 1) * pitch + 3W * es (W, H cropped, es the element size, pitch = row_pitch or the tight row); YUV420P: xgpu_pic_output_size's. */
size_t xgpu_output_format_size(const xgpu_output_format *f, int width, int height, int bit_depth);
/* xgpu_output_format_size with the context's picture size and coding depth */
size_t xgpu_pic_output_device_size(const xgpu_ctx *ctx, const xgpu_output_format *f);
/* Non-blocking.  d_dst: device memory of the context's device, aligned to the element size, >= xgpu_pic_output_device_size bytes (checked - with
   hipPointerGetAttributes - before anything is queued: XGPU_ERR_INVALID_ARGUMENT and no launch otherwise).  stream = NULL: the context's stream;
   else the kernel runs on `stream` (a hipStream_t - e.g. torch.cuda.current_stream().cuda_stream) behind the picture's kernels, and the context's
   stream waits for it before it touches the picture slot or the DRA tables again. */
int    xgpu_pic_output_device(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, void *d_dst, size_t dst_size, void *stream);
/* Host only, no context: the fixed-point coefficients the kernel uses for format `f` at coding depth `bit_depth` - coef = { cy, crv, cgu, cgv, cbu }
   with `shift` = S (integer dtypes; zeros for float dtypes), fcoef = the float32 ones (2^D - 1 = 1).  0, or a negative code for an invalid format. */
int    xgpu_output_coeffs(const xgpu_output_format *f, int bit_depth, int32_t coef[5], int *shift, float fcoef[5]);
/* ---- colour-managed RGB output (k_output_cm.hip): the R'G'B' of the two RGB layouts taken from the stream's colour space to the caller's.  After the
   fixed-point Y'CbCr -> R'G'B' of the U16 form (the code at the coding depth B, whatever the output dtype): (1) linearise with the inverse of the source
   transfer characteristic, (2) source -> destination primaries, (3) tone curve or linear_scale, clip to [0, 1], (4) re-encode with the destination
   transfer characteristic, then the output dtype.  Transfer characteristics (H.273): 1 / 6 / 14 / 15 the BT.709 curve, 4 gamma 2.2, 5 gamma 2.8, 8 linear,
   13 sRGB, 16 PQ (1.0 linear = 10000 cd/m2), 18 HLG (the BT.2100 OETF and its inverse: scene light); others XGPU_ERR_UNSUPPORTED.  Primaries (H.273):
   1 BT.709, 5 BT.601 625, 6 / 7 BT.601 525 / SMPTE 240M, 9 BT.2020, 12 P3-D65 (all D65, no chromatic adaptation); others XGPU_ERR_UNSUPPORTED.
   tone_map = 0: step 3 multiplies by linear_scale (0 means 1).  tone_map = 1: step 3 multiplies the three channels by g(Y) / Y (one IEEE float32 division), Y the luminance in the source
   primaries, g = the display luminance of Y (PQ: 10000 Y; HLG: the BT.2100 OOTF src_peak * Y^gamma, gamma = 1.2 + 0.42 log10(src_peak / 1000); else
   src_peak * Y) through the BT.2390 EETF from src_peak to dst_peak (identity when dst_peak >= src_peak), divided by the destination's white (10000 for PQ,
   else dst_peak); linear_scale is not read; destination HLG is XGPU_ERR_UNSUPPORTED with tone_map.  Peaks in cd/m2, 0 = 1000 for a PQ / HLG side, 100 otherwise.
   No powf / exp2f in the kernel: table lookups in tables made here in double precision, and float32 multiplies and adds rounded one by one - the contract,
   operation by operation, is INTEGRATION.md section 8b; tests/colour_cm_ref.py restates it in numpy, bit for bit. */
typedef struct xgpu_colour_transform {
    int   src_primaries, src_transfer;      /* H.273 ColourPrimaries / TransferCharacteristics of the stream */
    int   dst_primaries, dst_transfer;      /* of the output                                                  */
    int   tone_map;                         /* 0 | 1                                                          */
    float src_peak, dst_peak;               /* cd/m2, tone_map = 1 only; 0 = the default                      */
    float linear_scale;                     /* tone_map = 0 only; 0 = 1                                       */
} xgpu_colour_transform;
/* A curve table: a function of v in [0, 1] sampled at 0, at the floats 2^-64 * 2^(j / 32) ... - exactly: at the float32 values whose bit pattern is
   XGPU_CM_CURVE_U0 + (j << 18), j = 0 .. 2048 (2^-64 .. 1.0, 32 per octave) - and one repeat of the last entry.  Evaluation (section 8b): v < 2^-64:
   k = 0, t = v * 2^64; else k = 1 + ((bits(v) - U0) >> 18), t = (bits(v) & 0x3FFFF) * 2^-18; value = T[k] + t * (T[k + 1] - T[k]). */
#define XGPU_CM_CURVE_U0    0x1F800000u
#define XGPU_CM_CURVE_SIZE  (64 * 32 + 3)
typedef struct xgpu_colour_tables_t {
    int   n_lin;                            /* 2^bit_depth                                                                            */
    int   use_matrix, use_tone, use_encode; /* step 2 runs (primaries differ) / step 3 reads `tone` / step 4 reads `encode` (destination not linear) */
    float lin[4096];                        /* step 1: linear light of the R'G'B' code k, k = 0 .. n_lin - 1                          */
    float matrix[9];                        /* step 2: row-major, destination = matrix x source                                       */
    float luma[3];                          /* step 3: Y = luma . (R, G, B) in the source primaries                                   */
    float scale;                            /* step 3 with tone_map = 0                                                               */
    float tone[XGPU_CM_CURVE_SIZE];         /* step 3 with tone_map = 1: g(Y), in the destination's linear range                      */
    float encode[XGPU_CM_CURVE_SIZE];       /* step 4: the destination transfer characteristic                                        */
} xgpu_colour_tables_t;
/* Host only, no context: everything the kernel reads for transform `cm` on the RGB format `f` at coding depth `bit_depth`.  0, XGPU_ERR_UNSUPPORTED for a
   transfer characteristic or primaries outside the lists above, XGPU_ERR_INVALID_ARGUMENT for the rest (a layout that is not RGB, a negative peak or scale). */
int    xgpu_colour_tables(const xgpu_output_format *f, const xgpu_colour_transform *cm, int bit_depth, xgpu_colour_tables_t *out);
/* xgpu_pic_output_device with the colour transform `cm` (NULL: xgpu_pic_output_device itself).  RGB layouts only - with any other layout
   XGPU_ERR_INVALID_ARGUMENT; every refusal comes before anything is queued.  The tables are kept per context and made and uploaded again - on the stream the
   kernel runs on, ordered like the DRA tables - only when `cm` or the depth differ from the previous call's. */
int    xgpu_pic_output_device_cm(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_colour_transform *cm,
                                 void *d_dst, size_t dst_size, void *stream);
/* ---- scaled output (k_output_scaled.hip): the picture resized to the size a model takes, converted and normalised, from the picture read once.  The source is
   the active picture minus f->crop (even; it doubles as the region of interest), Ws x Hs luma samples; the destination is sc->width x sc->height elements per
   channel, in one of the four three-channel layouts (XGPU_OUT_RGB_PLANAR / _INTERLEAVED, XGPU_OUT_YUV444_PLANAR / _INTERLEAVED; any other:
   XGPU_ERR_INVALID_ARGUMENT).  Y is filtered from the luma plane, Cb and Cr straight from their half-resolution planes onto the destination grid, placed by
   f->chroma_loc (f->upsample is not read).  Two separable passes of non-negative 14-bit integer taps, vertical first: t = (sum qy * sample + 2^10) >> 11, then
   v = (sum qx * t + 2^16) >> 17; every source sample is DRA-mapped (when `dra` is given) and clipped to [0, 2^B - 1] first.  (Y, Cb, Cr) of the destination
   pixel then go through the conversion of xgpu_pic_output_device (matrix, range, bgr, integer and float rules unchanged).  normalize (float dtypes only):
   out = (v - mean[k]) * inv_std[k] after the clip, in float32, subtraction and multiplication rounded one by one, k the channel's position in the output (after
   bgr); then the F16 / BF16 rounding.
     XGPU_SCALE_BILINEAR   the triangle widened by the reduction ratio - the window of torch / PIL resizing with antialias=True; plain bilinear when enlarging
     XGPU_SCALE_AREA       the box: every destination sample is the mean of the source area it covers
   Limits: 2 <= width, height <= 16384, and per axis Ws / 64 <= width <= 8 Ws: XGPU_ERR_UNSUPPORTED outside.  normalize with an integer dtype, a non-finite mean
   or inv_std: XGPU_ERR_INVALID_ARGUMENT.  Every refusal comes before anything is queued.  With the destination the size of the source and XGPU_UPSAMPLE_LINEAR the
   result is xgpu_pic_output_device's, bit for bit, for every chroma_loc (R'G'B' floats: see INTEGRATION.md).  The exact contract: INTEGRATION.md section 8d;
   tests/scale_ref.py restates it in numpy, the taps with fractions.Fraction. */
#define XGPU_SCALE_BILINEAR 0
#define XGPU_SCALE_AREA     1
typedef struct xgpu_scale_params { int width, height, filter, normalize; float mean[3], inv_std[3]; } xgpu_scale_params;
/* Host only, no context: the taps of one axis of one plane - n_plane samples, subsampling 1 (luma) or 2 (chroma), the chroma grid siting_half_luma / 2 luma
   samples behind the luma grid (0, 1, 2; luma: 0), n_dst destination samples.  Destination sample o reads samples first[o] .. first[o] + count[o] - 1 with the
   weights w[o * w_stride + k] (sum 16384, none negative; the rest of the row is set to 0).  Returns the widest row (w = NULL: first and count alone), or
   XGPU_ERR_UNSUPPORTED for a size outside the limits above, XGPU_ERR_INVALID_ARGUMENT for the rest (w_stride narrower than a row included).  Integer arithmetic
   only: no float or double takes part. */
int    xgpu_scale_taps(int n_plane, int subsampling, int siting_half_luma, int n_dst, int filter, int32_t *first, int32_t *count, int16_t *w, int w_stride);
/* Host only, no context: the bytes (f, sc) need at d_dst for a picture of width x height (the uncropped size) at coding depth bit_depth - xgpu_output_format_size
   with sc->width x sc->height in the place of the cropped size; 0: refused.  xgpu_output_scaled_check: 0, or the code xgpu_pic_output_device_scaled refuses with. */
size_t xgpu_output_scaled_size(const xgpu_output_format *f, const xgpu_scale_params *sc, int width, int height, int bit_depth);
int    xgpu_output_scaled_check(const xgpu_output_format *f, const xgpu_scale_params *sc, int width, int height, int bit_depth);
/* Non-blocking; d_dst, dst_size and stream as xgpu_pic_output_device takes them.  The tap tables and the intermediate of the vertical pass belong to the context:
   the tables are made and uploaded again - on the stream the kernels run on, ordered like the DRA tables - only when the source size, the destination size, the
   filter or chroma_loc differ from the previous call's; the intermediate grows on demand (growing it waits for the device).  Calls on different streams are ordered
   one behind the other through the context's stream, so they never overlap on either. */
int    xgpu_pic_output_device_scaled(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                                     void *d_dst, size_t dst_size, void *stream);
/* ---- regions of interest (k_output_rois.hip): n_rois rectangles of one picture, each resized to the same sc->width x sc->height, converted and normalised, as a
   batch of images - [N, 3, H, W] or [N, H, W, 3] - from one call: two kernel launches and one upload, however many rectangles.  Image i is laid out as
   xgpu_pic_output_device_scaled lays out its one image (the four layouts, the five dtypes, f->row_pitch) and starts rp->image_pitch * i bytes behind d_dst;
   image_pitch 0 = tight: rows x row pitch (3 H rows planar, H interleaved); otherwise a multiple of the element size, not shorter than one image (the bytes
   xgpu_output_scaled_size counts).  A rectangle is given in luma samples inside the picture minus f->crop; x, y, width and height are even.  It is a source of its
   own, exactly as a crop is for the scaled output: taps end at its edge and nothing outside it reaches a result.  Rectangles may overlap and repeat.
     XGPU_FIT_STRETCH     the rectangle fills the image: image i is, bit for bit, what xgpu_pic_output_device_scaled writes with f->crop set to rectangle i
     XGPU_FIT_LETTERBOX   the rectangle keeps its shape: with Ws x Hs the rectangle and Wd x Hd the image, Ws Hd >= Hs Wd gives the inner size Wi = Wd,
                          Hi = min(Hd, max(2, (2 Hs Wd + Ws) / (2 Ws))) (integer division), else Hi = Hd and Wi by the same rule with the axes exchanged; the
                          inner part lies at ((Wd - Wi) >> 1, (Hd - Hi) >> 1) and is the scaled output of the rectangle at Wi x Hi; every other element of the
                          image is rp->pad[k], k the channel's position in the output (after bgr, as for mean).  Float dtypes: pad[k] is a finite float32 in the
                          domain before the normalise and goes through the same (v - mean[k]) * inv_std[k] and the F16 / BF16 rounding; integer dtypes: an
                          integer in [0, 2^D - 1] (D = 8 for U8, else the coding depth).  pad is not read with XGPU_FIT_STRETCH.
   xgpu_roi_inner (host only): x, y, width, height of the filtered part inside the image - what maps a detection in image i back into rectangle i.
   Refusals, all before anything is queued; *bad_index (may be NULL) receives the index of the rectangle the refusal names, else -1:
     XGPU_ERR_INVALID_ARGUMENT   n_rois outside 1 .. XGPU_MAX_ROIS, an odd rectangle or one that leaves the picture minus f->crop, an unknown fit, a bad pad, a bad
                                 image_pitch, and whatever xgpu_pic_output_device_scaled refuses with this code
     XGPU_ERR_UNSUPPORTED        sc->width or sc->height outside 2 .. 16384; a rectangle whose inner size is outside the scaled output's limits per axis
                                 (2 <= Wi, Ws / 64 <= Wi <= 8 Ws, the height alike); a call whose intermediate - the sum over the rectangles of
                                 Hi * (align8(Ws) + 2 * align8(Ws / 2)) * 2 bytes, align8 rounding up to a multiple of 8 - exceeds 512 MiB (bad_index: the
                                 rectangle at which the sum passes the limit) */
typedef struct xgpu_roi { int x, y, width, height; } xgpu_roi;
#define XGPU_FIT_STRETCH   0
#define XGPU_FIT_LETTERBOX 1
#define XGPU_MAX_ROIS      1024
typedef struct xgpu_roi_params { int fit; float pad[3]; size_t image_pitch; } xgpu_roi_params;
int    xgpu_roi_inner(const xgpu_roi *r, const xgpu_scale_params *sc, int fit, int inner[4]);
/* Host only, no context: 0 or the code the call refuses with / the bytes the call needs at d_dst (0: refused), for a picture of width x height at bit_depth */
int    xgpu_output_rois_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois,
                              int width, int height, int bit_depth, int *bad_index);
size_t xgpu_output_rois_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois,
                             int width, int height, int bit_depth);
/* Non-blocking; d_dst, dst_size and stream as xgpu_pic_output_device takes them.  `rois` is host memory, read during the call.  The descriptor block and the
   intermediate belong to the context, grow on demand (growing waits for the device) and are ordered like the scaled output's buffers; the tap tables the scaled
   output caches are left alone. */
int    xgpu_pic_output_device_rois(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                                   const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois, void *d_dst, size_t dst_size, void *stream);
/* ---- colour-managed scaled output (k_output_scaled_cm.hip): xgpu_pic_output_device_scaled and xgpu_pic_output_device_rois with the colour transform `cm` of
   xgpu_pic_output_device_cm between the filter and the store - model-sized, normalised sRGB (or any listed destination) from a PQ / HLG / BT.2020 stream without
   the full-size tensor.  Per destination pixel: (Y, Cb, Cr) at the coding depth as the scaled output filters them (the encoded Y'CbCr samples are filtered, not
   linear light); the integer R'G'B' code at the coding depth (the U16 form's matrix, whatever the dtype); the transform's steps 1 to 4; integers
   rint(q * (2^D - 1)), floats q; then bgr, the normalise and the F16 / BF16 rounding as the scaled output does them.  A letterbox pad value is written as
   xgpu_pic_output_device_rois writes it: a value of the destination space, normalised like a pixel, never transformed.  The exact contract: INTEGRATION.md
   section 8m; tests/scaled_cm_ref.py restates it on top of tests/scale_ref.py, tests/colour_cm_ref.py and tests/roi_ref.py.
   cm = NULL: the plain call itself.  Destination sizes: xgpu_output_scaled_size / xgpu_output_rois_size.  Refusals, all before anything is queued, in this order:
   the plain call's, with its codes; a layout that is not RGB: XGPU_ERR_INVALID_ARGUMENT; whatever xgpu_colour_tables returns for `cm`.  The tables are the
   context's cache of xgpu_pic_output_device_cm: a full-size call and a scaled one with the same transform and depth upload once.
   xgpu_output_scaled_cm_check (host only, no context): 0, or the code xgpu_pic_output_device_scaled_cm refuses with. */
int    xgpu_output_scaled_cm_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_colour_transform *cm, int width, int height, int bit_depth);
int    xgpu_pic_output_device_scaled_cm(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                                        const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream);
int    xgpu_pic_output_device_rois_cm(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                                      const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois, const xgpu_colour_transform *cm, void *d_dst, size_t dst_size,
                                      void *stream);
/* ---- scaled output filtered in linear light (k_output_scaled_lin.hip): the two calls above with the filter moved behind the linearisation - what a reduced PQ / HLG
   picture needs where it has fine, high-contrast detail (averaging code values darkens it; the mean of a black and a white stripe is half the white's light).
   Per source pixel at luma resolution: (Y, Cb, Cr) as xgpu_pic_output_device forms them (f->upsample and f->chroma_loc ARE read here: chroma is upsampled on the
   source's own chroma plane, edge-clamped there), the integer R'G'B' code at the coding depth, L_c = lin[code_c].  Vertical pass, luma row table for all three
   channels: T_c = sum over k ascending of float32(qy[k]) * L_c.  Horizontal pass: V_c = (sum over k ascending of float32(qx[k]) * T_c) * 2^-28.  Every multiply
   and add is rounded to float32 on its own; an accumulator starts as the first product.  (V_R, V_G, V_B) then run the transform from its primaries matrix on
   (steps 2 to 4), and bgr, the normalise and the F16 / BF16 rounding follow as in the scaled output.  Image i of a stretched batch is, bit for bit, the single
   call with the crop set to rectangle i; a letterbox pad value is never transformed.  The exact contract: INTEGRATION.md section 8n; tests/scaled_lin_ref.py
   restates it.  Destination sizes: xgpu_output_scaled_size / xgpu_output_rois_size.  The intermediate (the context's, grown on demand) is float32 at luma width:
   3 x Hd x align8(Ws) x 4 bytes, summed over the rectangles (Hd: the inner height).
   Refusals, all before anything is queued, in this order: the plain call's, with its codes - the batch's 512 MiB rule counts the float32 intermediate, with
   *bad_index as xgpu_output_rois_check sets it; the single call's intermediate above 512 MiB: XGPU_ERR_UNSUPPORTED; cm = NULL: XGPU_ERR_INVALID_ARGUMENT (without
   a transform there is no linear light); a layout that is not RGB: XGPU_ERR_INVALID_ARGUMENT; whatever xgpu_colour_tables returns for `cm`.
   xgpu_output_scaled_lin_check / xgpu_output_rois_lin_check (host only, no context): 0, or the code the call refuses with. */
int    xgpu_output_scaled_lin_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_colour_transform *cm, int width, int height, int bit_depth);
int    xgpu_output_rois_lin_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois,
                                  const xgpu_colour_transform *cm, int width, int height, int bit_depth, int *bad_index);
int    xgpu_pic_output_device_scaled_lin(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                                         const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream);
int    xgpu_pic_output_device_rois_lin(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                                       const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois, const xgpu_colour_transform *cm, void *d_dst, size_t dst_size,
                                       void *stream);
/* ---- bicubic resize (k_output_resampled.hip): the scaled output and the host-box batch with a cubic BC-spline in place of the triangle / box - the resize CLIP /
   SigLIP, DINOv2 and most timm configurations were trained with.  Calls of their own with a parameter struct of their own: xgpu_scale_params.filter keeps its two
   values.  Layouts, dtypes, row_pitch / image_pitch, the crop, DRA, chroma_loc, matrix, range, bgr, the normalise, stretch / letterbox and the pad value, stream
   ordering, the limits (2 .. 16384 per axis, Ws / 64 <= Wd <= 8 Ws, 512 MiB of intermediate per batch) and every refusal are section 8d's and 8e's; an unknown
   kernel or an antialias other than 0 / 1 is XGPU_ERR_INVALID_ARGUMENT.  Only the two passes differ (tests/resample_ref.py restates it):
     taps     one axis of one plane in section 8d's notation, f = antialias ? max(1, n / N) : 1: the row of destination sample o is every plane sample i in
              0 .. n - 1 with |i - c| < 2 f, weighted k((i - c) / f) with k the BC-spline of the kernel; q(i) = floor(w(i) / W * 16384 + 1/2), 16384 - sum q goes
              to the largest q (the first of equals); negative and zero q stay in the row.  xgpu_resample_taps builds a table on the host, in integers only, as
              xgpu_scale_taps does (same arguments and return value); a row with W <= 0 or sum |q| > 32768 makes it return XGPU_ERR_UNSUPPORTED.
     passes   t = (sum qy * clip(dra(sample), 0, 2^B - 1) + 2^11) >> 12 (arithmetic shift), a signed 16-bit value with two fraction bits, not clipped;
              v = clip((sum qx * t + 2^15) >> 16, 0, 2^B - 1).  (Y, Cb, Cr) then take the scaled output's conversion, bgr and normalise.
   The intermediate (the context's, grown on demand) has the scaled output's size; image i of a batch is, bit for bit, the single call with the crop set to
   rectangle i.  Not offered: Lanczos, boxes in device memory, the colour-managed and linear-light forms, the ladder, warp and remap. */
#define XGPU_RESAMPLE_CATMULL_ROM 0   /* Keys a = -1/2 = BC(0, 1/2): PIL BICUBIC, torch bicubic with antialias=True */
#define XGPU_RESAMPLE_CUBIC_075   1   /* Keys a = -3/4 = BC(0, 3/4): torch bicubic with antialias=False, OpenCV INTER_CUBIC */
#define XGPU_RESAMPLE_MITCHELL    2   /* BC(1/3, 1/3) */
typedef struct xgpu_resample_params { int width, height, kernel, antialias, normalize; float mean[3], inv_std[3]; } xgpu_resample_params;
int    xgpu_resample_taps(int n_plane, int subsampling, int siting_half_luma, int n_dst, int kernel, int antialias,
                          int32_t *first, int32_t *count, int16_t *w, int w_stride);
size_t xgpu_output_resampled_size(const xgpu_output_format *f, const xgpu_resample_params *rs, int width, int height, int bit_depth);
int    xgpu_output_resampled_check(const xgpu_output_format *f, const xgpu_resample_params *rs, int width, int height, int bit_depth);
int    xgpu_pic_output_device_resampled(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_resample_params *rs,
                                        void *d_dst, size_t dst_size, void *stream);
int    xgpu_output_rois_resampled_check(const xgpu_output_format *f, const xgpu_resample_params *rs, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois,
                                        int width, int height, int bit_depth, int *bad_index);
size_t xgpu_output_rois_resampled_size(const xgpu_output_format *f, const xgpu_resample_params *rs, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois,
                                       int width, int height, int bit_depth);
int    xgpu_pic_output_device_rois_resampled(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_resample_params *rs,
                                             const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois, void *d_dst, size_t dst_size, void *stream);
/* ---- packed display surfaces (k_output_packed.hip): the picture as one word per pixel for a compositor or a swap chain, or as packed 4:2:2 for a capture /
   SDI path or an encoder that takes it.  Calls of their own with a format struct of their own: xgpu_output_format keeps its seven layouts.  W x H: the picture
   minus crop, B the coding depth, es the element size.
     XGPU_PACKED_RGBA     H rows of W x 4 elements R G B A (bgr: B G R A), dtype U8 | U16 | F16 | BF16 | F32.  R, G, B are, bit for bit, the three elements
                          xgpu_pic_output_device writes for XGPU_OUT_RGB_INTERLEAVED with the same dtype, matrix, full_range, chroma_loc, upsample, bgr, crop and
                          DRA - with `cm` those of xgpu_pic_output_device_cm; out_bit_depth 0 or B.  A: integer dtypes floor(alpha * (2^D - 1) + 0.5), made once
                          on the host in double, D = 8 for U8, else B; float dtypes: float32(alpha) through the dtype's rounding.
     XGPU_PACKED_RGB10A2  H rows of W little-endian 32-bit words R | G << 10 | B << 20 | A << 30 (bgr: B low, R at 20); dtype and out_bit_depth 0; d_dst aligned
                          to 4.  The channels are 10-bit codes of the integer rule above with D = 10 whatever B is: coefficients round(k * 1023 / range * 2^17),
                          channel = clip((sum + 2^16) >> 17, 0, 1023) - on a 10-bit stream the U16 output's values.  With `cm` the code at depth B goes into the
                          transform (as for every dtype) and the store is rint(q * 1023).  A = floor(alpha * 3 + 0.5).
     XGPU_PACKED_YUYV     4:2:2, H rows of W x 2 elements, per pair of pixels Y0 Cb Y1 Cr; XGPU_PACKED_UYVY: Cb Y0 Cr Y1.  Luma is NV12's.  Chroma stays at half
                          width and goes to full height: row r from the rows around i = r >> 1 of the cropped chroma plane, edge-clamped, every sample DRA-mapped
                          first - NEAREST: row i; LINEAR: even r (ve0 * C[max(i-1, 0)] + ve1 * C[i] + 2) >> 2, odd r (vo0 * C[i] + vo1 * C[min(i+1, H/2-1)] + 2) >> 2
                          with the vertical quarter weights of chroma_loc (centred (1,3) / (3,1), top (0,4) / (2,2), bottom (2,2) / (4,0); its horizontal bit is
                          not read).  Every sample then takes xgpu_pic_output's depth conversion to D.  U8: out_bit_depth must be 8 (YUY2 / UYVY); U16: D =
                          out_bit_depth (0 = B, else 8..16), word = sample << (16 - D), P016's rule (D = 10 is Y210).  bgr must be 0; matrix, full_range and
                          alpha are not read; a transform is XGPU_ERR_INVALID_ARGUMENT.
   A row is 4 W es (RGBA), 4 W (RGB10A2) or 2 W es (4:2:2) bytes; row_pitch (0 = tight) is a multiple of the element (of 4 for RGB10A2) and not shorter than a row;
   the size is (H - 1) * pitch + row.  Crop, picture size and depth limits are xgpu_output_format_size's.  alpha (RGBA, RGB10A2) must be finite and in [0, 1].  An
   unsupported matrix or transform is XGPU_ERR_UNSUPPORTED, every other refusal XGPU_ERR_INVALID_ARGUMENT, all before anything is queued.  d_dst, dst_size, stream
   and the ordering are xgpu_pic_output_device's; the colour tables are xgpu_pic_output_device_cm's cache.  The exact contract: INTEGRATION.md section 8p;
   tests/packed_ref.py restates it in numpy. */
#define XGPU_PACKED_RGBA     0   /* four elements per pixel: R G B A (bgr: B G R A); dtype U8 | U16 | F16 | BF16 | F32          */
#define XGPU_PACKED_RGB10A2  1   /* one little-endian 32-bit word per pixel: R | G << 10 | B << 20 | A << 30 (bgr: B low, R at 20) */
#define XGPU_PACKED_YUYV     2   /* 4:2:2, per pair of pixels Y0 Cb Y1 Cr; U8 (YUY2) or U16 (Y210 / Y212 / Y216)                 */
#define XGPU_PACKED_UYVY     3   /* Cb Y0 Cr Y1; U8 or U16                                                                        */
typedef struct xgpu_packed_format {
    int layout, bgr, dtype, out_bit_depth;
    int matrix, full_range, chroma_loc, upsample;   /* as xgpu_output_format reads them */
    int crop[4];
    size_t row_pitch;                               /* bytes between rows; 0 = tight */
    float alpha;                                    /* RGBA, RGB10A2: in [0, 1] */
} xgpu_packed_format;
/* Host only, no context.  _size: the bytes at d_dst, 0: refused.  _check: 0 or the code the call would refuse (f, cm) with.  _coeffs (RGBA, RGB10A2; no transform):
   xgpu_output_coeffs' results for the layout - RGB10A2: D = 10, S = 17 - and alpha_code = the A element (float dtypes: the float32 bits of alpha, before the
   dtype's rounding). */
size_t xgpu_output_packed_size(const xgpu_packed_format *f, int width, int height, int bit_depth);
int    xgpu_output_packed_check(const xgpu_packed_format *f, const xgpu_colour_transform *cm, int width, int height, int bit_depth);
int    xgpu_output_packed_coeffs(const xgpu_packed_format *f, int bit_depth, int32_t coef[5], int *shift, float fcoef[5], uint32_t *alpha_code);
int    xgpu_pic_output_device_packed(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_packed_format *f,
                                     const xgpu_colour_transform *cm /* NULL: none */, void *d_dst, size_t dst_size, void *stream);
/* ---- 3D LUT output (k_output_lut3d.hip): the R'G'B' of the two RGB layouts and of the packed RGBA / RGB10A2 surfaces through a colour transform that exists
   only as a table - a .cube look, a camera log to display conversion, a vendor's HDR to SDR mapping, gamut mapping that is more than a clip.  Calls of their own:
   xgpu_pic_output_device, _cm and _packed keep their kernels and their bits.  All integers (tests/lut3d_ref.py restates it in numpy):
     input    per pixel the integer R'G'B' code c_k at the coding depth B of the U16 form (crop, DRA, chroma upsampling, matrix, range, clip to 0 .. M = 2^B - 1)
     shaper   three tables S_k[0 .. M] of uint16 positions, p_k = S_k[c_k]; the identity is S[c] = floor((2 * 65535 * c + M) / (2 M))
     cube     n nodes per axis, 2 <= n <= 65, three uint16 values per node, host order the .cube order: red fastest, node (r, g, b) at r + n * (g + n * b)
     cell     q_k = p_k * (n - 1), i_k = min(q_k / 65535, n - 2), f_k = q_k - 65535 * i_k in [0, 65535]
     tetrahedral interpolation: with the axes ordered f_a >= f_b >= f_c, V0 = node(i), V1 = V0 stepped on axis a, V2 = V1 stepped on axis b, V3 = node(i + 1);
              per output channel s = (65535 - f_a) V0 + (f_a - f_b) V1 + (f_b - f_c) V2 + f_c V3 and v = (s + 32767) / 65535 (floor; s + 32767 < 2^32)
     store    integer dtypes o = (v * (2^D - 1) + 32767) / 65535 with D = 8 for U8, D = B for U16 (out_bit_depth 0 or B), D = 16 for U16 with out_bit_depth 16
              (o = v; only xgpu_pic_output_device_lut3d takes it), D = 10 for RGB10A2; float dtypes float32(v) * float32(1 / 65535), F16 / BF16 that value rounded
              to nearest even.  bgr, alpha, row_pitch and the layouts are those of the calls without a LUT.
   With the identity shaper and the identity cube e_i = floor((2 * 65535 * i + n - 1) / (2 (n - 1))), v = p: the U16 output is xgpu_pic_output_device's U16 RGB
   bit for bit at every depth and the U8 output its U8 RGB at B = 8 - not at other depths (U8 is then a rescaled code at depth B, not the 8-bit matrix) and not
   in the float dtypes (v / 65535 is not the float matrix).
   Host-only helpers, no context, double arithmetic with + - * / and floor only, so that every host makes the same table:
     xgpu_lut3d_from_float   n^3 x 3 floats in .cube order -> uint16 nodes floor(clip(v, 0, 1) * 65535 + 0.5), NaN -> 0
     xgpu_lut3d_identity     the identity cube
     xgpu_lut3d_shaper       out[k][c] for c = 0 .. M: x = c / M, t = clip((x - in_min[k]) / (in_max[k] - in_min[k]), 0, 1) (in_min / in_max NULL: 0 / 1; in_max <=
                             in_min or not finite: XGPU_ERR_INVALID_ARGUMENT); without a curve the position is floor(t * 65535 + 0.5) - with 0 / 1 bounds the
                             identity above -, with a curve (n_curve >= 2 rows of 3 floats, column k for channel k) u = t * (n_curve - 1), j = min(floor(u),
                             n_curve - 2), y = clip(curve[j] + (u - j) * (curve[j + 1] - curve[j]), 0, 1), NaN -> 0, position floor(y * 65535 + 0.5)
   A LUT lives in a context as a handle 0 .. XGPU_MAX_LUT3D - 1: xgpu_lut3d_create uploads nodes (n^3 x 3, .cube order) and shaper (3 x 2^B, NULL: the identity)
   once and blocks until they are on the device; xgpu_lut3d_destroy waits for every queued reader first.  n outside 2 .. 65: XGPU_ERR_UNSUPPORTED; no free handle:
   XGPU_ERR_OUT_OF_MEMORY.
   The two output calls take xgpu_pic_output_device's / xgpu_pic_output_device_packed's format, destination (xgpu_output_format_size / xgpu_output_packed_size),
   stream and ordering.  Refusals, all before anything is queued, in this order: the plain call's, with its codes (U16 with out_bit_depth 16 passes);
   a layout that is not RGB (the 4:2:2 layouts): XGPU_ERR_INVALID_ARGUMENT; a handle that names no LUT: XGPU_ERR_INVALID_ARGUMENT.  xgpu_output_lut3d_check
   (host only; exactly one of f and pf is not NULL; n stands for the handle): 0 or that code, n outside 2 .. 65: XGPU_ERR_UNSUPPORTED, last. */
#define XGPU_MAX_LUT3D 8
int    xgpu_lut3d_from_float(const float *rgb, int n, uint16_t *nodes);
int    xgpu_lut3d_identity(int n, uint16_t *nodes);
int    xgpu_lut3d_shaper(int bit_depth, const float *curve /* NULL or n_curve x 3 */, int n_curve, const float in_min[3], const float in_max[3],
                         uint16_t *out /* 3 x 2^bit_depth */);
int    xgpu_output_lut3d_check(const xgpu_output_format *f, const xgpu_packed_format *pf, int n, int width, int height, int bit_depth);
int    xgpu_lut3d_create(xgpu_ctx *ctx, int n, const uint16_t *nodes, const uint16_t *shaper /* NULL: identity */, int *handle);
int    xgpu_lut3d_destroy(xgpu_ctx *ctx, int handle);
int    xgpu_pic_output_device_lut3d(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, int lut, void *d_dst, size_t dst_size,
                                    void *stream);
int    xgpu_pic_output_device_packed_lut3d(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_packed_format *f, int lut, void *d_dst,
                                           size_t dst_size, void *stream);
/* ---- dithered output (k_output_dither.hip): the integer forms of the RGB layouts, of NV12 / P016 and of the packed RGBA / RGB10A2 surfaces with an ordered
   (Bayer) or blue-noise dither in place of the final rounding, so that an 8-bit surface from a 10- or 12-bit stream keeps its gradients.  Calls of their own:
   every other call keeps its kernels and its bits.  INTEGRATION.md section 8r is the contract; tests/dither_ref.py restates it in numpy.
     matrix   mh x mw ranks, uint16, row-major; mw, mh powers of two in 1 .. 128; L = 2^k levels, 1 <= k <= 14; every rank < L (no permutation required)
     rank     of output pixel (x, y) in cropped destination coordinates: r = M[(y + phase_y) & (mh - 1)][(x + phase_x) & (mw - 1)]; all channels of a pixel
              share it; a chroma sample of NV12 / P016 uses its chroma-plane coordinates (j, i), Cb and Cr share r
     rule     clip(floor(v + r / L)), v the unrounded value in output code units:
              matrix path (RGB, RGBA, RGB10A2 without a transform)   ch = clip((sum + (r << (S - k))) >> S, 0, 2^D - 1), sum the matrix' sum before its rounding
                                                                     constant, S = 27 - D (k <= S required)
              depth conversion (NV12, P016 with D below the coding depth)   the rounding constant 1 << (shift - 1) of either rule becomes (r << shift) >> k;
                                                                     signedness and clip stay; with shift <= 0 the sample is the plain call's
              with a transform (integer dtypes)                      code = min(rd(q * outmax (+) r / L), outmax): float32 product, float32 sum, rounded down
   A 1 x 1 matrix with k = 1 and rank 1 (threshold 1/2) gives the plain calls' integers bit for bit, except with a transform, whose plain rule rounds ties to even.
   Host-only constructors, integers only:
     xgpu_dither_bayer   side n = 2^log2n (log2n 1 .. 7), L = n^2: for bit b of x and y, bit 2 (log2n - 1 - b) + 1 of the rank is bit b of x ^ y, bit
                         2 (log2n - 1 - b) is bit b of y
     xgpu_dither_blue    side n = 2^log2n (log2n 2 .. 7), L = n^2, a permutation by greedy void filling on the torus: int64 energy E = 0; tie = a permutation of
                         0 .. n^2 - 1 (Fisher-Yates from the back, j = (s >> 33) % (i + 1) with s = s * 6364136223846793005 + 1442695040888963407 mod 2^64 before
                         every draw, s0 = seed); for rank 0, 1, ...: the unfilled cell with the least E * n^2 + tie gets the rank, and an integer Gaussian (radius 6,
                         wrapping, sigma^2 = 2.25, scaled by 2^20, a table by dx^2 + dy^2) centred on it is added to E
     xgpu_dither_phase   px = ((uint32)(index * 0x9E3779B1) >> 16) & (mw - 1), py = ((uint32)(index * 0x85EBCA6B) >> 16) & (mh - 1): a phase per picture
   A matrix lives in a context as a handle 0 .. XGPU_MAX_DITHER - 1: xgpu_dither_create uploads it once and blocks until it is on the device; xgpu_dither_destroy
   waits for every queued reader first.  Sizes or k outside their ranges: XGPU_ERR_UNSUPPORTED; a rank >= L: XGPU_ERR_INVALID_ARGUMENT; no free handle:
   XGPU_ERR_OUT_OF_MEMORY.
   The two output calls take the plain calls' format, destination (xgpu_output_format_size / xgpu_output_packed_size), stream and ordering.  Refusals, all before
   anything is queued, in this order: the plain call's, with its codes; a float dtype: XGPU_ERR_UNSUPPORTED; a layout outside RGB planar / interleaved, NV12, P016,
   RGBA, RGB10A2: XGPU_ERR_INVALID_ARGUMENT; a transform with NV12 / P016: XGPU_ERR_INVALID_ARGUMENT (then the transform's own refusals, as the plain call has
   them); a handle that names no matrix: XGPU_ERR_INVALID_ARGUMENT; a phase outside the matrix: XGPU_ERR_INVALID_ARGUMENT; sizes or k outside their ranges, or
   k > S: XGPU_ERR_UNSUPPORTED.  xgpu_output_dither_check (host only; exactly one of f and pf is not NULL; mw, mh, k stand for the handle, the phase is not seen):
   0 or that code. */
#define XGPU_MAX_DITHER 4
typedef struct xgpu_dither_params { int handle, phase_x, phase_y; } xgpu_dither_params;
int    xgpu_dither_bayer(int log2n, uint16_t *rank /* n x n */);
int    xgpu_dither_blue(int log2n, uint32_t seed, uint16_t *rank /* n x n */);
int    xgpu_dither_phase(uint32_t index, int mw, int mh, int *px, int *py);
int    xgpu_output_dither_check(const xgpu_output_format *f, const xgpu_packed_format *pf, const xgpu_colour_transform *cm, int mw, int mh, int k, int width,
                                int height, int bit_depth);
int    xgpu_dither_create(xgpu_ctx *ctx, int mw, int mh, int k, const uint16_t *rank, int *handle);
int    xgpu_dither_destroy(xgpu_ctx *ctx, int handle);
int    xgpu_pic_output_device_dithered(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f,
                                       const xgpu_colour_transform *cm /* NULL: none */, const xgpu_dither_params *dp, void *d_dst, size_t dst_size, void *stream);
int    xgpu_pic_output_device_packed_dithered(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_packed_format *f,
                                              const xgpu_colour_transform *cm /* NULL: none */, const xgpu_dither_params *dp, void *d_dst, size_t dst_size,
                                              void *stream);
/* ---- overlaid output (k_output_overlay.hip): the integer forms of the RGB layouts, of NV12 / P016 and of the packed RGBA / RGB10A2 surfaces with a list of
   layers - bitmaps in device memory, boxes from the host, boxes a detector left in device memory - alpha-blended over the plain call's picture, in the output's
   own code domain, all in integers.  Calls of their own: every other call keeps its kernels and its bits.  INTEGRATION.md section 8s is the contract;
   tests/overlay_ref.py restates it in numpy.
     positions   cropped destination coordinates (the W x H image the call writes); they may be negative or beyond the image, what falls outside is clipped
     per pixel   a layer yields a colour (R, G, B in 0 .. 255) and an alpha A8:
                 RGBA8 / BGRA8   the bitmap's pixel (straight alpha)
                 A8              colour's RGB, A8 = (m * colour[3] + 127) / 255 with m the mask byte
                 BOX             a pixel of the unclipped rectangle whose distance to the nearest side (0 at the side) is below `thickness` takes `colour`,
                                 every other pixel of it `fill` (fill alpha 0: nothing)
                 effective alpha a = (A8 * opacity + 127) / 255; every division is a floor division of non-negative integers
     order       the device boxes in index order, then the host layers in list order, each onto the result of those before it
     blend       M = the element maximum (255 for U8, 2^D - 1 for U16 at depth D, 1023 for 10:10:10:2), v = the plain call's element or the previous layer's
                 result; a == 0: the element is left alone; else cD = (c8 * M + 127) / 255, out = (min(max(v, 0), M) * (255 - a) + cD * a + 127) / 255.
                 The A element of RGBA and the two alpha bits of 10:10:10:2 stay the call's constant; bgr swaps the layer's colour as it swaps the picture's;
                 no transform is applied to a layer: its colour is a code of the destination
     NV12/P016   blend in Y'CbCr on the D-bit sample, before P016's left shift.  The colour goes through the forward matrix of the format's matrix / full_range
                 (xgpu_overlay_coeffs): S = 28 - D, m[i][j] = round(k[i][j] * range_i / 255 * 2^S), range = 219 << (D - 8) (luma), 224 << (D - 8) (chroma) or
                 2^D - 1 (full range); component = offset_i + ((m[i] . (R, G, B) + 2^(S-1)) >> S) clipped to [0, M].  Luma blends as above.  Chroma sample (j, i)
                 covers luma pixels (2j .. 2j+1, 2i .. 2i+1); per layer A = the sum of the four a, C = the sum of a_k * c_k (c_k: the converted chroma of pixel
                 k), out = (min(max(v, 0), M) * (1020 - A) + C + 510) / 1020; A == 0 leaves the sample alone; Cb and Cr share A.
     device boxes (xgpu_overlay_boxes, optional): `capacity` boxes of box_format at d_boxes, the live ones the first min(max(*d_count, 0), capacity) (d_count NULL:
                 all).  Snapping (xgpu_overlay_box_snap): XYWH_I32 - skipped if w < 1 or h < 1, else [clamp(x), clamp(x + w)) and y alike, clamp to +-2^20;
                 XYXY_F32 - skipped if a coordinate is not finite, else each clamped to +-2^20, x0 = (int)floorf(x1), x1' = (int)ceilf(x2), y alike; skipped if
                 empty.  Box i is a BOX layer of opacity 255 with colour palette[((label % n) + n) % n] (label 0 without d_labels), fill the same RGB with
                 fill_alpha.  The host reads none of the arrays; the call does not synchronise.  Bitmaps and boxes are read on `stream`.
   The two output calls take the plain calls' format, destination, stream and ordering.  Refusals, all before anything is queued, in this order: the plain call's,
   with its codes; a float dtype: XGPU_ERR_UNSUPPORTED; a layout outside RGB planar / interleaved, NV12, P016, RGBA, RGB10A2: XGPU_ERR_INVALID_ARGUMENT; a
   transform with NV12 / P016: XGPU_ERR_INVALID_ARGUMENT (then the transform's own refusals; for NV12 / P016 a matrix outside the supported list:
   XGPU_ERR_UNSUPPORTED, full_range outside 0 / 1: XGPU_ERR_INVALID_ARGUMENT); then the layers: more than XGPU_MAX_OVERLAY_LAYERS, an unknown kind, a size,
   position, opacity, thickness, pitch, n_palette, capacity, box_format or fill_alpha outside its range, a bitmap or box pointer that is NULL or misaligned:
   XGPU_ERR_INVALID_ARGUMENT.  xgpu_output_overlay_check (host only; exactly one of f and pf is not NULL) returns 0 or that code and does not look at the
   pointers' memory; the calls also refuse a bitmap that is not (height - 1) * pitch + width * bpp bytes of device memory of the context's device, and box arrays
   that are not device memory of it. */
#define XGPU_MAX_OVERLAY_LAYERS 16
#define XGPU_MAX_OVERLAY_BOXES  256
#define XGPU_OVL_RGBA8 0   /* bitmap, 4 bytes per pixel R G B A, straight alpha */
#define XGPU_OVL_BGRA8 1   /* bitmap, B G R A */
#define XGPU_OVL_A8    2   /* bitmap, 1 byte per pixel: coverage of `colour` (text, glyphs, subtitle masks) */
#define XGPU_OVL_BOX   3   /* no pixels: a frame `thickness` wide in `colour`, interior in `fill` */
typedef struct xgpu_overlay_layer {
    int kind, x, y, width, height;      /* |x|, |y| <= 1 << 20; width, height 1 .. 16384 */
    int opacity;                        /* 0 .. 255, multiplies every alpha of the layer */
    const void *d_pixels; size_t pitch; /* bitmaps: device memory of the context's device; pitch 0 = tight; RGBA8 / BGRA8: pointer and pitch multiples of 4 */
    uint8_t colour[4], fill[4];         /* R G B A.  A8: colour; BOX: frame colour and interior (fill alpha 0 = none) */
    int thickness;                      /* BOX: >= 1 */
} xgpu_overlay_layer;
typedef struct xgpu_overlay_boxes {
    int box_format;                     /* XGPU_BOX_XYWH_I32 or XGPU_BOX_XYXY_F32 */
    const void *d_boxes;                /* capacity boxes of 16 bytes, aligned to 4 */
    int capacity;                       /* 1 .. XGPU_MAX_OVERLAY_BOXES */
    const int32_t *d_count;             /* or NULL: all of them */
    const int32_t *d_labels;            /* one per box, or NULL: label 0 */
    uint8_t palette[16][4]; int n_palette;      /* R G B A; 1 .. 16 */
    int thickness;                      /* >= 1 */
    int fill_alpha;                     /* 0 .. 255, 0 = no interior */
} xgpu_overlay_boxes;
int    xgpu_overlay_coeffs(const xgpu_output_format *f /* NV12 / P016 */, int bit_depth, int32_t m[9], int32_t offsets[3], int *shift);
int    xgpu_overlay_box_snap(int box_format, const void *box, int rect[4] /* x0, y0, x1, y1 */);      /* 1: live, 0: skipped, or a negative code */
int    xgpu_output_overlay_check(const xgpu_output_format *f, const xgpu_packed_format *pf, const xgpu_colour_transform *cm, const xgpu_overlay_layer *layers,
                                 int n_layers, const xgpu_overlay_boxes *boxes, int width, int height, int bit_depth);
int    xgpu_pic_output_device_overlaid(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f,
                                       const xgpu_colour_transform *cm /* NULL: none */, const xgpu_overlay_layer *layers, int n_layers,
                                       const xgpu_overlay_boxes *boxes /* NULL: none */, void *d_dst, size_t dst_size, void *stream);
int    xgpu_pic_output_device_packed_overlaid(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_packed_format *f,
                                              const xgpu_colour_transform *cm /* NULL: none */, const xgpu_overlay_layer *layers, int n_layers,
                                              const xgpu_overlay_boxes *boxes /* NULL: none */, void *d_dst, size_t dst_size, void *stream);
/* ---- regions of interest from device memory (k_output_rois_dev.hip): xgpu_pic_output_device_rois for boxes that a detector left on the GPU.  d_boxes points
   to `capacity` boxes in device memory (1 .. XGPU_MAX_ROIS), d_count (may be NULL: all of them) to a device int32 - the live boxes are the first
   min(max(*d_count, 0), capacity).  The host reads neither; the call does not synchronise and nothing comes back to the host.  Descriptors and tap tables are
   made on the device (k_rois_prepare) on `stream`, behind whatever wrote the boxes there; the two passes are section 8e's.  Image i is, bit for bit, what
   xgpu_pic_output_device_rois writes for the rectangle `used` of box i.
   The device cannot refuse a box, so every box is snapped (pw x ph: the picture minus f->crop):
     XGPU_BOX_XYWH_I32   x0 = max(x & ~1, 0), x1 = min((x + w + 1) & ~1, pw), y alike
     XGPU_BOX_XYXY_F32   a non-finite coordinate: XGPU_ROI_INVALID; else each coordinate clamped to +-2^20, x0 = max(2 * (int)floorf(x1 * 0.5f), 0),
                         x1' = min(2 * (int)ceilf(x2 * 0.5f), pw), y alike - every step exact in float32
   and gets a status - in d_results[i] (may be NULL; `used`, `inner` are zeros unless XGPU_ROI_OK; inner: what xgpu_roi_inner gives for `used`):
     XGPU_ROI_OK          the image is written
     XGPU_ROI_UNUSED      index at or above the count: no element of the image is written
     XGPU_ROI_INVALID     a non-finite coordinate
     XGPU_ROI_EMPTY       the snapped width or height is below 2
     XGPU_ROI_TOO_LARGE   the snapped rectangle exceeds `bounds` (or the LDS span the call was sized for - which bounds rule out)
     XGPU_ROI_RATIO       the inner size is outside the scaled output's limits per axis
   For INVALID, EMPTY, TOO_LARGE and RATIO the whole image is rp->pad (through the normalise), each element written once: rp->pad is validated for both fits.
   bounds: the largest snapped rectangle the call is sized for - the grids, the LDS of pass 2, a slot of tap tables and of the intermediate per box; 0 = the picture
   minus the crop.  Refusals, all before anything is queued: what xgpu_pic_output_device_rois refuses that does not depend on a rectangle; an unknown box_format,
   negative bounds or bounds beyond the picture minus the crop, capacity outside 1 .. XGPU_MAX_ROIS (XGPU_ERR_INVALID_ARGUMENT); capacity x
   sc->height * (align8(Mw) + 2 * align8(Mw / 2)) * 2 bytes of intermediate above 512 MiB, or descriptors and table slots of 4 GiB (XGPU_ERR_UNSUPPORTED). */
#define XGPU_BOX_XYWH_I32 0   /* xgpu_roi in device memory: x, y, width, height */
#define XGPU_BOX_XYXY_F32 1   /* float x1, y1, x2, y2: what detectors emit */
#define XGPU_ROI_OK        0
#define XGPU_ROI_UNUSED    1
#define XGPU_ROI_INVALID   2
#define XGPU_ROI_EMPTY     3
#define XGPU_ROI_TOO_LARGE 4
#define XGPU_ROI_RATIO     5
typedef struct xgpu_roi_bounds { int max_width, max_height; } xgpu_roi_bounds;   /* of a snapped rectangle; 0: the picture minus the crop */
typedef struct xgpu_roi_result { int status; xgpu_roi used; int inner[4]; } xgpu_roi_result;   /* 9 ints */
/* Host only, no context: 0 or the code the call refuses with / the bytes the call needs at d_dst - (capacity - 1) * image_pitch + one image; 0: refused */
int    xgpu_output_rois_dev_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi_bounds *bounds, int box_format,
                                  int capacity, int width, int height, int bit_depth);
size_t xgpu_output_rois_dev_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi_bounds *bounds, int box_format,
                                 int capacity, int width, int height, int bit_depth);
/* Host only: the device's snapping rule on one box (an xgpu_roi or four floats) for a pic_w x pic_h picture (minus the crop): XGPU_ROI_OK, _INVALID or _EMPTY,
   *used the rectangle (zeros unless XGPU_ROI_OK); XGPU_ERR_INVALID_ARGUMENT for an unknown format, a NULL or a picture size that is not positive and even */
int    xgpu_roi_snap(int box_format, const void *box, int pic_w, int pic_h, xgpu_roi *used);
/* Non-blocking.  Buffers and ordering as for xgpu_pic_output_device_rois: the context's block and intermediate (sized from bounds and capacity, grown on demand),
   a start behind the context stream's event, the context's stream waiting at the end; stream = NULL: the context's stream. */
int    xgpu_pic_output_device_rois_dev(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                                       const xgpu_roi_params *rp, const xgpu_roi_bounds *bounds, int box_format, const void *d_boxes, int capacity,
                                       const int *d_count, xgpu_roi_result *d_results, void *d_dst, size_t dst_size, void *stream);
/* ---- warped regions of interest (k_output_warp.hip): n affine maps of one picture, each giving one sc->width x sc->height image, converted and normalised like
   the scaled output, as a batch - [N, 3, H, W] or [N, H, W, 3] - from one kernel launch and at most one upload: rotated text lines, crops aligned by a similarity
   transform from landmarks, the rotated boxes of an oriented detector, augmentation by a small rotation, shear or flip.  The arithmetic is integer from the map to
   the (Y, Cb, Cr) triple; the exact contract is INTEGRATION.md section 8j and tests/warp_ref.py restates it in numpy, bit for bit.
   The source is the picture minus f->crop (even), Ws x Hs luma samples, as for the scaled output; nothing outside it reaches a result.
   A map is six Q16 integers: destination pixel (ox, oy) reads the source at X = m[0] ox + m[1] oy + m[2], Y = m[3] ox + m[4] oy + m[5], in 1 / 65536 luma sample,
   0 = the centre of luma sample 0 of the source.  Limits: |m[0]|, |m[1]|, |m[3]|, |m[4]| <= 64 << 16, |m[2]|, |m[5]| <= 1 << 36.
   samples S = 1, 2 or 4 (antialiases reductions up to about S per axis): sub-position (i, j), i, j = 0 .. S - 1, lies at
   Xij = X + ((m[0] (2i + 1 - S) + m[1] (2j + 1 - S)) >> log2(2S)) (arithmetic shift), Y alike.
   Luma at a sub-position: Xr = (Xij + 128) >> 8 clamped to [0, (Ws - 1) << 8], ix = Xr >> 8, fx = Xr & 255, ix1 = min(ix + 1, Ws - 1), rows alike;
   s = (256 - fx)(256 - fy) p00 + fx (256 - fy) p01 + (256 - fx) fy p10 + fx fy p11.  Cb, Cr alike from their half-resolution planes at
   Xc = (Xij - sh * 32768 + 256) >> 9 clamped to [0, (Ws / 2 - 1) << 8], Yc with sv and Hs / 2; sh, sv are xgpu_scale_taps' siting_half_luma of f->chroma_loc.
   Every source sample is DRA-mapped (when `dra` is given) and clipped to [0, 2^B - 1] first, as for the scaled output.
   v = (sum of the S * S sums + (1 << (15 + 2 log2 S))) >> (16 + 2 log2 S) per component; (Y, Cb, Cr) then go through the conversion of
   xgpu_pic_output_device_scaled (matrix, range, bgr, the five dtypes, the normalise of `sc`) unchanged.
     XGPU_WARP_CLAMP   the rule above: the edge of the source is replicated
     XGPU_WARP_PAD     a destination pixel whose own position (X, Y, before supersampling) has Xr < 0, Xr > (Ws - 1) << 8 or the same for Y - each before
                       its clamp - is wp->pad[k] (xgpu_roi_params' rules: floats before the normalise, integers in [0, 2^D - 1]); no blending
   pad is validated only where it is read: with XGPU_WARP_PAD, or with maps in device memory.  image_pitch as for xgpu_roi_params.  From `sc` the call reads
   width, height, normalize, mean and inv_std; sc->filter must be XGPU_SCALE_BILINEAR.
   Refusals, all before anything is queued; *bad_index (may be NULL) receives the index of the map the refusal names, else -1:
     XGPU_ERR_INVALID_ARGUMENT   n outside 1 .. XGPU_MAX_ROIS, samples not 1, 2 or 4, an unknown border, a filter other than XGPU_SCALE_BILINEAR, a layout that
                                 is not one of the four three-channel ones, a map outside the limits, a bad pad where it is read, a bad image_pitch, and
                                 whatever xgpu_pic_output_device_scaled refuses with this code
     XGPU_ERR_UNSUPPORTED        sc->width or sc->height outside 2 .. 16384 */
typedef struct xgpu_warp_map { int64_t m[6]; } xgpu_warp_map;
#define XGPU_WARP_CLAMP 0
#define XGPU_WARP_PAD   1
typedef struct xgpu_warp_params { int samples, border; float pad[3]; size_t image_pitch; } xgpu_warp_params;
/* Host only, no context: the map of theta, which takes destination pixel centres (ox + 0.5, oy + 0.5) to continuous source coordinates (sample i covers
   [i, i + 1)): m[0] = llround(theta[0] * 65536), m[1] alike, m[2] = llround(((theta[0] + theta[1]) * 0.5 + theta[2] - 0.5) * 65536), the second row alike -
   double operations in exactly this order, none contracted.  A non-finite entry or a result outside the limits: XGPU_ERR_INVALID_ARGUMENT. */
int    xgpu_warp_from_matrix(const double theta[6], xgpu_warp_map *out);
/* Host only: the image shows the w x h box centred at (cx, cy) and turned by angle_deg (y pointing down).  With c, s the cosine and sine of
   angle_deg * (pi / 180): theta = { w c / dst_w, -h s / dst_h, cx - (w c - h s) / 2, w s / dst_w, h c / dst_h, cy - (w s + h c) / 2 }, then xgpu_warp_from_matrix. */
int    xgpu_warp_from_rotated_box(double cx, double cy, double w, double h, double angle_deg, int dst_w, int dst_h, xgpu_warp_map *out);
/* Host only, no context: 0 or the code the call refuses with (maps = NULL: maps in device memory, which the host does not read) / the bytes the call needs at
   d_dst - (n - 1) * image_pitch + one image; 0: refused - for a picture of width x height at bit_depth */
int    xgpu_output_warp_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_warp_params *wp, const xgpu_warp_map *maps, int n,
                              int width, int height, int bit_depth, int *bad_index);
size_t xgpu_output_warp_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_warp_params *wp, int n, int width, int height, int bit_depth);
/* Non-blocking; d_dst, dst_size, stream and the ordering as for xgpu_pic_output_device_rois.  maps_on_device = 0: `maps` is host memory, validated here and
   uploaded in one copy into the context's block (which grows on demand and is ordered like the descriptor block of the regions of interest); d_status is not
   written.  maps_on_device = 1: `maps` is an int64 [n][6] array on the context's device; the host does not read it and the call does not synchronise.  The kernel
   checks the limits per map: a map outside them gives an image that is all wp->pad, and d_status[i] (int32 [n] on the device, may be NULL) is 1 - else 0, the
   image is written.  Whatever a map holds, every position is clamped before it addresses memory, and the position arithmetic wraps in 64 bits. */
int    xgpu_pic_output_device_warp(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                                   const xgpu_warp_params *wp, const xgpu_warp_map *maps, int maps_on_device, int n, int32_t *d_status, void *d_dst,
                                   size_t dst_size, void *stream);
/* ---- remapped output (k_output_remap.hip): n coordinate grids of one picture, each giving one sc->width x sc->height image whose every pixel reads the source at
   a position of its own - lens undistortion, fisheye dewarping into virtual views, perspective maps, the previous picture pulled through a flow field - converted
   and normalised like the scaled output, as a batch from one kernel launch.  The general case of the warp above, whose gather, conversion, normalise, layouts,
   dtypes and ordering rules it shares; the exact contract is INTEGRATION.md section 8k and tests/remap_ref.py restates it in numpy, bit for bit.
   Geometry and grid
     The source is the picture minus f->crop (even), Ws x Hs luma samples, as for the warp.  Nothing outside it reaches a result.
     A position is Q16 in 1 / 65536 luma sample.  0 is the centre of luma sample 0 of the source (the warp's convention, and OpenCV's for maps).
     The destination is sc->width x sc->height = dw x dh, each in 2 .. 16384 (outside: XGPU_ERR_UNSUPPORTED), and there are n images, 1 .. XGPU_MAX_ROIS.
     The grid has step_log2 = k in 0 .. 6.  Node (j, i) belongs to destination pixel (i << k, j << k).  gw = ((dw - 1) >> k) + 1 + (k > 0), and gh alike.  Rows are
     tight.  A node is the pair (x, y) in 8 bytes.  Grid g starts grid_pitch * g bytes behind d_grid; grid_pitch 0 means tight, else a multiple of 8 not shorter
     than one grid.  The grid always lives in device memory: a map is made once and used for every picture, the host never reads it and the call does not
     synchronise.  The caller states grid_size in bytes; it is checked on the host against (n - 1) * pitch + gh * gw * 8.
   Grid formats
     XGPU_GRID_Q16_I32   int32 x, y.  A node with INT32_MIN in either coordinate is invalid.  Every other bit pattern is a valid position.
     XGPU_GRID_F32       float x, y in luma samples.  A non-finite coordinate makes the node invalid.  Otherwise c = min(max(v, -32767.0f), 32767.0f) and
                         q = (int32)rintf(c * 65536.0f).  Every step is exact in float32, so numpy's np.rint on float32 restates it.
   Position of pixel (ox, oy), in int64, arithmetic shifts
     k = 0: P = node (oy, ox).
     k > 0: i = ox >> k, fx = ox & (2^k - 1), j and fy alike, M = 2^k.  The four nodes are P00 = (j, i), P01 = (j, i + 1), P10 = (j + 1, i), P11 = (j + 1, i + 1).
            X = ((M - fx)(M - fy) X00 + fx (M - fy) X01 + (M - fx) fy X10 + fx fy X11 + 2^(2k - 1)) >> 2k, and Y alike.
   Derivatives, read only when samples S > 1
     k > 0: D0x = ((M - fy)(X01 - X00) + fy (X11 - X10) + 2^(2k - 1)) >> 2k.
            D1x = ((M - fx)(X10 - X00) + fx (X11 - X01) + 2^(2k - 1)) >> 2k.  D0y and D1y alike.
     k = 0: D0 = P(oy, xa + 1) - P(oy, xa) with xa = min(ox, dw - 2).
            D1 = P(ya + 1, ox) - P(ya, ox) with ya = min(oy, dh - 2).
   Sub-positions and sampling, S = 1, 2 or 4
     Xij = X + ((D0x (2i + 1 - S) + D1x (2j + 1 - S)) >> log2(2S)), and Y alike.
     From Xij on, everything is the warp's, word for word: the luma and chroma bilinear sums with Q8 fractions, the chroma offset by f->chroma_loc, DRA and the
     clip on every source sample, the rounding shift over S x S, then the conversion and normalise of xgpu_pic_output_device_scaled.
     sc->filter must be XGPU_SCALE_BILINEAR, as for the warp.
   Border and invalid pixels
     XGPU_WARP_CLAMP and XGPU_WARP_PAD are reused, with the warp's rule applied to the pixel's own (X, Y).
     A pixel for which any node that its formulas read is invalid is `pad` in both border modes.  For S = 1 that is the one node or the four of its cell.  For
     S > 1 and k = 0 it also covers the derivative nodes.
     pad is validated with XGPU_WARP_PAD's rules, and always, for either grid format, since both can carry invalid nodes.
     Every position is clamped before it becomes an index, whatever the grid holds.  No node index beyond gw - 1 or gh - 1 is ever formed.
   An affine grid (xgpu_remap_from_warp of a map whose nodes stay inside +-32767 samples) reproduces xgpu_pic_output_device_warp bit for bit at every k and S: the
   interpolation of an affine function is exact, and the derivatives are the map's linear part.
   Refusals, all before anything is queued:
     XGPU_ERR_INVALID_ARGUMENT   n outside 1 .. XGPU_MAX_ROIS, step_log2 outside 0 .. 6, an unknown grid_format or border, samples not 1, 2 or 4, a filter other
                                 than XGPU_SCALE_BILINEAR, a layout that is not one of the four three-channel ones, a bad pad, a bad image_pitch or grid_pitch,
                                 grid_size or dst_size too short, a grid or destination that is not device memory or not aligned (grid: 8 bytes), and whatever
                                 xgpu_pic_output_device_scaled refuses with this code
     XGPU_ERR_UNSUPPORTED        sc->width or sc->height outside 2 .. 16384 */
#define XGPU_GRID_Q16_I32 0
#define XGPU_GRID_F32     1
typedef struct xgpu_remap_params { int grid_format, step_log2, samples, border; float pad[3]; size_t grid_pitch, image_pitch; } xgpu_remap_params;
/* Brown-Conrady lens with OpenCV's pixel convention: the camera that took the picture (fx, fy, cx, cy and the five coefficients) and the new, undistorted camera
   whose image is wanted (nfx, nfy, ncx, ncy) */
typedef struct xgpu_remap_lens { double fx, fy, cx, cy, k1, k2, p1, p2, k3, nfx, nfy, ncx, ncy; } xgpu_remap_lens;
/* Host only, no context.  The nodes per row and the rows of a grid for a dst_w x dst_h image (dst_w, dst_h >= 1; gw, gh may be NULL) / the bytes the call reads
   at d_grid, (n - 1) * pitch + gh * gw * 8, 0: refused (from `sc` width and height, from `rp` step_log2 and grid_pitch) */
int    xgpu_remap_grid_dims(int dst_w, int dst_h, int step_log2, int *gw, int *gh);
size_t xgpu_remap_grid_size(const xgpu_scale_params *sc, const xgpu_remap_params *rp, int n);
/* Host only, no context: 0 or the code the call refuses with (everything but the sizes and the memory of d_grid and d_dst) / the bytes the call needs at d_dst -
   (n - 1) * image_pitch + one image; 0: refused - for a picture of width x height at bit_depth */
int    xgpu_output_remap_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_remap_params *rp, int n, int width, int height, int bit_depth);
size_t xgpu_output_remap_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_remap_params *rp, int n, int width, int height, int bit_depth);
/* Host only: write one XGPU_GRID_Q16_I32 grid of gh * gw nodes (xgpu_remap_grid_dims; dst_w, dst_h >= 2) into host memory, which the caller uploads once.
   Node (j, i) is evaluated at ox = i << k, oy = j << k.  A value v in luma samples becomes t = v * 65536.0, then llround(min(max(t, -2147483647.0),
   2147483647.0)); a non-finite t makes the node invalid (INT32_MIN, INT32_MIN).  Double operations in exactly the order written, none contracted.
     from_warp        x = m[0] ox + m[1] oy + m[2], y = m[3] ox + m[4] oy + m[5] in int64 (exact: the map must be inside the warp's limits), clamped to
                      [-INT32_MAX, INT32_MAX]
     from_homography  u = ox + 0.5, v = oy + 0.5, den = (h[6] * u + h[7] * v) + h[8], x = ((h[0] * u + h[1] * v) + h[2]) / den - 0.5,
                      y = ((h[3] * u + h[4] * v) + h[5]) / den - 0.5; den <= 0 (or NaN) makes the node invalid
     from_lens        x = (ox - ncx) / nfx, y = (oy - ncy) / nfy, r2 = x * x + y * y, rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3)),
                      xd = (x * rad + ((2 * p1) * x) * y) + p2 * (r2 + (2 * x) * x), yd = (y * rad + p1 * (r2 + (2 * y) * y)) + ((2 * p2) * x) * y,
                      X = fx * xd + cx, Y = fy * yd + cy
   XGPU_ERR_INVALID_ARGUMENT: a NULL, a size below 2, step_log2 outside 0 .. 6, a map outside the warp's limits. */
int    xgpu_remap_from_warp(const xgpu_warp_map *map, int dst_w, int dst_h, int step_log2, int32_t *grid);
int    xgpu_remap_from_homography(const double h[9], int dst_w, int dst_h, int step_log2, int32_t *grid);
int    xgpu_remap_from_lens(const xgpu_remap_lens *lens, int dst_w, int dst_h, int step_log2, int32_t *grid);
/* Non-blocking; d_dst, dst_size, stream and the ordering as for xgpu_pic_output_device_warp.  d_grid: grid_size bytes of grids on the context's device, written
   before the call on `stream` (or complete); the host does not read them and the call does not synchronise or upload anything. */
int    xgpu_pic_output_device_remap(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                                    const xgpu_remap_params *rp, const void *d_grid, size_t grid_size, int n, void *d_dst, size_t dst_size, void *stream);
/* ---- scaled video surfaces (k_output_ladder.hip): n renditions ("rungs", 1 .. XGPU_MAX_RUNGS) of one decoded picture as 4:2:0 video surfaces, each at its own
   even width x height in its own destination, all in one layout - XGPU_OUT_YUV420P, XGPU_OUT_NV12 or XGPU_OUT_P016 (any other: XGPU_ERR_INVALID_ARGUMENT): the
   2160p / 1080p / 720p / 360p ladder of an adaptive-bitrate transcode from one call - two kernel launches and one upload, however many rungs.
   The source is the active picture minus f->crop (even), Ws x Hs luma samples, DRA-mapped (when `dra` is given) and clipped to [0, 2^B - 1], as for the scaled
   output.  Luma of a rung is the scaled output's luma unchanged: rows xgpu_scale_taps(Hs, 1, 0, Hd), columns xgpu_scale_taps(Ws, 1, 0, Wd), vertical first,
   t = (sum qy * sample + 2^10) >> 11, then v = (sum qx * t + 2^16) >> 17.  A chroma plane of Wd / 2 x Hd / 2 is filtered straight from the Ws / 2 x Hs / 2 plane by
   the same two passes with the tables of xgpu_scale_taps_ex(Hs / 2, 2, dy, Hd / 2, 2, Dy) and (Ws / 2, 2, dx, Wd / 2, 2, Dx): (dx, dy) the siting of f->chroma_loc,
   (Dx, Dy) that of lp->dst_chroma_loc (-1: f->chroma_loc) on the rung's own grid, in half luma samples.  No pass goes through luma resolution.  Every rung is
   filtered from the source, so rung i of a call is what a call with that rung alone writes.  The filtered sample (coding depth B) then goes through the depth rule
   of xgpu_pic_output to D = f->out_bit_depth (0: B) and is packed as xgpu_pic_output_device packs the layout: YUV420P tight (row_pitch 0; U8 at D = 8, else U16),
   NV12 U8 / U16 with the value in the low bits, P016 the word shifted left by 16 - D; the dtype / out_bit_depth pairs accepted are those of xgpu_pic_output_device.
   matrix, full_range, upsample and f->row_pitch are not read; bgr must be 0.  With a rung the size of the source and the destination siting the source's, the rung
   is xgpu_pic_output_device's surface bit for bit (dra NULL, or tables that map inside [0, 2^B - 1]).
   lp->filter: XGPU_SCALE_BILINEAR or XGPU_SCALE_AREA.  A rung: width, height, row_pitch (bytes between rows, 0: tight; a multiple of the element size and at least
   a row), d_dst / dst_size (device memory of the context's device, element-aligned, at least xgpu_output_ladder_rung_size bytes).
     XGPU_ERR_INVALID_ARGUMENT   n outside 1 .. XGPU_MAX_RUNGS, an odd rung size, an odd crop, an unknown filter, dst_chroma_loc outside -1 .. 5, a layout outside the
                                 three, a dtype / out_bit_depth pair xgpu_pic_output_device refuses, a pitch with YUV420P or shorter than a row, a NULL, misaligned,
                                 undersized or host destination, two rungs whose byte ranges overlap
     XGPU_ERR_UNSUPPORTED        a rung outside 2 .. 16384 or outside Ws / 64 <= Wd <= 8 Ws per axis; intermediates of all rungs above 512 MiB together
   Every refusal comes before anything is queued.  The exact contract: INTEGRATION.md section 8l; tests/ladder_ref.py restates it in numpy. */
#define XGPU_MAX_RUNGS 8
typedef struct xgpu_surface_rung { int width, height; size_t row_pitch; void *d_dst; size_t dst_size; } xgpu_surface_rung;
typedef struct xgpu_ladder_params { int filter; int dst_chroma_loc; } xgpu_ladder_params;
/* Host only, no context: xgpu_scale_taps for a destination with a subsampling (1, 2) and a siting (0, 1, 2 half luma samples of the destination grid) of its
   own.  Per axis, n plane samples of subsampling s and siting d onto N samples of subsampling S and siting D: r = n s / (N S), f = max(1, r S / s),
   c(o) = ((S o + D + 1/2) r - 1/2 - d) / s; everything behind c and f is xgpu_scale_taps'.  The limits count luma samples: N S >= 2, N <= 16384,
   n s / 64 <= N S <= 8 n s.  dst_subsampling 1 and dst_siting_half_luma 0 give xgpu_scale_taps row for row.  Integer arithmetic only. */
int    xgpu_scale_taps_ex(int n_plane, int subsampling, int siting_half_luma, int n_dst, int dst_subsampling, int dst_siting_half_luma, int filter,
                          int32_t *first, int32_t *count, int16_t *w, int w_stride);
/* Host only, no context: the bytes a rung of rung_width x rung_height needs at its d_dst - xgpu_output_format_size of the layout at that size with that pitch and
   no crop; 0: refused.  xgpu_output_ladder_check: 0, or the code xgpu_pic_output_device_ladder refuses with for a picture of width x height (uncropped) at coding
   depth bit_depth; it reads dst_size and does not look at d_dst. */
size_t xgpu_output_ladder_rung_size(const xgpu_output_format *f, int rung_width, int rung_height, size_t row_pitch, int bit_depth);
int    xgpu_output_ladder_check(const xgpu_output_format *f, const xgpu_ladder_params *lp, const xgpu_surface_rung *rungs, int n, int width, int height,
                                int bit_depth);
/* Non-blocking; stream as xgpu_pic_output_device takes it.  The records and the tap tables of all rungs lie in one block of the context, uploaded once per call: the
   tables are made again only when the source size, the rung sizes, the filter or either siting differ from the previous call's (else the upload is the records
   alone); the intermediate is the scaled output's and grows on demand (growing it waits for the device).  Ordered like the scaled output: calls on different streams
   follow one another through the context's stream. */
int    xgpu_pic_output_device_ladder(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_ladder_params *lp,
                                     const xgpu_surface_rung *rungs, int n, void *stream);
/* ---- coding side information (k_side_info.hip): what the decoder knows about a picture besides its samples - motion vectors per 4x4 luma unit, the
   reference each one points at, intra / inter / skip / IBC, QP, coded-residual flag, block edges - read out of the SCU map the in-loop filters read
   (the reference's map_scu / map_refi / map_mv, src_base/xevd_def.h:372-438).
   The map is per CONTEXT, not per picture: the next picture's reconstruction overwrites it.  So the information belongs to THE PICTURE DECODED LAST and is
   taken at decoding time: `pic` must be the slot of the picture whose xgpu_frame_end came last (and returned XGPU_OK), with no xgpu_frame_begin since -
   another slot, no picture yet, or a frame open: XGPU_ERR_INVALID_ARGUMENT, nothing queued.
     XGPU_SIDE_BLOCKS   nine int16 planes of h_scu x w_scu (height / 4, width / 4), plane p at p * h_scu * row_pitch; unit (j, i) covers luma samples
                        [4i, 4i + 4) x [4j, 4j + 4) of the UNCROPPED picture (crop must be 0); dtype XGPU_OUT_U16 (the element size; the values are signed):
                          0, 1  list 0 vector x, y as the map holds it: quarter luma samples, unclipped       2, 3  list 1 vector x, y
                          4, 5  refp_poc[refi][list] - poc of the frame parameters, saturated to int16; 0 where refi < 0 (a reference never has the
                                picture's own POC: 0 is unambiguous)
                          6     XGPU_MODE_INTRA 0, _INTER 1, _SKIP 2, _IBC 6 (the map cannot tell direct mode from inter: 1)
                          7     the QP the deblocking filter reads (bits 16-22 of map_scu: qp_y - 6 * (bit_depth - 8))
                          8     bit 0 luma cbf (map_scu bit 24), bit 1 / 2 the unit's left / top edge is a CU border or a 64-sample transform border inside a
                                wider CU, bit 3 ats_inter != 0
                        Intra units: vectors 0, POC planes 0.  IBC units: the block vector in planes 0 / 1 as the batch gave it - in WHOLE luma
                        samples, not quarter samples (xgpu_cu_batch.mv of an XGPU_MODE_IBC CU) -, POC planes 0.  Affine CUs: one vector per sub-block (xevdm_set_affine_mvf).  DMVR-refined CUs: the vectors the
                        sequence's deblocking filter reads - UNREFINED with tool_addb, refined with the baseline filter of the Main library.
     XGPU_SIDE_FLOW_PLANAR / _INTERLEAVED   a dense motion field at luma resolution: 2 channels (x, y) per requested list (lists 1: list 0, 2: list 1, 3: both -
                        list 0 first), [C, H, W] planar (plane k at k * H * row_pitch) or [H, W, C], H x W cropped; pixel (y, x) takes the unit
                        ((y + crop_top) >> 2, (x + crop_left) >> 2).  Value in float32, every operation rounded on its own: v = float32(mv) * 0.25f (luma
                        samples); with per_poc v = v / float32(dpoc), one IEEE division, dpoc the unsaturated POC difference of planes 4 / 5; a list the unit
                        does not use (intra and IBC units included) gives +0.0.  XGPU_OUT_F16: that value rounded to nearest even.  The sign is the codec's: the
                        reference block lies at position + v.
   The exact contract: INTEGRATION.md section 8c; tests/side_info_ref.py restates it in numpy. */
#define XGPU_SIDE_BLOCKS           0
#define XGPU_SIDE_FLOW_PLANAR      1
#define XGPU_SIDE_FLOW_INTERLEAVED 2
typedef struct xgpu_side_format {
    int layout;        /* XGPU_SIDE_BLOCKS | XGPU_SIDE_FLOW_PLANAR | XGPU_SIDE_FLOW_INTERLEAVED */
    int dtype;         /* BLOCKS: XGPU_OUT_U16 (the planes are int16); FLOW: XGPU_OUT_F16 | _F32 */
    int lists;         /* FLOW: 1 = list 0, 2 = list 1, 3 = both (BLOCKS: not read) */
    int per_poc;       /* FLOW: 0 | 1 (BLOCKS: not read) */
    int crop[4];       /* FLOW: left, right, top, bottom luma samples, even; BLOCKS: all 0 */
    size_t row_pitch;  /* bytes between rows, a multiple of the element size; 0 = tight */
} xgpu_side_format;
/* Host only, no context: the bytes format `f` needs at d_dst for a picture of width x height (the uncropped size, multiples of 8), the last row tight; 0:
   invalid format or size.  BLOCKS: (9 h_scu - 1) * pitch + 2 w_scu; FLOW planar: (C H - 1) * pitch + W * es, interleaved: (H - 1) * pitch + C W * es. */
size_t xgpu_side_info_size(const xgpu_side_format *f, int width, int height);
/* Non-blocking.  d_dst and stream as xgpu_pic_output_device takes them: device memory of the context's device, aligned to the element size, >=
   xgpu_side_info_size bytes (checked before anything is queued); stream = NULL: the context's stream; else the kernel runs on `stream` behind the picture's
   kernels, and the context's stream waits for it before the next picture may write the map.  Reads the map only: the picture is not touched. */
int    xgpu_frame_side_info(xgpu_ctx *ctx, int pic, const xgpu_side_format *f, void *d_dst, size_t dst_size, void *stream);
/* ---- the prediction residual (k_residual.hip): the third product of a decoder, next to the samples and the side information.  The residual pass of a batch
   (dequantisation + inverse transform) leaves its output in the batch's arena on the device, where the reconstruction kernels add it to the prediction; this
   call writes it out as dense, picture-shaped planes.  r(c, x, y) is the s16 the arena holds for component c at picture position (x, y) - exactly what is
   added before the clip - and 0 where nothing is coded: the CU's cbf bit of c is clear; the position lies outside the TU of an ATS-inter CU; it lies in a
   64x64 sub-block of a CU above 64 whose cbf_sub bit is clear; no CU of the batch covers it (another tile's or slice's units).  Inside a local dual tree luma
   comes from the luma-only CUs and chroma from the chroma-only CU that closes the tree.  Every element of the destination is written (zeros included): the
   caller does not clear it.  Values are signed; dtype XGPU_OUT_U16 names the element size, as for XGPU_SIDE_BLOCKS.
     XGPU_RESID_YUV420            int16 (XGPU_OUT_U16 only): Y h rows of w, then Cb and Cr h / 2 rows of w / 2 each - the plane order and tight layout of
                                  xgpu_pic_output; row_pitch is the LUMA pitch (a multiple of 4), the chroma pitch is half of it, Cb starts at h * row_pitch,
                                  Cr at h * row_pitch + (h / 2) * (row_pitch / 2)
     XGPU_RESID_444_PLANAR        [3, h, w], plane k at k * h * row_pitch; _INTERLEAVED: [h, w, 3].  Chroma is replicated, c[(y + crop_top) >> 1][(x + crop_left) >> 1]
                                  - no interpolation: a residual is not an image.  XGPU_OUT_U16: the s16; XGPU_OUT_F32: float32(r) * 2^-B with B the component's
                                  bit depth (a power of two: every value is exact); XGPU_OUT_F16: that value rounded to nearest even (|r| * 2^-8 <= 128 fits)
     XGPU_RESID_ENERGY            [3, h_scu, w_scu] float32 (XGPU_OUT_F32 only), crop must be 0: per 4x4 luma unit - the grid of XGPU_SIDE_BLOCKS - plane 0 the
                                  sum of |r| over its 16 luma samples, planes 1 / 2 over its 2x2 Cb / Cr samples (integers <= 2^19: exact)
   w x h: the picture minus crop (left, right, top, bottom luma samples, even).  The exact contract: INTEGRATION.md section 8g; tests/residual_ref.py restates it
   in numpy. */
#define XGPU_RESID_YUV420            0
#define XGPU_RESID_444_PLANAR        1
#define XGPU_RESID_444_INTERLEAVED   2
#define XGPU_RESID_ENERGY            3
typedef struct xgpu_resid_format {
    int layout;        /* XGPU_RESID_* */
    int dtype;         /* YUV420: XGPU_OUT_U16; 444: XGPU_OUT_U16 | _F16 | _F32; ENERGY: XGPU_OUT_F32 */
    int crop[4];       /* left, right, top, bottom luma samples, even; ENERGY: all 0 */
    size_t row_pitch;  /* bytes between rows, a multiple of the element size (YUV420: of 4); 0 = tight */
} xgpu_resid_format;
/* Host only, no context: the bytes format `f` needs at d_dst for a picture of width x height (the uncropped size, multiples of 8), the last row tight; 0:
   invalid format or size.  YUV420: h * pitch + (h - 1) * (pitch / 2) + w; 444 planar: (3 h - 1) * pitch + w * es, interleaved: (h - 1) * pitch + 3 w * es;
   ENERGY: (3 h_scu - 1) * pitch + 4 w_scu. */
size_t xgpu_resid_size(const xgpu_resid_format *f, int width, int height);
/* Non-blocking.  Valid from the moment the batch's residual pass is queued - xgpu_batch_recon(_ahead) of db, xgpu_batch_prepare(db), or db passed as `next`
   of xgpu_batch_recon_ahead - until xgpu_batch_destroy(db); before that: XGPU_ERR_INVALID_ARGUMENT, nothing queued.  d_dst and stream as
   xgpu_frame_side_info takes them: device memory of the context's device, aligned to the element size, >= xgpu_resid_size bytes (checked before anything is
   queued); a destination, pitch and plane distance that are multiples of 16 bytes take vector stores.  stream = NULL: the context's stream; else the kernel
   runs on `stream` behind the residual pass, and the context's stream waits for it, so the batch may be destroyed right after the call.  Reads the batch
   only: neither the picture nor the SCU map is touched. */
int    xgpu_batch_residual(xgpu_ctx *ctx, xgpu_dbatch *db, const xgpu_resid_format *f, void *d_dst, size_t dst_size, void *stream);
/* ---- comparing pictures (k_compare.hip): a picture of the context against another one - a slot, or 4:2:0 planes in device memory - in one pass over both:
   per component the number of samples, the sum of squared differences, how many samples differ, the largest difference and where the first one is; an exact
   integer SSIM; optionally the SSE of every 16x16 luma block (8x8 chroma block).  Everything is defined in integers - the SSIM in individually rounded
   binary64 operations whose result is quantised and summed as an integer -, so the result does not depend on the device, the launch or the scheduling.
     Samples     both pictures are read as unsigned 16-bit patterns as they lie in memory (U8: zero-extended); nothing is clipped or masked, and every integer
                 below is exact for ANY 16-bit contents.  The coding depth B enters only through the SSIM constants.
     Census      over the w x h plane of each component (the picture minus crop; chroma: half of it): n = w * h, sse = sum (a - r)^2, n_diff = samples with
                 a != r, max_abs = max |a - r|, first_diff = (y << 32) | x of the first differing sample in raster order of the cropped plane, ~0: none.
     SSIM        the 8x8-window, stride-4 integer form of x264 / ffmpeg: windows at (4i, 4j), i < (w >> 2) - 1, j < (h >> 2) - 1 (none for w < 8 or h < 8;
                 trailing w % 4 columns and h % 4 rows lie in no window).  Per window, in integers: s1 = sum a, s2 = sum r, ss = sum (a^2 + r^2), s12 = sum a r,
                 vars = 64 ss - s1^2 - s2^2, cov = 64 s12 - s1 s2; with L = 2^B - 1: c1 = (64 L^2 + 5000) / 10000, c2 = (9 * 64 * 63 L^2 + 5000) / 10000
                 (integer division; B = 8: 416 and 235963).  In binary64, every operation rounded once, no fused multiply-add:
                     num = double(2 s1 s2 + c1) * double(2 cov + c2),  den = double(s1^2 + s2^2 + c1) * double(vars + c2),
                     q = (int64) floor(num / den * 2^30 + 0.5)
                 (the four integers stay below 2^53: the conversions are exact).  ssim_q30 = sum of q over the windows, ssim_windows their number: identical
                 pictures give exactly ssim_windows << 30.  ssim = 0: both fields are written as 0.
     Block map   [3][ceil(h / 16)][ceil(w / 16)] uint64, tight: plane 0 the SSE of the 16x16 luma blocks of the cropped plane, planes 1 and 2 of the co-located
                 8x8 Cb and Cr blocks, clipped at the plane's edge; every element is written, and those of plane c sum to sse[c].
   Not offered: DRA (the slot's samples are compared as they are), a reference at another depth or chroma format, a reference in host memory.
   The exact contract: INTEGRATION.md section 8h; tests/metrics_ref.py restates it in numpy. */
#define XGPU_CMP_REF_PIC     0   /* another picture slot of the same context */
#define XGPU_CMP_REF_YUV420  1   /* device memory in xgpu_pic_output's plane order: Y h rows of w, then Cb, Cr h/2 rows of w/2 */
typedef struct xgpu_compare_ref {
    int kind;            /* XGPU_CMP_REF_* */
    int pic;             /* REF_PIC: the slot (may equal the picture compared) */
    const void *d_yuv;   /* REF_YUV420: first luma sample of the UNCROPPED reference picture */
    size_t size;         /* REF_YUV420: bytes available at d_yuv */
    int dtype;           /* REF_YUV420: XGPU_OUT_U8 (only when the coding depth is 8) | XGPU_OUT_U16 */
    size_t row_pitch;    /* REF_YUV420: LUMA pitch in bytes, 0 = tight, a multiple of 2 elements; chroma pitch = half of it;
                            Cb at h * pitch, Cr at h * pitch + (h / 2) * (pitch / 2)  (xgpu_resid_format's YUV420 rule) */
} xgpu_compare_ref;
typedef struct xgpu_compare_params {
    int crop[4];         /* left, right, top, bottom luma samples, even: applied to BOTH pictures */
    int ssim;            /* 0 | 1 */
    int block_map;       /* 0 | 1: also write the per-block SSE map */
} xgpu_compare_params;
typedef struct xgpu_compare_result {      /* written by the device; 160 bytes, every field at a multiple of its size */
    uint64_t n[3];           /* samples compared, per component Y, Cb, Cr */
    uint64_t sse[3];         /* sum of (a - r)^2 */
    uint64_t n_diff[3];      /* samples with a != r */
    uint64_t first_diff[3];  /* (y << 32) | x of the first differing sample in raster order of the cropped plane; ~0 if none */
    uint32_t max_abs[3];     /* max |a - r| */
    uint32_t reserved;       /* written as 0 */
    uint64_t ssim_windows[3];
    int64_t  ssim_q30[3];    /* sum over the windows of floor(ssim * 2^30 + 0.5) */
} xgpu_compare_result;
/* Host only, no context.  xgpu_compare_ref_size: the bytes a REF_YUV420 reference of width x height (the uncropped size, positive and even) spans from d_yuv,
   the last row tight - h * pitch + (h - 1) * (pitch / 2) + (w / 2) * es; 0: an invalid reference (dtype, a pitch shorter than a row or not a multiple of 2
   elements) or XGPU_CMP_REF_PIC, which has no memory to size.  xgpu_compare_map_size: 3 * ceil(h / 16) * ceil(w / 16) * 8 bytes for the cropped w x h; 0: invalid
   parameters, or block_map == 0.  xgpu_compare_check: everything xgpu_pic_compare refuses without looking at a context or a pointer's memory - 0, or
   XGPU_ERR_INVALID_ARGUMENT for a NULL, a size that is not positive and even, a depth outside 8..12, an unknown kind, a negative slot, a NULL d_yuv, U8 with
   bit_depth != 8, a bad pitch, size < xgpu_compare_ref_size, an odd or negative crop or one that leaves nothing, ssim or block_map outside 0 | 1. */
size_t xgpu_compare_ref_size(const xgpu_compare_ref *r, int width, int height);
size_t xgpu_compare_map_size(const xgpu_compare_params *p, int width, int height);
int    xgpu_compare_check(const xgpu_compare_ref *r, const xgpu_compare_params *p, int width, int height, int bit_depth);
/* Non-blocking.  Compares slot `pic` with `ref` and writes *d_result and - with block_map - the map at d_map (map_size >= xgpu_compare_map_size bytes; else
   d_map is not read).  d_result, d_map and a REF_YUV420 reference must be device memory of the context's device, large enough, d_result and d_map 8-byte
   aligned, the reference aligned to its element (checked before anything is queued); a reference whose base and pitch are multiples of 16 bytes (U8: 8) is
   read with vector loads.  Every field of the result and every map element is written by the call, on the same stream - the result by the
   one workgroup that adds up the others' partial sums, a map element by the workgroup that owns its block: the caller clears nothing.  Both pictures are only read.  stream = NULL: the context's stream; else the kernels run on `stream` behind the
   picture's kernels, and the context's stream waits for them.  A refused call - what xgpu_compare_check refuses, a slot that holds no picture, a frame that
   is open (between xgpu_frame_begin and xgpu_frame_end), a pointer that fails the checks above - queues nothing, returns XGPU_ERR_INVALID_ARGUMENT and
   leaves a message in xgpu_last_error. */
int    xgpu_pic_compare(xgpu_ctx *ctx, int pic, const xgpu_compare_ref *ref, const xgpu_compare_params *p,
                        xgpu_compare_result *d_result, uint64_t *d_map, size_t map_size, void *stream);
/* ---- picture statistics (k_stats.hip): what is in ONE picture, from one pass over the slot - per component the census (n, sum, sum of squares, minimum,
   maximum), a histogram and two percentiles of it; optionally the histogram of max(R', G', B') at luma resolution and the light level it implies (what HDR10
   metadata calls MaxCLL and MaxFALL).  Everything is defined in integers but light_sum / light_mean, which are binary64 in a fixed order of individually
   rounded operations: the result does not depend on the device, the launch or the scheduling.  B is the coding depth.
     Samples     read as unsigned 16-bit patterns as they lie in the slot, as for xgpu_pic_compare; nothing is clipped or masked, and the census is exact for ANY
                 16-bit contents.
     Census      over the w x h plane of each component (the picture minus crop; chroma: half of it): n = w * h, sum = sum s, sum_sq = sum s^2, min, max.
     Histogram   hist_bits != 0: [3][2^hist_bits] uint32, bin = min(s >> (B - hist_bits), 2^hist_bits - 1) (a pattern above 2^B - 1 counts in the last bin); every
                 bin is written, and the bins of a component sum to n.
     Percentile  pctl[c][i] = b << (B - hist_bits) for the smallest bin b with cum(b) * 10000 >= max(pctl_e4[i] * n, 1), cum(b) = the samples in bins 0 .. b,
                 compared in 64-bit integers: the lower edge of that bin.  pctl_e4 = 0 gives the lowest occupied bin, 10000 the highest.  hist_bits = 0: 0.
     Light       light != 0, per luma sample of the cropped picture: m = the largest of the three U16 elements xgpu_pic_output_device writes for
                 XGPU_OUT_RGB_PLANAR, XGPU_OUT_U16, out_bit_depth 0, dra = NULL with the same matrix, full_range, chroma_loc, upsample and crop (the same code
                 runs): a code in 0 .. 2^B - 1.  The light histogram [2^B] uint32 counts m at full resolution; light_n = w * h; light_max_code = the highest
                 occupied code; light_pctl_code[i] = the percentile rule on this histogram; light_max = lin[light_max_code], light_pctl[i] =
                 lin[light_pctl_code[i]], lin = xgpu_stats_lin(transfer, B): the lin table of xgpu_colour_tables, linear light in [0, 1] of a code.
     light_sum   from the light histogram `count` alone, in binary64, every operation rounded once, nothing fused: for l = 0 .. 63, part[l] = 0 and, over
                 k = l, l + 64, ... ascending, part[l] = part[l] + double(count[k]) * double(lin[k]); light_sum = part[0] + part[1] + ... + part[63], added left to
                 right; light_mean = light_sum / double(light_n), one division.
     Meaning     the scaling is the caller's: for PQ (transfer 16) 10000 * light_max is the picture's MaxCLL contribution and 10000 * light_mean its MaxFALL
                 contribution in cd/m2; for HLG (18) lin is scene light; for the SDR curves it is relative to the display's white.
   d_hist holds uint32 [3][2^hist_bits] (hist_bits != 0), then [2^B] for max(R', G', B') (light != 0).
   Not offered: DRA (the slot's samples are counted as they are), a picture in host memory, and deriving src_peak inside xgpu_pic_output_device_cm - its tables
   are made on the host: the caller reads light_pctl and passes it (times 10000 for PQ) as src_peak.
   The exact contract: INTEGRATION.md section 8i; tests/stats_ref.py restates it in numpy. */
typedef struct xgpu_stats_params {
    int crop[4];        /* left, right, top, bottom luma samples, even */
    int hist_bits;      /* 0: no histogram; else 4 .. coding depth B: 2^hist_bits bins per component */
    int pctl_e4[2];     /* two percentiles in 1/10000, 0 .. 10000 (read when hist_bits != 0 or light != 0) */
    int light;          /* 0 | 1: also the max(R',G',B') histogram and light level */
    int matrix, full_range, chroma_loc, upsample;   /* light: as xgpu_output_format */
    int transfer;       /* light: H.273 TransferCharacteristics of the stream (the list of xgpu_colour_transform) */
} xgpu_stats_params;
typedef struct xgpu_stats_result {        /* written by the device; 176 bytes, every field at a multiple of its size */
    uint64_t n[3], sum[3], sum_sq[3];     /* per component Y, Cb, Cr over the cropped plane: offsets 0, 24, 48 */
    uint32_t min[3], max[3];              /* 72, 84 */
    uint32_t pctl[3][2];                  /* 96: bin << (B - hist_bits); 0 when hist_bits == 0 */
    uint64_t light_n;                     /* 120; everything from here on: 0 when light == 0 */
    double   light_sum, light_mean;       /* 128, 136 */
    uint32_t light_max_code, light_pctl_code[2], reserved;      /* 144, 148, 156 (written as 0) */
    float    light_max, light_pctl[2], reserved2;               /* 160, 164, 172 (written as 0) */
} xgpu_stats_result;
/* Host only, no context.  xgpu_stats_hist_size: (3 * 2^hist_bits (hist_bits != 0) + 2^B (light != 0)) * 4 bytes; 0: invalid parameters (what xgpu_stats_check
   refuses without a picture size), or nothing to write.  xgpu_stats_check: everything xgpu_pic_stats refuses without looking at a context or a pointer's memory -
   0, or XGPU_ERR_INVALID_ARGUMENT for a NULL, a size that is not positive and even, a depth outside 8..12, width * height >= 2^31, an odd or negative crop or
   one that leaves nothing, hist_bits outside {0, 4 .. B}, a percentile outside 0 .. 10000 (where they are read), light outside 0 | 1 and - with light - a
   full_range outside 0 | 1, a chroma_loc outside 0 .. 5 or an upsample that is neither XGPU_UPSAMPLE_NEAREST nor _LINEAR; then, with light,
   XGPU_ERR_UNSUPPORTED for a matrix outside 1, 4, 5, 6, 7, 9 or a transfer outside xgpu_colour_transform's list.  xgpu_stats_lin: lin[k] = float32 of the linear
   light of code k / (2^B - 1) under the inverse of `transfer`, k < 2^B, 0 behind - the lin of xgpu_colour_tables for that source transfer, bit for bit; 0,
   XGPU_ERR_UNSUPPORTED for a transfer outside the list, XGPU_ERR_INVALID_ARGUMENT for a NULL or a depth outside 8..12. */
size_t xgpu_stats_hist_size(const xgpu_stats_params *p, int bit_depth);
int    xgpu_stats_check(const xgpu_stats_params *p, int width, int height, int bit_depth);
int    xgpu_stats_lin(int transfer, int bit_depth, float lin[4096]);
/* Non-blocking.  Takes the statistics of slot `pic` and writes *d_result and - where xgpu_stats_hist_size is not 0 - the histograms at d_hist (hist_size >=
   xgpu_stats_hist_size bytes; else d_hist is not read).  d_result and d_hist must be device memory of the context's device, large enough, d_result 8-byte and
   d_hist 4-byte aligned (checked before anything is queued).  Every field of the result and every histogram element is written by the call, on the same stream,
   by the one workgroup that runs behind the others: the caller clears nothing, and a second call into the same buffers leaves the same bytes.  The picture is
   only read.  stream = NULL: the context's stream; else the kernels run on `stream` behind the picture's kernels, and the context's stream waits for them.  A
   refused call - what xgpu_stats_check refuses, with its code; a slot that holds no picture, a frame that is open (between xgpu_frame_begin and
   xgpu_frame_end), a pointer that fails the checks above: XGPU_ERR_INVALID_ARGUMENT - queues nothing and leaves a message in xgpu_last_error. */
int    xgpu_pic_stats(xgpu_ctx *ctx, int pic, const xgpu_stats_params *p, xgpu_stats_result *d_result, uint32_t *d_hist, size_t hist_size, void *stream);
/* The picture signature on the device: the MD5 of every plane over its rows of width x 2 bytes of 16-bit samples (8-bit pictures too), as xevd_md5_imgb makes it
   (src_base/xevd_util.c:985-1002) and xevd_picbuf_check_signature compares it with the SEI (:1557-1572) - of the DRA-mapped picture when `dra` is given, which is
   what the Main decoder signs when the PPS names a DRA parameter set (src_main/xevdm.c:3256-3287).  digest[plane] = the 16 bytes of the SEI payload.  Blocking; the
   picture's own kernels need not have finished when it is called.  An MD5 is one serial chain per plane: the device walks the three chains in three lanes of one
   wave at ~80 MB/s each (measured: 48 ms for a 1080p picture, 0.22 s at 4K, 0.87 s at 8K; a host core hashes at ~700 MB/s) - it takes the hashing off a CPU-bound
   host, it does not make it faster. */
int  xgpu_pic_md5(xgpu_ctx *ctx, int pic, const xgpu_dra_luts *dra, uint8_t digest[3][16]);
/* whole padded buffers (XEVD_PIC.buf_y/u/v layout: stride = w + 2*pad, rows = h + 2*pad): for tests, and - luma alone, buf_u = buf_v = NULL - for a
   front end that refines merge vectors itself on the reference samples (xhost_parser_set_ref_luma, include/xevd_host.h).  Blocking.                 */
int  xgpu_pic_download_padded(xgpu_ctx *ctx, int pic, int16_t *buf_y, int16_t *buf_u, int16_t *buf_v);
int  xgpu_pic_upload_padded(xgpu_ctx *ctx, int pic, const int16_t *buf_y, const int16_t *buf_u, const int16_t *buf_v);

/* ------------------------------------------------------------------ per picture ------------------- */
int  xgpu_frame_begin(xgpu_ctx *ctx, const xgpu_frame_params *fp);
/* copy a batch into HBM (one pinned staging block + one async H2D copy) and build its device work lists.  The arrays behind `b`
   are read before the call returns.  Device and staging blocks come from a per-context pool: no allocation in steady state. */
int  xgpu_batch_create(xgpu_ctx *ctx, const xgpu_cu_batch *b, xgpu_dbatch **out);
/* xgpu_batch_create / xgpu_batch_destroy are the two entry points that may run on ANOTHER thread than the one driving the context (a builder
   thread preparing picture k+1 while picture k is being launched): the upload goes through the context's own upload stream, and
   xgpu_batch_recon makes the kernels wait for it.  Several threads may be inside xgpu_batch_create of ONE context at a time (pictures built side
   by side: examples/evc_decode --builders, bench.py's end-to-end leg); the staging-block pool is locked, every thread has its own scratch and
   worker pool.  xgpu_batch_wait_upload blocks until the batch's arrays have left host memory.                                             */
int  xgpu_batch_wait_upload(xgpu_ctx *ctx, xgpu_dbatch *db);
/* DMVR: the vectors the decoder stores for temporal prediction (map_mv / dmvr_mv, src_main/xevdm_mc.c:1783-1797, xevdm.c:1553-1563) after
   xgpu_batch_recon: for every CU of the batch with the dmvr flag, two references and at least 8x8 samples - in batch order, its 16x16
   sub-blocks in raster order - mv[list][x/y] in quarter samples: refined where the refinement ran, the CU's own otherwise.  `n` = capacity of
   `mv` in sub-blocks; returns the number of sub-blocks (also with mv = NULL), or a negative error.  Blocking.                                 */
int  xgpu_batch_dmvr_mvs(xgpu_ctx *ctx, xgpu_dbatch *db, int16_t *mv, int n);
/* Host threads xgpu_batch_create may spread its per-CU passes over (validation + counting, record / TB-list construction, the owner map); 1..64, default 1.
   The device arrays it builds do not depend on the count. */
int  xgpu_set_builder_threads(xgpu_ctx *ctx, int n);
/* what the batch builder made of the batch (measurement / diagnostics): info[0] CUs, [1] transform blocks, [2] work items of the transform kernel,
   [3] nodes of the order-dependent kernel (intra / IBC CUs, HTDF nodes), [4] of them without a node among their neighbours, [5] depth of the
   dependency graph (levels), [6] DMVR sub-blocks, [7] affine tiles.                                                                            */
#define XGPU_BATCH_INFO_COUNT 8
int  xgpu_batch_info(xgpu_ctx *ctx, const xgpu_dbatch *db, int info[XGPU_BATCH_INFO_COUNT]);
/* returns the batch's blocks to the pool.  Does not wait for the device: it may follow xgpu_batch_recon immediately (kernels already
   queued keep their data - later batches of this context are written through the same HIP stream, behind them). */
void xgpu_batch_destroy(xgpu_ctx *ctx, xgpu_dbatch *db);
/* Optional, for a caller that has the NEXT picture's batch at hand while the current one is being reconstructed: queues the batch's residual pass (dequant +
   inverse transform - it depends on nothing but the batch) on a side stream behind the k_inter launched last, so that it runs under the current picture's
   dependency kernel and filters; xgpu_batch_recon of that batch then only waits for it.  Call between xgpu_batch_recon of picture k and of picture k + 1.     */
int  xgpu_batch_prepare(xgpu_ctx *ctx, xgpu_dbatch *db);
/* dequant + inverse transform of every coded TB, then MC + residual add + clip of every inter CU, and the
   SCU map update (xevd_set_dec_info) the in-loop filters read.  Asynchronous on the ctx stream.          */
int  xgpu_batch_recon(xgpu_ctx *ctx, xgpu_dbatch *db);
/* xgpu_batch_recon of `db`, with the residual pass of the NEXT picture's batch (`next`, may be NULL; its upload may still be in flight) queued on the
   same stream: inside this picture's data-flow intra launch when it has one - that launch is a chain of memory round trips that leaves most of the GPU
   idle - or behind this picture's last kernel.  xgpu_batch_recon(_ahead) of `next` then starts with its MC kernel.  The preferred form of
   xgpu_batch_prepare: no second stream, no cross-stream event.                                                                                    */
int  xgpu_batch_recon_ahead(xgpu_ctx *ctx, xgpu_dbatch *db, xgpu_dbatch *next);
/* both deblocking passes over the current picture (vertical edges, then horizontal edges)               */
int  xgpu_deblock(xgpu_ctx *ctx);
/* adaptive loop filter: 4x4 block classification + 7x7 luma / 5x5 chroma diamond filters (ctx->fn_alf)    */
int  xgpu_alf(xgpu_ctx *ctx, const xgpu_alf_params *ap);
/* replicate the picture border into the 144/72-sample padding                                            */
int  xgpu_pad(xgpu_ctx *ctx);
int  xgpu_frame_end(xgpu_ctx *ctx);

/* ------------------------------------------------------------------ measurement ------------------- */
/* Kernel families timed with HIP events on the ctx stream (the stream the kernels are launched on).      */
enum { XGPU_K_ITDQ = 0, XGPU_K_INTER = 1, XGPU_K_DBK_V = 2, XGPU_K_DBK_H = 3, XGPU_K_PAD = 4, XGPU_K_INTRA = 5,
       XGPU_K_ALF = 6, XGPU_K_AFFINE = 7, XGPU_K_DMVR = 8, XGPU_K_COUNT = 9 };
int  xgpu_timing_enable(xgpu_ctx *ctx, int on);
int  xgpu_timing_reset(xgpu_ctx *ctx);
/* resolves pending events (synchronises) and returns accumulated milliseconds and launch counts          */
int  xgpu_timing_get(xgpu_ctx *ctx, double ms[XGPU_K_COUNT], long long launches[XGPU_K_COUNT]);
/* plain device-to-device copy bandwidth (bytes read + written per second) - the "measured roofline"      */
int  xgpu_measure_copy_bw(xgpu_ctx *ctx, size_t bytes, int iters, double *gbps);

/* ------------------------------------------------------------------ fine-grained test shims ------- */
/* Host buffers in, host buffers out, one block per call, reference function-table signatures.
   `ref` points INTO a host plane that has at least the filter margin around the addressed window.       */
int xgpu_test_mc_l(xgpu_ctx *ctx, const int16_t *ref_plane, int plane_w, int plane_h, int ref_x, int ref_y,
                   int has_dx, int has_dy, int gmv_x, int gmv_y, int16_t *pred, int w, int h, int bit_depth);
int xgpu_test_mc_c(xgpu_ctx *ctx, const int16_t *ref_plane, int plane_w, int plane_h, int ref_x, int ref_y,
                   int has_dx, int has_dy, int gmv_x, int gmv_y, int16_t *pred, int w, int h, int bit_depth);
/* residual arena of a batch after xgpu_batch_recon (what xevd_sub_block_itdq leaves in core->coef), n_coef s16   */
/* fn_recon (src_base/xevd_def.h:1466; xevd_recon, xevd_recon.c:35-71): rec[cuh][s_rec] = clip(pred + coef) or pred, through the kernels' residual add */
int xgpu_test_recon(xgpu_ctx *ctx, const int16_t *coef, const int16_t *pred, int is_coef, int cuw, int cuh, int s_rec, int16_t *rec, int bit_depth);
/* fn_dbk / fn_dbk_chroma (XEVD_DBK / XEVD_DBK_CH, src_base/xevd_def.h:363-364; deblock_scu_hor / _ver[_chroma], xevd_df.c:96-289): ONE 4-sample (chroma:
   2-sample) edge segment of a host plane of pw x ph samples through the kernels' line filters, in place; (x, y) = first sample on the far side of the
   edge, hor = the edge is horizontal, st = the strength from xevd_tbl_df_st (0 leaves a chroma plane untouched) */
int xgpu_test_dbk(xgpu_ctx *ctx, int16_t *plane, int pw, int ph, int x, int y, int st, int hor, int bit_depth);
int xgpu_test_dbk_chroma(xgpu_ctx *ctx, int16_t *u, int16_t *v, int pw, int ph, int x, int y, int st_u, int st_v, int hor, int bit_depth);
int xgpu_test_batch_resid(xgpu_ctx *ctx, xgpu_dbatch *db, int16_t *resid);
/* The host batch builder alone - no device, no HIP call (runs on a machine without a GPU): builds the staging block of `b` for a sequence `sp` on `threads`
   builder threads and returns an FNV-1a digest per array of the block (CU records, CTU starts, TB records, itdq work items, intra records, dependency lists,
   affine tiles, control points, DMVR sub-blocks, owner map, coefficients, and k_inter's two arrays: the items of the whole tiles and the roles per region), the counts of xgpu_batch_info and the builder's wall time in milliseconds.  The CPU
   suite pins the builder with it: the arrays do not depend on the thread count, and their digests are golden values. */
#define XGPU_TEST_BUILD_DIGESTS 13
int xgpu_test_build_batch(const xgpu_seq_params *sp, const xgpu_cu_batch *b, int threads, uint64_t digest[XGPU_TEST_BUILD_DIGESTS], int info[XGPU_BATCH_INFO_COUNT], double *ms);
/* ... and k_inter's two work arrays themselves, as the builder leaves them (no device, no HIP call either): work[k] = the roles of 64x64 region k in the kernel's
   strip order (0x100: the region lies inside one CU; else two bits per 32x32 tile q = 0 .. 3, 1: the tile lies inside one CU, 2: it holds SCUs of the batch, 0: nothing),
   items[4 * k + q] = the CU the whole tile q lies in, 0xFFFFFFFF where there is none.  *n_work receives the number of regions.  work == items == NULL asks for
   the count alone; one of them alone, or cap_work below the count, is XGPU_ERR_INVALID_ARGUMENT (nothing written, the count returned).  The CPU suite holds its restatement of the role rule to them (tests/mc_launch.py). */
int xgpu_test_inter_lists(const xgpu_seq_params *sp, const xgpu_cu_batch *b, int threads, uint32_t *work, uint32_t *items, int cap_work, int *n_work);
/* dequant + 2-D inverse transform of n blocks of one size, in place (xevd_itdq, src_base/xevd_itdq.c:494) */
int xgpu_test_itdq(xgpu_ctx *ctx, int16_t *coef, int n_blocks, int log2w, int log2h, const uint8_t *qp, int bit_depth);
/* ... naming the transform pair and the row stride.  tr_v / tr_h (vertical = first stage, horizontal = second): 0 DCT-II, 1 DST-VII, 2 DCT-VIII; DST-VII and
   DCT-VIII come as a pair and only for blocks of 4 .. 32 a side (src_main/xevdm_itdq.c:406-421), anything else is refused.  log2s >= log2w is the log2 of the row
   stride: `coef` holds n_blocks blocks of (h << log2s) samples, block i starting at i * (h << log2s), and the samples outside a block's columns come back untouched
   (a 64x64 sub-block of a larger CU keeps the CU's stride, src_base/xevd_itdq.c:573-584).  A stride beyond the width needs a width of at least 8 and a block of more than 16 samples. */
int xgpu_test_itdq_ex(xgpu_ctx *ctx, int16_t *coef, int n_blocks, int log2w, int log2h, const uint8_t *qp, int bit_depth, int tr_v, int tr_h, int log2s);
/* The same blocks through the pair form of the residual pass (two entries of the item list per workgroup, the way the pass rides in the data-flow intra launch of an IQT
   sequence; a context without tool_iqt is refused): ceil(items / 2) workgroups.  The residual arena is filled with 0x5A5A first and comes back whole, so the samples
   outside a block's columns - and a block nobody processed - read 0x5A5A. */
int xgpu_test_itdq_pairs(xgpu_ctx *ctx, int16_t *coef, int n_blocks, int log2w, int log2h, const uint8_t *qp, int bit_depth, int tr_v, int tr_h, int log2s);
/* ... n_groups groups in one launch; groups[6 * g ..] = { n_blocks, log2w, log2h, tr_v, tr_h, log2s } of group g, each held to the rules above; qp has one entry per block
   in group order.  Group g's blocks lie back to back from the next multiple of 64 samples behind group g - 1 (group 0 at 0), and the item list is cut group by group:
   where a group has an odd number of items, items of two classes or two transform pairs meet in one workgroup and run one after the other. */
int xgpu_test_itdq_pairs_mixed(xgpu_ctx *ctx, int16_t *coef, int n_groups, const int32_t *groups, const uint8_t *qp, int bit_depth);
/* xgpu_scale_taps made by the device's row builder (the one k_rois_prepare runs, one lane per row): same arguments, same results, same return value; w_stride
   must hold the widest row.  Blocking. */
int xgpu_test_scale_taps_device(xgpu_ctx *ctx, int n_plane, int subsampling, int siting_half_luma, int n_dst, int filter, int32_t *first, int32_t *count,
                                int16_t *w, int w_stride);

#ifdef __cplusplus
}
#endif
#endif /* XEVD_HIP_H */
