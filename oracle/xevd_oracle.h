/*
 * xevd_oracle.h - CPU restatement of the reference's per-CU reconstruction path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under xevd_amd/ (the product) includes, links, loads or executes this;
 * only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg do, and only as the checker / the
 * timed CPU baseline.  Parity status: PINNED - every function here is checked against the reference itself
 * (oracle/_ref/libxevd_ref.so, built from /root/reference by oracle/Makefile.ref) in tests/test_oracle_vs_ref.py,
 * and the golden vectors under tests/golden/ were produced by the reference (tests/golden/make_golden.py).
 *
 * Each function cites the reference file:line whose arithmetic it restates (paths relative to the
 * mpeg5/xevd v0.7.0 tree).
 */
#ifndef XEVD_ORACLE_H
#define XEVD_ORACLE_H
#include <stdint.h>
#include "../include/xevd_hip.h"   /* shares the batch / parameter structs with the product ABI */

#ifdef __cplusplus
extern "C" {
#endif

/* a picture: pointers to the first ACTIVE sample of each plane (XEVD_PIC.y/u/v), strides in samples;
   the planes must carry the 144/72-sample padding around them (src_base/xevd_def.h:211-212) */
typedef struct orc_pic {
    int16_t *y, *u, *v;
    int      s_l, s_c;
    int      poc;
} orc_pic;

/* SCU maps written by reconstruction and read by the in-loop filters (ctx->map_scu / map_refi / map_mv,
   src_base/xevd_def.h:372-438, xevd_util.c:1574-1660) */
typedef struct orc_maps {
    uint32_t *map_scu;     /* [w_scu*h_scu] */
    int8_t   *map_refi;    /* [w_scu*h_scu][2] */
    int16_t  *map_mv;      /* [w_scu*h_scu][2][2] */
    uint8_t  *map_ats;     /* [w_scu*h_scu] mctx->map_ats_inter (src_main/xevdm_util.c:4321), may be NULL */
    int       w_scu, h_scu;
    const uint8_t *map_tidx; /* [w_scu*h_scu] ctx->map_tidx or NULL: orc_recon_batch_ex fills it in for its own use from batch->tiles */
} orc_maps;

typedef struct orc_frame {
    orc_pic cur;
    orc_pic refp[XGPU_MAX_REFS][2];     /* ctx->refp[idx][list] */
    int     qp_u_offset, qp_v_offset;
} orc_frame;

/* ---- block level (function-table surface) ---- */
/* xevd_mc_l_{00,n0,0n,nn}: src_base/xevd_mc.c:169-288; tables :80-98 / src_main/xevdm_mc.c:121-139 */
void orc_mc_l(const int16_t *ref, int gmv_x, int gmv_y, int s_ref, int s_pred, int16_t *pred, int w, int h,
              int bit_depth, int has_dx, int has_dy, int admvp);
/* xevd_mc_c_{00,n0,0n,nn}: src_base/xevd_mc.c:290-408; tables :100-134 / src_main/xevdm_mc.c:141-175 */
void orc_mc_c(const int16_t *ref, int gmv_x, int gmv_y, int s_ref, int s_pred, int16_t *pred, int w, int h,
              int bit_depth, int has_dx, int has_dy, int admvp);
/* xevd_mc: src_base/xevd_mc.c:435-557 (MV clip, variant select, identical-motion early-out, bi average).
   pred[list][comp] are contiguous w*h / (w/2)*(h/2) buffers of capacity 128*128. Returns number of lists predicted. */
int  orc_mc_cu(const xgpu_seq_params *sp, const orc_frame *fr, int x, int y, int w, int h,
               const int8_t refi[2], const int16_t mv[2][2], int16_t *pred0[3], int16_t *pred1[3]);
/* xevdm_mc with apply_DMVR: src_main/xevdm_mc.c:1860-2038, processDMVR :1647-1829.  1 = refined and averaged into pred0 (refined[k][list][x/y]:
   quarter-sample vectors of the 16x16 sub-blocks), 0 = the conditions failed, nothing predicted */
int  orc_dmvr_cu(const xgpu_seq_params *sp, const orc_frame *fr, int x, int y, int w, int h, const int8_t refi[2], const int16_t mv[2][2],
                 int16_t *pred0[3], int16_t *pred1[3], int16_t (*refined)[2][2]);
/* xevdm_affine_mc: src_main/xevdm_mc.c:2606-2685 (sub-block size / EIF decision xevdm_util.c:1870-2125; EIF :2108-2150, :2393-2604).
   mv[list][vertex][x/y] quarter-pel control points, vn = 2 or 3.  Same pred layout as orc_mc_cu. */
int  orc_affine_mc_cu(const xgpu_seq_params *sp, const orc_frame *fr, int x, int y, int log2w, int log2h, const int8_t refi[2],
                      const int16_t mv[2][3][2], int vn, int16_t *pred0[3], int16_t *pred1[3]);
/* xevd_dquant + xevd_itrans (xevd_itdq): src_base/xevd_itdq.c:473-542; IQT variant src_main/xevdm_itdq.c:708-788 */
void orc_itdq(int16_t *coef, int log2w, int log2h, int qp, int bit_depth, int iqt);
/* ATS (Main, intra CUs): dequant + DST-VII / DCT-VIII 2-D inverse transform, src_main/xevdm_itdq.c:81-421, 732-788.
   tr_v / tr_h: 0 = DST-VII, 1 = DCT-VIII for the vertical / horizontal stage (xevd_tbl_tr_subset_intra) */
void orc_itdq_ats(int16_t *coef, int log2w, int log2h, int qp, int bit_depth, int iqt, int tr_v, int tr_h);
const int16_t *orc_ats_tm(int type, int log2n);   /* xevd_tbl_tr{4,8,16,32}[DCT8=0|DST7=1] as the init code builds them */
/* 1-D stages exposed for table-level checks: xevd_itx_pb*b (step 0 / step 1), src_base/xevd_itdq.c:48-461 */
void orc_itx_pass0(const int16_t *src, int32_t *dst, int log2n, int line);
void orc_itx_pass1(const int32_t *src, int16_t *dst, int log2n, int line, int shift);
const int8_t *orc_tm(int log2n);  /* xevd_tbl_tm2..64, src_base/xevd_tbl.c:89-243 (generated by formula) */
/* xevd_recon: src_base/xevd_recon.c:35-71 */
void orc_recon(const int16_t *coef, const int16_t *pred, int is_coef, int cuw, int cuh, int s_rec, int16_t *rec, int bit_depth);
/* deblock_scu_{ver,hor}[_chroma]: src_base/xevd_df.c:96-289 */
void orc_dbk_luma(int16_t *buf, int st, int stride, int bit_depth, int is_ver);
void orc_dbk_chroma(int16_t *u, int16_t *v, int st_u, int st_v, int stride, int bit_depth, int is_ver);

/* ---- picture level ---- */
/* every inter CU of the batch: itdq -> mc -> recon -> set_dec_info  (xevd_recon_unit, src_base/xevd.c:678-756);
   intra CUs only update the maps.  `resid_out` (optional, n_coef s16) receives the residual arena. */
int  orc_recon_batch(const xgpu_seq_params *sp, const orc_frame *fr, const xgpu_cu_batch *b, orc_maps *maps, int16_t *resid_out);
int  orc_recon_batch_ex(const xgpu_seq_params *sp, const orc_frame *fr, const xgpu_cu_batch *b, orc_maps *maps, int16_t *resid_out, int16_t *dmvr_mv_out);
/* both baseline deblocking passes in the reference's order (src_base/xevd.c:1116-1243,1909-1976; xevd_df.c:291-546) */
int  orc_deblock_baseline(const xgpu_seq_params *sp, const orc_frame *fr, const xgpu_cu_batch *b, orc_maps *maps);
/* ADDB deblocking, both passes (src_main/xevdm_df.c:361-1135, driver src_main/xevdm.c:1935-2103, 3142-3205) */
int  orc_deblock_addb(const xgpu_seq_params *sp, const orc_frame *fr, const xgpu_cu_batch *b, orc_maps *maps, int alpha_off, int beta_off);
/* adaptive loop filter of one picture, in place (alf_process_tile + classification + filters, src_main/xevdm_alf.c:38-429, 901-1165) */
int  orc_alf(const xgpu_seq_params *sp, const orc_pic *pic, const xgpu_alf_params *ap);
/* picbuf_expand: src_base/xevd_util.c:365-427 */
void orc_pad(const xgpu_seq_params *sp, const orc_pic *p);
/* Output conversion of one plane, the application's imgb_cpy_codec_to_out (app/xevd_app_util.h:665-708 with :464-552):
   to 8 bit: bytes, (v + round) >> shift clipped to [0,255]; to a lower depth: the same clipped to the range, 16 bit;
   to a higher depth: v << shift; equal: copy.  src stride in samples; dst rows are tight. */
/* DRA sample processing in place on tight planes (xevd_apply_dra_chroma_plane / _luma_plane with backward_map,
   src_main/xevdm_dra.c:272-355, in xevd_apply_filter's order xevdm.c:3342-3344: Cb, Cr - reading the UNMAPPED luma at (2j, 2k) -
   then luma).  luts: luma_inv_scale_lut[1024], int_chroma_inv_scale_lut[2][1024] of DRA_CONTROL after xevd_init_dra. */
void orc_dra_apply(int16_t *y, int16_t *u, int16_t *v, int w, int h, const int32_t *luma_inv, const int32_t *cb_inv, const int32_t *cr_inv);
void orc_output_convert(const int16_t *src, int stride, int w, int h, int src_bd, int dst_bd, void *dst);
/* default chroma QP mapping table (static table of xevd_tbl.c:334-357 after xevd_tbl_derived_chroma_qp_mapping_tables, :364-426) */
const int8_t *orc_default_chroma_qp_table(void);   /* 58 entries for qp 0..57 (8-bit) */

/* ---- census ----
   Counters the functions above bump where they take a branch (process-wide, not thread-safe: the tests run them one at a time).  They exist so that a
   test can assert that its inputs REACH the arithmetic it was written for - the top of the ADDB tables, both rails of every clip, all ALF classes -
   instead of assuming it.  [2] arrays of clips are { below 0, above max }. */
typedef struct orc_census {
    uint32_t addb_index_a[2][52], addb_index_b[2][52]; /* [luma / chroma] indexA / indexB of every 4-sample segment (chroma: per plane) */
    uint32_t addb_gate[2][5][2];                       /* [luma / chroma][bS][skipped by the alpha-beta gate / filtered], sample lines */
    uint32_t addb_bs4[2][2];                           /* luma bS 4, [p side / q side][weak 3-tap / strong (ap resp. aq and the (alpha >> 2) + 2 test)] */
    uint32_t addb_apq[4];                              /* luma bS 1..3: ap | aq << 1 */
    uint32_t addb_d0[2][2];                            /* [luma / chroma] bS 1..3: d0 inside +-c0 / clipped to it */
    uint32_t addb_out_clip[2][2];                      /* [luma / chroma] bS 1..3: p0 + d0, q0 - d0 clipped */
    uint32_t addb_lost[3];                             /* values that lost bits to the u8 casts: beta, c1 (luma) / c0 (chroma) from the table, luma c0 = c1 + (ap + aq) */
    uint32_t addb_tile_edge[2];                        /* segments not filtered because they lie on a tile border: all / those in an interior 64x64 filter area */
    uint32_t alf_class[25], alf_tr[4];                 /* luma 4x4 blocks by class and by transposition */
    uint32_t alf_clip[3][2];                           /* [plane] filtered samples clipped */
    uint32_t mc_clip[3][2];                            /* [plane] interpolated samples clipped (xevd_mc_{l,c}_{n0,0n,nn}) */
    uint32_t mc_stage1_wrap;                           /* first-stage sums of the 2-D filter that did not fit the s16 intermediate */
    uint32_t mc_bi[3];                                 /* [plane] bi-averaged samples */
    uint32_t mc_bi_rails[3];                           /* luma bi-averaged pairs 0 + 0 / max + max / 0 + max */
    uint32_t mv_clip[4];                               /* vectors moved by xevd_mv_clip: left / right / top / bottom threshold */
    uint32_t recon_coded, recon_wrap;                  /* residual-added samples / sums that wrapped in s16 */
    uint32_t recon_clip[2];                            /* reconstructed samples clipped */
    /* DMVR (orc_dmvr_cu / dmvr_process).  Sub-blocks are the refined 16x16 (or smaller) units; sides are left / right / top / bottom like mv_clip */
    uint32_t dmvr_shape[4];                            /* refined sub-blocks of 8x8 / 8x16 / 16x8 / 16x16 (w x h) */
    uint32_t dmvr_not_refined[2];                      /* flagged bi-predicted CUs of at least 8x8 left to the ordinary path: references not POC-symmetric / identical motion */
    uint32_t dmvr_exit[5];                             /* how the search ended: early (cost < dx * dy) / centre won round 0 / cost 0 after round 0's move / centre won round 1 / moved twice */
    uint32_t dmvr_win[2][5];                           /* [round] the winner of a round that moved: below / above / right / left / the diagonal */
    uint32_t dmvr_diag[4];                             /* the diagonal tried, per round: (x < 0) | (y < 0) << 1 */
    uint32_t dmvr_tie[2];                              /* rounds with right == left / below == above at the <= that picks the diagonal */
    uint32_t dmvr_subpel[2][18];                       /* [x / y] sub-sample step -8 .. 8 at [step + 8]; [17]: denominator 0, no step */
    uint32_t dmvr_total[5][5];                         /* [y + 2][x + 2] whole-sample displacement the search ended at */
    uint32_t dmvr_start_clip[4];                       /* starting vectors (per list) of refined CUs moved by mv_clip */
    uint32_t dmvr_sub_clip[4];                         /* refined vectors (per list and sub-block) clipped at the sub-block (dmvr_clip_one) */
    uint32_t dmvr_win_off[2][8];                       /* [luma / chroma] whole-sample offset of the refined position from the window fetched at the starting vector, both axes and
                                                          lists: -3 .. 3 at [offset + 3]; [7]: further */
    uint32_t dmvr_regime[3][4];                        /* [bilinear (per CU and list) / luma / chroma (per sub-block and list)][(fx != 0) * 2 + (fy != 0)] */
    /* affine (orc_affine_mc_cu / affine_set_mvf).  [path]: 0 EIF, 1 sub-block translation.  "per list": per used list of a CU.  [axis]: 0 x, 1 y */
    uint32_t aff_shape[2][5][5];                       /* CUs by [path][log2w - 3][log2h - 3] */
    uint32_t aff_vn[2];                                /* CUs with 2 / 3 control points */
    uint32_t aff_lists[3];                             /* CUs using list 0 only / list 1 only / both */
    uint32_t aff_w[2][6];                              /* per list: [wx / wy] = 0, 1, 2, 3, 4, above 4 (the largest delta per sample along x / y, aff_subblock) */
    uint32_t aff_sub[2][6];                            /* per CU: the resulting [sub_w / sub_h] = 4, 8, 16, 32, 64, 128 */
    uint32_t aff_applic[2][3];                         /* per list examined, [list]: EIF applicable / dv[1] < -one / too many fetched lines */
    uint32_t aff_applic_skipped;                       /* CUs whose list 1 was not examined because list 0 had failed */
    uint32_t aff_lifted;                               /* CUs whose sub-block was raised to 8 (EIF not applicable, a side below 8) */
    uint32_t aff_band[2];                              /* EIF, per list: memory band exceeded (the range is centre +- spread) / kept (the picture range) */
    uint32_t aff_band_vn[2];                           /* ... exceeded, by control points: 2 (unreachable, tests/test_oracle_extremes.py) / 3 */
    uint32_t aff_range[2][3];                          /* with the band exceeded, per list, [axis]: window below min_pic / above max_pic / inside */
    uint32_t aff_spread[5];                            /* with the band exceeded, per list and axis: spread 128 / 256 / 544 / 1120 / 2272 */
    uint32_t aff_range_clip18[2][2];                   /* EIF, per list, [axis]: min / max of the range moved by clip18 */
    uint32_t aff_eif_clamp[2][2][2];                   /* EIF luma samples (window of (w + 2) x (h + 2)) clamped: [axis][low / high][picture range / band] */
    uint32_t aff_eif_frac[2][32];                      /* EIF luma samples: [axis] fraction fx / fy in 1/32 */
    uint32_t aff_eif_neg[2];                           /* EIF luma samples whose whole-sample offset is negative, [axis] */
    uint32_t aff_eif_clip[3][2];                       /* [plane] EIF samples clipped at the end of the enhancement filter */
    uint32_t aff_sub_mvclip[4];                        /* translation, per list: vector clipped left / right / top / bottom (as in mv_clip) */
    uint32_t aff_sub_mvclip_frac[4];                   /* ... of which the unclipped vector had a luma fraction: the fractional filter runs with the phase-0 row of the tap table */
    uint32_t aff_sub_clip18[2];                        /* translation, per list: [axis] vector moved by clip18 */
    uint32_t aff_sub_regime[2][4];                     /* translation, per list: [luma / chroma][(dx != 0) * 2 + (dy != 0)] of the unclipped vector */
    uint32_t aff_sub_luma_whole_chroma_half[2];        /* translation, per list: [axis] luma at a whole sample, chroma at a half one */
    uint32_t aff_mvf[4];                               /* map vectors per sub-block and list: control point 0 / 1 / 2 / the formula */
    uint32_t aff_mvf_bl_vn2;                           /* ... the bottom-left sub-block (not also the first or the top-right one) of a two-point CU: the formula */
    uint32_t aff_mvf_clip18;                           /* map vector components moved by clip18 */
    uint32_t aff_mvf_whole_cu;                         /* the sub-block is the whole CU: the first branch wins over the others */
    uint32_t aff_ats[2][4][2];                         /* CUs with an ATS-inter TU: [path][idx - 1][pos] */
    uint32_t aff_cbf[2][8];                            /* CUs by [path][cbf] */
    /* HTDF (orc_htdf, avail_intra and the call in orc_recon_batch_ex; only with maps and batch->htdf_slice_qp).  [side]: 0 left, 1 up, 2 right.  Neighbour kinds: 0 intra,
       1 IBC, 2 inter filtered, 3 inter not filtered, 4 nothing there (picture edge), 5 there but not reconstructed yet or in another tile */
    uint32_t htdf_shape[2][5][5];                      /* filtered CUs by [intra / inter][log2w - 2][log2h - 2] */
    uint32_t htdf_skip[7];                             /* CUs not filtered: QP <= 17 / area < 64 / a side of 128 / inter with min >= 32 / inter without luma cbf / IBC / chroma-only tree */
    uint32_t htdf_table[2][5];                         /* filtered CUs by [the slice QP / after the - 8 of square intra CUs of 32 and 64][table 0 .. 4] */
    uint32_t htdf_idx_neg;                             /* ... whose index was negative before the clamp to 0 */
    uint32_t htdf_avail[9][2];                         /* filtered CUs by availability bit 0 .. 8 [clear / set] (2 and 4 do not exist: always clear) */
    uint32_t htdf_src[3][3];                           /* border samples by [side][the neighbour's sample / the CU's own edge: side unavailable / own edge: constrained intra refused the unit] */
    uint32_t htdf_side_mixed[3];                       /* filtered CUs whose [side] holds both neighbours' samples and units constrained intra refused */
    uint32_t htdf_tile_refused[7];                     /* left / up / right / up-left / up-right / low-left / low-right refused only because the neighbour lies in another tile */
    uint32_t htdf_stale_corner[2];                     /* low-left / low-right flag set while the SCU actually read (row ys + scuh) is not reconstructed yet */
    uint32_t htdf_lut[5][16], htdf_pass[5];            /* [table] AC terms looked up by index 0 .. 15 / passed through (a >= thr) */
    uint32_t htdf_thr_edge[5][2];                      /* [table] AC terms with a == thr - 1 (the last one looked up) / a == thr (the first one passed) */
    uint32_t htdf_out_clip[2];                         /* output samples clipped */
    uint32_t htdf_nbr[3][6];                           /* filtered CUs by [side][kind of a neighbouring CU along that side] (a side with several kinds counts in each) */
    /* IBC (the copy in orc_recon_batch_ex; needs maps) */
    uint32_t ibc_shape[5][5];                          /* IBC CUs by [log2w - 2][log2h - 2] */
    uint32_t ibc_luma_only;                            /* ... in a luma-only tree */
    uint32_t ibc_bv[2][3][2];                          /* vector components by [x / y][negative / zero / positive][even / odd] */
    uint32_t ibc_region[3];                            /* the source lies wholly in CTU rows above / wholly in CTUs to the left (not above) / reaches into the CU's own CTU */
    uint32_t ibc_src_cus[3];                           /* distinct CUs under the luma source: 1 / 2 .. 4 / more */
    uint32_t ibc_src_kind[4];                          /* the source holds samples of intra / IBC / HTDF-filtered / inter CUs (one CU may count in several) */
    uint32_t ibc_touch[2];                             /* the source ends exactly at the CU's own left / top edge */
    uint32_t ibc_nbr_of_cintra[2];                     /* intra CUs under constrained intra prediction with an IBC CU along their left / upper side */
    /* intra prediction (intra_neighbours / intra_neighbours_eipd, intra_predict / intra_predict_eipd, ang_sample and the intra branch of orc_recon_batch_ex; needs maps).
       [lr]: avail_lr 0 .. 3.  [side]: 0 up, 1 left, 2 right.  [plane class]: 0 luma, 1 chroma.  Predictor counters are per predicted block (each plane is one), the
       angular ones per sample, the neighbour ones per unit of 4 luma / 2 chroma samples */
    uint32_t ip_shape[2][6][6];                        /* intra CUs by [Baseline / EIPD][log2w - 2][log2h - 2] */
    uint32_t ip_mode_lr[33][4];                        /* EIPD CUs with luma by [luma mode][lr] */
    uint32_t ip_mode_aspect[33][3];                    /* ... by [luma mode][wide / square / tall] */
    uint32_t ip_cmode_lr[5][4];                        /* EIPD CUs with chroma by [chroma mode][lr] */
    uint32_t ip_dm_luma[33];                           /* ... of chroma mode 0 (DM) by the luma mode it resolved to */
    uint32_t ip_base_mode[2][5];                       /* Baseline CUs by [luma / chroma][mode] */
    uint32_t ip_base_c_differs;                        /* Baseline CUs (all planes) whose chroma mode differs from the luma mode */
    uint32_t ip_dc[2][8];                              /* EIPD DC blocks by [lr != 3 / lr == 3][index into the 4096 / (2^k + 1) table] */
    uint32_t ip_plan[2][6][6];                         /* planar blocks by [left form / mirrored right form][iw][ih] (indices into mult / shift) */
    uint32_t ip_plan_clip[2];                          /* planar samples clipped */
    uint32_t ip_bi_form[3];                            /* bilinear blocks: left column / lr == 2 (mirrored) / lr == 3 (both columns) */
    uint32_t ip_bi_corner[2][2];                       /* one-column bilinear blocks by [left / lr == 2][square: (a + b + 1) >> 1 / not square: wc_tbl] */
    uint32_t ip_bi_wc[6];                              /* ... by the wc_tbl index 1 .. 5 ([0] stays empty) */
    uint32_t ip_bi_clip[2];                            /* one-column bilinear samples clipped */
    uint32_t ip_hor[3];                                /* mode 24 blocks: from the left column (lr 0 / 1) / from the right one (lr 2) / interpolated between the two (lr 3) */
    uint32_t ip_ang_src[3][3];                         /* angular samples by [mode < 12 / 13 .. 23 / > 24][reference read from up / left / right] */
    uint32_t ip_ang_frac[2];                           /* ... fraction o == 0 / o != 0 */
    uint32_t ip_ang_clamp[2];                          /* ... with a tap position clamped at -1 / at w + h - 1 */
    uint32_t ip_ang_clip[2];                           /* ... clipped at the end */
    uint32_t ip_nbr[2][3][2][3];                       /* neighbour units by [EIPD builder / Baseline builder][side][plane class][available / unavailable behind an earlier unit: the
                                                          sample before it repeated (Baseline: mid) / unavailable first unit: up takes the corner or mid, left the corner, right up[w] (Baseline: mid)] */
    uint32_t ip_unavail[4];                            /* unavailable units by reason: outside the picture / not reconstructed yet / in another tile / refused by constrained intra prediction */
    uint32_t ip_corner[3];                             /* the corner sample: available / not, takes up[0] read from the picture (EIPD) / not, takes mid (EIPD: up[0] unavailable as well; Baseline) */
    uint32_t ip_tree[3];                               /* intra CUs by tree: 0 / luma only / chroma only */
    uint32_t ip_cbf[8];                                /* intra CUs by cbf */
    /* residual pass (orc_itdq / orc_itdq_ats, their stages, and the calls in orc_recon_batch_ex, which say what the TB is; a call from elsewhere counts as a contiguous luma
       TB, DCT-II resp. ATS-intra).  [kind]: 0 DCT-II, 1 ATS-intra, 2 the TU of an ATS-inter CU (all planes, whichever matrices it takes).  [arith]: the arithmetic of the
       two stages, 0 the 32-bit intermediate of xevd_itrans (non-IQT), 1 the clipped s16 one of xevdm_itrans (IQT), 2 ATS.  [parity]: (log2w + log2h) & 1, the odd classes
       carry the factor 181 / 256.  Pairs: two adjacent coefficient rows (columns), the unit of the kernel's sparsity masks */
    uint32_t it_tb[3][6][6];                           /* TBs by [kind][log2w - 1][log2h - 1] */
    uint32_t it_plane[3][3];                           /* TBs by [kind][plane] */
    uint32_t it_ats_pair[2][2];                        /* TBs through the ATS matrices by [vertical][horizontal], 0 DST-VII, 1 DCT-VIII */
    uint32_t it_ats_shape[2][2][4][4];                 /* ... by [vertical][horizontal][log2w - 2][log2h - 2] */
    uint32_t it_ats_inter[4][2][2];                    /* luma TUs of ATS-inter CUs by [idx - 1][pos][DST-VII / DCT-VIII (CU at most 32x32) / DCT-II] */
    uint32_t it_strided[4];                            /* TBs whose row stride exceeds their width (sub-blocks of a CU above 64) by sub-block index (j << 1) | i */
    uint32_t it_qp[96];                                /* TBs by QP (above 95: in [95]) */
    uint32_t it_dq_clip[2][2];                         /* [parity] dequantised coefficients clipped below / above */
    uint32_t it_dq_zero[2];                            /* [parity] non-zero levels that dequantise to 0 */
    uint32_t it_dq_cmax[2][2];                         /* [parity] levels of magnitude 2^23 >> (qp / 6) / one beyond */
    uint32_t it_high[2];                               /* non-zero levels at positions 32 .. 63 of a 64-point dimension, [vertical / horizontal] */
    uint32_t it_s1_clip[2][2];                         /* first stage, [IQT / ATS]: results clipped low / high */
    uint32_t it_s1_negfrac;                            /* first stage, non-IQT: negative intermediates with non-zero low 15 bits */
    uint32_t it_s1_mag[5];                             /* first stage, non-IQT: intermediates of magnitude below 2^15 / 2^24 / 2^27 / 2^28 / from 2^28 */
    uint32_t it_s2_clip[3][2];                         /* second stage, [arith]: results clipped low / high */
    uint32_t it_s2_undef;                              /* second stage, non-IQT: output sums with sum_k |tm[k][n]| * |t[k]| >= 2^31, where the reference's 32-bit products may wrap */
    uint32_t it_undef_tb;                              /* ... TBs holding such a sum */
    uint32_t it_nz_pairs[2][5];                        /* TBs by the number of [row / column] pairs with a non-zero level: 0 / 1 / 2 .. 4 / 5 or more, not all / all */
    uint32_t it_single[32][32];                        /* TBs holding one non-zero level, a side of at least 16, by [row pair][column pair] of it */
    uint32_t it_single_dim[2][3][32];                  /* ... by [vertical / horizontal][that dimension 16 / 32 / 64][pair] */
    /* translational motion compensation (orc_mc_cu and its call in orc_recon_batch_ex): the plain inter CUs - not affine, not refined by DMVR, not IBC.  "per list": per
       list the CU is predicted from, i.e. after the identical-motion test.  Sides are left / right / top / bottom like mv_clip */
    uint32_t mc_phase[2][4][4];                        /* per list, [Baseline / Main tap table][fx][fy]: quarter-sample fraction of the CLIPPED position (row 4 fx of k_luma_taps) */
    uint32_t mc_cphase[2][8][8];                       /* ... eighth-sample fraction of the clipped position (row 4 fx of k_chroma_taps) */
    uint32_t mc_regime[2][4];                          /* per list: [luma / chroma][(dx != 0) * 2 + (dy != 0)] of the UNCLIPPED vector */
    uint32_t mc_luma_whole_chroma_half[2];             /* per list: [axis] luma at a whole sample, chroma at a half one */
    uint32_t mc_lists[4];                              /* CUs using list 0 only / list 1 only / both / both, collapsed to list 0 by identical motion on equal POCs */
    uint32_t mc_refi[2][XGPU_MAX_REFS];                /* per list: [list][reference index] */
    uint32_t mc_shape[6][6];                           /* CUs by [log2w - 2][log2h - 2] */
    uint32_t mc_edge[4][2];                            /* per list: the luma window (the block, and the filter's margin along an axis it filters) reaches over the picture's
                                                          [side], [partly / with every sample] - the replicated border read as samples */
    uint32_t mc_tu[5][2];                              /* CUs by ATS-inter [idx 0 .. 4][pos] */
    uint32_t mc_cbf[8];                                /* CUs by cbf */
    uint32_t mc_skip;                                  /* CUs in skip mode */
    uint32_t mc_dmvr_fallback;                         /* CUs carrying the DMVR flag that are predicted here after all */
} orc_census;
void orc_census_reset(void);
void orc_census_get(orc_census *out);
int  orc_census_size(void);

#ifdef __cplusplus
}
#endif
#endif
