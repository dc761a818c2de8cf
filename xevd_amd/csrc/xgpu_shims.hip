// xgpu_shims.hip - the fine-grained test shims of include/xevd_hip.h (xgpu_test_*): one block per call through the kernels' device functions, with the reference's
// per-block function-table call shapes.
#include "xgpu_host.h"

// ------------------------------------------------------------------------------------------------ test shims
static int test_mc(xgpu_ctx *c, const int16_t *plane, int pw, int ph, int ref_x, int ref_y, int has_dx, int has_dy,
                   int gmv_x, int gmv_y, int16_t *pred, int w, int h, int bd, int luma)
{
    ARGCHK(c, c != NULL); ARGCHK(c, plane && pred && pw > 0 && ph > 0 && w > 0 && h > 0);
    ARGCHK(c, luma ? ((w & 3) == 0 && (h & 3) == 0) : ((w & 1) == 0 && (h & 1) == 0));
    int16_t *dp = NULL, *dq = NULL;
    const size_t pb = sizeof(int16_t) * (size_t)pw * ph + 64, qb = sizeof(int16_t) * (size_t)w * h;
    HIPCHK(c, hipMalloc((void **)&dp, pb));
    HIPCHK(c, hipMalloc((void **)&dq, qb));
    HIPCHK(c, hipMemcpyAsync(dp, plane, pb - 64, hipMemcpyHostToDevice, c->stream));
    launch_test_mc(c, dp, pw, ref_x, ref_y, has_dx, has_dy, gmv_x, gmv_y, dq, w, h, bd, luma);
    HIPCHK(c, hipMemcpyAsync(pred, dq, qb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(dp); (void)hipFree(dq);
    return XGPU_OK;
}
int xgpu_test_mc_l(xgpu_ctx *c, const int16_t *plane, int pw, int ph, int ref_x, int ref_y, int has_dx, int has_dy,
                   int gmv_x, int gmv_y, int16_t *pred, int w, int h, int bd)
{ return test_mc(c, plane, pw, ph, ref_x, ref_y, has_dx, has_dy, gmv_x, gmv_y, pred, w, h, bd, 1); }
int xgpu_test_mc_c(xgpu_ctx *c, const int16_t *plane, int pw, int ph, int ref_x, int ref_y, int has_dx, int has_dy,
                   int gmv_x, int gmv_y, int16_t *pred, int w, int h, int bd)
{ return test_mc(c, plane, pw, ph, ref_x, ref_y, has_dx, has_dy, gmv_x, gmv_y, pred, w, h, bd, 0); }

int xgpu_test_recon(xgpu_ctx *c, const int16_t *coef, const int16_t *pred, int is_coef, int cuw, int cuh, int s_rec, int16_t *rec, int bit_depth)
{
    ARGCHK(c, c != NULL); ARGCHK(c, coef && pred && rec && cuw >= 2 && cuh >= 1 && !(cuw & 1) && cuw <= 128 && cuh <= 128 && s_rec >= cuw && bit_depth >= 8 && bit_depth <= 12);
    const size_t nb = sizeof(int16_t) * (size_t)cuw * cuh, rb = sizeof(int16_t) * (size_t)s_rec * cuh;
    int16_t *d = NULL;
    HIPCHK(c, hipMalloc((void **)&d, 2 * nb + rb));
    int16_t *dc = d, *dp = d + (size_t)cuw * cuh, *dr = dp + (size_t)cuw * cuh;
    HIPCHK(c, hipMemcpyAsync(dc, coef, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dp, pred, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dr, rec, rb, hipMemcpyHostToDevice, c->stream));
    launch_test_recon(c, dc, dp, is_coef, cuw, cuh, dr, s_rec, bit_depth);
    HIPCHK(c, hipMemcpyAsync(rec, dr, rb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(d);
    return XGPU_OK;
}
// plane(s): pw x ph samples, host, in and out; (x, y) = the first sample on the far side of the edge
static int test_dbk(xgpu_ctx *c, int16_t *plane, int16_t *plane_v, int pw, int ph, int x, int y, int st, int st_v, int hor, int bd, int chroma)
{
    ARGCHK(c, c != NULL); ARGCHK(c, plane && (!chroma || plane_v) && pw > 0 && ph > 0 && bd >= 8 && bd <= 12 && st >= 0 && st_v >= 0);
    const int len = chroma ? 2 : 4;
    ARGCHK(c, hor ? (y >= 2 && y + 2 <= ph && x >= 0 && x + len <= pw) : (x >= 2 && x + 2 <= pw && y >= 0 && y + len <= ph));
    const size_t nb = sizeof(int16_t) * (size_t)pw * ph;
    int16_t *d = NULL;
    HIPCHK(c, hipMalloc((void **)&d, 2 * nb));
    HIPCHK(c, hipMemcpyAsync(d, plane, nb, hipMemcpyHostToDevice, c->stream));
    if (chroma) HIPCHK(c, hipMemcpyAsync(d + (size_t)pw * ph, plane_v, nb, hipMemcpyHostToDevice, c->stream));
    launch_test_dbk(c, d + (size_t)y * pw + x, d + (size_t)pw * ph + (size_t)y * pw + x, st, st_v, pw, bd, hor, chroma);
    HIPCHK(c, hipMemcpyAsync(plane, d, nb, hipMemcpyDeviceToHost, c->stream));
    if (chroma) HIPCHK(c, hipMemcpyAsync(plane_v, d + (size_t)pw * ph, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(d);
    return XGPU_OK;
}
int xgpu_test_dbk(xgpu_ctx *c, int16_t *plane, int pw, int ph, int x, int y, int st, int hor, int bit_depth)
{ return test_dbk(c, plane, NULL, pw, ph, x, y, st, 0, hor, bit_depth, 0); }
int xgpu_test_dbk_chroma(xgpu_ctx *c, int16_t *u, int16_t *v, int pw, int ph, int x, int y, int st_u, int st_v, int hor, int bit_depth)
{ return test_dbk(c, u, v, pw, ph, x, y, st_u, st_v, hor, bit_depth, 1); }

int xgpu_test_batch_resid(xgpu_ctx *c, xgpu_dbatch *db, int16_t *resid)
{
    ARGCHK(c, c != NULL); ARGCHK(c, db != NULL && resid != NULL);
    if (db->n_coef) HIPCHK(c, hipMemcpyAsync(resid, db->d_resid, sizeof(int16_t) * db->n_coef, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return XGPU_OK;
}

// Blocks of one size class and one transform pair through launch_itdq; block i starts at i * (h << log2s) and keeps the row stride 2^log2s.  The whole buffer goes into the
// coefficient arena AND the residual arena, so what the kernel does not write comes back as the caller gave it.
int xgpu_test_itdq_ex(xgpu_ctx *c, int16_t *coef, int n_blocks, int log2w, int log2h, const uint8_t *qp, int bit_depth, int tr_v, int tr_h, int log2s)
{
    ARGCHK(c, c != NULL); ARGCHK(c, coef && qp && n_blocks > 0 && log2w >= 1 && log2w <= 6 && log2h >= 1 && log2h <= 6 && bit_depth >= 8 && bit_depth <= 16);
    ARGCHK(c, tr_v >= TR_DCT2 && tr_v <= TR_DCT8 && tr_h >= TR_DCT2 && tr_h <= TR_DCT8);
    // the builder's rule (tr_code): DST-VII / DCT-VIII come as a pair, for TBs of 4 .. 32 a side
    ARGCHK(c, (tr_v == TR_DCT2 && tr_h == TR_DCT2) || (tr_v != TR_DCT2 && tr_h != TR_DCT2 && log2w >= 2 && log2w <= 5 && log2h >= 2 && log2h <= 5));
    // a row stride beyond the width: the kernel fetches 8 samples of one row at a time, so the row holds at least 8, and the classes of at most 16 samples load their
    // block as one piece (the builder gives a stride to 64x64 / 32x32 sub-blocks only)
    ARGCHK(c, log2s >= log2w && log2s <= 12 && (log2s == log2w || (log2w >= 3 && log2w + log2h > 4)));
    const size_t per = (size_t)1 << (log2s + log2h), nb = per * n_blocks * sizeof(int16_t);
    ARGCHK(c, per * n_blocks <= 0x7FFFFFFFu);
    std::vector<TbRec> tbs(n_blocks);
    std::vector<TbWave> wv;
    for (int i = 0; i < n_blocks; i++) { tbs[i].off = (uint32_t)(per * i); tbs[i].log2w = (uint8_t)log2w; tbs[i].log2h = (uint8_t)log2h; tbs[i].qp = qp[i]; tbs[i].log2s = (uint8_t)log2s; }
    const int pw = itdq_group_size(log2w, log2h);
    for (int f = 0; f < n_blocks; f += pw)
        wv.push_back({ (uint32_t)f, (uint16_t)std::min(pw, n_blocks - f), (uint8_t)log2w, (uint8_t)log2h, (uint8_t)tr_v, (uint8_t)tr_h, { 0, 0 } });
    int16_t *dc = NULL, *dr = NULL; TbRec *dt = NULL; TbWave *dw = NULL;
    HIPCHK(c, hipMalloc((void **)&dc, nb)); HIPCHK(c, hipMalloc((void **)&dr, nb));
    HIPCHK(c, hipMalloc((void **)&dt, sizeof(TbRec) * tbs.size())); HIPCHK(c, hipMalloc((void **)&dw, sizeof(TbWave) * wv.size()));
    HIPCHK(c, hipMemcpyAsync(dc, coef, nb, hipMemcpyHostToDevice, c->stream));
    if (log2s != log2w) HIPCHK(c, hipMemcpyAsync(dr, coef, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dt, tbs.data(), sizeof(TbRec) * tbs.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dw, wv.data(), sizeof(TbWave) * wv.size(), hipMemcpyHostToDevice, c->stream));
    ItdqArgs ia; ia.coef = dc; ia.resid = dr; ia.tbs = dt; ia.waves = dw; ia.n_waves = (int)wv.size(); ia.bd = bit_depth; ia.iqt = c->sp.tool_iqt;
    launch_itdq(c, ia, c->stream);
    HIPCHK(c, hipMemcpyAsync(coef, dr, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(dc); (void)hipFree(dr); (void)hipFree(dt); (void)hipFree(dw);
    return XGPU_OK;
}
int xgpu_test_itdq(xgpu_ctx *c, int16_t *coef, int n_blocks, int log2w, int log2h, const uint8_t *qp, int bit_depth)
{ return xgpu_test_itdq_ex(c, coef, n_blocks, log2w, log2h, qp, bit_depth, TR_DCT2, TR_DCT2, log2w); }

// Groups of blocks, each of one size class and one transform pair, through launch_itdq_pairs (two entries of the item list per workgroup, as k_intra_itdq's residual side
// takes them): a group's blocks lie back to back from the next multiple of 64 samples behind the group before it, the item list is cut group by group, so entries of different groups meet in one workgroup wherever a group has an odd
// number of entries.  The residual arena is filled with 0x5A5A first and comes back whole: an entry nobody ran, and the samples outside a block's columns, read 0x5A5A.
int xgpu_test_itdq_pairs_mixed(xgpu_ctx *c, int16_t *coef, int n_groups, const int32_t *groups, const uint8_t *qp, int bit_depth)
{
    ARGCHK(c, c != NULL); ARGCHK(c, coef && groups && qp && n_groups > 0 && bit_depth >= 8 && bit_depth <= 16);
    ARGCHK(c, c->sp.tool_iqt);                                // the pair form exists in the IQT instantiations only
    std::vector<TbRec> tbs;
    std::vector<TbWave> wv;
    size_t total = 0;
    for (int gi = 0; gi < n_groups; gi++) {
        const int32_t *g = groups + 6 * gi;
        const int n_blocks = g[0], log2w = g[1], log2h = g[2], tr_v = g[3], tr_h = g[4], log2s = g[5];
        ARGCHK(c, n_blocks > 0 && log2w >= 1 && log2w <= 6 && log2h >= 1 && log2h <= 6);
        ARGCHK(c, tr_v >= TR_DCT2 && tr_v <= TR_DCT8 && tr_h >= TR_DCT2 && tr_h <= TR_DCT8);
        ARGCHK(c, (tr_v == TR_DCT2 && tr_h == TR_DCT2) || (tr_v != TR_DCT2 && tr_h != TR_DCT2 && log2w >= 2 && log2w <= 5 && log2h >= 2 && log2h <= 5));      // as xgpu_test_itdq_ex
        ARGCHK(c, log2s >= log2w && log2s <= 12 && (log2s == log2w || (log2w >= 3 && log2w + log2h > 4)));
        const size_t per = (size_t)1 << (log2s + log2h);
        total = (total + 63) & ~(size_t)63;                  // a group starts at a multiple of 64 samples (the builder's arena keeps a TB aligned to its vector stores)
        ARGCHK(c, total + per * n_blocks <= 0x7FFFFFFFu);
        const int pw = itdq_group_size(log2w, log2h), first = (int)tbs.size();
        for (int i = 0; i < n_blocks; i++) {
            TbRec t; t.off = (uint32_t)(total + per * i); t.log2w = (uint8_t)log2w; t.log2h = (uint8_t)log2h; t.qp = qp[first + i]; t.log2s = (uint8_t)log2s;
            tbs.push_back(t);
        }
        for (int f = 0; f < n_blocks; f += pw)
            wv.push_back({ (uint32_t)(first + f), (uint16_t)std::min(pw, n_blocks - f), (uint8_t)log2w, (uint8_t)log2h, (uint8_t)tr_v, (uint8_t)tr_h, { 0, 0 } });
        total += per * n_blocks;
    }
    const size_t nb = total * sizeof(int16_t);
    int16_t *dc = NULL, *dr = NULL; TbRec *dt = NULL; TbWave *dw = NULL;
    HIPCHK(c, hipMalloc((void **)&dc, nb)); HIPCHK(c, hipMalloc((void **)&dr, nb));
    HIPCHK(c, hipMalloc((void **)&dt, sizeof(TbRec) * tbs.size())); HIPCHK(c, hipMalloc((void **)&dw, sizeof(TbWave) * wv.size()));
    HIPCHK(c, hipMemcpyAsync(dc, coef, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dr, 0x5A, nb, c->stream));
    HIPCHK(c, hipMemcpyAsync(dt, tbs.data(), sizeof(TbRec) * tbs.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dw, wv.data(), sizeof(TbWave) * wv.size(), hipMemcpyHostToDevice, c->stream));
    ItdqArgs ia; ia.coef = dc; ia.resid = dr; ia.tbs = dt; ia.waves = dw; ia.n_waves = (int)wv.size(); ia.bd = bit_depth; ia.iqt = 1;
    launch_itdq_pairs(c, ia, c->stream);
    HIPCHK(c, hipMemcpyAsync(coef, dr, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(dc); (void)hipFree(dr); (void)hipFree(dt); (void)hipFree(dw);
    return XGPU_OK;
}
// ... one group: the arguments of xgpu_test_itdq_ex, ceil(items / 2) workgroups
int xgpu_test_itdq_pairs(xgpu_ctx *c, int16_t *coef, int n_blocks, int log2w, int log2h, const uint8_t *qp, int bit_depth, int tr_v, int tr_h, int log2s)
{
    const int32_t g[6] = { n_blocks, log2w, log2h, tr_v, tr_h, log2s };
    return xgpu_test_itdq_pairs_mixed(c, coef, 1, g, qp, bit_depth);
}

// xgpu_scale_taps through the device's row builder (k_output_rois_dev.hip): the arguments are checked by the host function itself, which also says how wide
// the widest row is; then one lane per row on the device, and the three arrays come back
int xgpu_test_scale_taps_device(xgpu_ctx *c, int n_plane, int subsampling, int siting_half_luma, int n_dst, int filter, int32_t *first, int32_t *count, int16_t *w,
                                int w_stride)
{
    ARGCHK(c, c != NULL);
    const int widest = xgpu_scale_taps(n_plane, subsampling, siting_half_luma, n_dst, filter, first, count, NULL, 0);
    if (widest < 0) return widest;
    ARGCHK(c, !w || w_stride >= widest);
    const size_t ib = sizeof(int32_t) * (size_t)n_dst, wb = w ? sizeof(int16_t) * (size_t)n_dst * w_stride : 0;
    uint8_t *d = NULL;
    HIPCHK(c, hipSetDevice(c->sp.device));
    HIPCHK(c, hipMalloc((void **)&d, 2 * ib + wb + 16));
    HIPCHK(c, hipMemsetAsync(d, 0xFF, 2 * ib + wb, c->stream));      // nothing of the host's pass survives in what is compared
    int32_t *df = (int32_t *)d, *dc = df + n_dst;
    int16_t *dw = w ? (int16_t *)(dc + n_dst) : NULL;
    launch_test_scale_taps(n_plane, subsampling, siting_half_luma, n_dst, filter, df, dc, dw, w_stride, c->stream);
    HIPCHK(c, hipMemcpyAsync(first, df, ib, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(count, dc, ib, hipMemcpyDeviceToHost, c->stream));
    if (w) HIPCHK(c, hipMemcpyAsync(w, dw, wb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(d);
    int wide = 0;
    for (int o = 0; o < n_dst; o++) wide = count[o] > wide ? count[o] : wide;
    return wide;
}
