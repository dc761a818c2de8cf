// k_residual.hip - the prediction residual of a batch as dense, picture-shaped planes (xgpu_batch_residual): the third product of a decoder next to the
// samples and the side information.  The arena k_itdq / k_intra_itdq fill (xgpu_dbatch.d_resid) is only read here, with the addressing of the batch builder
// and k_inter: per CU the component blocks Y, Cb, Cr, each present only with its cbf bit, row stride = the block's width, the block of an ATS-inter CU being
// its TU.  The contract is INTEGRATION.md section 8g; tests/residual_ref.py restates it in numpy.
//
// k_resid_planes (YUV420, 444 planar / interleaved): a lane owns 8 output pixels of a row and the (up to) four output rows of one row of 4x4 units: the two -
// with a left crop that is not a multiple of 4: three - units under its pixels.  Per unit the chain is owner -> CU record (two 16-byte loads) -> four 8-byte
// luma rows and two 4-byte rows per chroma plane.  The loads of a stage are issued together and unconditionally: a unit that holds nothing (no CU of the
// batch, a clear cbf bit, outside the TU) reads the arena's first bytes with stride 0 and is zeroed by a select, so no branch separates the loads of the
// units.  Stores go through store_run: 16 bytes per row and plane (8 for a 4:2:0 chroma row) when the alignment allows, elements otherwise and in a row's
// last group.  Every element of the destination is written, zeros included.
// k_resid_energy: sum |r| per unit and component, a lane owns 4 units of a row; the same loads, reduced in registers.
// k_resid_chroma: local dual trees.  The owner map names the luma CUs of such a block, and a luma-only CU has no chroma coefficients: the kernels above
// write zero chroma there.  This launch - one workgroup per chroma-only CU with coded chroma, only when the batch has any - then writes those CUs' chroma
// over the zeros, element by element.
#pragma clang fp contract(off)
#include "output_common.h"

#define RESID_NONE 0xFFFFFFFFu

// where the three component blocks of one 4x4 luma unit lie in the arena, from the unit's CU record (k_inter.hip: inter_tile / load_resid); a component that
// is not there: the arena's start with stride 0 and ok = false
struct ResidUnit { uint32_t off_l, off_b, off_r; int st_l, st_c; bool ok_l, ok_b, ok_r; };
__device__ __forceinline__ ResidUnit resid_unit(uint32_t own, const uint4 r0, const uint4 r1, int sx, int sy)
{
    const int cu_x = r0.x & 0xFFFF, cu_y = r0.x >> 16;
    const int lw = r0.y & 0xFF, lh = (r0.y >> 8) & 0xFF, pred_mode = (r0.y >> 16) & 0xF, cbf = r0.y >> 24;
    const int cw = 1 << (lw & 7), chh = 1 << (lh & 7);
    const int ai = (pred_mode == XGPU_MODE_INTRA || pred_mode == XGPU_MODE_IBC) ? 0 : (int)((r1.w >> 8) & 0xFF);
    int tu_x = 0, tu_y = 0, tu_w = cw, tu_h = chh;
    if (ai) {
        const int idx = ai & 15, pos = ai >> 4;
        if (idx == 2 || idx == 4) { tu_h = chh >> (idx == 4 ? 2 : 1); tu_y = pos ? chh - tu_h : 0; }
        else                      { tu_w = cw >> (idx == 3 ? 2 : 1);  tu_x = pos ? cw - tu_w : 0; }
    }
    const int lx = (sx << 2) - cu_x - tu_x, ly = (sy << 2) - cu_y - tu_y;      // position inside the TU
    const bool in = own != RESID_NONE && (uint32_t)lx < (uint32_t)tu_w && (uint32_t)ly < (uint32_t)tu_h;
    const int cwc = tu_w >> 1;
    ResidUnit u;
    u.ok_l = in && (cbf & 1); u.ok_b = in && (cbf & 2); u.ok_r = in && (cbf & 4);
    uint32_t off = r0.w;
    u.off_l = u.ok_l ? off + (uint32_t)(ly * tu_w + lx) : 0u;
    if (cbf & 1) off += (uint32_t)(tu_w * tu_h);
    const uint32_t in_c = (uint32_t)((ly >> 1) * cwc + (lx >> 1));
    u.off_b = u.ok_b ? off + in_c : 0u;
    if (cbf & 2) off += (uint32_t)(cwc * (tu_h >> 1));
    u.off_r = u.ok_r ? off + in_c : 0u;
    u.st_l = u.ok_l ? tu_w : 0;
    u.st_c = cwc;
    return u;
}

// the samples of NU neighbouring units of unit row sy from column ub on (clamped to the row): l[k][r] the four luma samples of row r, cb / cr[k][r] the two
// chroma samples of chroma row r, as packed s16 pairs; zero where nothing is coded.  live[k] = false: unit k is not wanted (zeros, nothing loaded)
template <int NU>
__device__ __forceinline__ void resid_load_units(const ResidArgs &a, int ub, int sy, const bool (&live)[NU], uint2 (&l)[NU][4], uint32_t (&cb)[NU][2], uint32_t (&cr)[NU][2])
{
    uint32_t own[NU];
    int sx[NU];
    #pragma unroll
    for (int k = 0; k < NU; k++) {
        sx[k] = min(ub + k, a.w_scu - 1);
        own[k] = live[k] ? a.owner[(size_t)sy * a.w_scu + sx[k]] : RESID_NONE;
    }
    uint4 r0[NU], r1[NU];
    #pragma unroll
    for (int k = 0; k < NU; k++) {
        const uint4 *p = (const uint4 *)(a.cus + (own[k] == RESID_NONE ? 0u : own[k]));      // (no CU: record 0 is read and not used)
        r0[k] = p[0]; r1[k] = p[1];
    }
    ResidUnit u[NU];
    #pragma unroll
    for (int k = 0; k < NU; k++) u[k] = resid_unit(own[k], r0[k], r1[k], sx[k], sy);
    #pragma unroll
    for (int k = 0; k < NU; k++) {
        #pragma unroll
        for (int r = 0; r < 4; r++) l[k][r] = *(const uint2 *)(a.resid + u[k].off_l + r * u[k].st_l);
        #pragma unroll
        for (int r = 0; r < 2; r++) {
            cb[k][r] = *(const uint32_t *)(a.resid + u[k].off_b + (u[k].ok_b ? r * u[k].st_c : 0));
            cr[k][r] = *(const uint32_t *)(a.resid + u[k].off_r + (u[k].ok_r ? r * u[k].st_c : 0));
        }
    }
    #pragma unroll
    for (int k = 0; k < NU; k++) {
        #pragma unroll
        for (int r = 0; r < 4; r++) if (!u[k].ok_l) l[k][r] = make_uint2(0, 0);
        #pragma unroll
        for (int r = 0; r < 2; r++) { if (!u[k].ok_b) cb[k][r] = 0; if (!u[k].ok_r) cr[k][r] = 0; }
    }
}

// one residual sample of component c -> the bits of the output element: the s16 itself, or float32(r) * 2^-B (exact) and its float16 rounding
template <int DT> __device__ __forceinline__ uint32_t resid_elem(const ResidArgs &a, int c, int v)
{
    if (OutT<DT>::is_float) return fbits<DT>((float)v * a.scale[c]);
    return (uint32_t)(uint16_t)v;
}
__device__ __forceinline__ int s16_lo(uint32_t w) { return (int)(int16_t)(w & 0xFFFFu); }
__device__ __forceinline__ int s16_hi(uint32_t w) { return (int)(int16_t)(w >> 16); }

// LAYOUT: XGPU_RESID_YUV420 (DT = U16), _444_PLANAR, _444_INTERLEAVED
template <int LAYOUT, int DT>
__global__ __launch_bounds__(256) void k_resid_planes(const ResidArgs a)
{
    constexpr int SZ = OutT<DT>::size;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int uy = (a.crop_t >> 2) + blockIdx.y * 4 + threadIdx.y;      // the row of units this lane serves
    if (x0 >= a.w || uy >= a.h_scu || 4 * uy - a.crop_t >= a.h) return;
    const int n = min(8, a.w - x0);                                     // pixels of this lane in the row (even)
    const bool vec = a.aligned && n == 8;
    const int ub = (x0 + a.crop_l) >> 2, sub = (a.crop_l & 3) >> 1;     // sub = 1: the pixels start at the third sample of unit ub and end in unit ub + 2
    const bool live[3] = { true, true, sub != 0 };
    uint2 l[3][4];
    uint32_t cb[3][2], cr[3][2];
    resid_load_units<3>(a, ub, uy, live, l, cb, cr);

    #pragma unroll
    for (int r = 0; r < 4; r++) {
        const int y = 4 * uy + r - a.crop_t;
        if (y < 0 || y >= a.h) continue;
        // the row's sample pairs under the lane: luma pair j = pixels 2j, 2j + 1; chroma sample j = the one under that pair
        const uint32_t dl[6] = { l[0][r].x, l[0][r].y, l[1][r].x, l[1][r].y, l[2][r].x, l[2][r].y };
        const uint32_t db[3] = { cb[0][r >> 1], cb[1][r >> 1], cb[2][r >> 1] }, dr[3] = { cr[0][r >> 1], cr[1][r >> 1], cr[2][r >> 1] };
        int lv[8], bv[4], rv[4];
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t w = sub ? dl[j + 1] : dl[j];
            lv[2 * j] = s16_lo(w); lv[2 * j + 1] = s16_hi(w);
            const int q = j + 1;                                        // with sub: chroma sample j + 1 of the six
            const uint32_t wb = sub ? db[q >> 1] : db[j >> 1], wr = sub ? dr[q >> 1] : dr[j >> 1];
            const bool hi = sub ? (q & 1) : (j & 1);
            bv[j] = hi ? s16_hi(wb) : s16_lo(wb);
            rv[j] = hi ? s16_hi(wr) : s16_lo(wr);
        }
        if (LAYOUT == XGPU_RESID_YUV420) {
            uint32_t e[8];
            #pragma unroll
            for (int m = 0; m < 8; m++) e[m] = (uint32_t)(uint16_t)lv[m];
            store_run<8, 2>(a.dst + (size_t)y * a.pitch + (size_t)x0 * 2, e, vec, n);
            if (!(r & 1)) {                                             // the chroma row under luma rows r, r + 1 (crop_t is even: it is inside when they are)
                uint32_t eb[4], er[4];
                #pragma unroll
                for (int j = 0; j < 4; j++) { eb[j] = (uint32_t)(uint16_t)bv[j]; er[j] = (uint32_t)(uint16_t)rv[j]; }
                const size_t o = (size_t)(y >> 1) * a.pitch_c + (size_t)x0;      // x0 / 2 samples of 2 bytes
                store_run<4, 2>(a.dst + a.off_c[0] + o, eb, vec, n >> 1);
                store_run<4, 2>(a.dst + a.off_c[1] + o, er, vec, n >> 1);
            }
        } else {
            uint32_t ch[3][8];
            #pragma unroll
            for (int m = 0; m < 8; m++) {
                ch[0][m] = resid_elem<DT>(a, 0, lv[m]);
                ch[1][m] = resid_elem<DT>(a, 1, bv[m >> 1]);
                ch[2][m] = resid_elem<DT>(a, 2, rv[m >> 1]);
            }
            if (LAYOUT == XGPU_RESID_444_PLANAR) {
                uint8_t *d = a.dst + (size_t)y * a.pitch + (size_t)x0 * SZ;
                #pragma unroll
                for (int c = 0; c < 3; c++) store_run<8, SZ>(d + c * a.plane, ch[c], vec, n);
            } else {
                uint32_t e[24];
                #pragma unroll
                for (int m = 0; m < 8; m++) { e[3 * m] = ch[0][m]; e[3 * m + 1] = ch[1][m]; e[3 * m + 2] = ch[2][m]; }
                store_run<24, SZ>(a.dst + (size_t)y * a.pitch + (size_t)x0 * 3 * SZ, e, vec, 3 * n);
            }
        }
    }
}

__device__ __forceinline__ int abs_pair(uint32_t w) { return abs(s16_lo(w)) + abs(s16_hi(w)); }

__global__ __launch_bounds__(256) void k_resid_energy(const ResidArgs a)
{
    const int u0 = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int row = blockIdx.y * 4 + threadIdx.y;
    if (u0 >= a.w_scu || row >= a.h_scu) return;
    const int n = min(4, a.w_scu - u0);
    const bool vec = a.aligned && n == 4;
    const bool live[4] = { true, n > 1, n > 2, n > 3 };
    uint2 l[4][4];
    uint32_t cb[4][2], cr[4][2];
    resid_load_units<4>(a, u0, row, live, l, cb, cr);
    uint32_t e[3][4];
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        int sl = 0;
        #pragma unroll
        for (int r = 0; r < 4; r++) sl += abs_pair(l[k][r].x) + abs_pair(l[k][r].y);
        e[0][k] = __float_as_uint((float)sl);
        e[1][k] = __float_as_uint((float)(abs_pair(cb[k][0]) + abs_pair(cb[k][1])));
        e[2][k] = __float_as_uint((float)(abs_pair(cr[k][0]) + abs_pair(cr[k][1])));
    }
    uint8_t *d = a.dst + (size_t)row * a.pitch + (size_t)u0 * 4;
    #pragma unroll
    for (int c = 0; c < 3; c++) store_run<4, 4>(d + c * a.plane, e[c], vec, n);
}

// LAYOUT: any of the four.  One workgroup per chroma-only CU (whole-CU blocks: such a CU is intra-predicted)
template <int LAYOUT, int DT>
__global__ __launch_bounds__(256) void k_resid_chroma(const ResidArgs a)
{
    constexpr int SZ = OutT<DT>::size;
    const uint4 *p = (const uint4 *)(a.cus + a.chroma_cus[blockIdx.x]);
    const uint4 r0 = p[0];
    const int cu_x = r0.x & 0xFFFF, cu_y = r0.x >> 16;
    const int lw = r0.y & 7, lh = (r0.y >> 8) & 7, cbf = r0.y >> 24;
    const int cwc = 1 << (lw - 1);
    uint32_t off = r0.w + ((cbf & 1) ? 1u << (lw + lh) : 0u);
    for (int c = 1; c < 3; c++) {
        if (!((cbf >> c) & 1)) continue;
        const int16_t *blk = a.resid + off;
        off += 1u << (lw + lh - 2);
        if (LAYOUT == XGPU_RESID_YUV420) {
            for (int i = threadIdx.x; i < (1 << (lw + lh - 2)); i += 256) {
                const int ox = (cu_x >> 1) + (i & (cwc - 1)) - (a.crop_l >> 1), oy = (cu_y >> 1) + (i >> (lw - 1)) - (a.crop_t >> 1);
                if ((uint32_t)ox < (uint32_t)(a.w >> 1) && (uint32_t)oy < (uint32_t)(a.h >> 1))
                    *(uint16_t *)(a.dst + a.off_c[c - 1] + (size_t)oy * a.pitch_c + (size_t)ox * 2) = (uint16_t)blk[i];
            }
        } else if (LAYOUT == XGPU_RESID_ENERGY) {
            for (int i = threadIdx.x; i < (1 << (lw + lh - 4)); i += 256) {
                const int ux = i & ((1 << (lw - 2)) - 1), uyy = i >> (lw - 2);
                const int16_t *q = blk + (2 * uyy) * cwc + 2 * ux;
                const int s = abs((int)q[0]) + abs((int)q[1]) + abs((int)q[cwc]) + abs((int)q[cwc + 1]);
                *(float *)(a.dst + c * a.plane + (size_t)((cu_y >> 2) + uyy) * a.pitch + (size_t)((cu_x >> 2) + ux) * 4) = (float)s;
            }
        } else {
            for (int i = threadIdx.x; i < (1 << (lw + lh)); i += 256) {
                const int lx = i & ((1 << lw) - 1), ly = i >> lw;
                const int ox = cu_x + lx - a.crop_l, oy = cu_y + ly - a.crop_t;
                if ((uint32_t)ox >= (uint32_t)a.w || (uint32_t)oy >= (uint32_t)a.h) continue;
                const uint32_t e = resid_elem<DT>(a, c, (int)blk[(ly >> 1) * cwc + (lx >> 1)]);
                if (LAYOUT == XGPU_RESID_444_PLANAR) store_elem<SZ>(a.dst + c * a.plane + (size_t)oy * a.pitch + (size_t)ox * SZ, e);
                else                                 store_elem<SZ>(a.dst + (size_t)oy * a.pitch + ((size_t)ox * 3 + c) * SZ, e);
            }
        }
    }
}

template <int LAYOUT, int DT>
static void launch_resid_planes(const ResidArgs &a, hipStream_t s)
{
    const int unit_rows = ((a.h - 1 + a.crop_t) >> 2) - (a.crop_t >> 2) + 1;
    const dim3 grid((unsigned)(((a.w + 7) / 8 + 63) / 64), (unsigned)((unit_rows + 3) / 4));
    hipLaunchKernelGGL((k_resid_planes<LAYOUT, DT>), grid, dim3(64, 4), 0, s, a);
    if (a.n_chroma_cus) hipLaunchKernelGGL((k_resid_chroma<LAYOUT, DT>), dim3((unsigned)a.n_chroma_cus), dim3(256), 0, s, a);
}
template <int LAYOUT>
static void launch_resid_444(const ResidArgs &a, int dtype, hipStream_t s)
{
    if (dtype == XGPU_OUT_U16)      launch_resid_planes<LAYOUT, XGPU_OUT_U16>(a, s);
    else if (dtype == XGPU_OUT_F16) launch_resid_planes<LAYOUT, XGPU_OUT_F16>(a, s);
    else                            launch_resid_planes<LAYOUT, XGPU_OUT_F32>(a, s);
}

void launch_residual(const ResidArgs &a, int layout, int dtype, hipStream_t s)
{
    if (layout == XGPU_RESID_YUV420) launch_resid_planes<XGPU_RESID_YUV420, XGPU_OUT_U16>(a, s);
    else if (layout == XGPU_RESID_444_PLANAR) launch_resid_444<XGPU_RESID_444_PLANAR>(a, dtype, s);
    else if (layout == XGPU_RESID_444_INTERLEAVED) launch_resid_444<XGPU_RESID_444_INTERLEAVED>(a, dtype, s);
    else {
        const dim3 grid((unsigned)(((a.w_scu + 3) / 4 + 63) / 64), (unsigned)((a.h_scu + 3) / 4));
        hipLaunchKernelGGL(k_resid_energy, grid, dim3(64, 4), 0, s, a);
        if (a.n_chroma_cus) hipLaunchKernelGGL((k_resid_chroma<XGPU_RESID_ENERGY, XGPU_OUT_F32>), dim3((unsigned)a.n_chroma_cus), dim3(256), 0, s, a);
    }
}
