// k_side_info.hip - the coding side information of the picture decoded last, read out of the SCU map (xgpu_frame_side_info): the second product of a
// decoder next to the samples.  ScuRec (xgpu_internal.h) - one 16-byte record per 4x4 luma unit, written by k_inter (every CU), k_affine (sub-block vectors)
// and k_dmvr (refined vectors under the baseline filter) - is only read here; nothing in this file writes the map.  The contract is INTEGRATION.md section
// 8c; tests/side_info_ref.py restates it in numpy, bit for bit.
//
// k_side_blocks: the record taken apart into nine int16 planes of h_scu x w_scu.  A lane owns 8 consecutive units of a map row: eight 16-byte loads that are
// 128 contiguous bytes, and - when dst, the row pitch and the plane distance are multiples of 16 bytes - nine 16-byte stores; element stores otherwise and
// in a row's last group.  Units past the row's end are not loaded (the row behind the last one is not the map's).
//
// k_side_flow: a dense motion field at luma resolution, two channels (x, y) per requested list, in luma samples (optionally per unit of POC distance).  It
// writes 8 to 32 bytes per pixel and reads one byte: a lane owns 8 pixels of a row and the (up to) four output rows of one row of units, loads the two - with
// a left crop that is not a multiple of 4: three - records under its pixels once, and stores 16 bytes per row and channel when the alignment allows.
// The arithmetic is float32, every operation rounded on its own (no contraction): v = float(mv) * 0.25f, then one IEEE division by float(dpoc).
#pragma clang fp contract(off)
#include "output_common.h"

// POC distance of the reference a unit's list points at: refp_poc[refi][list] - poc, 0 for an unused list.  (An index the map cannot hold for a valid
// picture is clamped: the table has XGPU_MAX_REFS rows.)
__device__ __forceinline__ int side_dpoc(const SideArgs &a, int refi, int list)
{
    return refi < 0 ? 0 : a.refp_poc[min(refi, XGPU_MAX_REFS - 1)][list] - a.poc;
}
__device__ __forceinline__ int sat16(int v) { return min(max(v, -32768), 32767); }

__global__ __launch_bounds__(256) void k_side_blocks(const SideArgs a)
{
    const int u0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int row = blockIdx.y * 4 + threadIdx.y;
    if (u0 >= a.w_scu || row >= a.h_scu) return;
    const int n = min(8, a.w_scu - u0);
    const bool vec = a.aligned && n == 8;
    const uint4 *src = (const uint4 *)(a.maps + (size_t)row * a.w_scu + u0);
    uint4 r[8];
    #pragma unroll
    for (int k = 0; k < 8; k++) r[k] = k < n ? src[k] : make_uint4(0, 0, 0, 0);

    uint32_t pl[9][8];
    #pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t m = r[k].x;
        const int refi0 = (int)(int8_t)(r[k].y & 0xFF), refi1 = (int)(int8_t)((r[k].y >> 8) & 0xFF);
        pl[0][k] = r[k].z & 0xFFFFu; pl[1][k] = r[k].z >> 16;
        pl[2][k] = r[k].w & 0xFFFFu; pl[3][k] = r[k].w >> 16;
        pl[4][k] = (uint32_t)(uint16_t)sat16(side_dpoc(a, refi0, 0));
        pl[5][k] = (uint32_t)(uint16_t)sat16(side_dpoc(a, refi1, 1));
        pl[6][k] = ((m >> 15) & 1) ? XGPU_MODE_INTRA : ((m >> 26) & 1) ? XGPU_MODE_IBC : ((m >> 23) & 1) ? XGPU_MODE_SKIP : XGPU_MODE_INTER;
        pl[7][k] = (m >> 16) & 0x7Fu;
        pl[8][k] = ((m >> 24) & 1u) | ((m & SCU_EDGE_L) ? 2u : 0u) | ((m & SCU_EDGE_T) ? 4u : 0u) | ((r[k].y >> 16) ? 8u : 0u);
    }
    uint8_t *d = a.dst + (size_t)row * a.pitch + (size_t)u0 * 2;
    #pragma unroll
    for (int p = 0; p < 9; p++) store_run<8, 2>(d + p * a.plane, pl[p], vec, n);
}

void launch_side_blocks(const SideArgs &a, hipStream_t s)
{
    const dim3 grid((unsigned)(((a.w_scu + 7) / 8 + 63) / 64), (unsigned)((a.h_scu + 3) / 4));
    hipLaunchKernelGGL(k_side_blocks, grid, dim3(64, 4), 0, s, a);
}

// NL: number of lists written (1: list a.list0, 2: both)
template <bool PLANAR, int DT, int NL>
__global__ __launch_bounds__(256) void k_side_flow(const SideArgs a)
{
    constexpr int SZ = OutT<DT>::size, C = 2 * NL;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int uy = (a.crop_t >> 2) + blockIdx.y * 4 + threadIdx.y;      // the row of units this lane serves
    const int y_first = max(4 * uy - a.crop_t, 0), y_end = min(4 * uy - a.crop_t + 4, a.h);      // its output rows
    if (x0 >= a.w || y_first >= y_end) return;
    const int n = min(8, a.w - x0);
    const bool vec = a.aligned && n == 8;

    // the records under pixels x0 .. x0 + 7: unit columns ub .. ub + 2 (the third only with a left crop of 4k + 2); clamped to the row for a row's last group
    const int ub = (x0 + a.crop_l) >> 2, sub = a.crop_l & 3;
    const ScuRec *row = a.maps + (size_t)uy * a.w_scu;
    uint32_t val[3][C];
    #pragma unroll
    for (int k = 0; k < 3; k++) {
        if (k == 2 && sub == 0) {
            #pragma unroll
            for (int ch = 0; ch < C; ch++) val[2][ch] = 0;
            break;
        }
        const uint4 r = *(const uint4 *)(row + min(ub + k, a.w_scu - 1));
        #pragma unroll
        for (int j = 0; j < NL; j++) {
            const int l = NL == 2 ? j : a.list0;
            const int refi = (int)(int8_t)((r.y >> (8 * l)) & 0xFF);
            const uint32_t mv = l ? r.w : r.z;
            float vx = 0.f, vy = 0.f;
            if (refi >= 0) {
                vx = (float)(int)(int16_t)(mv & 0xFFFFu) * 0.25f;
                vy = (float)(int)(int16_t)(mv >> 16) * 0.25f;
                if (a.per_poc) {
                    const float dp = (float)side_dpoc(a, refi, l);
                    vx = vx / dp; vy = vy / dp;
                }
            }
            val[k][2 * j] = fbits<DT>(vx); val[k][2 * j + 1] = fbits<DT>(vy);
        }
    }
    uint32_t px[C][8];
    #pragma unroll
    for (int m = 0; m < 8; m++) {
        const int k = (m + sub) >> 2;      // sub is 0 or 2: k = 0, 1 - or 2 for the last two pixels with sub = 2
        #pragma unroll
        for (int ch = 0; ch < C; ch++) px[ch][m] = k == 0 ? val[0][ch] : k == 1 ? val[1][ch] : val[2][ch];
    }
    for (int y = y_first; y < y_end; y++) {
        if (PLANAR) {
            uint8_t *d = a.dst + (size_t)y * a.pitch + (size_t)x0 * SZ;
            #pragma unroll
            for (int ch = 0; ch < C; ch++) store_run<8, SZ>(d + ch * a.plane, px[ch], vec, n);
        } else {
            uint32_t e[8 * C];
            #pragma unroll
            for (int m = 0; m < 8; m++) {
                #pragma unroll
                for (int ch = 0; ch < C; ch++) e[C * m + ch] = px[ch][m];
            }
            store_run<8 * C, SZ>(a.dst + (size_t)y * a.pitch + (size_t)x0 * C * SZ, e, vec, C * n);
        }
    }
}

template <bool PLANAR, int DT>
static void launch_flow_dt(const SideArgs &a, int n_lists, dim3 grid, hipStream_t s)
{
    if (n_lists == 2) hipLaunchKernelGGL((k_side_flow<PLANAR, DT, 2>), grid, dim3(64, 4), 0, s, a);
    else              hipLaunchKernelGGL((k_side_flow<PLANAR, DT, 1>), grid, dim3(64, 4), 0, s, a);
}

void launch_side_flow(const SideArgs &a, bool planar, int dtype, int n_lists, hipStream_t s)
{
    const int unit_rows = ((a.h - 1 + a.crop_t) >> 2) - (a.crop_t >> 2) + 1;
    const dim3 grid((unsigned)(((a.w + 7) / 8 + 63) / 64), (unsigned)((unit_rows + 3) / 4));
    if (planar) { if (dtype == XGPU_OUT_F16) launch_flow_dt<true, XGPU_OUT_F16>(a, n_lists, grid, s); else launch_flow_dt<true, XGPU_OUT_F32>(a, n_lists, grid, s); }
    else        { if (dtype == XGPU_OUT_F16) launch_flow_dt<false, XGPU_OUT_F16>(a, n_lists, grid, s); else launch_flow_dt<false, XGPU_OUT_F32>(a, n_lists, grid, s); }
}
