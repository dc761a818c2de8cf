// k_output_remap.hip - n coordinate grids of one decoded picture, each giving one dw x dh image whose every pixel reads the source at a position of its own, converted
// and normalised like the scaled output, as a batch of images in the caller's device memory (xgpu_pic_output_device_remap): lens
// undistortion, fisheye dewarping into virtual views, perspective maps, the previous picture pulled through a flow field.  tests/remap_ref.py restates the
// contract in numpy int64.
//
// One kernel, grid (dw / 64, dh / 4, n), block (64, 4): one destination pixel per lane, one destination row per wave, one grid per workgroup - the warp's shape.
//   A node is 8 bytes, (x, y) as int32 Q16 or as float32 luma samples; remap_node brings either to Q16 with INT32_MIN in x for "invalid" (a converted float is
//   within +-32767 << 16, so the marker is free), and every later step is the same for both formats.
//   MESH = false (step_log2 = 0): the pixel's node is one coalesced 8-byte load per lane; with S > 1 four more give the two differences.
//   MESH = true  (step_log2 = k >= 1): the 64 x 4 pixels of a workgroup lie in (64 >> k) + 1 columns and 2 (k = 1: 3) rows of nodes, at most 33 x 3.  Lane
//   (column, row) of the block loads and converts node (row, column) of that patch ONCE into 792 bytes of LDS; after one barrier every lane reads the four nodes
//   of its cell from there and interpolates position and derivatives in int64, exactly (weights below 2^12, nodes below 2^31).  No node index beyond gw - 1,
//   gh - 1 is formed: the patch is cut at the grid's edge, and a pixel inside the image never needs more.
//   (The other staging - every lane fetching its four nodes from global memory, converting each - is the #if branch below; it was measured once)
//   From (X, Y) and the derivatives on, the arithmetic is k_output_warp's with D0, D1 in place of the map's linear part: S x S sub-positions, the bilinear gather
//   of output_common.h (every position clamped to the plane before it becomes an index, whatever the grid holds), DRA and clip per source sample, the rounding
//   shift, scaled_pixel, store_pixel.  A pixel with an invalid node among those its formulas read is pad under either border mode.  No intermediate, no context buffer.
#pragma clang fp contract(off)
#include "output_common.h"

#ifndef XGPU_REMAP_NODES_FROM_GLOBAL
#define XGPU_REMAP_NODES_FROM_GLOBAL 0
#endif

// node (j, i) of grid g (inside the grid) -> Q16, x = INT32_MIN: invalid
__device__ __forceinline__ int2 remap_node(const RemapOutArgs &a, const int2 *g, int j, int i)
{
    int2 r = g[(size_t)j * a.gw + i];
    if (a.f32) {
        const float vx = __int_as_float(r.x), vy = __int_as_float(r.y);
        const bool ok = __builtin_isfinite(vx) && __builtin_isfinite(vy);
        r.x = ok ? (int)rintf(fminf(fmaxf(vx, -32767.0f), 32767.0f) * 65536.0f) : INT32_MIN;
        r.y = ok ? (int)rintf(fminf(fmaxf(vy, -32767.0f), 32767.0f) * 65536.0f) : 0;
    } else if (r.y == INT32_MIN) {
        r.x = INT32_MIN;
    }
    return r;
}
// one axis of a cell: position and the two derivatives from its four nodes, all exact in int64
__device__ __forceinline__ void remap_cell(int v00, int v01, int v10, int v11, int M, int fx, int fy, int k2, bool ss, int64_t &p, int64_t &d0, int64_t &d1)
{
    const int64_t rnd = (int64_t)1 << (k2 - 1);
    p = ((int64_t)((M - fx) * (M - fy)) * v00 + (int64_t)(fx * (M - fy)) * v01 + (int64_t)((M - fx) * fy) * v10 + (int64_t)(fx * fy) * v11 + rnd) >> k2;
    if (ss) {
        d0 = ((int64_t)(M - fy) * ((int64_t)v01 - v00) + (int64_t)fy * ((int64_t)v11 - v10) + rnd) >> k2;
        d1 = ((int64_t)(M - fx) * ((int64_t)v10 - v00) + (int64_t)fx * ((int64_t)v11 - v01) + rnd) >> k2;
    }
}

template <bool PLANAR, int DT, template <int> class CONV, bool SS, bool MESH>
__global__ __launch_bounds__(256) void k_output_remap(const RemapOutArgs a)
{
    constexpr int SZ = OutT<DT>::size;
    const int z = blockIdx.z;
    const int2 *g = (const int2 *)(a.grid + (size_t)z * a.grid_pitch);      // uniform per workgroup
    const int oy = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y), ox = blockIdx.x * 64 + (int)threadIdx.x;
    int64_t X, Y, D0x = 0, D0y = 0, D1x = 0, D1y = 0;
    bool ok;
    if (MESH) {
        const int k = a.k, M = 1 << k, fx = ox & (M - 1), fy = oy & (M - 1);
        int2 p00, p01, p10, p11;
#if XGPU_REMAP_NODES_FROM_GLOBAL
        if (oy >= a.dh || ox >= a.dw) return;
        const int i = ox >> k, j = oy >> k;
        p00 = remap_node(a, g, j, i); p01 = remap_node(a, g, j, i + 1); p10 = remap_node(a, g, j + 1, i); p11 = remap_node(a, g, j + 1, i + 1);
#else
        __shared__ int2 nodes[3 * 33];
        const int i0 = (int)(blockIdx.x * 64) >> k, j0 = (int)(blockIdx.y * 4) >> k, nc = (64 >> k) + 1, nr = k == 1 ? 3 : 2;
        const int tc = (int)threadIdx.x, tr = (int)threadIdx.y;
        if (tc < nc && tr < nr && i0 + tc < a.gw && j0 + tr < a.gh) nodes[tr * nc + tc] = remap_node(a, g, j0 + tr, i0 + tc);
        __syncthreads();
        if (oy >= a.dh || ox >= a.dw) return;
        const int at = ((oy >> k) - j0) * nc + (ox >> k) - i0;      // at most (nr - 2) * nc + nc - 2: the cell's far corner is the patch's last node
        p00 = nodes[at]; p01 = nodes[at + 1]; p10 = nodes[at + nc]; p11 = nodes[at + nc + 1];
#endif
        ok = p00.x != INT32_MIN && p01.x != INT32_MIN && p10.x != INT32_MIN && p11.x != INT32_MIN;
        remap_cell(p00.x, p01.x, p10.x, p11.x, M, fx, fy, 2 * k, SS, X, D0x, D1x);
        remap_cell(p00.y, p01.y, p10.y, p11.y, M, fx, fy, 2 * k, SS, Y, D0y, D1y);
    } else {
        if (oy >= a.dh || ox >= a.dw) return;
        const int2 p = remap_node(a, g, oy, ox);
        ok = p.x != INT32_MIN;
        X = p.x; Y = p.y;
        if (SS) {      // the differences along the row and the column, one-sided at the last column and row (dw, dh >= 2)
            const int xa = min(ox, a.dw - 2), ya = min(oy, a.dh - 2);
            const int2 l = remap_node(a, g, oy, xa), r = remap_node(a, g, oy, xa + 1), t = remap_node(a, g, ya, ox), b = remap_node(a, g, ya + 1, ox);
            ok = ok && l.x != INT32_MIN && r.x != INT32_MIN && t.x != INT32_MIN && b.x != INT32_MIN;
            D0x = (int64_t)r.x - l.x; D0y = (int64_t)r.y - l.y;
            D1x = (int64_t)b.x - t.x; D1y = (int64_t)b.y - t.y;
        }
    }
    const int xtop = (a.w - 1) << 8, ytop = (a.h - 1) << 8, xctop = (a.cw - 1) << 8, yctop = (a.ch - 1) << 8;
    bool in = ok;
    if (a.border == XGPU_WARP_PAD) {      // the pixel's own position, before supersampling and before the clamp
        const int64_t x0 = (X + 128) >> 8, y0 = (Y + 128) >> 8;
        in = in && x0 >= 0 && x0 <= xtop && y0 >= 0 && y0 <= ytop;
    }
    uint32_t e[3];
    if (in) {
        const uint64_t cx = (uint64_t)(int64_t)(256 - a.sh * 32768), cy = (uint64_t)(int64_t)(256 - a.sv * 32768);
        const int S = SS ? 1 << a.ls : 1;
        uint32_t acc[3] = { 0, 0, 0 };
        for (int q = 0; q < S * S; q++) {
            int64_t Xs = X, Ys = Y;
            if (SS) {      // sub-position (i, j): uniform per workgroup
                const int64_t ci = 2 * (q & (S - 1)) + 1 - S, cj = 2 * (q >> a.ls) + 1 - S;
                Xs += (D0x * ci + D1x * cj) >> (a.ls + 1);
                Ys += (D0y * ci + D1y * cj) >> (a.ls + 1);
            }
            acc[0] += warp_bilinear(a, 0, a.y, a.sy, a.w, a.h, warp_q8((uint64_t)Xs, 128, 8, xtop), warp_q8((uint64_t)Ys, 128, 8, ytop));
            const int xc = warp_q8((uint64_t)Xs, cx, 9, xctop), yc = warp_q8((uint64_t)Ys, cy, 9, yctop);
            acc[1] += warp_bilinear(a, 1, a.u, a.sc, a.cw, a.ch, xc, yc);
            acc[2] += warp_bilinear(a, 2, a.v, a.sc, a.cw, a.ch, xc, yc);
        }
        const int sh = 16 + (SS ? 2 * a.ls : 0);
        scaled_pixel<DT, CONV>(a, (int)((acc[0] + (1u << (sh - 1))) >> sh), (int)((acc[1] + (1u << (sh - 1))) >> sh), (int)((acc[2] + (1u << (sh - 1))) >> sh), e);
    } else {
        #pragma unroll
        for (int c = 0; c < 3; c++) e[c] = OutT<DT>::is_float ? scaled_float_elem<DT>(a, c, a.padv[c]) : (uint32_t)(int)a.padv[c];
    }
    store_pixel<PLANAR, SZ>(a.dst + (size_t)z * a.image_pitch + (size_t)oy * a.pitch, a.plane, ox, e);
}

template <bool PLANAR, int DT, template <int> class CONV>
static void launch_remap_ss(const RemapOutArgs &a, dim3 grid, hipStream_t s)
{
    if (a.k) {
        if (a.ls) hipLaunchKernelGGL((k_output_remap<PLANAR, DT, CONV, true, true>), grid, dim3(64, 4), 0, s, a);
        else      hipLaunchKernelGGL((k_output_remap<PLANAR, DT, CONV, false, true>), grid, dim3(64, 4), 0, s, a);
    } else {
        if (a.ls) hipLaunchKernelGGL((k_output_remap<PLANAR, DT, CONV, true, false>), grid, dim3(64, 4), 0, s, a);
        else      hipLaunchKernelGGL((k_output_remap<PLANAR, DT, CONV, false, false>), grid, dim3(64, 4), 0, s, a);
    }
}
template <bool PLANAR, template <int> class CONV>
static void launch_remap_dt(const RemapOutArgs &a, int dtype, dim3 grid, hipStream_t s)
{
    switch (dtype) {
    case XGPU_OUT_U8:   launch_remap_ss<PLANAR, XGPU_OUT_U8, CONV>(a, grid, s); break;
    case XGPU_OUT_U16:  launch_remap_ss<PLANAR, XGPU_OUT_U16, CONV>(a, grid, s); break;
    case XGPU_OUT_F16:  launch_remap_ss<PLANAR, XGPU_OUT_F16, CONV>(a, grid, s); break;
    case XGPU_OUT_BF16: launch_remap_ss<PLANAR, XGPU_OUT_BF16, CONV>(a, grid, s); break;
    default:            launch_remap_ss<PLANAR, XGPU_OUT_F32, CONV>(a, grid, s); break;
    }
}

void launch_output_remap(const RemapOutArgs &a, int layout, int dtype, hipStream_t s)
{
    const dim3 grid((unsigned)((a.dw + 63) / 64), (unsigned)((a.dh + 3) / 4), (unsigned)a.n);
    const bool planar = layout == XGPU_OUT_RGB_PLANAR || layout == XGPU_OUT_YUV444_PLANAR;
    const bool rgb = layout == XGPU_OUT_RGB_PLANAR || layout == XGPU_OUT_RGB_INTERLEAVED;
    if (rgb) { if (planar) launch_remap_dt<true, RgbConv>(a, dtype, grid, s); else launch_remap_dt<false, RgbConv>(a, dtype, grid, s); }
    else     { if (planar) launch_remap_dt<true, YuvConv>(a, dtype, grid, s); else launch_remap_dt<false, YuvConv>(a, dtype, grid, s); }
}
