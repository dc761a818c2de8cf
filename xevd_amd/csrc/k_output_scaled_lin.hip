// k_output_scaled_lin.hip - the scaled outputs filtered in linear light: a decoded 4:2:0 picture (or a batch of its rectangles) resized to the caller's size by
// filtering the linear-light R, G, B of the source primaries, then taken to the caller's colour space, normalised, in the caller's device memory
// (xgpu_pic_output_device_scaled_lin, xgpu_pic_output_device_rois_lin).  k_output_scaled_cm.hip filters the encoded Y'CbCr samples and transforms the result, which
// darkens fine high-contrast detail of a PQ / HLG picture the more it is reduced; here the mean of a black and a white stripe is half the white's light.  The
// contract is INTEGRATION.md section 8n and tests/scaled_lin_ref.py restates it: every float32 multiply and add is rounded on its own (no contraction into FMA),
// the taps are summed in ascending order, the accumulator starts as the first product.
//
// Two passes over a float32 intermediate at luma width - R, G, B planes of [rows][align8(Ws)] - with the 14-bit luma taps of xgpu_scale_taps for all three channels:
//   k_lin_vertical / k_lin_rois_vertical       T_c(x, o) = sum_k float(qy[o][k]) * lin[code_c(x, first[o] + k)]
//     Lanes walk columns and a wave keeps one destination row, as in k_scale_vertical: row index, tap row and weight are scalar.  A lane makes the 8 pixels from x0
//     of every tap row the way the full-size output makes them - output_common.h's chroma_row for the edge-clamped, DRA-mapped chroma samples, the vertical and
//     horizontal quarter weights of three_channel_rows for one luma row instead of a pair (a tap range starts and ends at any row) - then cm_transform.h's
//     cm_linearise, and keeps 24 float accumulators.  The lin table (4 KB at 10 bit, 16 KB at 12) is copied into LDS by every workgroup: a workgroup converts
//     4 x 512 pixels per tap row, tens of thousands in all, and three lookups per pixel sit on the pass' critical path (DESIGN.md section 5c has the measurement
//     against reading it from global memory; the instances that did were dropped after it).
//   k_lin_horizontal / k_lin_rois_horizontal   V_c(ox, o) = (sum_k float(qx[ox][k]) * T_c(first[ox] + k, o)) * 2^-28, then cm_from_linear, scaled_finish, store_pixel
//     The bodies are k_scale_horizontal's and k_rois_horizontal's (output_resize.h) with LinRow and LinPixel below.
//     A workgroup is 64 destination columns x `rows` destination rows, one wave per row, one lane per pixel, as in k_scale_horizontal.  Each wave stages the float
//     spans of all three channels of its row in LDS: 12 bytes per source column where the plain pass has 4.  The group stays 64 columns wide and the three
//     channels are filtered together (one weight load and one index per tap for three products); `rows` is 4, 2 or 1 by the plain passes' 48 KB rule.  At the
//     limit ratio (Ws = 64 Wd) the 64 columns of a group reach 63 x 64 + 128 source columns and their 8-sample alignment: under 4200 floats per channel, 50 KB for
//     one row - more than 48 KB, so that rule ends at one row, and under the 64 KB a plain launch may request, which the host checks before it queues anything.
//     The tone and encode tables are read from global memory, as in k_output_scaled_cm.hip and for its reason.
#pragma clang fp contract(off)
#include "cm_transform.h"
#include "output_resize.h"

// the lin table a workgroup of 64 x 4 reads: copied into LDS by all of its threads
__device__ __forceinline__ const float *lin_fill_lds(const CmParams &p, float *lds)
{
    for (int i = threadIdx.y * 64 + threadIdx.x; i < p.n_lin; i += 256) lds[i] = p.lin[i];
    __syncthreads();
    return lds;
}

// linear light of the 8 pixels from x0 of luma row `row` of the source g (x0 < g.w, row < g.h): three_channel_rows' pixels of one row, through cm_linearise.
// Every sample is clipped to [0, 2^B - 1] behind its DRA mapping, as in the other scaled outputs (g.maxv: the U16 form's, 2^B - 1); a decoded sample is inside
// already, so without DRA these are the full-size output's pixels.
template <int UP>
__device__ __forceinline__ void lin_row(const RgbOutArgs &g, const float *lin, int x0, int row, float (&L)[3][8])
{
    const int i = row >> 1, par = row & 1, j0 = x0 >> 1;
    int cv[2][6];      // chroma, vertically interpolated for this row's parity: columns j0-1+k
    #pragma unroll
    for (int c = 0; c < 2; c++) {
        int r0[6];
        chroma_row(g, c + 1, i, j0, r0);
        #pragma unroll
        for (int k = 0; k < 6; k++) r0[k] = min(max(r0[k], 0), g.maxv);
        if (UP == XGPU_UPSAMPLE_NEAREST) {
            #pragma unroll
            for (int k = 0; k < 6; k++) cv[c][k] = r0[k];
        } else {      // even rows: ve[0] * row (i-1) + ve[1] * row i; odd rows: vo[0] * row i + vo[1] * row (i+1)
            int r1[6];
            chroma_row(g, c + 1, par ? min(i + 1, g.ch - 1) : max(i - 1, 0), j0, r1);
            #pragma unroll
            for (int k = 0; k < 6; k++) r1[k] = min(max(r1[k], 0), g.maxv);
            const int w0 = par ? g.vo[0] : g.ve[1], w1 = par ? g.vo[1] : g.ve[0];
            #pragma unroll
            for (int k = 0; k < 6; k++) cv[c][k] = w0 * r0[k] + w1 * r1[k];
        }
    }
    const S16x8u ly = *(const S16x8u *)(g.y + (size_t)row * g.sy + x0);
    #pragma unroll
    for (int m = 0; m < 8; m++) {
        int y = ly.v[m];
        if (g.dra) y = dra1(g.dra, 0, y, 0);
        y = min(max(y, 0), g.maxv);
        const int jj = m >> 1;                // chroma column j0 + jj = index jj + 1
        int cc[2];
        #pragma unroll
        for (int c = 0; c < 2; c++) {
            if (UP == XGPU_UPSAMPLE_NEAREST) cc[c] = cv[c][jj + 1];
            else if (m & 1) cc[c] = ((2 + g.hc) * cv[c][jj + 1] + (2 - g.hc) * cv[c][jj + 2] + 8) >> 4;
            else            cc[c] = (g.hc * cv[c][jj] + (4 - g.hc) * cv[c][jj + 1] + 8) >> 4;
        }
        cm_linearise(g, lin, y, cc[0], cc[1], L[0][m], L[1][m], L[2][m]);
    }
}

// Vertical pass, one lane: 8 neighbouring columns from x0 of one destination row - `cnt` source rows from `first` with the weights q; d: where the 8 results of R
// go, G and B `plane` floats further each
template <int UP>
__device__ __forceinline__ void lin_vertical_lane(const RgbOutArgs &g, const float *lin, int first, int cnt, const int16_t *q, int x0, float *d, size_t plane)
{
    float acc[3][8];
    #pragma unroll
    for (int c = 0; c < 3; c++) {
        #pragma unroll
        for (int m = 0; m < 8; m++) acc[c][m] = 0.f;
    }
    for (int k = 0; k < cnt; k++) {
        const float qk = (float)q[k];
        float L[3][8];
        lin_row<UP>(g, lin, x0, first + k, L);
        #pragma unroll
        for (int c = 0; c < 3; c++) {
            #pragma unroll
            for (int m = 0; m < 8; m++) { const float p = qk * L[c][m]; acc[c][m] = k ? acc[c][m] + p : p; }
        }
    }
    #pragma unroll
    for (int c = 0; c < 3; c++) {
        *(float4 *)(d + c * plane) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
        *(float4 *)(d + c * plane + 4) = make_float4(acc[c][4], acc[c][5], acc[c][6], acc[c][7]);
    }
}

template <int UP>
__global__ __launch_bounds__(256) void k_lin_vertical(const ScaledCmOutArgs a)
{
    extern __shared__ float lin_lds[];
    const float *lin = lin_fill_lds(a.cm, lin_lds);      // (every thread of the workgroup, before the lanes outside the picture leave)
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int o = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y);      // one destination row per wave
    if (x0 >= a.w || o >= a.dh) return;
    lin_vertical_lane<UP>(a, lin, a.yl.first[o], a.yl.count[o], a.yl.w + (size_t)o * a.yl.stride, x0, (float *)a.mid + (size_t)o * a.mpy + x0, (size_t)a.dh * a.mpy);
}

// the same with the rectangle taken from blockIdx.z: the source is the rectangle, so the chroma clamp and every tap end at its edge
template <int UP>
__global__ __launch_bounds__(256) void k_lin_rois_vertical(const RoisCmOutArgs a)
{
    extern __shared__ float lin_lds[];
    const RoiDesc &d = ((const RoiDesc *)a.blk)[blockIdx.z];
    if ((int)(blockIdx.x * 512) >= d.w || (int)(blockIdx.y * 4) >= d.ih) return;      // a workgroup past a smaller rectangle: all of it leaves, before the copy
    const float *lin = lin_fill_lds(a.cm, lin_lds);
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int o = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y);
    if (x0 >= d.w || o >= d.ih) return;
    RgbOutArgs g = a;
    g.y = a.y + (size_t)d.y * a.sy + d.x;
    g.u = a.u + (size_t)(d.y >> 1) * a.sc + (d.x >> 1);
    g.v = a.v + (size_t)(d.y >> 1) * a.sc + (d.x >> 1);
    g.w = d.w; g.h = d.h; g.cw = d.w >> 1; g.ch = d.h >> 1;
    const ScaleTaps t = roi_taps(a.blk, d, 0);
    lin_vertical_lane<UP>(g, lin, t.first[o], t.count[o], t.w + (size_t)o * t.stride, x0, (float *)a.mid + d.mid + (size_t)o * d.mpy + x0, (size_t)d.ih * d.mpy);
}


// The row of the horizontal pass (output_resize.h's ROW): the float spans of R, G, B of one row, `cap` floats apart in the wave's part of LDS, under the luma taps
struct LinRow {
    typedef float Value;
    static size_t row_bytes(int capy, int) { return (size_t)3 * capy * sizeof(float); }
    const ScaleTaps &xl;
    float *l;
    int cap, s0, s1;
    __device__ __forceinline__ LinRow(void *lds, int capy, int, const ScaleTaps &xl_, const ScaleTaps &, int o0, int o1) : xl(xl_), cap(capy)
    {
        l = (float *)lds + (size_t)threadIdx.y * 3 * capy;
        s0 = xl.first[o0] & ~7; s1 = xl.first[o1] + xl.count[o1];
    }
    // the span [s0, s1) of the row of every channel (s0 a multiple of 8), 4 floats per lane and step
    __device__ __forceinline__ void stage(const uint16_t *mid, uint32_t off, int rows, int mpy, int, int row) const
    {
        const float *m = (const float *)mid + off + (size_t)row * mpy;
        #pragma unroll
        for (int c = 0; c < 3; c++) {
            const float *mc = m + (size_t)c * rows * mpy;
            for (int i = threadIdx.x * 4; i < s1 - s0; i += 256) *(float4 *)(l + c * cap + i) = *(const float4 *)(mc + s0 + i);
        }
    }
    // destination column o of the staged row: v[c] = (sum qx * t_c) * 2^-28
    __device__ __forceinline__ void column(int o, int, float (&v)[3]) const
    {
        const float *p = l + (xl.first[o] - s0);
        const int16_t *q = xl.w + o;
        const int n = xl.count[o];
        float acc[3] = { 0.f, 0.f, 0.f };
        for (int k = 0; k < n; k++) {
            const float qk = (float)q[(size_t)k * xl.stride];
            #pragma unroll
            for (int c = 0; c < 3; c++) { const float t = qk * p[c * cap + k]; acc[c] = k ? acc[c] + t : t; }
        }
        #pragma unroll
        for (int c = 0; c < 3; c++) v[c] = acc[c] * 0x1p-28f;
    }
};
// one filtered pixel -> the bits of its three elements in output order: the rest of the transform (for the float dtypes its F32 instance, so that the normalise
// sees the clipped float32), then scaled_finish
struct LinPixel {
    template <int DT, class A> __device__ static __forceinline__ void apply(const A &a, const float (&v)[3], uint32_t (&e)[3])
    {
        const CmTables t = { a.cm.lin, a.cm.tone, a.cm.enc };
        cm_from_linear<OutT<DT>::is_float ? XGPU_OUT_F32 : DT>(a.cm, t, v[0], v[1], v[2], e[0], e[1], e[2]);
        scaled_finish<DT>(a, e);
    }
};

template <bool PLANAR, int DT>
__global__ __launch_bounds__(256) void k_lin_horizontal(const ScaledCmOutArgs a)
{
    scale_horizontal<LinRow, LinPixel, PLANAR, DT>(a);
}
// k_rois_horizontal_cm over the float intermediate
template <bool PLANAR, int DT>
__global__ __launch_bounds__(256) void k_lin_rois_horizontal(const RoisCmOutArgs a)
{
    rois_horizontal<LinRow, LinPixel, false, PLANAR, DT>(a);
}
struct LinHorizontal     { template <bool PLANAR, bool RGB, int DT> static auto kernel() { return k_lin_horizontal<PLANAR, DT>; } };
struct LinRoisHorizontal { template <bool PLANAR, bool RGB, int DT> static auto kernel() { return k_lin_rois_horizontal<PLANAR, DT>; } };

void launch_output_scaled_lin(const ScaledCmOutArgs &a, int layout, int dtype, int upsample, hipStream_t s)
{
    const dim3 grid = vertical_grid(a.w, a.dh, 1u), block(64, 4);
    const size_t lds = sizeof(float) * a.cm.n_lin;
    if (upsample == XGPU_UPSAMPLE_NEAREST) hipLaunchKernelGGL(k_lin_vertical<XGPU_UPSAMPLE_NEAREST>, grid, block, lds, s, a);
    else                                   hipLaunchKernelGGL(k_lin_vertical<XGPU_UPSAMPLE_LINEAR>, grid, block, lds, s, a);
    launch_horizontal<LinHorizontal, LinRow>(a, layout, dtype, 1u, s);
}

// max_w: the widest rectangle; max_ih: the tallest inner part
void launch_output_rois_lin(const RoisCmOutArgs &a, int layout, int dtype, int upsample, int max_w, int max_ih, hipStream_t s)
{
    const dim3 grid = vertical_grid(max_w, max_ih, (unsigned)a.n), block(64, 4);
    const size_t lds = sizeof(float) * a.cm.n_lin;
    if (upsample == XGPU_UPSAMPLE_NEAREST) hipLaunchKernelGGL(k_lin_rois_vertical<XGPU_UPSAMPLE_NEAREST>, grid, block, lds, s, a);
    else                                   hipLaunchKernelGGL(k_lin_rois_vertical<XGPU_UPSAMPLE_LINEAR>, grid, block, lds, s, a);
    launch_horizontal<LinRoisHorizontal, LinRow>(a, layout, dtype, (unsigned)a.n, s);
}
