// k_output_dither.hip - the integer device outputs with an ordered or blue-noise dither in place of the final rounding (xgpu_pic_output_device_dithered,
// xgpu_pic_output_device_packed_dithered): out = clip(floor(v + r / L)) with r the rank of the pixel's position in the call's matrix.  The contract is
// INTEGRATION.md section 8r; tests/dither_ref.py restates it in numpy.  Only integer dtypes are built here, so a second kernel around the same integer source
// is exact (k_output_packed.hip's note on float contraction does not bite), and the transform keeps contraction off as k_output_cm.hip does.
//
// k_output_dither_rgb: k_output_packed_rgb's shape - 64 x 4 lanes, 8 pixels of two luma rows per lane, three_channel_rows (output_common.h) for load, edge clamp,
// DRA and chroma upsampling, the same code.  three_channel_rows hands its CONV no position, and it stays as it is: the CONVs here stop one step short of the
// quantisation - the matrix' three sums without the rounding constant (DitherSumConv), or the transform's three float32 values q in [0, 1] (cm_apply's F32
// instance) - and the sink, which knows row and column, fetches the lane's 8 ranks of that row and finishes: (sum + (r << (S - k))) >> S clipped, or
// min(rd(q * outmax + r / L), outmax).  Sinks: the planar and the interleaved RGB image, RGBA, 10:10:10:2.
//
// k_output_dither_semiplanar: k_output_semiplanar's shape - 16 luma columns of two rows and 8 + 8 chroma samples per lane - with conv1's rounding constant
// replaced by (r << shift) >> k.  A chroma sample's rank is that of its chroma-plane position; Cb and Cr share it.
//
// The ranks are read from global memory: a slot's rows are extended by their own first 16 entries (DitherSlot), so a lane's run of 8 or 16 ranks from any phase
// is one contiguous 16- or 32-byte load at 2-byte alignment.  A workgroup reads 8 matrix rows of at most 288 bytes; the whole matrix is at most 36 KB and stays
// in L2.
#pragma clang fp contract(off)
#include "cm_transform.h"
#include <type_traits>

struct __attribute__((packed, aligned(2))) U16x8u { uint16_t v[8]; };

// the 8 ranks of columns x0 .. x0 + 7 of row y (cropped destination coordinates, or chroma-plane coordinates)
__device__ __forceinline__ U16x8u dither_ranks(const DitherArgs &d, int x0, int y)
{
    return *(const U16x8u *)(d.tab + (size_t)((y + d.py) & d.mhm) * d.stride + ((x0 + d.px) & d.mwm));
}

// the CONV of three_channel_rows on the matrix path: RgbConv's three sums before its rounding constant, as the bits of an int
struct DitherSumConv {
__device__ static __forceinline__ void apply(const RgbOutArgs &a, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const int yy = y - a.yo, u = cb - a.co, v = cr - a.co;
    const int ty = a.coef[0] * yy;
    r = (uint32_t)(ty + a.coef[1] * v);
    g = (uint32_t)(ty + a.coef[2] * u + a.coef[3] * v);
    b = (uint32_t)(ty + a.coef[4] * u);
}
};
// ... and with a transform: the float32 q of every channel, before the code is made of it (the tables at the front of dynamic LDS, k_output_cm.hip's arrangement)
struct DitherCmConv {
__device__ static __forceinline__ void apply(const RgbOutArgs &a0, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const CmOutArgs &a = static_cast<const CmOutArgs &>(a0);
    extern __shared__ float cm_lds[];
    cm_apply<XGPU_OUT_F32>(a, a.cm, cm_lds_tables(a.cm, cm_lds), y, cb, cr, r, g, b);
}
};

template <int SINK, int DT, int UP, bool CM>
__global__ __launch_bounds__(256) void k_output_dither_rgb(const DitherRgbArgs a)
{
    using CONV = std::conditional_t<CM, DitherCmConv, DitherSumConv>;
    constexpr int SZ = OutT<DT>::size;
    if (CM) {
        extern __shared__ float cm_lds[];
        cm_fill_lds(a.cm, cm_lds);                // (every thread of the workgroup, before the lanes outside the picture leave)
    }
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.w || i >= a.ch) return;
    const int n = min(8, a.w - x0);               // pixels of this lane in the row (even)
    const bool vec = a.aligned && n == 8;
    const int up = a.shift - a.di.k;              // matrix path: the rank's shift to the sum's scale (>= 0: the host refuses k > S)
    const float inv_l = __uint_as_float((uint32_t)(127 - a.di.k) << 23);      // 2^-k: r * 2^-k is exact
    const int omax = (int)a.cm.outmax;
    three_channel_rows<UP, CONV>(a, x0, i, [&](int row, uint32_t (&ch)[3][8]) {
        const U16x8u rk = dither_ranks(a.di, x0, row);
        #pragma unroll
        for (int m = 0; m < 8; m++) {
            const int r = rk.v[m];
            #pragma unroll
            for (int c = 0; c < 3; c++) {
                if (CM) ch[c][m] = (uint32_t)min(__float2int_rd(__fadd_rn(__fmul_rn(__uint_as_float(ch[c][m]), a.cm.outmax), __fmul_rn((float)r, inv_l))), omax);
                else    ch[c][m] = (uint32_t)min(max(((int)ch[c][m] + (r << up)) >> a.shift, 0), a.maxv);
            }
        }
        if (a.bgr) {
            #pragma unroll
            for (int m = 0; m < 8; m++) { const uint32_t t = ch[0][m]; ch[0][m] = ch[2][m]; ch[2][m] = t; }
        }
        if (SINK == DITHER_SINK_PLANAR) {
            uint8_t *d = a.dst + (size_t)row * a.pitch + (size_t)x0 * SZ;
            #pragma unroll
            for (int c = 0; c < 3; c++) store_run<8, SZ>(d + c * a.plane, ch[c], vec, n);
        } else if (SINK == DITHER_SINK_INTERLEAVED) {
            uint32_t e[24];
            #pragma unroll
            for (int m = 0; m < 8; m++) { e[3 * m] = ch[0][m]; e[3 * m + 1] = ch[1][m]; e[3 * m + 2] = ch[2][m]; }
            store_run<24, SZ>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 3 * SZ, e, vec, 3 * n);
        } else if (SINK == DITHER_SINK_RGBA) {
            uint32_t e[32];
            #pragma unroll
            for (int m = 0; m < 8; m++) { e[4 * m] = ch[0][m]; e[4 * m + 1] = ch[1][m]; e[4 * m + 2] = ch[2][m]; e[4 * m + 3] = a.alpha; }
            store_run<32, SZ>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 4 * SZ, e, vec, 4 * n);
        } else {                                  // 10:10:10:2 - the channels are clipped to 0 .. 1023, the alpha code to 0 .. 3
            uint32_t e[8];
            #pragma unroll
            for (int m = 0; m < 8; m++) e[m] = ch[0][m] | (ch[1][m] << 10) | (ch[2][m] << 20) | (a.alpha << 30);
            store_run<8, 4>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 4, e, vec, n);
        }
    });
}

template <int SINK, int DT, int UP>
static void launch_dither_rgb_cm(const DitherRgbArgs &a, bool cm, dim3 grid, hipStream_t s)
{
    if (cm) {
        const size_t lds = sizeof(float) * cm_table_floats(a.cm.n_lin, a.cm.tone != NULL, a.cm.enc != NULL);      // at most 32.8 KB
        hipLaunchKernelGGL((k_output_dither_rgb<SINK, DT, UP, true>), grid, dim3(64, 4), lds, s, a);
    } else {
        hipLaunchKernelGGL((k_output_dither_rgb<SINK, DT, UP, false>), grid, dim3(64, 4), 0, s, a);
    }
}
template <int SINK, int DT>
static void launch_dither_rgb_up(const DitherRgbArgs &a, int upsample, bool cm, dim3 grid, hipStream_t s)
{
    if (upsample == XGPU_UPSAMPLE_NEAREST) launch_dither_rgb_cm<SINK, DT, XGPU_UPSAMPLE_NEAREST>(a, cm, grid, s);
    else                                   launch_dither_rgb_cm<SINK, DT, XGPU_UPSAMPLE_LINEAR>(a, cm, grid, s);
}
template <int SINK>
static void launch_dither_rgb_dt(const DitherRgbArgs &a, int dtype, int upsample, bool cm, dim3 grid, hipStream_t s)
{
    if (dtype == XGPU_OUT_U8) launch_dither_rgb_up<SINK, XGPU_OUT_U8>(a, upsample, cm, grid, s);
    else                      launch_dither_rgb_up<SINK, XGPU_OUT_U16>(a, upsample, cm, grid, s);
}
void launch_output_dither_rgb(const DitherRgbArgs &a, int sink, int dtype, int upsample, bool cm, hipStream_t s)
{
    const dim3 grid((unsigned)(((a.w + 7) / 8 + 63) / 64), (unsigned)((a.ch + 3) / 4));
    switch (sink) {
    case DITHER_SINK_PLANAR:      launch_dither_rgb_dt<DITHER_SINK_PLANAR>(a, dtype, upsample, cm, grid, s); break;
    case DITHER_SINK_INTERLEAVED: launch_dither_rgb_dt<DITHER_SINK_INTERLEAVED>(a, dtype, upsample, cm, grid, s); break;
    case DITHER_SINK_RGBA:        launch_dither_rgb_dt<DITHER_SINK_RGBA>(a, dtype, upsample, cm, grid, s); break;
    default:                      launch_dither_rgb_up<DITHER_SINK_RGB10A2, XGPU_OUT_U16>(a, upsample, cm, grid, s); break;
    }
}

// conv1 with the rounding constant replaced by (r << shift) >> k; with shift <= 0 nothing is added and the sample is conv1's
__device__ __forceinline__ int dither_conv1(int v, int shift, int maxv, int out8, int r, int k)
{
    if (shift <= 0) return conv1(v, shift, maxv, out8);
    const int add = (r << shift) >> k;
    if (out8) return min(max((v + add) >> shift, 0), 255);
    return min(((int)(uint16_t)v + add) >> shift, maxv);
}
__device__ __forceinline__ uint32_t dither_semi_elem(const DitherSemiArgs &a, int v, int r)
{
    return (uint32_t)(uint16_t)(dither_conv1(v, a.shift, a.maxv, a.out8, r, a.di.k) << a.lsh);
}

template <int DT>
__global__ __launch_bounds__(256) void k_output_dither_semiplanar(const DitherSemiArgs a)
{
    constexpr int SZ = OutT<DT>::size;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 16;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.w || i >= a.ch) return;
    const int n = min(16, a.w - x0);              // luma columns of this lane (even) = elements of its run of the interleaved chroma row
    const bool vec = a.aligned && n == 16;

    S16x8u ly[2][2];
    #pragma unroll
    for (int par = 0; par < 2; par++) {
        const int16_t *l = a.y + (size_t)(2 * i + par) * a.sy + x0;
        ly[par][0] = *(const S16x8u *)l;
        ly[par][1] = *(const S16x8u *)(l + 8);
    }
    const S16x8u cb = *(const S16x8u *)(a.u + (size_t)i * a.sc + (x0 >> 1));
    const S16x8u cr = *(const S16x8u *)(a.v + (size_t)i * a.sc + (x0 >> 1));

    uint32_t e[16];
    {
        const U16x8u rk = dither_ranks(a.di, x0 >> 1, i);      // chroma-plane coordinates
        #pragma unroll
        for (int k = 0; k < 8; k++) {
            int b = cb.v[k], r = cr.v[k];
            if (a.dra) {                          // the factor of chroma column j comes from the unmapped luma sample (2i, 2j)
                const int luma = ly[0][k >> 2].v[(2 * k) & 7];
                b = dra1(a.dra, 1, b, luma);
                r = dra1(a.dra, 2, r, luma);
            }
            e[2 * k]     = dither_semi_elem(a, b, rk.v[k]);
            e[2 * k + 1] = dither_semi_elem(a, r, rk.v[k]);
        }
        store_run<16, SZ>(a.dst + a.chroma_off + (size_t)i * a.pitch + (size_t)x0 * SZ, e, vec, n);
    }

    #pragma unroll
    for (int par = 0; par < 2; par++) {
        const int row = 2 * i + par;
        const uint16_t *t = a.di.tab + (size_t)((row + a.di.py) & a.di.mhm) * a.di.stride + ((x0 + a.di.px) & a.di.mwm);
        const U16x8u rk[2] = { *(const U16x8u *)t, *(const U16x8u *)(t + 8) };
        #pragma unroll
        for (int m = 0; m < 16; m++) {
            int y = ly[par][m >> 3].v[m & 7];
            if (a.dra) y = dra1(a.dra, 0, y, 0);
            e[m] = dither_semi_elem(a, y, rk[m >> 3].v[m & 7]);
        }
        store_run<16, SZ>(a.dst + (size_t)row * a.pitch + (size_t)x0 * SZ, e, vec, n);
    }
}

void launch_output_dither_semiplanar(const DitherSemiArgs &a, int dtype, hipStream_t s)
{
    const dim3 grid((unsigned)(((a.w + 15) / 16 + 63) / 64), (unsigned)((a.ch + 3) / 4));
    if (dtype == XGPU_OUT_U8) hipLaunchKernelGGL(k_output_dither_semiplanar<XGPU_OUT_U8>, grid, dim3(64, 4), 0, s, a);
    else                      hipLaunchKernelGGL(k_output_dither_semiplanar<XGPU_OUT_U16>, grid, dim3(64, 4), 0, s, a);
}
