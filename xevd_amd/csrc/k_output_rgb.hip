// k_output_rgb.hip - a decoded 4:2:0 picture as R'G'B' in the caller's device memory (xgpu_pic_output_device): optional DRA, conformance-window
// crop, chroma upsampling to luma resolution, Y'CbCr -> R'G'B' and the store in one pass.  The exact arithmetic is the contract of include/xevd_hip.h
// and INTEGRATION.md section 8; tests/colour_ref.py restates it in numpy.
//
// A pure stream: ~1.5 samples x 2 bytes read and 3 elements written per pixel, no reuse beyond neighbouring chroma samples.  One thread makes
// 8 horizontal pixels of the two luma rows that share chroma row i: two 16-byte luma loads, and per chroma row it reads (i-1, i, i+1 for LINEAR,
// i for NEAREST) one 16-byte load of the chroma samples j0-2 .. j0+5 around its four columns j0 .. j0+3 - the neighbouring lanes' loads overlap
// and hit L1 / L2.  Loads past the cropped area stay inside the padded device picture (>= 72 chroma / 144 luma samples of border and margin on
// every side); the values of the columns outside it are replaced by the edge column's (the clamp of the contract) before they are used.
// Stores: when dst, the row pitch and the plane distance are multiples of 16 bytes, each lane writes its run of every row with vector stores -
// 8 bytes (u8 planar), 16 bytes (16-bit planar, every interleaved form but u8), three 8-byte stores (u8 interleaved: 24 bytes at 8-byte alignment);
// otherwise, and in the last column group of a row, element by element (any element-aligned destination: frame k of a [N, 3, H, W] batch).
// Templated over layout x dtype x upsampling mode; chroma siting, matrix, range and channel order are uniform arguments.
#include "xgpu_internal.h"
#include <hip/hip_fp16.h>

struct __attribute__((packed, aligned(2))) S16x8u { int16_t v[8]; };

// DRA of one sample, as k_output's dra1 (xevdm_dra.c:272-355): luma through its table, chroma scaled around 512 by the factor of the unmapped
// co-located luma sample
__device__ __forceinline__ int dra_rgb(const int32_t *lut, int c, int v, int luma)
{
    if (c == 0) return (int)(int16_t)lut[min(max(v, 0), 1023)];
    const int sv = v - 512;
    int off = (abs(sv) * lut[c * 1024 + min(max(luma, 0), 1023)] + (1 << 8)) >> 9;
    if (sv < 0) off = -off;
    return (int)(int16_t)(512 + off);
}

// the six chroma samples of columns j0-1 .. j0+4 of row `row` (already clamped) of one chroma plane, edge-clamped to 0 .. cw-1
__device__ __forceinline__ void chroma_row(const RgbOutArgs &a, int c, int row, int j0, int e[6])
{
    const int16_t *pl = (c == 1 ? a.u : a.v) + (size_t)row * a.sc;
    const S16x8u s = *(const S16x8u *)(pl + j0 - 2);
    #pragma unroll
    for (int k = 0; k < 6; k++) e[k] = s.v[k + 1];
    if (j0 == 0) e[0] = e[1];
    const int nv = a.cw - j0;                     // valid columns from j0 on (>= 1)
    int last = e[1];
    #pragma unroll
    for (int k = 2; k < 6; k++) if (nv >= k) last = e[k];
    #pragma unroll
    for (int k = 2; k < 6; k++) if (k > nv) e[k] = last;
    if (a.dra) {                                  // e[k] = the sample of column j (clamped); its DRA factor comes from luma (2 row, 2 j)
        const int16_t *l = a.y + (size_t)(2 * row) * a.sy;
        #pragma unroll
        for (int k = 0; k < 6; k++) e[k] = dra_rgb(a.dra, c, e[k], l[2 * min(max(j0 - 1 + k, 0), a.cw - 1)]);
    }
}

template <int DT> struct OutT;
template <> struct OutT<XGPU_OUT_U8>   { static constexpr int size = 1, is_float = 0; };
template <> struct OutT<XGPU_OUT_U16>  { static constexpr int size = 2, is_float = 0; };
template <> struct OutT<XGPU_OUT_F16>  { static constexpr int size = 2, is_float = 1; };
template <> struct OutT<XGPU_OUT_BF16> { static constexpr int size = 2, is_float = 1; };
template <> struct OutT<XGPU_OUT_F32>  { static constexpr int size = 4, is_float = 1; };

template <int DT> __device__ __forceinline__ uint32_t fbits(float f)
{
    if (DT == XGPU_OUT_F32) return __float_as_uint(f);
    if (DT == XGPU_OUT_F16) return (uint32_t)__half_as_ushort(__float2half_rn(f));
    const uint32_t u = __float_as_uint(f);        // bf16, round to nearest even (f is finite, in [0, 1])
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// one pixel: three channel values (as the bits of the output element) in R, G, B order
template <int DT> __device__ __forceinline__ void convert(const RgbOutArgs &a, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const int yy = y - a.yo, u = cb - a.co, v = cr - a.co;
    if (OutT<DT>::is_float) {
        const float fy = a.fcoef[0] * (float)yy, fu = (float)u, fv = (float)v;
        r = fbits<DT>(fminf(fmaxf(fy + a.fcoef[1] * fv, 0.f), 1.f));
        g = fbits<DT>(fminf(fmaxf(fy + a.fcoef[2] * fu + a.fcoef[3] * fv, 0.f), 1.f));
        b = fbits<DT>(fminf(fmaxf(fy + a.fcoef[4] * fu, 0.f), 1.f));
    } else {
        const int ty = a.coef[0] * yy + (1 << (a.shift - 1));
        r = (uint32_t)min(max((ty + a.coef[1] * v) >> a.shift, 0), a.maxv);
        g = (uint32_t)min(max((ty + a.coef[2] * u + a.coef[3] * v) >> a.shift, 0), a.maxv);
        b = (uint32_t)min(max((ty + a.coef[4] * u) >> a.shift, 0), a.maxv);
    }
}

// N elements of SZ bytes, packed into 32-bit words and stored: vector stores at `dst` (aligned) or one element at a time (first n elements)
template <int N, int SZ> __device__ __forceinline__ void store_run(uint8_t *dst, const uint32_t (&e)[N], bool vec, int n)
{
    if (vec) {
        constexpr int NW = N * SZ / 4;
        uint32_t w[NW];
        #pragma unroll
        for (int i = 0; i < NW; i++) w[i] = 0;
        #pragma unroll
        for (int i = 0; i < N; i++) w[i * SZ / 4] |= e[i] << (8 * ((i * SZ) % 4));
        if (NW % 4 == 0) {
            #pragma unroll
            for (int i = 0; i < NW; i += 4) *(uint4 *)(dst + 4 * i) = make_uint4(w[i], w[i + 1], w[i + 2], w[i + 3]);
        } else {
            #pragma unroll
            for (int i = 0; i < NW; i += 2) *(uint2 *)(dst + 4 * i) = make_uint2(w[i], w[i + 1]);
        }
    } else {
        #pragma unroll
        for (int i = 0; i < N; i++) {
            if (i >= n) break;
            if (SZ == 1) dst[i] = (uint8_t)e[i];
            else if (SZ == 2) ((uint16_t *)dst)[i] = (uint16_t)e[i];
            else ((uint32_t *)dst)[i] = e[i];
        }
    }
}

template <int LAYOUT, int DT, int UP>
__global__ __launch_bounds__(256) void k_output_rgb(const RgbOutArgs a)
{
    constexpr int SZ = OutT<DT>::size;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.w || i >= a.ch) return;
    const int j0 = x0 >> 1;
    const int n = min(8, a.w - x0);               // pixels of this lane in the row (even)
    const bool vec = a.aligned && n == 8;

    // chroma, vertically interpolated per row parity: cv[c][parity][k], columns j0-1+k
    int cv[2][2][6];
    #pragma unroll
    for (int c = 0; c < 2; c++) {
        int r0[6];
        chroma_row(a, c + 1, i, j0, r0);
        if (UP == XGPU_UPSAMPLE_NEAREST) {
            #pragma unroll
            for (int k = 0; k < 6; k++) cv[c][0][k] = cv[c][1][k] = r0[k];
        } else {
            int rm[6], rp[6];
            chroma_row(a, c + 1, max(i - 1, 0), j0, rm);
            chroma_row(a, c + 1, min(i + 1, a.ch - 1), j0, rp);
            #pragma unroll
            for (int k = 0; k < 6; k++) {
                cv[c][0][k] = a.ve[0] * rm[k] + a.ve[1] * r0[k];
                cv[c][1][k] = a.vo[0] * r0[k] + a.vo[1] * rp[k];
            }
        }
    }

    #pragma unroll
    for (int par = 0; par < 2; par++) {
        const int row = 2 * i + par;
        const S16x8u ly = *(const S16x8u *)(a.y + (size_t)row * a.sy + x0);
        uint32_t ch[3][8];
        #pragma unroll
        for (int m = 0; m < 8; m++) {
            int y = ly.v[m];
            if (a.dra) y = dra_rgb(a.dra, 0, y, 0);
            const int jj = m >> 1;                // chroma column j0 + jj = index jj + 1
            int cc[2];
            #pragma unroll
            for (int c = 0; c < 2; c++) {
                if (UP == XGPU_UPSAMPLE_NEAREST) cc[c] = cv[c][par][jj + 1];
                else if (m & 1) cc[c] = ((2 + a.hc) * cv[c][par][jj + 1] + (2 - a.hc) * cv[c][par][jj + 2] + 8) >> 4;
                else            cc[c] = (a.hc * cv[c][par][jj] + (4 - a.hc) * cv[c][par][jj + 1] + 8) >> 4;
            }
            convert<DT>(a, y, cc[0], cc[1], ch[0][m], ch[1][m], ch[2][m]);
        }
        if (a.bgr) {
            #pragma unroll
            for (int m = 0; m < 8; m++) { const uint32_t t = ch[0][m]; ch[0][m] = ch[2][m]; ch[2][m] = t; }
        }
        if (LAYOUT == XGPU_OUT_RGB_PLANAR) {
            uint8_t *d = a.dst + (size_t)row * a.pitch + (size_t)x0 * SZ;
            #pragma unroll
            for (int c = 0; c < 3; c++) store_run<8, SZ>(d + c * a.plane, ch[c], vec, n);
        } else {
            uint32_t e[24];
            #pragma unroll
            for (int m = 0; m < 8; m++) { e[3 * m] = ch[0][m]; e[3 * m + 1] = ch[1][m]; e[3 * m + 2] = ch[2][m]; }
            store_run<24, SZ>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 3 * SZ, e, vec, 3 * n);
        }
    }
}

template <int LAYOUT, int DT>
static void launch_dt(const RgbOutArgs &a, int upsample, dim3 grid, hipStream_t s)
{
    if (upsample == XGPU_UPSAMPLE_NEAREST) hipLaunchKernelGGL((k_output_rgb<LAYOUT, DT, XGPU_UPSAMPLE_NEAREST>), grid, dim3(64, 4), 0, s, a);
    else                                   hipLaunchKernelGGL((k_output_rgb<LAYOUT, DT, XGPU_UPSAMPLE_LINEAR>), grid, dim3(64, 4), 0, s, a);
}
template <int LAYOUT>
static void launch_layout(const RgbOutArgs &a, int dtype, int upsample, dim3 grid, hipStream_t s)
{
    switch (dtype) {
    case XGPU_OUT_U8:   launch_dt<LAYOUT, XGPU_OUT_U8>(a, upsample, grid, s); break;
    case XGPU_OUT_U16:  launch_dt<LAYOUT, XGPU_OUT_U16>(a, upsample, grid, s); break;
    case XGPU_OUT_F16:  launch_dt<LAYOUT, XGPU_OUT_F16>(a, upsample, grid, s); break;
    case XGPU_OUT_BF16: launch_dt<LAYOUT, XGPU_OUT_BF16>(a, upsample, grid, s); break;
    default:            launch_dt<LAYOUT, XGPU_OUT_F32>(a, upsample, grid, s); break;
    }
}

void launch_output_rgb(const RgbOutArgs &a, int layout, int dtype, int upsample, hipStream_t s)
{
    const dim3 grid((unsigned)(((a.w + 7) / 8 + 63) / 64), (unsigned)((a.ch + 3) / 4));
    if (layout == XGPU_OUT_RGB_PLANAR) launch_layout<XGPU_OUT_RGB_PLANAR>(a, dtype, upsample, grid, s);
    else                               launch_layout<XGPU_OUT_RGB_INTERLEAVED>(a, dtype, upsample, grid, s);
}
