// output_common.h - what the output kernels share (k_output.hip, k_output_rgb.hip, k_output_yuv.hip; k_stats.hip's light pass): the per-sample depth conversion and DRA
// mapping, the edge-clamped chroma loads and the 4:2:0 -> luma-resolution upsampling of the device-output contract (INTEGRATION.md section 8a,
// step 2), the element types and the vector / element stores.  One version of each: a layout that is "the same samples, another place" runs
// the same code.  The kernels that write three channels at luma resolution share their bodies here too: output_three_channels (k_output_rgb, k_output_yuv444,
// k_output_cm, k_output_lut3d), output_three_sinks with its four sinks (the packed surfaces, the 3D LUT on them, the dither) and the launch of either; so do NV12 /
// P016 and their dithered form (output_semiplanar).  Further down: the lanes' work of the scaled outputs' two passes (the kernel bodies built on it are output_resize.h's) and the gather of the
// warped and the remapped output.
#pragma once
#include "xgpu_internal.h"
#include <hip/hip_fp16.h>

struct __attribute__((packed, aligned(2))) S16x8u { int16_t v[8]; };

// xgpu_pic_output's depth conversion (imgb_cpy_codec_to_out, app/xevd_app_util.h:465-552): to 8 bit a rounding shift of the signed sample
// clipped to [0, 255]; to a lower depth the same on the unsigned sample clipped to maxv; to a higher depth a left shift; else a copy
__device__ __forceinline__ int conv1(int v, int shift, int maxv, int out8)
{
    if (out8) return min(max((v + (shift ? 1 << (shift - 1) : 0)) >> shift, 0), 255);            // signed samples (:464-494)
    if (shift > 0) return min(((int)(uint16_t)v + (1 << (shift - 1))) >> shift, maxv);            // unsigned samples (:519-552)
    return shift < 0 ? (int)(uint16_t)(v << -shift) : v;
}

// DRA of one sample (xevdm_dra.c:272-355): luma through its table, chroma scaled around 512 by the factor of the unmapped co-located luma sample.
// v: the plane's sample; luma: the unmapped luma sample at (2y, 2x) for a chroma plane
__device__ __forceinline__ int dra1(const int32_t *lut, int c, int v, int luma)
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
        for (int k = 0; k < 6; k++) e[k] = dra1(a.dra, c, e[k], l[2 * min(max(j0 - 1 + k, 0), a.cw - 1)]);
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
    const uint32_t u = __float_as_uint(f);        // bf16, round to nearest even (f is finite, in [-0.5, 1])
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// N elements of SZ bytes, packed into 32-bit words and stored: vector stores at `dst` (aligned for them: 4 bytes for a run of one word, 16 for runs of whole groups of
// four words, 8 for the others) or one element at a time (first n elements)
template <int N, int SZ> __device__ __forceinline__ void store_run(uint8_t *dst, const uint32_t (&e)[N], bool vec, int n)
{
    if (vec) {
        constexpr int NW = N * SZ / 4;
        uint32_t w[NW];
        #pragma unroll
        for (int i = 0; i < NW; i++) w[i] = 0;
        #pragma unroll
        for (int i = 0; i < N; i++) w[i * SZ / 4] |= e[i] << (8 * ((i * SZ) % 4));
        if (NW == 1) {
            *(uint32_t *)dst = w[0];
        } else if (NW % 4 == 0) {
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

// The two CONVs: one pixel's (Y, Cb, Cr) at the coding depth -> the bits of three output elements.  Here, not in k_output_rgb.hip / k_output_yuv.hip, because the
// scaled output (k_output_scaled.hip) ends in the same conversions.
// RgbConv - the matrix of k_output_rgb.
// one pixel: three channel values (as the bits of the output element) in R, G, B order
template <int DT> struct RgbConv {
__device__ static __forceinline__ void apply(const RgbOutArgs &a, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
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
};

// YuvConv - the 4:4:4 layouts of k_output_yuv.
// one pixel: Y, Cb, Cr at the coding depth B -> the bits of three output elements.  u8: the 8-bit rule of xgpu_pic_output (a.shift = B - 8);
// u16: the sample; floats: E'Y = (Y - yo) * fy in [0, 1], E'Cb = (Cb - 2^(B-1)) * fc in [-0.5, 0.5], E'Cr alike - a.fcoef[0] = fy = float32(1 / yr),
// a.fcoef[1] = fc = float32(1 / cr), each product one float32 multiplication (nothing to contract with)
template <int DT> struct YuvConv {
__device__ static __forceinline__ void apply(const RgbOutArgs &a, int y, int cb, int cr, uint32_t &o0, uint32_t &o1, uint32_t &o2)
{
    if (OutT<DT>::is_float) {
        o0 = fbits<DT>(fminf(fmaxf((float)(y - a.yo) * a.fcoef[0], 0.f), 1.f));
        o1 = fbits<DT>(fminf(fmaxf((float)(cb - a.co) * a.fcoef[1], -0.5f), 0.5f));
        o2 = fbits<DT>(fminf(fmaxf((float)(cr - a.co) * a.fcoef[1], -0.5f), 0.5f));
    } else if (DT == XGPU_OUT_U8) {
        o0 = (uint32_t)conv1(y, a.shift, 255, 1);
        o1 = (uint32_t)conv1(cb, a.shift, 255, 1);
        o2 = (uint32_t)conv1(cr, a.shift, 255, 1);
    } else {
        o0 = (uint32_t)(uint16_t)y;
        o1 = (uint32_t)(uint16_t)cb;
        o2 = (uint32_t)(uint16_t)cr;
    }
}
};

// The pixels of one lane of the kernels that work at luma resolution (k_output_rgb, k_output_yuv444; k_stats' light pass): 8 horizontal pixels from x0 of the
// two luma rows that share chroma row i (x0 < a.w, i < a.ch).  Load, edge clamp, DRA and upsampling are here, once; CONV::apply turns one pixel's (Y, Cb, Cr) at
// the coding depth into the bits of three output elements; sink(row, ch) takes the 3 x 8 elements of luma row `row` (those past the picture's width too).
template <int UP, class CONV, class SINK>
__device__ __forceinline__ void three_channel_rows(const RgbOutArgs &a, int x0, int i, SINK &&sink)
{
    const int j0 = x0 >> 1;

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
            if (a.dra) y = dra1(a.dra, 0, y, 0);
            const int jj = m >> 1;                // chroma column j0 + jj = index jj + 1
            int cc[2];
            #pragma unroll
            for (int c = 0; c < 2; c++) {
                if (UP == XGPU_UPSAMPLE_NEAREST) cc[c] = cv[c][par][jj + 1];
                else if (m & 1) cc[c] = ((2 + a.hc) * cv[c][par][jj + 1] + (2 - a.hc) * cv[c][par][jj + 2] + 8) >> 4;
                else            cc[c] = (a.hc * cv[c][par][jj] + (4 - a.hc) * cv[c][par][jj + 1] + 8) >> 4;
            }
            CONV::apply(a, y, cc[0], cc[1], ch[0][m], ch[1][m], ch[2][m]);
        }
        sink(row, ch);
    }
}

// The body of the kernels that write three channels at luma resolution (k_output_rgb, k_output_yuv444): one lane makes the pixels of three_channel_rows and
// stores them.  PLANAR: three planes a.plane bytes apart, else the three elements of a pixel side by side.
template <bool PLANAR, int DT, int UP, class CONV>
__device__ __forceinline__ void output_three_channels(const RgbOutArgs &a)
{
    constexpr int SZ = OutT<DT>::size;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.w || i >= a.ch) return;
    const int n = min(8, a.w - x0);               // pixels of this lane in the row (even)
    const bool vec = a.aligned && n == 8;
    three_channel_rows<UP, CONV>(a, x0, i, [&](int row, uint32_t (&ch)[3][8]) {
        if (a.bgr) {
            #pragma unroll
            for (int m = 0; m < 8; m++) { const uint32_t t = ch[0][m]; ch[0][m] = ch[2][m]; ch[2][m] = t; }
        }
        if (PLANAR) {
            uint8_t *d = a.dst + (size_t)row * a.pitch + (size_t)x0 * SZ;
            #pragma unroll
            for (int c = 0; c < 3; c++) store_run<8, SZ>(d + c * a.plane, ch[c], vec, n);
        } else {
            uint32_t e[24];
            #pragma unroll
            for (int m = 0; m < 8; m++) { e[3 * m] = ch[0][m]; e[3 * m + 1] = ch[1][m]; e[3 * m + 2] = ch[2][m]; }
            store_run<24, SZ>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 3 * SZ, e, vec, 3 * n);
        }
    });
}

// The same body with the sink a template argument, for the kernels that are exact by rule (integer arithmetic, or float with contraction off): the packed display
// surfaces (k_output_packed_rgb), the 3D LUT on them (k_output_packed_lut3d) and the dithered outputs (k_output_dither_rgb).  One lane of 64 x 4 makes the
// pixels of three_channel_rows; finish(row, x0, ch) may rework a row's elements (the dither's rank step); then the bgr swap and the store of the row's 3 x 8
// elements from pixel x0 - `vec`: vector stores, else the first n pixels element by element.  alpha: the argument struct's A element - for RGBA in a float dtype
// the float32 bits of alpha, rounded to the dtype here; for 10:10:10:2 the 2-bit code (the channels are at most 1023 there).
// The sinks stand in the lambda itself, not in a function of their own that it calls: through such a function - __forceinline__, same text - the dithered
// instances took up to 12 more VGPRs and four of them lost a wave per SIMD, while this form compiles to the code of the three copies it replaces.
// The planar and the interleaved sink are output_three_channels' lambda a second time, on purpose.  That body cannot become an instance of this one: with either
// placement of the bgr swap the compiler allocates k_output_rgb's registers differently, and that kernel alone runs RgbConv's float matrix with FMA contraction left
// to the compiler, so its f16 / bf16 roundings are its code generation's.  The pull request that writes RgbConv with explicit __fmaf_rn /
// __fmul_rn lifts this: then output_three_channels is output_three_sinks<PLANAR ? OUT_SINK_PLANAR : OUT_SINK_INTERLEAVED, ...>.
struct NoFinish { __device__ __forceinline__ void operator()(int, int, uint32_t (&)[3][8]) const {} };
template <int SINK, int DT, int UP, class CONV, class FINISH = NoFinish>
__device__ __forceinline__ void output_three_sinks(const RgbOutArgs &a, uint32_t alpha_bits, FINISH &&finish = FINISH())
{
    constexpr int SZ = OutT<DT>::size;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.w || i >= a.ch) return;
    const int n = min(8, a.w - x0);               // pixels of this lane in the row (even)
    const bool vec = a.aligned && n == 8;
    const uint32_t alpha = SINK == OUT_SINK_RGBA && OutT<DT>::is_float ? fbits<DT>(__uint_as_float(alpha_bits)) : alpha_bits;
    three_channel_rows<UP, CONV>(a, x0, i, [&](int row, uint32_t (&ch)[3][8]) {
        finish(row, x0, ch);
        if (a.bgr) {
            #pragma unroll
            for (int m = 0; m < 8; m++) { const uint32_t t = ch[0][m]; ch[0][m] = ch[2][m]; ch[2][m] = t; }
        }
        if (SINK == OUT_SINK_PLANAR) {
            uint8_t *d = a.dst + (size_t)row * a.pitch + (size_t)x0 * SZ;
            #pragma unroll
            for (int c = 0; c < 3; c++) store_run<8, SZ>(d + c * a.plane, ch[c], vec, n);
        } else if (SINK == OUT_SINK_INTERLEAVED) {
            uint32_t e[24];
            #pragma unroll
            for (int m = 0; m < 8; m++) { e[3 * m] = ch[0][m]; e[3 * m + 1] = ch[1][m]; e[3 * m + 2] = ch[2][m]; }
            store_run<24, SZ>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 3 * SZ, e, vec, 3 * n);
        } else if (SINK == OUT_SINK_RGBA) {
            uint32_t e[32];
            #pragma unroll
            for (int m = 0; m < 8; m++) { e[4 * m] = ch[0][m]; e[4 * m + 1] = ch[1][m]; e[4 * m + 2] = ch[2][m]; e[4 * m + 3] = alpha; }
            store_run<32, SZ>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 4 * SZ, e, vec, 4 * n);
        } else {
            uint32_t e[8];
            #pragma unroll
            for (int m = 0; m < 8; m++) e[m] = ch[0][m] | (ch[1][m] << 10) | (ch[2][m] << 20) | (alpha << 30);
            store_run<8, 4>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 4, e, vec, n);
        }
    });
}

// The launch of a kernel family built on output_three_channels or output_three_sinks: 64 lanes x 4 chroma rows per workgroup, the instance picked by layout or
// sink, dtype and upsampling mode.  K::launch<L, DT, UP>(a, grid, stream) launches the family's kernel of that instance; L is the family's own first argument,
// PLANAR (launch_three_channels) or an OUT_SINK_* (launch_three_packed, k_output_dither.hip).  A family that has no kernel for an instance (a float dtype of the
// packed surfaces without a transform, of the dither) leaves its launch<> empty there.
static dim3 three_channel_grid(const RgbOutArgs &a) { return dim3((unsigned)(((a.w + 7) / 8 + 63) / 64), (unsigned)((a.ch + 3) / 4)); }
template <class K, auto L, int DT>
static void launch_three_dt(const RgbOutArgs &a, int upsample, hipStream_t s)
{
    if (upsample == XGPU_UPSAMPLE_NEAREST) K::template launch<L, DT, XGPU_UPSAMPLE_NEAREST>(a, three_channel_grid(a), s);
    else                                   K::template launch<L, DT, XGPU_UPSAMPLE_LINEAR>(a, three_channel_grid(a), s);
}
template <class K, auto L>
static void launch_three_layout(const RgbOutArgs &a, int dtype, int upsample, hipStream_t s)
{
    switch (dtype) {
    case XGPU_OUT_U8:   launch_three_dt<K, L, XGPU_OUT_U8>(a, upsample, s); break;
    case XGPU_OUT_U16:  launch_three_dt<K, L, XGPU_OUT_U16>(a, upsample, s); break;
    case XGPU_OUT_F16:  launch_three_dt<K, L, XGPU_OUT_F16>(a, upsample, s); break;
    case XGPU_OUT_BF16: launch_three_dt<K, L, XGPU_OUT_BF16>(a, upsample, s); break;
    default:            launch_three_dt<K, L, XGPU_OUT_F32>(a, upsample, s); break;
    }
}
template <class K>
static void launch_three_channels(const RgbOutArgs &a, bool planar, int dtype, int upsample, hipStream_t s)
{
    if (planar) launch_three_layout<K, true>(a, dtype, upsample, s);
    else        launch_three_layout<K, false>(a, dtype, upsample, s);
}
// the packed sinks: RGBA in the five dtypes; 10:10:10:2 is the U16 instance, whatever `dtype` says
template <class K>
static void launch_three_packed(const RgbOutArgs &a, bool rgb10a2, int dtype, int upsample, hipStream_t s)
{
    if (rgb10a2) launch_three_dt<K, OUT_SINK_RGB10A2, XGPU_OUT_U16>(a, upsample, s);
    else         launch_three_layout<K, OUT_SINK_RGBA>(a, dtype, upsample, s);
}

// ---- NV12 / P016 (k_output_semiplanar) and their dithered form (k_output_dither_semiplanar)
// the matrix of a dithered call: the address of the rank of column x0 of row y (cropped destination coordinates, or chroma-plane coordinates) - DitherSlot's rows
// are extended by their own first 16 entries, so the 8 or 16 ranks from there are contiguous at 2-byte alignment
struct __attribute__((packed, aligned(2))) U16x8u { uint16_t v[8]; };
__device__ __forceinline__ const U16x8u *dither_ranks(const DitherArgs &d, int x0, int y)
{
    return (const U16x8u *)(d.tab + (size_t)((y + d.py) & d.mhm) * d.stride + ((x0 + d.px) & d.mwm));
}
// conv1 with the rounding constant replaced by (r << shift) >> k; with shift <= 0 nothing is added and the sample is conv1's
__device__ __forceinline__ int dither_conv1(int v, int shift, int maxv, int out8, int r, int k)
{
    if (shift <= 0) return conv1(v, shift, maxv, out8);
    const int add = (r << shift) >> k;
    if (out8) return min(max((v + add) >> shift, 0), 255);
    return min(((int)(uint16_t)v + add) >> shift, maxv);
}
// one sample as the bits of its output element: xgpu_pic_output's conversion (DITHER: with rank r in its rounding), the P016 shift, cut to the 16 bits k_output
// stores (a DRA-mapped sample copied at its own depth may lie outside 0 .. 2^D - 1)
template <bool DITHER, class A> __device__ __forceinline__ uint32_t semi_elem(const A &a, int v, int r)
{
    int e;
    if constexpr (DITHER) e = dither_conv1(v, a.shift, a.maxv, a.out8, r, a.di.k);
    else                  e = conv1(v, a.shift, a.maxv, a.out8);
    return (uint32_t)(uint16_t)(e << a.lsh);
}
// One lane of 64 x 4: 16 luma columns of the two luma rows that share chroma row i, and the 8 Cb and 8 Cr samples below them (k_output_yuv.hip has the account of
// the loads and stores).  A: SemiPlanarArgs, or with DITHER DitherSemiArgs - the ranks are loaded only there.  A chroma sample's rank is that of its chroma-plane
// position; Cb and Cr share it.
template <int DT, bool DITHER, class A>
__device__ __forceinline__ void output_semiplanar(const A &a)
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
    U16x8u rk[2] = {};
    if constexpr (DITHER) rk[0] = *dither_ranks(a.di, x0 >> 1, i);
    #pragma unroll
    for (int k = 0; k < 8; k++) {
        int b = cb.v[k], r = cr.v[k];
        if (a.dra) {                              // the factor of chroma column j comes from the unmapped luma sample (2i, 2j)
            const int luma = ly[0][k >> 2].v[(2 * k) & 7];
            b = dra1(a.dra, 1, b, luma);
            r = dra1(a.dra, 2, r, luma);
        }
        e[2 * k]     = semi_elem<DITHER>(a, b, rk[0].v[k]);
        e[2 * k + 1] = semi_elem<DITHER>(a, r, rk[0].v[k]);
    }
    store_run<16, SZ>(a.dst + a.chroma_off + (size_t)i * a.pitch + (size_t)x0 * SZ, e, vec, n);

    #pragma unroll
    for (int par = 0; par < 2; par++) {
        if constexpr (DITHER) { const U16x8u *t = dither_ranks(a.di, x0, 2 * i + par); rk[0] = t[0]; rk[1] = t[1]; }
        #pragma unroll
        for (int m = 0; m < 16; m++) {
            int y = ly[par][m >> 3].v[m & 7];
            if (a.dra) y = dra1(a.dra, 0, y, 0);
            e[m] = semi_elem<DITHER>(a, y, rk[m >> 3].v[m & 7]);
        }
        store_run<16, SZ>(a.dst + (size_t)(2 * i + par) * a.pitch + (size_t)x0 * SZ, e, vec, n);
    }
}
static dim3 semiplanar_grid(int w, int ch) { return dim3((unsigned)(((w + 15) / 16 + 63) / 64), (unsigned)((ch + 3) / 4)); }

// The lanes' work in the two passes of the scaled outputs (k_output_scaled.hip: one picture; k_output_rois.hip: a batch of rectangles; k_output_resampled.hip:
// either with cubic taps; k_output_ladder.hip: video surfaces); output_resize.h builds the kernels' bodies on it.  The files that use them switch float contraction
// off before they include this header: the normalise and the float matrix are rounded operation by operation.
// Vertical pass, one lane: 8 neighbouring columns from x0 of one destination row of one plane - `cnt` source rows from `first` with the weights q.  src / luma: the
// first sample of the source rectangle in the plane / in the luma plane (the DRA factor of chroma sample (row, x) comes from the unmapped luma sample (2 row, 2 x));
// d: where the 8 results go.  SIGNED picks the rounding shift and the pack, the only things the tap kinds differ in:
//   false  the non-negative 14-bit triangle taps: t = (sum qy * clip(dra(sample)) + 2^10) >> 11, three fraction bits, <= 32760: an unsigned 16-bit intermediate
//   true   the cubic taps of either sign: t = (sum qy * clip(dra(sample)) + 2^11) >> 12, two fraction bits, not clipped.  With
//          sum |q| <= 32768 (xgpu_resample_taps refuses a table with a wider row) |sum qy * sample| <= 4095 * 2^15 < 2^27 and |t| <= 32760: an int16 intermediate,
//          and int32 accumulators hold this sum as they hold the second pass' (|sum qx * t| <= 2^15 * 32760 < 2^30)
template <bool SIGNED = false>
__device__ __forceinline__ void scale_vertical_lane(const ScaledOutArgs &a, int plane, const int16_t *src, const int16_t *luma, int first, int cnt, const int16_t *q,
                                                    int x0, uint16_t *d)
{
    constexpr int SH = SIGNED ? 12 : 11;
    const int st = plane ? a.sc : a.sy;
    int acc[8];
    #pragma unroll
    for (int m = 0; m < 8; m++) acc[m] = 0;
    for (int k = 0; k < cnt; k++) {
        const int row = first + k, qk = q[k];
        const S16x8u s = *(const S16x8u *)(src + (size_t)row * st + x0);
        int v[8];
        #pragma unroll
        for (int m = 0; m < 8; m++) v[m] = s.v[m];
        if (a.dra) {
            if (plane == 0) {
                #pragma unroll
                for (int m = 0; m < 8; m++) v[m] = dra1(a.dra, 0, v[m], 0);
            } else {
                const int16_t *l = luma + (size_t)(2 * row) * a.sy + 2 * x0;
                const S16x8u l0 = *(const S16x8u *)l, l1 = *(const S16x8u *)(l + 8);
                #pragma unroll
                for (int m = 0; m < 8; m++) v[m] = dra1(a.dra, plane, v[m], m < 4 ? l0.v[2 * m] : l1.v[2 * m - 8]);
            }
        }
        #pragma unroll
        for (int m = 0; m < 8; m++) acc[m] += qk * min(max(v[m], 0), a.smax);
    }
    uint32_t w[4];
    #pragma unroll
    for (int m = 0; m < 4; m++) {
        const int lo = (acc[2 * m] + (1 << (SH - 1))) >> SH, hi = (acc[2 * m + 1] + (1 << (SH - 1))) >> SH;
        w[m] = SIGNED ? (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16) : (uint32_t)lo | ((uint32_t)hi << 16);
    }
    *(uint4 *)d = make_uint4(w[0], w[1], w[2], w[3]);
}

// the span [s0, s1) of one row of the intermediate (s0 a multiple of 8) into the wave's LDS, 8 samples per lane and step
__device__ __forceinline__ void stage_span(uint16_t *lds, const uint16_t *row, int s0, int s1)
{
    for (int i = threadIdx.x * 8; i < s1 - s0; i += 512) *(uint4 *)(lds + i) = *(const uint4 *)(row + s0 + i);
}
// destination column o of the staged row: v = (sum qx * t + 2^16) >> 17
__device__ __forceinline__ int filter_column(const uint16_t *lds, const ScaleTaps &t, int o, int s0)
{
    const uint16_t *l = lds + (t.first[o] - s0);
    const int16_t *q = t.w + o;
    const int n = t.count[o];
    int acc = 0;
    for (int k = 0; k < n; k++) acc += (int)q[(size_t)k * t.stride] * (int)l[k];
    return (acc + (1 << 16)) >> 17;
}
// destination column o of the staged row of signed samples: v = clip((sum qx * t + 2^15) >> 16, 0, smax)
__device__ __forceinline__ int resample_column(const int16_t *lds, const ScaleTaps &t, int o, int s0, int smax)
{
    const int16_t *l = lds + (t.first[o] - s0);
    const int16_t *q = t.w + o;
    const int n = t.count[o];
    int acc = 0;
    for (int k = 0; k < n; k++) acc += (int)q[(size_t)k * t.stride] * (int)l[k];
    return min(max((acc + (1 << 15)) >> 16, 0), smax);
}
template <int SZ> __device__ __forceinline__ void store_elem(uint8_t *p, uint32_t e)
{
    if (SZ == 1) *p = (uint8_t)e;
    else if (SZ == 2) *(uint16_t *)p = (uint16_t)e;
    else *(uint32_t *)p = e;
}
// float32 v at output position k -> the bits of the element: the normalise in two roundings, then the dtype's rounding
template <int DT> __device__ __forceinline__ uint32_t scaled_float_elem(const ScaledOutArgs &a, int k, float v)
{
    if (a.normalize) v = __fmul_rn(__fsub_rn(v, a.mean[k]), a.inv_std[k]);
    return fbits<DT>(v);
}
// one filtered pixel (Y, Cb, Cr at the coding depth) -> the bits of its three elements in output order: CONV (for the float dtypes its F32 instance, so that the
// normalise sees the clipped float32), bgr, the normalise, the dtype's rounding
// what follows the conversion (k_output_scaled_cm.hip converts with the colour transform and ends here too): e = R, G, B as the integer dtype's elements or as the
// bits of the clipped float32
template <int DT> __device__ __forceinline__ void scaled_finish(const ScaledOutArgs &a, uint32_t (&e)[3])
{
    if (a.bgr) { const uint32_t t = e[0]; e[0] = e[2]; e[2] = t; }
    if (OutT<DT>::is_float) {
        #pragma unroll
        for (int k = 0; k < 3; k++) e[k] = scaled_float_elem<DT>(a, k, __uint_as_float(e[k]));
    }
}
template <int DT, template <int> class CONV> __device__ __forceinline__ void scaled_pixel(const ScaledOutArgs &a, int y, int cb, int cr, uint32_t (&e)[3])
{
    CONV<OutT<DT>::is_float ? XGPU_OUT_F32 : DT>::apply(a, y, cb, cr, e[0], e[1], e[2]);      // floats: the clipped float32
    scaled_finish<DT>(a, e);
}
// the three elements of pixel ox of the destination row at `row`: three planes `plane` bytes apart, or side by side
template <bool PLANAR, int SZ> __device__ __forceinline__ void store_pixel(uint8_t *row, size_t plane, int ox, const uint32_t (&e)[3])
{
    if (PLANAR) {
        uint8_t *d = row + (size_t)ox * SZ;
        #pragma unroll
        for (int k = 0; k < 3; k++) store_elem<SZ>(d + k * plane, e[k]);
    } else {
        uint8_t *d = row + (size_t)ox * 3 * SZ;
        #pragma unroll
        for (int k = 0; k < 3; k++) store_elem<SZ>(d + k * SZ, e[k]);
    }
}
// ---- the gather of the warped and the remapped output (k_output_warp.hip, k_output_remap.hip; INTEGRATION.md sections 8j, 8k)
// Q16 position + `add` -> Q8 (shift 8: luma) or Q8 chroma samples (shift 9), clamped to [0, top]: what every index is made from
__device__ __forceinline__ int warp_q8(uint64_t pos, uint64_t add, int shift, int top)
{
    const int64_t r = (int64_t)(pos + add) >> shift;
    return (int)min(max(r, (int64_t)0), (int64_t)top);
}
// sample (row, col) of plane c (inside the plane): DRA (a chroma sample by the unmapped luma at (2 row, 2 col)), then the clip
__device__ __forceinline__ int warp_sample(const ScaledOutArgs &a, int c, const int16_t *pl, int st, int row, int col)
{
    int v = pl[(size_t)row * st + col];
    if (a.dra) v = dra1(a.dra, c, v, c ? (int)a.y[(size_t)(2 * row) * a.sy + 2 * col] : 0);
    return min(max(v, 0), a.smax);
}
// the bilinear sum of plane c (pw x ph samples) at the clamped Q8 position (xr, yr): below 2^16 * 2^B
__device__ __forceinline__ uint32_t warp_bilinear(const ScaledOutArgs &a, int c, const int16_t *pl, int st, int pw, int ph, int xr, int yr)
{
    const int ix = xr >> 8, fx = xr & 255, ix1 = min(ix + 1, pw - 1);
    const int iy = yr >> 8, fy = yr & 255, iy1 = min(iy + 1, ph - 1);
    const int p00 = warp_sample(a, c, pl, st, iy, ix), p01 = warp_sample(a, c, pl, st, iy, ix1);
    const int p10 = warp_sample(a, c, pl, st, iy1, ix), p11 = warp_sample(a, c, pl, st, iy1, ix1);
    return (uint32_t)((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p01 + (256 - fx) * fy * p10 + fx * fy * p11);
}
