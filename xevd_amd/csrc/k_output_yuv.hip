// k_output_yuv.hip - a decoded 4:2:0 picture as a video surface in the caller's device memory (xgpu_pic_output_device): semi-planar NV12 / P016
// (P010, P012: the sample in the high bits of a 16-bit word) for encoders, display paths and other video libraries, and Y'CbCr 4:4:4 (three
// channels at luma resolution, integers or H.273's normalised floats) for models that work on Y'CbCr.  The contract is INTEGRATION.md section 8a;
// tests/yuv_ref.py restates it in numpy.
//
// k_output_semiplanar: the samples of xgpu_pic_output (conv1 at depth D, after the optional DRA), in another place.  One lane owns 16 luma columns
// of the two luma rows that share chroma row i, and the 8 Cb and 8 Cr samples below them: four 16-byte luma loads and one 16-byte load per chroma
// plane at the 2-byte-aligned crop position, Cb / Cr interleaved in registers, and - when dst, the row pitch and the chroma-plane offset are
// multiples of 16 bytes - one (u8) or two (u16) 16-byte stores per row; element stores otherwise and in a row's last column group.  Every sample is
// read once and written once; nothing is shared between lanes.  Loads past the cropped area stay inside the padded device picture (>= 72 chroma /
// 144 luma samples of border and margin on every side) and their values are not stored.
//
// k_output_yuv444: output_three_channels (output_common.h) - the load, edge clamp, DRA and chroma upsampling of k_output_rgb, the same code - with
// the matrix replaced by the depth conversion (u8), a copy (u16) or one float32 multiplication and a clip per channel (f32 / f16 / bf16).
#include "output_common.h"

// one sample as the bits of its output element: xgpu_pic_output's conversion, the P016 shift, cut to the 16 bits k_output stores (a DRA-mapped
// sample copied at its own depth may lie outside 0 .. 2^D - 1)
__device__ __forceinline__ uint32_t semi_elem(const SemiPlanarArgs &a, int v)
{
    return (uint32_t)(uint16_t)(conv1(v, a.shift, a.maxv, a.out8) << a.lsh);
}

template <int DT>
__global__ __launch_bounds__(256) void k_output_semiplanar(const SemiPlanarArgs a)
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
    #pragma unroll
    for (int k = 0; k < 8; k++) {
        int b = cb.v[k], r = cr.v[k];
        if (a.dra) {                              // the factor of chroma column j comes from the unmapped luma sample (2i, 2j)
            const int luma = ly[0][k >> 2].v[(2 * k) & 7];
            b = dra1(a.dra, 1, b, luma);
            r = dra1(a.dra, 2, r, luma);
        }
        e[2 * k]     = semi_elem(a, b);
        e[2 * k + 1] = semi_elem(a, r);
    }
    store_run<16, SZ>(a.dst + a.chroma_off + (size_t)i * a.pitch + (size_t)x0 * SZ, e, vec, n);

    #pragma unroll
    for (int par = 0; par < 2; par++) {
        #pragma unroll
        for (int m = 0; m < 16; m++) {
            int y = ly[par][m >> 3].v[m & 7];
            if (a.dra) y = dra1(a.dra, 0, y, 0);
            e[m] = semi_elem(a, y);
        }
        store_run<16, SZ>(a.dst + (size_t)(2 * i + par) * a.pitch + (size_t)x0 * SZ, e, vec, n);
    }
}

void launch_output_semiplanar(const SemiPlanarArgs &a, int dtype, hipStream_t s)
{
    const dim3 grid((unsigned)(((a.w + 15) / 16 + 63) / 64), (unsigned)((a.ch + 3) / 4));
    if (dtype == XGPU_OUT_U8) hipLaunchKernelGGL(k_output_semiplanar<XGPU_OUT_U8>, grid, dim3(64, 4), 0, s, a);
    else                      hipLaunchKernelGGL(k_output_semiplanar<XGPU_OUT_U16>, grid, dim3(64, 4), 0, s, a);
}

template <bool PLANAR, int DT, int UP>
__global__ __launch_bounds__(256) void k_output_yuv444(const RgbOutArgs a)
{
    output_three_channels<PLANAR, DT, UP, YuvConv<DT>>(a);
}

struct Yuv444Kernels {
    template <bool PLANAR, int DT, int UP> static void launch(const RgbOutArgs &a, dim3 grid, hipStream_t s)
    {
        hipLaunchKernelGGL((k_output_yuv444<PLANAR, DT, UP>), grid, dim3(64, 4), 0, s, a);
    }
};

void launch_output_yuv444(const RgbOutArgs &a, int layout, int dtype, int upsample, hipStream_t s)
{
    launch_three_channels<Yuv444Kernels>(a, layout == XGPU_OUT_YUV444_PLANAR, dtype, upsample, s);
}
