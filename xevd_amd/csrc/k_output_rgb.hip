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
// The body is output_three_channels (output_common.h), shared with k_output_yuv444; this file adds the matrix (RgbConv).
#include "output_common.h"

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

template <int LAYOUT, int DT, int UP>
__global__ __launch_bounds__(256) void k_output_rgb(const RgbOutArgs a)
{
    output_three_channels<LAYOUT == XGPU_OUT_RGB_PLANAR, DT, UP, RgbConv<DT>>(a);
}

struct RgbKernels {
    template <bool PLANAR, int DT, int UP> static void launch(const RgbOutArgs &a, dim3 grid, hipStream_t s)
    {
        hipLaunchKernelGGL((k_output_rgb<PLANAR ? XGPU_OUT_RGB_PLANAR : XGPU_OUT_RGB_INTERLEAVED, DT, UP>), grid, dim3(64, 4), 0, s, a);
    }
};

void launch_output_rgb(const RgbOutArgs &a, int layout, int dtype, int upsample, hipStream_t s)
{
    launch_three_channels<RgbKernels>(a, layout == XGPU_OUT_RGB_PLANAR, dtype, upsample, s);
}
