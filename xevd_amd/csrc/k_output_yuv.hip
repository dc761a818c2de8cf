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

// (the body is output_common.h's output_semiplanar: k_output_dither_semiplanar is its other instance)
template <int DT>
__global__ __launch_bounds__(256) void k_output_semiplanar(const SemiPlanarArgs a)
{
    output_semiplanar<DT, false>(a);
}

void launch_output_semiplanar(const SemiPlanarArgs &a, int dtype, hipStream_t s)
{
    if (dtype == XGPU_OUT_U8) hipLaunchKernelGGL(k_output_semiplanar<XGPU_OUT_U8>, semiplanar_grid(a.w, a.ch), dim3(64, 4), 0, s, a);
    else                      hipLaunchKernelGGL(k_output_semiplanar<XGPU_OUT_U16>, semiplanar_grid(a.w, a.ch), dim3(64, 4), 0, s, a);
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
