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
// The body is output_three_channels (output_common.h), shared with k_output_yuv444, and the matrix is RgbConv (output_common.h too: the scaled output shares it).
#include "output_common.h"

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
