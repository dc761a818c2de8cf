// k_output_cm.hip - k_output_rgb with a colour transform between the matrix and the store (xgpu_pic_output_device_cm): the R'G'B' code of the fixed-point
// path at the coding depth -> linear light (one table lookup per channel) -> destination primaries (3x3) -> tone curve or scale, clip -> destination
// transfer characteristic (an interpolated table lookup per channel) -> the output dtype.  Load, clamp, DRA, upsampling and the stores are
// output_three_channels (output_common.h), untouched; this file runs it with the CONV of the transform (CmConv, cm_transform.h).  The arithmetic is the contract of INTEGRATION.md section 8b and
// tests/colour_cm_ref.py restates it bit for bit, so: no powf / exp2f / log2f, every float32 multiply and add rounded on its own (contraction into FMA is
// switched off for this file), tables made by the host in double precision (xgpu_colour.hip).  The transform itself is cm_transform.h's, shared with
// k_output_scaled_cm.hip.
// The tables (4 KB .. 16 KB of linearisation, 8 KB per curve) are copied into LDS by every workgroup: at 8K 10 bit that is 1.2 - 1.45 times faster than
// reading them from global memory through L1 / L2 on a picture of random samples, although each workgroup copies ~5000 floats for its 4096 pixels
// (DESIGN.md section 5c has both measurements; the instances that read global memory were dropped after it).
#pragma clang fp contract(off)
#include "cm_transform.h"

template <int LAYOUT, int DT, int UP>
__global__ __launch_bounds__(256) void k_output_cm(const CmOutArgs a)
{
    extern __shared__ float cm_lds[];
    cm_fill_lds(a.cm, cm_lds);      // (every thread of the workgroup, before the lanes outside the picture leave)
    output_three_channels<LAYOUT == XGPU_OUT_RGB_PLANAR, DT, UP, CmConv<DT>>(a);
}

struct CmKernels {
    template <bool PLANAR, int DT, int UP> static void launch(const RgbOutArgs &a0, dim3 grid, hipStream_t s)
    {
        const CmOutArgs &a = static_cast<const CmOutArgs &>(a0);      // launch_three_channels hands the reference through
        hipLaunchKernelGGL((k_output_cm<PLANAR ? XGPU_OUT_RGB_PLANAR : XGPU_OUT_RGB_INTERLEAVED, DT, UP>), grid, dim3(64, 4), cm_lds_bytes(a.cm), s, a);
    }
};

void launch_output_cm(const CmOutArgs &a, int layout, int dtype, int upsample, hipStream_t s)
{
    launch_three_channels<CmKernels>(a, layout == XGPU_OUT_RGB_PLANAR, dtype, upsample, s);
}
