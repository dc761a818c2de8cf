// k_output_scaled.hip - a decoded 4:2:0 picture resized to the caller's size, converted and normalised in the caller's device memory
// (xgpu_pic_output_device_scaled): what a model takes - 224x224, 384x640 - made from the picture read once, instead of a full-size float tensor that a chain
// of framework kernels then shrinks.  The arithmetic is the contract of INTEGRATION.md section 8d; tests/scale_ref.py restates it in numpy, bit for bit.
//
// Two separable passes with non-negative 14-bit integer taps (xgpu_scale.hip), vertical first:
//   k_scale_vertical     t = (sum qy * clip(dra(sample)) + 2^10) >> 11       the sample with 3 fraction bits, <= 32760 at 12 bit: an unsigned 16-bit intermediate
//   k_scale_horizontal   v = (sum qx * t + 2^16) >> 17                       in [0, 2^B - 1] without a clip; then the unscaled path's CONV, the normalise, the store
// One tile cannot hold both: at 8K -> 224 the source footprint of a 16x16 destination tile is about 600x600 samples.  Vertical first because that pass is the one
// that reads the picture, and along rows it reads it in whole 16-byte groups.
//
// k_scale_vertical: one lane owns 8 neighbouring source columns of one destination row of one plane (blockIdx.z) and walks that row's taps: one 16-byte load per
// tap row - a wave reads 1 KB of one picture row, perfectly coalesced; loads past the cropped width stay inside the padded device picture (>= 72 chroma / 144 luma
// samples on every side) and the columns they make are never read - DRA and the clip per sample, 8 int32 accumulators, one 16-byte store.  The row index is
// uniform per wave, so first / count / weights are scalar loads.  Neighbouring destination rows share about half their source rows (the triangle is 2 f wide):
// those come from L2.  The intermediate is dh x (ws + 2 (ws / 2)) samples - 5 MB for 8K -> 224 rows - and stays in L2 / MALL for the second pass.
//
// k_scale_horizontal: a workgroup is 64 destination columns x `rows` destination rows (4; 2 or 1 when the spans are long), one wave per row, one lane per pixel.
// Each wave stages the spans of its row of the intermediate that its 64 columns reach - Y, Cb, Cr: 16-byte loads from 8-sample-aligned starts into its own part
// of LDS, whose size the host takes from the tap tables (dynamic shared memory: 36 KB per workgroup at 8K -> 224, under 1 KB for 8K -> 1080p) - then every lane
// walks its taps: the weights come transposed (w[k][column]), so a wave's weight loads are neighbours; the samples are 16-bit LDS reads at a lane stride of the
// reduction ratio.  The pixel then goes through RgbConv / YuvConv (output_common.h - for the float dtypes the F32 instance, so that the normalise sees the clipped
// float32 before the F16 / BF16 rounding, which is what those instances do last) and is stored element by element: the lanes of a wave write neighbouring elements
// of a row, and the destination is the small side of this kernel.  Any element-aligned destination works; there is no vector / element split to get wrong.
//
// The lanes' work - the vertical pass of 8 columns, the staging, the column filter, the conversion with its normalise, the stores - is in output_common.h
// (scale_vertical_lane, stage_span, filter_column, scaled_pixel, store_pixel): k_output_rois.hip runs the same functions on a batch of rectangles.  The body of
// k_scale_horizontal is output_resize.h's scale_horizontal with the row of the triangle taps and the plain pixel (k_output_scaled_cm.hip and
// k_output_scaled_lin.hip call it with theirs), and the launch of the pass - the rows rule, the grid, the instance by layout and dtype - is launch_horizontal there.
//
// Float arithmetic in this file is rounded operation by operation (no contraction into FMA): the normalise is (v - mean) * inv_std in two roundings by contract,
// and the matrix of the float dtypes is section 8a's formula as tests/colour_ref.py evaluates it.
#pragma clang fp contract(off)
#include "output_resize.h"

__global__ __launch_bounds__(256) void k_scale_vertical(const ScaledOutArgs a)
{
    const int plane = blockIdx.z;
    const int pw = plane ? a.cw : a.w;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int o = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y);      // one destination row per wave
    if (x0 >= pw || o >= a.dh) return;
    const ScaleTaps &t = plane ? a.yc : a.yl;
    uint16_t *d = a.mid + (plane == 0 ? (size_t)0 : (size_t)a.dh * a.mpy + (size_t)(plane - 1) * a.dh * a.mpc) + (size_t)o * (plane ? a.mpc : a.mpy) + x0;
    scale_vertical_lane(a, plane, plane == 0 ? a.y : plane == 1 ? a.u : a.v, a.y, t.first[o], t.count[o], t.w + (size_t)o * t.stride, x0, d);
}

template <bool PLANAR, int DT, template <int> class CONV>
__global__ __launch_bounds__(256) void k_scale_horizontal(const ScaledOutArgs a)
{
    scale_horizontal<TriangleRow, PlainPixel<CONV>, PLANAR, DT>(a);
}
struct ScaleHorizontal {
    template <bool PLANAR, bool RGB, int DT> static auto kernel()
    {
        if constexpr (RGB) return k_scale_horizontal<PLANAR, DT, RgbConv>; else return k_scale_horizontal<PLANAR, DT, YuvConv>;
    }
};

void launch_scale_vertical(const ScaledOutArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_scale_vertical, vertical_grid(a.w, a.dh, 3), dim3(64, 4), 0, s, a);
}

void launch_output_scaled(const ScaledOutArgs &a, int layout, int dtype, hipStream_t s)
{
    launch_scale_vertical(a, s);
    launch_horizontal<ScaleHorizontal, TriangleRow>(a, layout, dtype, 1u, s);
}
