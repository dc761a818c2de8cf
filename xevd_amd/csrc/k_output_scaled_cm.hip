// k_output_scaled_cm.hip - the scaled outputs with a colour transform: a decoded 4:2:0 picture (or a batch of its rectangles) resized to the caller's size, taken from
// the stream's colour space to the caller's, normalised, in the caller's device memory (xgpu_pic_output_device_scaled_cm, xgpu_pic_output_device_rois_cm): what a
// model trained on sRGB takes from a PQ / HLG / BT.2020 stream, without the full-size colour-managed tensor.  The contract is INTEGRATION.md section 8m: the
// filtered (Y, Cb, Cr) of section 8d, then the transform of section 8b on the R'G'B' code at the coding depth, then bgr, the normalise and the dtype's rounding;
// tests/scaled_cm_ref.py restates it on top of the numpy restatements of both.
//
// The vertical passes are k_scale_vertical / k_rois_vertical as they are (k_output_scaled.hip, k_output_rois.hip).  This file is the horizontal pass with the
// transform between the column filter and the store: the two bodies of output_resize.h with the plain passes' row (TriangleRow) and the pixel below, whose work
// is cm_transform.h's (cm_apply) and output_common.h's (scaled_finish) - neither arithmetic exists twice.
//
// The transform's tables are read from global memory (the context's d_cm, 20 KB at 10 bit: it stays in L1 / L2), and dynamic LDS holds the staged spans only, laid
// out and sized as in the plain passes (`rows` = 4, 2 or 1 by their 48 KB rule).  k_output_cm.hip copies the tables into LDS per workgroup and wins by it: there a
// workgroup has 4096 pixels.  Here it has 64 x rows <= 256, a copy per workgroup is ~20 table floats per pixel, and letting a workgroup fill once and walk several
// row groups of its strip leaves too few workgroups, each holding 53 - 64 KB of LDS: at 8K 10 bit PQ -> sRGB that form was 1.04 (224x224) to 1.25 (1080p) times
// slower than this one (DESIGN.md section 5c has both measurements; the instances that fill LDS were dropped after it).
#pragma clang fp contract(off)
#include "cm_transform.h"
#include "output_resize.h"

// one filtered pixel -> the bits of its three elements in output order: the transform (for the float dtypes its F32 instance, so that the normalise sees the
// clipped float32), then scaled_finish
struct CmPixel {
    template <int DT, class A> __device__ static __forceinline__ void apply(const A &a, const int (&v)[3], uint32_t (&e)[3])
    {
        const CmTables t = { a.cm.lin, a.cm.tone, a.cm.enc };
        cm_apply<OutT<DT>::is_float ? XGPU_OUT_F32 : DT>(a, a.cm, t, v[0], v[1], v[2], e[0], e[1], e[2]);
        scaled_finish<DT>(a, e);
    }
};

// k_scale_horizontal with the transform
template <bool PLANAR, int DT>
__global__ __launch_bounds__(256) void k_scale_horizontal_cm(const ScaledCmOutArgs a)
{
    scale_horizontal<TriangleRow, CmPixel, PLANAR, DT>(a);
}
// k_rois_horizontal with the transform.  (Host rectangles only: no record is marked skip.)  Eight waves per SIMD are asked for by name: left alone, the compiler
// loads the transform's forty-odd uniform arguments ahead of the column filter and holds them across it - 92 to 100 SGPRs, more than a SIMD has for eight waves
// (80 each), and the batch of 64 tiles at 8K ran 6 % longer for it.  With the bound the loads stay behind the filter: 78 SGPRs, the same 49 VGPRs.
template <bool PLANAR, int DT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_rois_horizontal_cm(const RoisCmOutArgs a)
{
    rois_horizontal<TriangleRow, CmPixel, false, PLANAR, DT>(a);
}
struct ScaleHorizontalCm { template <bool PLANAR, bool RGB, int DT> static auto kernel() { return k_scale_horizontal_cm<PLANAR, DT>; } };
struct RoisHorizontalCm  { template <bool PLANAR, bool RGB, int DT> static auto kernel() { return k_rois_horizontal_cm<PLANAR, DT>; } };

void launch_output_scaled_cm(const ScaledCmOutArgs &a, int layout, int dtype, hipStream_t s)
{
    launch_scale_vertical(a, s);
    launch_horizontal<ScaleHorizontalCm, TriangleRow>(a, layout, dtype, 1u, s);
}

// max_w: the widest rectangle; max_ih: the tallest inner part
void launch_output_rois_cm(const RoisCmOutArgs &a, int layout, int dtype, int max_w, int max_ih, hipStream_t s)
{
    launch_rois_vertical(a, max_w, max_ih, s);
    launch_horizontal<RoisHorizontalCm, TriangleRow>(a, layout, dtype, (unsigned)a.n, s);
}
