// k_output_scaled_cm.hip - the scaled outputs with a colour transform: a decoded 4:2:0 picture (or a batch of its rectangles) resized to the caller's size, taken from
// the stream's colour space to the caller's, normalised, in the caller's device memory (xgpu_pic_output_device_scaled_cm, xgpu_pic_output_device_rois_cm): what a
// model trained on sRGB takes from a PQ / HLG / BT.2020 stream, without the full-size colour-managed tensor.  The contract is INTEGRATION.md section 8m: the
// filtered (Y, Cb, Cr) of section 8d, then the transform of section 8b on the R'G'B' code at the coding depth, then bgr, the normalise and the dtype's rounding;
// tests/scaled_cm_ref.py restates it on top of the numpy restatements of both.
//
// The vertical passes are k_scale_vertical / k_rois_vertical as they are (k_output_scaled.hip, k_output_rois.hip).  This file is the horizontal pass with the
// transform between the column filter and the store: the lanes' work is output_common.h's (stage_span, filter_column, scaled_finish, store_pixel) and
// cm_transform.h's (cm_apply) - neither arithmetic exists twice.
//
// The transform's tables are read from global memory (the context's d_cm, 20 KB at 10 bit: it stays in L1 / L2), and dynamic LDS holds the staged spans only, laid
// out and sized as in the plain passes (`rows` = 4, 2 or 1 by their 48 KB rule).  k_output_cm.hip copies the tables into LDS per workgroup and wins by it: there a
// workgroup has 4096 pixels.  Here it has 64 x rows <= 256, a copy per workgroup is ~20 table floats per pixel, and letting a workgroup fill once and walk several
// row groups of its strip leaves too few workgroups, each holding 53 - 64 KB of LDS: at 8K 10 bit PQ -> sRGB that form was 1.04 (224x224) to 1.25 (1080p) times
// slower than this one (DESIGN.md section 5c has both measurements; the instances that fill LDS were dropped after it).
#pragma clang fp contract(off)
#include "cm_transform.h"

// one filtered pixel -> the bits of its three elements in output order: the transform (for the float dtypes its F32 instance, so that the normalise sees the
// clipped float32), then scaled_finish
template <int DT> __device__ __forceinline__ void scaled_cm_pixel(const ScaledOutArgs &a, const CmParams &p, int y, int cb, int cr, uint32_t (&e)[3])
{
    const CmTables t = { p.lin, p.tone, p.enc };
    cm_apply<OutT<DT>::is_float ? XGPU_OUT_F32 : DT>(a, p, t, y, cb, cr, e[0], e[1], e[2]);
    scaled_finish<DT>(a, e);
}

// k_scale_horizontal with the transform: 64 destination columns x `rows` destination rows per workgroup, one wave per row, one lane per pixel
template <bool PLANAR, int DT>
__global__ __launch_bounds__(256) void k_scale_horizontal_cm(const ScaledCmOutArgs a)
{
    extern __shared__ uint4 lds4[];
    constexpr int SZ = OutT<DT>::size;
    const int oy = blockIdx.y * blockDim.y + threadIdx.y, ob = blockIdx.x * 64;
    const int row = min(oy, a.dh - 1), ol = min(ob + 63, a.dw - 1), ox = min(ob + (int)threadIdx.x, a.dw - 1);      // lanes past the edges work on the edge, and store nothing
    uint16_t *ly = (uint16_t *)lds4 + (size_t)threadIdx.y * (a.capy + 2 * a.capc), *lb = ly + a.capy, *lr = lb + a.capc;
    const int y0 = a.xl.first[ob] & ~7, y1 = a.xl.first[ol] + a.xl.count[ol];
    const int c0 = a.xc.first[ob] & ~7, c1 = a.xc.first[ol] + a.xc.count[ol];
    const uint16_t *mb = a.mid + (size_t)a.dh * a.mpy, *mr = mb + (size_t)a.dh * a.mpc;
    stage_span(ly, a.mid + (size_t)row * a.mpy, y0, y1);
    stage_span(lb, mb + (size_t)row * a.mpc, c0, c1);
    stage_span(lr, mr + (size_t)row * a.mpc, c0, c1);
    __syncthreads();
    const int y = filter_column(ly, a.xl, ox, y0), cb = filter_column(lb, a.xc, ox, c0), cr = filter_column(lr, a.xc, ox, c0);

    uint32_t e[3];
    scaled_cm_pixel<DT>(a, a.cm, y, cb, cr, e);
    if (oy >= a.dh || ob + (int)threadIdx.x >= a.dw) return;
    store_pixel<PLANAR, SZ>(a.dst + (size_t)oy * a.pitch, a.plane, ox, e);
}

// k_rois_horizontal with the transform: 64 columns x `rows` rows of the IMAGE of rectangle blockIdx.z; the pad value around the inner part is written as the plain
// call writes it - a value of the destination space, normalised like a pixel, never transformed.  (Host rectangles only: no record is marked skip.)
template <bool PLANAR, int DT>
__global__ __launch_bounds__(256) void k_rois_horizontal_cm(const RoisCmOutArgs a)
{
    extern __shared__ uint4 lds4[];
    constexpr int SZ = OutT<DT>::size;
    const RoiDesc &d = ((const RoiDesc *)a.blk)[blockIdx.z];
    const int oy = blockIdx.y * blockDim.y + threadIdx.y, ob = blockIdx.x * 64, ox = ob + (int)threadIdx.x;      // in the image
    // the inner columns and rows the workgroup covers (none: c0 > c1 or r0 > r1), and this wave's inner row
    const int c0 = max(ob - d.ix, 0), c1 = min(ob + 63 - d.ix, d.iw - 1);
    const int r0 = max((int)(blockIdx.y * blockDim.y) - d.iy, 0), r1 = min((int)((blockIdx.y + 1) * blockDim.y) - 1 - d.iy, d.ih - 1);
    const int row = oy - d.iy;
    const bool row_in = row >= 0 && row < d.ih;
    bool in = false;
    uint32_t e[3];
    if (c0 <= c1 && r0 <= r1) {      // uniform per workgroup
        const ScaleTaps xl = { (const int32_t *)(a.blk + d.first[2]), (const int32_t *)(a.blk + d.count[2]), (const int16_t *)(a.blk + d.wt[2]), d.stride[2] };
        const ScaleTaps xc = { (const int32_t *)(a.blk + d.first[3]), (const int32_t *)(a.blk + d.count[3]), (const int16_t *)(a.blk + d.wt[3]), d.stride[3] };
        uint16_t *ly = (uint16_t *)lds4 + (size_t)threadIdx.y * (a.capy + 2 * a.capc), *lb = ly + a.capy, *lr = lb + a.capc;
        const int y0 = xl.first[c0] & ~7, y1 = xl.first[c1] + xl.count[c1];
        const int b0 = xc.first[c0] & ~7, b1 = xc.first[c1] + xc.count[c1];
        if (row_in) {                // uniform per wave: a wave stages its own row into its own part of LDS
            const uint16_t *my = a.mid + d.mid, *mb = my + (size_t)d.ih * d.mpy, *mr = mb + (size_t)d.ih * d.mpc;
            stage_span(ly, my + (size_t)row * d.mpy, y0, y1);
            stage_span(lb, mb + (size_t)row * d.mpc, b0, b1);
            stage_span(lr, mr + (size_t)row * d.mpc, b0, b1);
        }
        __syncthreads();
        if (row_in) {
            const int oc = min(max(ox - d.ix, c0), c1);      // lanes beside the inner part work on its edge, and store the pad value instead
            const int y = filter_column(ly, xl, oc, y0), cb = filter_column(lb, xc, oc, b0), cr = filter_column(lr, xc, oc, b0);
            scaled_cm_pixel<DT>(a, a.cm, y, cb, cr, e);
            in = ox - d.ix == oc;
        }
    }
    if (!in) {
        #pragma unroll
        for (int k = 0; k < 3; k++) e[k] = OutT<DT>::is_float ? scaled_float_elem<DT>(a, k, a.padv[k]) : (uint32_t)(int)a.padv[k];
    }
    if (oy >= a.dh || ox >= a.dw) return;
    store_pixel<PLANAR, SZ>(a.dst + d.dst + (size_t)oy * a.pitch, a.plane, ox, e);
}

template <bool PLANAR> static void launch_horizontal(const ScaledCmOutArgs &a, int dtype, dim3 grid, dim3 block, size_t lds, hipStream_t s)
{
    switch (dtype) {
    case XGPU_OUT_U8:   hipLaunchKernelGGL((k_scale_horizontal_cm<PLANAR, XGPU_OUT_U8>), grid, block, lds, s, a); break;
    case XGPU_OUT_U16:  hipLaunchKernelGGL((k_scale_horizontal_cm<PLANAR, XGPU_OUT_U16>), grid, block, lds, s, a); break;
    case XGPU_OUT_F16:  hipLaunchKernelGGL((k_scale_horizontal_cm<PLANAR, XGPU_OUT_F16>), grid, block, lds, s, a); break;
    case XGPU_OUT_BF16: hipLaunchKernelGGL((k_scale_horizontal_cm<PLANAR, XGPU_OUT_BF16>), grid, block, lds, s, a); break;
    default:            hipLaunchKernelGGL((k_scale_horizontal_cm<PLANAR, XGPU_OUT_F32>), grid, block, lds, s, a); break;
    }
}
template <bool PLANAR> static void launch_horizontal(const RoisCmOutArgs &a, int dtype, dim3 grid, dim3 block, size_t lds, hipStream_t s)
{
    switch (dtype) {
    case XGPU_OUT_U8:   hipLaunchKernelGGL((k_rois_horizontal_cm<PLANAR, XGPU_OUT_U8>), grid, block, lds, s, a); break;
    case XGPU_OUT_U16:  hipLaunchKernelGGL((k_rois_horizontal_cm<PLANAR, XGPU_OUT_U16>), grid, block, lds, s, a); break;
    case XGPU_OUT_F16:  hipLaunchKernelGGL((k_rois_horizontal_cm<PLANAR, XGPU_OUT_F16>), grid, block, lds, s, a); break;
    case XGPU_OUT_BF16: hipLaunchKernelGGL((k_rois_horizontal_cm<PLANAR, XGPU_OUT_BF16>), grid, block, lds, s, a); break;
    default:            hipLaunchKernelGGL((k_rois_horizontal_cm<PLANAR, XGPU_OUT_F32>), grid, block, lds, s, a); break;
    }
}

// the horizontal pass over `images` images: as many rows per workgroup as 48 KB of LDS hold, 4 at most - k_output_scaled.hip's rule
template <class A> static void horizontal_cm(const A &a, int layout, int dtype, unsigned images, hipStream_t s)
{
    const size_t per_row = (size_t)(a.capy + 2 * a.capc) * sizeof(uint16_t);
    int rows = 4;
    while (rows > 1 && rows * per_row > 48 * 1024) rows >>= 1;
    const dim3 grid((unsigned)((a.dw + 63) / 64), (unsigned)((a.dh + rows - 1) / rows), images), block(64, rows);
    if (layout == XGPU_OUT_RGB_PLANAR) launch_horizontal<true>(a, dtype, grid, block, rows * per_row, s);
    else                               launch_horizontal<false>(a, dtype, grid, block, rows * per_row, s);
}

void launch_output_scaled_cm(const ScaledCmOutArgs &a, int layout, int dtype, hipStream_t s)
{
    launch_scale_vertical(a, s);
    horizontal_cm(a, layout, dtype, 1u, s);
}

// max_w: the widest rectangle; max_ih: the tallest inner part
void launch_output_rois_cm(const RoisCmOutArgs &a, int layout, int dtype, int max_w, int max_ih, hipStream_t s)
{
    launch_rois_vertical(a, max_w, max_ih, s);
    horizontal_cm(a, layout, dtype, (unsigned)a.n, s);
}
