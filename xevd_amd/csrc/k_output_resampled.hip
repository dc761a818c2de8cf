// k_output_resampled.hip - the bicubic resize of the scaled output and of the batch of rectangles (xgpu_pic_output_device_resampled / _rois_resampled; INTEGRATION.md
// section 8o).  One pair of kernels for both calls: the single picture is the batch of one stretched rectangle.  The pair has the shape of k_output_rois.hip's -
// the same descriptor block (RoiDesc, then the tap tables), the same grids, the same staging of a row's spans in LDS, the same pad lanes - and differs in the
// arithmetic alone: cubic weights have negative lobes, so the taps are signed (xgpu_resample_taps), the intermediate is int16 with two fraction bits and is not
// clipped, and the clip to the sample range follows the second pass (output_common.h: scale_vertical_lane<true>, resample_column).  tests/resample_ref.py
// restates it.  The vertical kernel is output_resize.h's rois_vertical and the launch its launch_horizontal (the row's bytes are TriangleRow's: 16-bit samples);
// k_resampled_horizontal keeps the text of rois_horizontal written out: as an instance of that body the 64 tiles of 224x224 at 8K measured 0.5 us (0.3 %) over
// the written-out kernel's median, once more than that kernel's own spread of 0.48 us.
//   k_resampled_vertical     grid (columns of the widest rectangle / 512, rows of the tallest inner part / 4, 3 n): plane blockIdx.z % 3 of rectangle blockIdx.z / 3.
//                            One lane owns 8 neighbouring columns of one destination row: a 16-byte load per tap row, a 16-byte store.  The row index is uniform
//                            per wave and the descriptor per workgroup, so descriptor, first / count and the weights are scalar loads.
//   k_resampled_horizontal   grid (dw / 64, dh / rows, n): 64 columns x `rows` rows of the IMAGE; the lanes that filter also write the pad elements, so every
//                            destination element is written exactly once.  A row's spans are wider than the triangle's - at a ratio of 64, (64 + 4) * 64 luma
//                            samples - so fewer rows fit 48 KB of LDS: 2 there.
// The intermediate is the context's sc_mid, read here as int16; what the 16-byte loads of the vertical pass read past a rectangle's width lands in columns of
// the intermediate that no tap reads.
#pragma clang fp contract(off)
#include "output_resize.h"

__global__ __launch_bounds__(256) void k_resampled_vertical(const RoisOutArgs a)
{
    rois_vertical<true>(a);
}

template <bool PLANAR, int DT, template <int> class CONV>
__global__ __launch_bounds__(256) void k_resampled_horizontal(const RoisOutArgs a)
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
            const int y = resample_column((const int16_t *)ly, xl, oc, y0, a.smax), cb = resample_column((const int16_t *)lb, xc, oc, b0, a.smax),
                      cr = resample_column((const int16_t *)lr, xc, oc, b0, a.smax);
            scaled_pixel<DT, CONV>(a, y, cb, cr, e);
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
struct ResampledHorizontal {
    template <bool PLANAR, bool RGB, int DT> static auto kernel()
    {
        if constexpr (RGB) return k_resampled_horizontal<PLANAR, DT, RgbConv>; else return k_resampled_horizontal<PLANAR, DT, YuvConv>;
    }
};

// max_w: the widest rectangle; max_ih: the tallest inner part
void launch_output_resampled(const RoisOutArgs &a, int layout, int dtype, int max_w, int max_ih, hipStream_t s)
{
    hipLaunchKernelGGL(k_resampled_vertical, vertical_grid(max_w, max_ih, (unsigned)(3 * a.n)), dim3(64, 4), 0, s, a);
    launch_horizontal<ResampledHorizontal, TriangleRow>(a, layout, dtype, (unsigned)a.n, s);      // on the widest span of the batch
}
