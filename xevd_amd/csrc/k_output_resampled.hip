// k_output_resampled.hip - the bicubic resize of the scaled output and of the batch of rectangles (xgpu_pic_output_device_resampled / _rois_resampled; INTEGRATION.md
// section 8o).  One pair of kernels for both calls: the single picture is the batch of one stretched rectangle.  The pair has the shape of k_output_rois.hip's -
// the same descriptor block (RoiDesc, then the tap tables), the same grids, the same staging of a row's spans in LDS, the same pad lanes - and differs in the
// arithmetic alone: cubic weights have negative lobes, so the taps are signed (xgpu_resample_taps), the intermediate is int16 with two fraction bits and is not
// clipped, and the clip to the sample range follows the second pass (output_common.h: resample_vertical_lane, resample_column).  tests/resample_ref.py restates it.
//   k_resampled_vertical     grid (columns of the widest rectangle / 512, rows of the tallest inner part / 4, 3 n): plane blockIdx.z % 3 of rectangle blockIdx.z / 3.
//                            One lane owns 8 neighbouring columns of one destination row: a 16-byte load per tap row, a 16-byte store.  The row index is uniform
//                            per wave and the descriptor per workgroup, so descriptor, first / count and the weights are scalar loads.
//   k_resampled_horizontal   grid (dw / 64, dh / rows, n): 64 columns x `rows` rows of the IMAGE; the lanes that filter also write the pad elements, so every
//                            destination element is written exactly once.  A row's spans are wider than the triangle's - at a ratio of 64, (64 + 4) * 64 luma
//                            samples - so fewer rows fit 48 KB of LDS: 2 there.
// The intermediate is the context's sc_mid, read here as int16; what the 16-byte loads of the vertical pass read past a rectangle's width lands in columns of
// the intermediate that no tap reads.
#pragma clang fp contract(off)
#include "output_common.h"

__global__ __launch_bounds__(256) void k_resampled_vertical(const RoisOutArgs a)
{
    const int r = blockIdx.z / 3, plane = blockIdx.z - 3 * r;
    const RoiDesc &d = ((const RoiDesc *)a.blk)[r];
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int o = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y);      // one destination row per wave
    if (x0 >= (plane ? d.w >> 1 : d.w) || o >= d.ih) return;
    const int t = plane ? 1 : 0;
    const int32_t *first = (const int32_t *)(a.blk + d.first[t]), *count = (const int32_t *)(a.blk + d.count[t]);
    const int16_t *q = (const int16_t *)(a.blk + d.wt[t]) + (size_t)o * d.stride[t];
    const int16_t *luma = a.y + (size_t)d.y * a.sy + d.x;
    const int16_t *src = plane == 0 ? luma : (plane == 1 ? a.u : a.v) + (size_t)(d.y >> 1) * a.sc + (d.x >> 1);
    int16_t *m = (int16_t *)a.mid + d.mid + (plane == 0 ? (size_t)0 : (size_t)d.ih * d.mpy + (size_t)(plane - 1) * d.ih * d.mpc) + (size_t)o * (plane ? d.mpc : d.mpy) + x0;
    resample_vertical_lane(a, plane, src, luma, first[o], count[o], q, x0, m);
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

template <bool PLANAR, template <int> class CONV>
static void launch_horizontal(const RoisOutArgs &a, int dtype, dim3 grid, dim3 block, size_t lds, hipStream_t s)
{
    switch (dtype) {
    case XGPU_OUT_U8:   hipLaunchKernelGGL((k_resampled_horizontal<PLANAR, XGPU_OUT_U8, CONV>), grid, block, lds, s, a); break;
    case XGPU_OUT_U16:  hipLaunchKernelGGL((k_resampled_horizontal<PLANAR, XGPU_OUT_U16, CONV>), grid, block, lds, s, a); break;
    case XGPU_OUT_F16:  hipLaunchKernelGGL((k_resampled_horizontal<PLANAR, XGPU_OUT_F16, CONV>), grid, block, lds, s, a); break;
    case XGPU_OUT_BF16: hipLaunchKernelGGL((k_resampled_horizontal<PLANAR, XGPU_OUT_BF16, CONV>), grid, block, lds, s, a); break;
    default:            hipLaunchKernelGGL((k_resampled_horizontal<PLANAR, XGPU_OUT_F32, CONV>), grid, block, lds, s, a); break;
    }
}

// max_w: the widest rectangle; max_ih: the tallest inner part
void launch_output_resampled(const RoisOutArgs &a, int layout, int dtype, int max_w, int max_ih, hipStream_t s)
{
    hipLaunchKernelGGL(k_resampled_vertical, dim3((unsigned)(((max_w + 7) / 8 + 63) / 64), (unsigned)((max_ih + 3) / 4), (unsigned)(3 * a.n)), dim3(64, 4), 0, s, a);
    // as many rows per workgroup as 48 KB of LDS hold, 4 at most - k_output_scaled.hip's rule, on the widest span of the batch
    const size_t per_row = (size_t)(a.capy + 2 * a.capc) * sizeof(int16_t);
    int rows = 4;
    while (rows > 1 && rows * per_row > 48 * 1024) rows >>= 1;
    const dim3 grid((unsigned)((a.dw + 63) / 64), (unsigned)((a.dh + rows - 1) / rows), (unsigned)a.n), block(64, rows);
    const bool planar = layout == XGPU_OUT_RGB_PLANAR || layout == XGPU_OUT_YUV444_PLANAR;
    const bool rgb = layout == XGPU_OUT_RGB_PLANAR || layout == XGPU_OUT_RGB_INTERLEAVED;
    if (rgb) { if (planar) launch_horizontal<true, RgbConv>(a, dtype, grid, block, rows * per_row, s); else launch_horizontal<false, RgbConv>(a, dtype, grid, block, rows * per_row, s); }
    else     { if (planar) launch_horizontal<true, YuvConv>(a, dtype, grid, block, rows * per_row, s); else launch_horizontal<false, YuvConv>(a, dtype, grid, block, rows * per_row, s); }
}
