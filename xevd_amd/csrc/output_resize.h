// output_resize.h - what the two-pass resize outputs share above the lanes' work of output_common.h (k_output_scaled.hip, k_output_rois.hip, k_output_scaled_cm.hip,
// k_output_scaled_lin.hip, k_output_resampled.hip): the body of the batch vertical pass, the two bodies of the horizontal pass - one picture, and a batch of
// rectangles behind a descriptor block - and the launcher of the horizontal pass.  A __global__ kernel of those files is one call of a body; what a family
// differs in comes in as two policies:
//   ROW   how a wave stages its row of the intermediate in LDS and filters one destination column of it: TriangleRow here, LinRow in
//         k_output_scaled_lin.hip.  A ROW has
//           Value                                 the type of a filtered value (three per pixel)
//           row_bytes(capy, capc)                 host: the bytes of LDS one row needs
//           ROW(lds, capy, capc, xl, xc, o0, o1)  the wave's part of the workgroup's LDS and the spans destination columns o0 .. o1 reach (uniform per workgroup)
//           stage(mid, off, rows, mpy, mpc, row)  row `row` of the intermediate of `rows` rows that begins `off` of its elements behind `mid`, into LDS (a barrier follows)
//           column(o, smax, v)                    destination column o of the staged row -> v[3]
//   PIX   what turns v[3] into the bits of three elements in output order: PlainPixel<CONV> here, CmPixel in k_output_scaled_cm.hip, LinPixel in
//         k_output_scaled_lin.hip
// (k_resampled_horizontal alone keeps rois_horizontal's text written out, under cubic taps; k_output_resampled.hip says why.)
// The single-image body is not the batch body with one rectangle: its taps are kernel arguments, not a descriptor in memory, and that difference is speed.
#pragma once
#include "output_common.h"

// ---- the vertical pass
// 8 columns per lane and 64 lanes x 4 destination rows per workgroup over `w` source columns and `rows` destination rows, z deep
static inline dim3 vertical_grid(int w, int rows, unsigned z) { return dim3((unsigned)(((w + 7) / 8 + 63) / 64), (unsigned)((rows + 3) / 4), z); }

// table t (0 yl, 1 yc, 2 xl, 3 xc) of a rectangle's descriptor
__device__ __forceinline__ ScaleTaps roi_taps(const uint8_t *blk, const RoiDesc &d, int t)
{
    return { (const int32_t *)(blk + d.first[t]), (const int32_t *)(blk + d.count[t]), (const int16_t *)(blk + d.wt[t]), d.stride[t] };
}

// k_rois_vertical / k_resampled_vertical (SIGNED: scale_vertical_lane's): plane blockIdx.z % 3 of rectangle blockIdx.z / 3.  The row index is uniform per wave and
// the descriptor per workgroup, so descriptor, first / count and the weights are scalar loads.  Workgroups past a smaller rectangle's columns or rows leave at once.
template <bool SIGNED> __device__ __forceinline__ void rois_vertical(const RoisOutArgs &a)
{
    const int r = blockIdx.z / 3, plane = blockIdx.z - 3 * r;
    const RoiDesc &d = ((const RoiDesc *)a.blk)[r];
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int o = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y);      // one destination row per wave
    if (x0 >= (plane ? d.w >> 1 : d.w) || o >= d.ih) return;
    const ScaleTaps t = roi_taps(a.blk, d, plane ? 1 : 0);
    const int16_t *luma = a.y + (size_t)d.y * a.sy + d.x;
    const int16_t *src = plane == 0 ? luma : (plane == 1 ? a.u : a.v) + (size_t)(d.y >> 1) * a.sc + (d.x >> 1);
    uint16_t *m = a.mid + d.mid + (plane == 0 ? (size_t)0 : (size_t)d.ih * d.mpy + (size_t)(plane - 1) * d.ih * d.mpc) + (size_t)o * (plane ? d.mpc : d.mpy) + x0;
    scale_vertical_lane<SIGNED>(a, plane, src, luma, t.first[o], t.count[o], t.w + (size_t)o * t.stride, x0, m);
}

// ---- the horizontal pass: the rows of the 16-bit intermediates
// Y, Cb and Cr spans of one row side by side in the wave's part of LDS (capy + 2 capc samples), staged by 16-byte loads from 8-sample-aligned starts; the weights
// come transposed (w[k][column]), so a wave's weight loads are neighbours, and the samples are 16-bit LDS reads at a lane stride of the reduction ratio
struct TriangleRow {
    typedef int Value;
    static size_t row_bytes(int capy, int capc) { return (size_t)(capy + 2 * capc) * sizeof(uint16_t); }
    const ScaleTaps &xl, &xc;
    uint16_t *ly, *lb, *lr;
    int y0, y1, b0, b1;
    __device__ __forceinline__ TriangleRow(void *lds, int capy, int capc, const ScaleTaps &xl_, const ScaleTaps &xc_, int o0, int o1) : xl(xl_), xc(xc_)
    {
        ly = (uint16_t *)lds + (size_t)threadIdx.y * (capy + 2 * capc); lb = ly + capy; lr = lb + capc;
        y0 = xl.first[o0] & ~7; y1 = xl.first[o1] + xl.count[o1];
        b0 = xc.first[o0] & ~7; b1 = xc.first[o1] + xc.count[o1];
    }
    __device__ __forceinline__ void stage(const uint16_t *mid, uint32_t off, int rows, int mpy, int mpc, int row) const
    {
        const uint16_t *my = mid + off, *mb = my + (size_t)rows * mpy, *mr = mb + (size_t)rows * mpc;
        stage_span(ly, my + (size_t)row * mpy, y0, y1);
        stage_span(lb, mb + (size_t)row * mpc, b0, b1);
        stage_span(lr, mr + (size_t)row * mpc, b0, b1);
    }
    __device__ __forceinline__ void column(int o, int smax, int (&v)[3]) const
    {
        v[0] = filter_column(ly, xl, o, y0); v[1] = filter_column(lb, xc, o, b0); v[2] = filter_column(lr, xc, o, b0);
    }
};
// (Y, Cb, Cr) at the coding depth through RgbConv / YuvConv, the normalise and the dtype's rounding
template <template <int> class CONV> struct PlainPixel {
    template <int DT, class A> __device__ static __forceinline__ void apply(const A &a, const int (&v)[3], uint32_t (&e)[3]) { scaled_pixel<DT, CONV>(a, v[0], v[1], v[2], e); }
};

// ---- the horizontal pass: the two bodies.  `a` is the kernel's own argument, by reference: a copy costs registers.
// One picture: a workgroup is 64 destination columns x `rows` destination rows (4; 2 or 1 when the spans are long), one wave per row, one lane per pixel.  The
// pixel is stored element by element: the lanes of a wave write neighbouring elements of a row, and the destination is the small side of this kernel.  Any
// element-aligned destination works; there is no vector / element split to get wrong.
template <class ROW, class PIX, bool PLANAR, int DT, class A> __device__ __forceinline__ void scale_horizontal(const A &a)
{
    extern __shared__ uint4 lds4[];
    constexpr int SZ = OutT<DT>::size;
    const int oy = blockIdx.y * blockDim.y + threadIdx.y, ob = blockIdx.x * 64;
    const int row = min(oy, a.dh - 1), ol = min(ob + 63, a.dw - 1), ox = min(ob + (int)threadIdx.x, a.dw - 1);      // lanes past the edges work on the edge, and store nothing
    const ROW r(lds4, a.capy, a.capc, a.xl, a.xc, ob, ol);
    r.stage(a.mid, 0, a.dh, a.mpy, a.mpc, row);
    __syncthreads();
    typename ROW::Value v[3];
    r.column(ox, a.smax, v);

    uint32_t e[3];
    PIX::template apply<DT>(a, v, e);
    if (oy >= a.dh || ob + (int)threadIdx.x >= a.dw) return;
    store_pixel<PLANAR, SZ>(a.dst + (size_t)oy * a.pitch, a.plane, ox, e);
}

// A batch: 64 columns x `rows` rows of the IMAGE of rectangle blockIdx.z, so that the same lanes that filter also write the pad elements around the inner part and
// every destination element is written exactly once; the pad value is a value of the destination space, normalised like a pixel, never converted.  A workgroup
// that the inner part does not reach stages nothing.  SKIP: the block may come from k_rois_prepare, which marks the records at or above the count.
template <class ROW, class PIX, bool SKIP, bool PLANAR, int DT, class A> __device__ __forceinline__ void rois_horizontal(const A &a)
{
    extern __shared__ uint4 lds4[];
    constexpr int SZ = OutT<DT>::size;
    const RoiDesc &d = ((const RoiDesc *)a.blk)[blockIdx.z];
    if (SKIP && d.skip) return;      // the image is not touched (uniform per workgroup)
    const int oy = blockIdx.y * blockDim.y + threadIdx.y, ob = blockIdx.x * 64, ox = ob + (int)threadIdx.x;      // in the image
    // the inner columns and rows the workgroup covers (none: c0 > c1 or r0 > r1), and this wave's inner row
    const int c0 = max(ob - d.ix, 0), c1 = min(ob + 63 - d.ix, d.iw - 1);
    const int r0 = max((int)(blockIdx.y * blockDim.y) - d.iy, 0), r1 = min((int)((blockIdx.y + 1) * blockDim.y) - 1 - d.iy, d.ih - 1);
    const int row = oy - d.iy;
    const bool row_in = row >= 0 && row < d.ih;
    bool in = false;
    uint32_t e[3];
    if (c0 <= c1 && r0 <= r1) {      // uniform per workgroup
        const ScaleTaps xl = roi_taps(a.blk, d, 2), xc = roi_taps(a.blk, d, 3);
        const ROW r(lds4, a.capy, a.capc, xl, xc, c0, c1);
        if (row_in) r.stage(a.mid, d.mid, d.ih, d.mpy, d.mpc, row);      // uniform per wave: a wave stages its own row into its own part of LDS
        __syncthreads();
        if (row_in) {
            const int oc = min(max(ox - d.ix, c0), c1);      // lanes beside the inner part work on its edge, and store the pad value instead
            typename ROW::Value v[3];
            r.column(oc, a.smax, v);
            PIX::template apply<DT>(a, v, e);
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

// ---- the launch of the horizontal pass over `images` images.  K::kernel<PLANAR, RGB, DT>() is the family's __global__ instance.
template <class K, bool PLANAR, bool RGB, class A>
static void launch_horizontal_dt(const A &a, int dtype, dim3 grid, dim3 block, size_t lds, hipStream_t s)
{
    switch (dtype) {
    case XGPU_OUT_U8:   hipLaunchKernelGGL((K::template kernel<PLANAR, RGB, XGPU_OUT_U8>()), grid, block, lds, s, a); break;
    case XGPU_OUT_U16:  hipLaunchKernelGGL((K::template kernel<PLANAR, RGB, XGPU_OUT_U16>()), grid, block, lds, s, a); break;
    case XGPU_OUT_F16:  hipLaunchKernelGGL((K::template kernel<PLANAR, RGB, XGPU_OUT_F16>()), grid, block, lds, s, a); break;
    case XGPU_OUT_BF16: hipLaunchKernelGGL((K::template kernel<PLANAR, RGB, XGPU_OUT_BF16>()), grid, block, lds, s, a); break;
    default:            hipLaunchKernelGGL((K::template kernel<PLANAR, RGB, XGPU_OUT_F32>()), grid, block, lds, s, a); break;
    }
}
// As many rows per workgroup as 48 KB of LDS hold, 4 at most.  A row's 16-bit spans are at most ~17 KB (64 columns at a ratio of 64; ~19 KB under cubic taps); one
// row of float spans may pass 48 KB, which the host has checked against LIN_LDS_LIMIT.
template <class K, class ROW, class A>
static void launch_horizontal(const A &a, int layout, int dtype, unsigned images, hipStream_t s)
{
    const size_t per_row = ROW::row_bytes(a.capy, a.capc);
    int rows = 4;
    while (rows > 1 && rows * per_row > 48 * 1024) rows >>= 1;
    const dim3 grid((unsigned)((a.dw + 63) / 64), (unsigned)((a.dh + rows - 1) / rows), images), block(64, rows);
    const bool planar = layout == XGPU_OUT_RGB_PLANAR || layout == XGPU_OUT_YUV444_PLANAR;
    const bool rgb = layout == XGPU_OUT_RGB_PLANAR || layout == XGPU_OUT_RGB_INTERLEAVED;
    if (rgb) { if (planar) launch_horizontal_dt<K, true, true>(a, dtype, grid, block, rows * per_row, s); else launch_horizontal_dt<K, false, true>(a, dtype, grid, block, rows * per_row, s); }
    else     { if (planar) launch_horizontal_dt<K, true, false>(a, dtype, grid, block, rows * per_row, s); else launch_horizontal_dt<K, false, false>(a, dtype, grid, block, rows * per_row, s); }
}
