// k_output_ladder.hip - one decoded 4:2:0 picture as n scaled video surfaces ("rungs": 2160p, 1080p, 720p ... of an adaptive-bitrate ladder), each YUV420P, NV12 or
// P016 at its own size in its own destination (xgpu_pic_output_device_ladder): what an encoder, a display path or another video library takes, from one call.  The
// arithmetic is the contract of INTEGRATION.md section 8l; tests/ladder_ref.py restates it in numpy, bit for bit.
//
// The two passes are the scaled output's (k_output_scaled.hip; the lane functions of output_common.h, so the arithmetic exists once), with two differences: a
// chroma plane is filtered from its Ws/2 x Hs/2 samples straight onto the Wd/2 x Hd/2 grid of the rung (tables of xgpu_scale_taps_ex: the destination has a
// subsampling and a siting of its own), and the planes stay apart - a plane of a rung is a record (LadderDesc) in the context's block, picked by blockIdx.z as
// k_output_rois.hip picks a rectangle: a call is two launches and one upload however many rungs it has.
//   k_ladder_vertical     grid (columns of the source's luma plane / 512, rows of the tallest rung / 4, 3 n): record blockIdx.z = plane z % 3 of rung z / 3.
//                         scale_vertical_lane as it is: 8 neighbouring columns per lane, one destination row per wave, first / count / weights scalar loads.
//                         Every rung reads the picture again; the rungs of one call follow each other through L2 / MALL.
//   k_ladder_horizontal   grid (columns of the widest plane / 256, rows of the tallest / rows per workgroup, records): Y, Cb, Cr of a rung (YUV420P) or Y and the
//                         interleaved Cb Cr rows (NV12 / P016).  Here the destination is the large side - 12 MB for a 2160p P010 rung -, so a lane owns
//                         LADDER_GROUP = 4 neighbouring positions of one plane row: it filters them from the span of the intermediate its wave staged in LDS
//                         (stage_span / filter_column, weights transposed), applies the depth rule of xgpu_pic_output (conv1) and P016's shift, and stores
//                         them packed - 4 bytes (u8 plane), 8 bytes (u16 plane, u8 Cb Cr pairs) or 16 bytes (u16 Cb Cr pairs) per lane, so a wave writes
//                         256 B .. 1 KB of one row.  For the interleaved rows a lane makes Cb and Cr of the same four positions, one plane after the other
//                         through the same LDS (a row's span is at most 256 columns x 64 + the window: 33 KB, which two planes side by side would not fit).
// The vector / element split is store_run's (output_common.h), decided per lane: a vector store when the lane has all four positions and their address is a
// multiple of the store's size, element stores otherwise - a row's tail, a row whose start the pitch or the pointer leaves unaligned.  Lanes past a row's end and
// waves past the last row work on the edge (the barriers need them) and store nothing.
// Nothing outside the source reaches a result: taps end at its edge, and what the 16-byte loads of the vertical pass read past its width lands in columns of the
// intermediate no tap reads - as with the scaled output.
#include "output_common.h"

__global__ __launch_bounds__(256) void k_ladder_vertical(const LadderOutArgs a)
{
    const LadderDesc &d = ((const LadderDesc *)a.blk)[blockIdx.z];
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int o = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y);      // one destination row per wave
    if (x0 >= d.sw || o >= d.rows) return;
    const int32_t *first = (const int32_t *)(a.blk + d.first), *count = (const int32_t *)(a.blk + d.count);
    const int16_t *q = (const int16_t *)(a.blk + d.wt) + (size_t)o * d.stride;
    const int16_t *src = d.plane == 0 ? a.y : d.plane == 1 ? a.u : a.v;
    scale_vertical_lane(a, d.plane, src, a.y, first[o], count[o], q, x0, a.mid + d.mid[0] + (size_t)o * d.mp + x0);
}

// LADDER_GROUP positions from x0 of the staged row as the bits of their elements
__device__ __forceinline__ void ladder_filter_group(const LadderOutArgs &a, const uint16_t *lds, const ScaleTaps &t, int x0, int cols, int s0, uint32_t (&e)[LADDER_GROUP])
{
    #pragma unroll
    for (int g = 0; g < LADDER_GROUP; g++) {
        const int v = filter_column(lds, t, min(x0 + g, cols - 1), s0);
        e[g] = (uint32_t)(uint16_t)(conv1(v, a.cshift, a.cmaxv, a.cout8) << a.clsh);
    }
}

template <int DT>
__global__ __launch_bounds__(256) void k_ladder_horizontal(const LadderOutArgs a)
{
    extern __shared__ uint4 lds4[];
    constexpr int SZ = OutT<DT>::size, G = LADDER_GROUP;
    const LadderDesc &d = ((const LadderDesc *)a.blk)[3 * a.n + blockIdx.z];
    const int ob = blockIdx.x * (64 * G);
    if (ob >= d.cols || (int)(blockIdx.y * blockDim.y) >= d.rows) return;      // a smaller rung, a chroma plane: uniform per workgroup
    const int oy = blockIdx.y * blockDim.y + threadIdx.y, row = min(oy, d.rows - 1);
    const int ol = min(ob + 64 * G - 1, d.cols - 1), x0 = ob + (int)threadIdx.x * G;
    const ScaleTaps t = { (const int32_t *)(a.blk + d.first), (const int32_t *)(a.blk + d.count), (const int16_t *)(a.blk + d.wt), d.stride };
    const int s0 = t.first[ob] & ~7, s1 = t.first[ol] + t.count[ol];
    uint16_t *lds = (uint16_t *)lds4 + (size_t)threadIdx.y * a.cap;
    const int n = min(G, d.cols - x0);            // positions of this lane in the row (<= 0: none)
    const bool live = oy < d.rows && n > 0;
    uint32_t e0[G];
    stage_span(lds, a.mid + d.mid[0] + (size_t)row * d.mp, s0, s1);
    __syncthreads();
    ladder_filter_group(a, lds, t, x0, d.cols, s0, e0);
    if (!d.pair) {
        uint8_t *p = (uint8_t *)d.dst + (size_t)oy * d.pitch + (size_t)x0 * SZ;
        if (live) store_run<G, SZ>(p, e0, n == G && ((uintptr_t)p % (G * SZ)) == 0, n);
        return;
    }
    uint32_t e1[G], e[2 * G];
    __syncthreads();                              // every lane is done with Cb's span
    stage_span(lds, a.mid + d.mid[1] + (size_t)row * d.mp, s0, s1);
    __syncthreads();
    ladder_filter_group(a, lds, t, x0, d.cols, s0, e1);
    #pragma unroll
    for (int g = 0; g < G; g++) { e[2 * g] = e0[g]; e[2 * g + 1] = e1[g]; }
    uint8_t *p = (uint8_t *)d.dst + (size_t)oy * d.pitch + (size_t)x0 * 2 * SZ;
    if (live) store_run<2 * G, SZ>(p, e, n == G && ((uintptr_t)p % (2 * G * SZ)) == 0, 2 * n);
}

void launch_output_ladder(const LadderOutArgs &a, int dtype, int max_sw, int max_vrows, int max_cols, int max_rows, hipStream_t s)
{
    hipLaunchKernelGGL(k_ladder_vertical, dim3((unsigned)(((max_sw + 7) / 8 + 63) / 64), (unsigned)((max_vrows + 3) / 4), (unsigned)(3 * a.n)), dim3(64, 4), 0, s, a);
    // as many rows per workgroup as 48 KB of LDS hold, 4 at most - k_output_scaled.hip's rule; one row is at most 33 KB
    const size_t per_row = (size_t)a.cap * sizeof(uint16_t);
    int rows = 4;
    while (rows > 1 && rows * per_row > 48 * 1024) rows >>= 1;
    const dim3 grid((unsigned)((max_cols + 64 * LADDER_GROUP - 1) / (64 * LADDER_GROUP)), (unsigned)((max_rows + rows - 1) / rows), (unsigned)a.nh), block(64, rows);
    if (dtype == XGPU_OUT_U8) hipLaunchKernelGGL(k_ladder_horizontal<XGPU_OUT_U8>, grid, block, rows * per_row, s, a);
    else                      hipLaunchKernelGGL(k_ladder_horizontal<XGPU_OUT_U16>, grid, block, rows * per_row, s, a);
}
