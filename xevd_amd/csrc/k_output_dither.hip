// k_output_dither.hip - the integer device outputs with an ordered or blue-noise dither in place of the final rounding (xgpu_pic_output_device_dithered,
// xgpu_pic_output_device_packed_dithered): out = clip(floor(v + r / L)) with r the rank of the pixel's position in the call's matrix.  The contract is
// INTEGRATION.md section 8r; tests/dither_ref.py restates it in numpy.  Only integer dtypes are built here, so a second kernel around the same integer source
// is exact (k_output_packed.hip's note on float contraction does not bite), and the transform keeps contraction off as k_output_cm.hip does.
//
// k_output_dither_rgb: k_output_packed_rgb's body, output_three_sinks (output_common.h) - 64 x 4 lanes, 8 pixels of two luma rows per lane, three_channel_rows
// for load, edge clamp, DRA and chroma upsampling, and the four sinks (the planar and the interleaved RGB image, RGBA, 10:10:10:2), the same code.
// three_channel_rows hands its CONV no position, and it stays as it is: the CONVs here stop one step short of the quantisation - the matrix' three sums without
// the rounding constant (DitherSumConv), or the transform's three float32 values q in [0, 1] (CmConv's F32 instance, cm_transform.h) - and the body's finish
// step, which knows row and column, fetches the lane's 8 ranks of that row and finishes: (sum + (r << (S - k))) >> S clipped, or min(rd(q * outmax + r / L), outmax).
//
// k_output_dither_semiplanar: the DITHER instance of k_output_semiplanar's body (output_semiplanar, output_common.h; dither_ranks and dither_conv1 are there with
// it) - 16 luma columns of two rows and 8 + 8 chroma samples per lane - with conv1's rounding constant replaced by (r << shift) >> k.  A chroma sample's rank
// is that of its chroma-plane position; Cb and Cr share it.
//
// The ranks are read from global memory: a slot's rows are extended by their own first 16 entries (DitherSlot), so a lane's run of 8 or 16 ranks from any phase
// is one contiguous 16- or 32-byte load at 2-byte alignment.  A workgroup reads 8 matrix rows of at most 288 bytes; the whole matrix is at most 36 KB and stays
// in L2.
#pragma clang fp contract(off)
#include "cm_transform.h"
#include <type_traits>

// the CONV of three_channel_rows on the matrix path: RgbConv's three sums before its rounding constant, as the bits of an int
struct DitherSumConv {
__device__ static __forceinline__ void apply(const RgbOutArgs &a, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const int yy = y - a.yo, u = cb - a.co, v = cr - a.co;
    const int ty = a.coef[0] * yy;
    r = (uint32_t)(ty + a.coef[1] * v);
    g = (uint32_t)(ty + a.coef[2] * u + a.coef[3] * v);
    b = (uint32_t)(ty + a.coef[4] * u);
}
};
// (with a transform the CONV is CmConv's F32 instance: the float32 q of every channel, before the code is made of it)

template <int SINK, int DT, int UP, bool CM>
__global__ __launch_bounds__(256) void k_output_dither_rgb(const DitherRgbArgs a)
{
    if (CM) {
        extern __shared__ float cm_lds[];
        cm_fill_lds(a.cm, cm_lds);                // (every thread of the workgroup, before the lanes outside the picture leave)
    }
    const int up = a.shift - a.di.k;              // matrix path: the rank's shift to the sum's scale (>= 0: the host refuses k > S)
    const float inv_l = __uint_as_float((uint32_t)(127 - a.di.k) << 23);      // 2^-k: r * 2^-k is exact
    const int omax = (int)a.cm.outmax;
    output_three_sinks<SINK, DT, UP, std::conditional_t<CM, CmConv<XGPU_OUT_F32>, DitherSumConv>>(a, a.alpha, [&](int row, int x0, uint32_t (&ch)[3][8]) {
        const U16x8u rk = *dither_ranks(a.di, x0, row);
        #pragma unroll
        for (int m = 0; m < 8; m++) {
            const int r = rk.v[m];
            #pragma unroll
            for (int c = 0; c < 3; c++) {
                if (CM) ch[c][m] = (uint32_t)min(__float2int_rd(__fadd_rn(__fmul_rn(__uint_as_float(ch[c][m]), a.cm.outmax), __fmul_rn((float)r, inv_l))), omax);
                else    ch[c][m] = (uint32_t)min(max(((int)ch[c][m] + (r << up)) >> a.shift, 0), a.maxv);
            }
        }
    });
}

// (integer dtypes only)
template <bool CM> struct DitherRgbKernels {
    template <int SINK, int DT, int UP> static void launch(const RgbOutArgs &a0, dim3 grid, hipStream_t s)
    {
        const DitherRgbArgs &a = static_cast<const DitherRgbArgs &>(a0);      // the launchers hand the reference through
        if constexpr (!OutT<DT>::is_float)
            hipLaunchKernelGGL((k_output_dither_rgb<SINK, DT, UP, CM>), grid, dim3(64, 4), CM ? cm_lds_bytes(a.cm) : 0, s, a);
    }
};
template <class K>
static void launch_dither_rgb(const DitherRgbArgs &a, int sink, int dtype, int upsample, hipStream_t s)
{
    if (sink == OUT_SINK_PLANAR)           launch_three_layout<K, OUT_SINK_PLANAR>(a, dtype, upsample, s);
    else if (sink == OUT_SINK_INTERLEAVED) launch_three_layout<K, OUT_SINK_INTERLEAVED>(a, dtype, upsample, s);
    else                                   launch_three_packed<K>(a, sink == OUT_SINK_RGB10A2, dtype, upsample, s);
}
void launch_output_dither_rgb(const DitherRgbArgs &a, int sink, int dtype, int upsample, bool cm, hipStream_t s)
{
    if (cm) launch_dither_rgb<DitherRgbKernels<true>>(a, sink, dtype, upsample, s);
    else    launch_dither_rgb<DitherRgbKernels<false>>(a, sink, dtype, upsample, s);
}

template <int DT>
__global__ __launch_bounds__(256) void k_output_dither_semiplanar(const DitherSemiArgs a)
{
    output_semiplanar<DT, true>(a);
}

void launch_output_dither_semiplanar(const DitherSemiArgs &a, int dtype, hipStream_t s)
{
    if (dtype == XGPU_OUT_U8) hipLaunchKernelGGL(k_output_dither_semiplanar<XGPU_OUT_U8>, semiplanar_grid(a.w, a.ch), dim3(64, 4), 0, s, a);
    else                      hipLaunchKernelGGL(k_output_dither_semiplanar<XGPU_OUT_U16>, semiplanar_grid(a.w, a.ch), dim3(64, 4), 0, s, a);
}
