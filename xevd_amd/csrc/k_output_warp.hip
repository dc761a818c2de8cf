// k_output_warp.hip - n affine maps of one decoded picture, each giving one dw x dh image, converted and normalised like the scaled output, as a batch of images in
// the caller's device memory (xgpu_pic_output_device_warp): rotated text lines, crops aligned by a similarity transform, rotated boxes of
// an oriented detector - [N, 3, H, W] from one launch.  tests/warp_ref.py restates the contract in numpy int64.
//
// One kernel, grid (dw / 64, dh / 4, n), block (64, 4): one destination pixel per lane, one destination row per wave, one map per workgroup.
//   The map m[6] (Q16, int64) comes from blockIdx.z: six scalar loads.  The row terms m[1] oy + m[2], m[4] oy + m[5] are wave-uniform (the row goes through
//   readfirstlane, as in k_rois_vertical); the column term is one 32 x 32 + 64 bit multiply-add per lane and axis - the limits on m[0], m[3] exist for that.
//   Position arithmetic is UNSIGNED 64 bit (it wraps, it cannot overflow), shifts are arithmetic shifts of the same bits, and every position is clamped to the
//   plane before it becomes an index: the maps of the device-map call are data nobody has checked, and whatever they hold, no load leaves the picture minus the
//   crop.  A map outside the limits gives an image that is all pad (and status 1); the check is uniform per workgroup.
//   Per sub-position (S x S of them, S = 1, 2, 4): four luma samples and four of each chroma plane through ordinary global loads of the slot's int16 planes - an
//   image touches a small part of the picture, which L2 holds -, each DRA-mapped and clipped as the scaled output's are, weighted by the Q8 fractions.  The sum of
//   all sub-positions stays below 2^32: unsigned accumulators.  No LDS, no intermediate.
//   (Y, Cb, Cr) then go through scaled_pixel (output_common.h) unchanged, and store_pixel writes the three elements: every element of the image exactly once,
//   nothing beyond dw / dh, no padding between rows or images.
// SS = false is S = 1 without the loop and its 64-bit offsets.
#pragma clang fp contract(off)
#include "output_common.h"

// (warp_q8, warp_sample, warp_bilinear - the gather this kernel shares with k_output_remap.hip - live in output_common.h)
template <bool PLANAR, int DT, template <int> class CONV, bool SS>
__global__ __launch_bounds__(256) void k_output_warp(const WarpOutArgs a)
{
    constexpr int SZ = OutT<DT>::size;
    const int z = blockIdx.z;
    const int64_t *mp = a.maps + (size_t)6 * z;      // uniform per workgroup
    uint64_t m[6];
    bool ok = true;
    #pragma unroll
    for (int k = 0; k < 6; k++) {
        const int64_t v = mp[k], lim = (k == 2 || k == 5) ? (int64_t)1 << 36 : (int64_t)64 << 16;
        ok = ok && v >= -lim && v <= lim;
        m[k] = (uint64_t)v;
    }
    if (a.status && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) a.status[z] = ok ? 0 : 1;
    const int oy = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y), ox = blockIdx.x * 64 + (int)threadIdx.x;
    if (oy >= a.dh || ox >= a.dw) return;
    // (a coefficient beyond the limits is cut to its low 32 bits here: its image is all pad)
    const uint64_t X = (uint64_t)((int64_t)(int32_t)m[0] * (int64_t)ox) + (m[1] * (uint64_t)oy + m[2]);
    const uint64_t Y = (uint64_t)((int64_t)(int32_t)m[3] * (int64_t)ox) + (m[4] * (uint64_t)oy + m[5]);
    const int xtop = (a.w - 1) << 8, ytop = (a.h - 1) << 8, xctop = (a.cw - 1) << 8, yctop = (a.ch - 1) << 8;
    bool in = ok;
    if (a.border == XGPU_WARP_PAD) {      // the pixel's own position, before supersampling and before the clamp
        const int64_t x0 = (int64_t)(X + 128) >> 8, y0 = (int64_t)(Y + 128) >> 8;
        in = in && x0 >= 0 && x0 <= xtop && y0 >= 0 && y0 <= ytop;
    }
    uint32_t e[3];
    if (in) {
        const uint64_t cx = (uint64_t)(int64_t)(256 - a.sh * 32768), cy = (uint64_t)(int64_t)(256 - a.sv * 32768);
        const int S = SS ? 1 << a.ls : 1;
        uint32_t acc[3] = { 0, 0, 0 };
        for (int k = 0; k < S * S; k++) {
            uint64_t Xs = X, Ys = Y;
            if (SS) {      // sub-position (i, j): uniform per workgroup
                const uint64_t ci = (uint64_t)(int64_t)(2 * (k & (S - 1)) + 1 - S), cj = (uint64_t)(int64_t)(2 * (k >> a.ls) + 1 - S);
                Xs += (uint64_t)((int64_t)(m[0] * ci + m[1] * cj) >> (a.ls + 1));
                Ys += (uint64_t)((int64_t)(m[3] * ci + m[4] * cj) >> (a.ls + 1));
            }
            acc[0] += warp_bilinear(a, 0, a.y, a.sy, a.w, a.h, warp_q8(Xs, 128, 8, xtop), warp_q8(Ys, 128, 8, ytop));
            const int xc = warp_q8(Xs, cx, 9, xctop), yc = warp_q8(Ys, cy, 9, yctop);
            acc[1] += warp_bilinear(a, 1, a.u, a.sc, a.cw, a.ch, xc, yc);
            acc[2] += warp_bilinear(a, 2, a.v, a.sc, a.cw, a.ch, xc, yc);
        }
        const int sh = 16 + (SS ? 2 * a.ls : 0);
        scaled_pixel<DT, CONV>(a, (int)((acc[0] + (1u << (sh - 1))) >> sh), (int)((acc[1] + (1u << (sh - 1))) >> sh), (int)((acc[2] + (1u << (sh - 1))) >> sh), e);
    } else {
        #pragma unroll
        for (int k = 0; k < 3; k++) e[k] = OutT<DT>::is_float ? scaled_float_elem<DT>(a, k, a.padv[k]) : (uint32_t)(int)a.padv[k];
    }
    store_pixel<PLANAR, SZ>(a.dst + (size_t)z * a.image_pitch + (size_t)oy * a.pitch, a.plane, ox, e);
}

template <bool PLANAR, int DT, template <int> class CONV>
static void launch_warp_ss(const WarpOutArgs &a, dim3 grid, hipStream_t s)
{
    if (a.ls) hipLaunchKernelGGL((k_output_warp<PLANAR, DT, CONV, true>), grid, dim3(64, 4), 0, s, a);
    else      hipLaunchKernelGGL((k_output_warp<PLANAR, DT, CONV, false>), grid, dim3(64, 4), 0, s, a);
}
template <bool PLANAR, template <int> class CONV>
static void launch_warp_dt(const WarpOutArgs &a, int dtype, dim3 grid, hipStream_t s)
{
    switch (dtype) {
    case XGPU_OUT_U8:   launch_warp_ss<PLANAR, XGPU_OUT_U8, CONV>(a, grid, s); break;
    case XGPU_OUT_U16:  launch_warp_ss<PLANAR, XGPU_OUT_U16, CONV>(a, grid, s); break;
    case XGPU_OUT_F16:  launch_warp_ss<PLANAR, XGPU_OUT_F16, CONV>(a, grid, s); break;
    case XGPU_OUT_BF16: launch_warp_ss<PLANAR, XGPU_OUT_BF16, CONV>(a, grid, s); break;
    default:            launch_warp_ss<PLANAR, XGPU_OUT_F32, CONV>(a, grid, s); break;
    }
}

void launch_output_warp(const WarpOutArgs &a, int layout, int dtype, hipStream_t s)
{
    const dim3 grid((unsigned)((a.dw + 63) / 64), (unsigned)((a.dh + 3) / 4), (unsigned)a.n);
    const bool planar = layout == XGPU_OUT_RGB_PLANAR || layout == XGPU_OUT_YUV444_PLANAR;
    const bool rgb = layout == XGPU_OUT_RGB_PLANAR || layout == XGPU_OUT_RGB_INTERLEAVED;
    if (rgb) { if (planar) launch_warp_dt<true, RgbConv>(a, dtype, grid, s); else launch_warp_dt<false, RgbConv>(a, dtype, grid, s); }
    else     { if (planar) launch_warp_dt<true, YuvConv>(a, dtype, grid, s); else launch_warp_dt<false, YuvConv>(a, dtype, grid, s); }
}
