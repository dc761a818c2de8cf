// k_output_packed.hip - a decoded 4:2:0 picture as a packed display surface in the caller's device memory (xgpu_pic_output_device_packed): one word per pixel -
// RGBA in the five dtypes, or 10:10:10:2 - for a compositor or a swap chain, and packed 4:2:2 (YUYV / UYVY; 16-bit: Y210 and its kin) for capture cards, SDI
// output and the encoders that take it.  The contract is INTEGRATION.md section 8p; tests/packed_ref.py restates it in numpy.
//
// k_output_packed_rgb: output_three_sinks (output_common.h) with the RGBA or the 10:10:10:2 sink - the lane, load, edge clamp, DRA, chroma upsampling and the
// sinks are there, shared with the 3D LUT and the dither, and the first four are k_output_rgb's, the same code - with RgbConv (the matrix) or, with a transform,
// CmConv (cm_transform.h) as k_output_cm.hip arranges it: the tables at the front of dynamic LDS, copied by every workgroup.  One lane makes 8 pixels of two luma rows; its run of a row is 32 contiguous bytes (RGBA u8, 10:10:10:2), 64 (the 16-bit dtypes) or 128 (f32),
// written as 16-byte stores when destination and pitch are multiples of 16, element by element otherwise and in a row's last lane.  10:10:10:2 is the U16
// instance with coef / shift / maxv of D = 10 in its arguments (with a transform: outmax = 1023) and the three codes and the alpha code or-ed into one word.
// The integer matrix and the transform (FMA contraction off, as in k_output_cm.hip) are exact rules, so R, G, B are the bits k_output_rgb / k_output_cm write.
// RgbConv's float matrix is not such a rule: which of its multiplications the compiler contracts into an FMA is decided per kernel (in k_output_rgb it differs
// from pixel to pixel of a lane), and a second kernel around the same source rounds a few elements in a million differently.  RGBA in a float dtype without a
// transform is therefore k_output_rgb itself, into the context's intermediate, and k_packed_rgba_from_rgb behind it, which adds the A element: the bits are that
// kernel's by construction.  (DESIGN.md section 5c has the measurement that led here and the price.)
//
// k_output_packed_422: the samples of k_output_semiplanar (conv1 at depth D after the optional DRA, the P016 shift for 16-bit words), chroma at half width and
// full height.  One lane owns 8 luma columns of the two luma rows that share chroma row i and chroma columns j0 .. j0+3 of rows i-1, i, i+1 (chroma_row: the edge
// clamp and the DRA mapping of every sample before the vertical weights); 16 elements per row and lane: one 16-byte store (u8) or two (u16).
#pragma clang fp contract(off)
#include "cm_transform.h"
#include <type_traits>

template <int SINK, int DT, int UP, bool CM>
__global__ __launch_bounds__(256) void k_output_packed_rgb(const PackedRgbArgs a)
{
    if (CM) {
        extern __shared__ float cm_lds[];
        cm_fill_lds(a.cm, cm_lds);                // (every thread of the workgroup, before the lanes outside the picture leave)
    }
    output_three_sinks<SINK, DT, UP, std::conditional_t<CM, CmConv<DT>, RgbConv<DT>>>(a, a.alpha);
}

// RGBA in a float dtype without a transform, second pass: the interleaved R'G'B' image k_output_rgb itself wrote to `mid` (rows mid_pitch bytes apart, a multiple
// of 16 that holds a multiple of 8 pixels) with the A element put behind every pixel.  One lane copies 8 pixels of a row: 16-byte loads, stores as above.
template <int DT>
__global__ __launch_bounds__(256) void k_packed_rgba_from_rgb(const PackedRgbArgs a, const uint8_t *mid, size_t mid_pitch)
{
    constexpr int SZ = OutT<DT>::size, NW = 24 * SZ / 4;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int row = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.w || row >= a.h) return;
    const int n = min(8, a.w - x0);
    const uint32_t alpha = fbits<DT>(__uint_as_float(a.alpha));
    const uint4 *src = (const uint4 *)(mid + (size_t)row * mid_pitch + (size_t)x0 * 3 * SZ);
    uint32_t wv[NW];
    #pragma unroll
    for (int k = 0; k < NW / 4; k++) { const uint4 v = src[k]; wv[4 * k] = v.x; wv[4 * k + 1] = v.y; wv[4 * k + 2] = v.z; wv[4 * k + 3] = v.w; }
    uint32_t e[32];
    #pragma unroll
    for (int m = 0; m < 8; m++) {
        #pragma unroll
        for (int k = 0; k < 3; k++) {
            const int idx = 3 * m + k;
            e[4 * m + k] = SZ == 4 ? wv[idx] : (wv[idx / 2] >> (16 * (idx & 1))) & 0xFFFFu;
        }
        e[4 * m + 3] = alpha;
    }
    store_run<32, SZ>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 4 * SZ, e, a.aligned && n == 8, 4 * n);
}
void launch_packed_rgba_from_rgb(const PackedRgbArgs &a, int dtype, const uint8_t *mid, size_t mid_pitch, hipStream_t s)
{
    const dim3 grid((unsigned)(((a.w + 7) / 8 + 63) / 64), (unsigned)((a.h + 3) / 4));
    if (dtype == XGPU_OUT_F16)       hipLaunchKernelGGL(k_packed_rgba_from_rgb<XGPU_OUT_F16>, grid, dim3(64, 4), 0, s, a, mid, mid_pitch);
    else if (dtype == XGPU_OUT_BF16) hipLaunchKernelGGL(k_packed_rgba_from_rgb<XGPU_OUT_BF16>, grid, dim3(64, 4), 0, s, a, mid, mid_pitch);
    else                             hipLaunchKernelGGL(k_packed_rgba_from_rgb<XGPU_OUT_F32>, grid, dim3(64, 4), 0, s, a, mid, mid_pitch);
}

// (no instance for a float dtype without a transform: the host side runs the two passes above instead)
template <bool CM> struct PackedRgbKernels {
    template <int SINK, int DT, int UP> static void launch(const RgbOutArgs &a0, dim3 grid, hipStream_t s)
    {
        const PackedRgbArgs &a = static_cast<const PackedRgbArgs &>(a0);      // launch_three_packed hands the reference through
        if constexpr (CM || !OutT<DT>::is_float)
            hipLaunchKernelGGL((k_output_packed_rgb<SINK, DT, UP, CM>), grid, dim3(64, 4), CM ? cm_lds_bytes(a.cm) : 0, s, a);
    }
};
void launch_output_packed_rgb(const PackedRgbArgs &a, int layout, int dtype, int upsample, bool cm, hipStream_t s)
{
    if (cm) launch_three_packed<PackedRgbKernels<true>>(a, layout == XGPU_PACKED_RGB10A2, dtype, upsample, s);
    else    launch_three_packed<PackedRgbKernels<false>>(a, layout == XGPU_PACKED_RGB10A2, dtype, upsample, s);
}

// one sample as the bits of its output element: k_output_semiplanar's - xgpu_pic_output's conversion, the P016 shift, cut to 16 bits
__device__ __forceinline__ uint32_t packed_elem(const Packed422Args &a, int v)
{
    return (uint32_t)(uint16_t)(conv1(v, a.cshift, a.cmax, a.out8) << a.lsh);
}

template <int DT, bool UYVY, int UP>
__global__ __launch_bounds__(256) void k_output_packed_422(const Packed422Args a)
{
    constexpr int SZ = OutT<DT>::size;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.w || i >= a.ch) return;
    const int n = min(8, a.w - x0);               // luma columns of this lane (even); 2 n elements of its run
    const bool vec = a.aligned && n == 8;
    const int j0 = x0 >> 1;

    // chroma of the two output rows 2i, 2i + 1: cv[c][parity][k], columns j0 + k (chroma_row's index k + 1)
    int cv[2][2][4];
    #pragma unroll
    for (int c = 0; c < 2; c++) {
        int r0[6];
        chroma_row(a, c + 1, i, j0, r0);
        if (UP == XGPU_UPSAMPLE_NEAREST) {
            #pragma unroll
            for (int k = 0; k < 4; k++) cv[c][0][k] = cv[c][1][k] = r0[k + 1];
        } else {
            int rm[6], rp[6];
            chroma_row(a, c + 1, max(i - 1, 0), j0, rm);
            chroma_row(a, c + 1, min(i + 1, a.ch - 1), j0, rp);
            #pragma unroll
            for (int k = 0; k < 4; k++) {
                cv[c][0][k] = (a.ve[0] * rm[k + 1] + a.ve[1] * r0[k + 1] + 2) >> 2;
                cv[c][1][k] = (a.vo[0] * r0[k + 1] + a.vo[1] * rp[k + 1] + 2) >> 2;
            }
        }
    }

    #pragma unroll
    for (int par = 0; par < 2; par++) {
        const int row = 2 * i + par;
        const S16x8u ly = *(const S16x8u *)(a.y + (size_t)row * a.sy + x0);
        uint32_t e[16];
        #pragma unroll
        for (int k = 0; k < 4; k++) {
            int y0 = ly.v[2 * k], y1 = ly.v[2 * k + 1];
            if (a.dra) { y0 = dra1(a.dra, 0, y0, 0); y1 = dra1(a.dra, 0, y1, 0); }
            const uint32_t ey0 = packed_elem(a, y0), ey1 = packed_elem(a, y1);
            const uint32_t eb = packed_elem(a, cv[0][par][k]), er = packed_elem(a, cv[1][par][k]);
            e[4 * k]     = UYVY ? eb : ey0;
            e[4 * k + 1] = UYVY ? ey0 : eb;
            e[4 * k + 2] = UYVY ? er : ey1;
            e[4 * k + 3] = UYVY ? ey1 : er;
        }
        store_run<16, SZ>(a.dst + (size_t)row * a.pitch + (size_t)x0 * 2 * SZ, e, vec, 2 * n);
    }
}

template <int DT, bool UYVY>
static void launch_packed_422_up(const Packed422Args &a, int upsample, dim3 grid, hipStream_t s)
{
    if (upsample == XGPU_UPSAMPLE_NEAREST) hipLaunchKernelGGL((k_output_packed_422<DT, UYVY, XGPU_UPSAMPLE_NEAREST>), grid, dim3(64, 4), 0, s, a);
    else                                   hipLaunchKernelGGL((k_output_packed_422<DT, UYVY, XGPU_UPSAMPLE_LINEAR>), grid, dim3(64, 4), 0, s, a);
}
void launch_output_packed_422(const Packed422Args &a, int dtype, bool uyvy, int upsample, hipStream_t s)
{
    const dim3 grid = three_channel_grid(a);
    if (dtype == XGPU_OUT_U8) { if (uyvy) launch_packed_422_up<XGPU_OUT_U8, true>(a, upsample, grid, s); else launch_packed_422_up<XGPU_OUT_U8, false>(a, upsample, grid, s); }
    else                      { if (uyvy) launch_packed_422_up<XGPU_OUT_U16, true>(a, upsample, grid, s); else launch_packed_422_up<XGPU_OUT_U16, false>(a, upsample, grid, s); }
}
