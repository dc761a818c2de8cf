// k_output_cm.hip - k_output_rgb with a colour transform between the matrix and the store (xgpu_pic_output_device_cm): the R'G'B' code of the fixed-point
// path at the coding depth -> linear light (one table lookup per channel) -> destination primaries (3x3) -> tone curve or scale, clip -> destination
// transfer characteristic (an interpolated table lookup per channel) -> the output dtype.  Load, clamp, DRA, upsampling and the stores are
// output_three_channels (output_common.h), untouched; this file adds the CONV.  The arithmetic is the contract of INTEGRATION.md section 8b and
// tests/colour_cm_ref.py restates it bit for bit, so: no powf / exp2f / log2f, every float32 multiply and add rounded on its own (contraction into FMA is
// switched off for this file), tables made by the host in double precision (xgpu_colour.hip).
// The tables (4 KB .. 16 KB of linearisation, 8 KB per curve) are copied into LDS by every workgroup: at 8K 10 bit that is 1.2 - 1.45 times faster than
// reading them from global memory through L1 / L2 on a picture of random samples, although each workgroup copies ~5000 floats for its 4096 pixels
// (DESIGN.md section 5c has both measurements; the instances that read global memory were dropped after it).
#pragma clang fp contract(off)
#include "output_common.h"

// a curve table at v in [0, 1] (+0 .. 1.0: cm_clip01's result; include/xevd_hip.h, XGPU_CM_CURVE_*): entries at the float32 bit patterns U0 + (j << 18), linear in between
__device__ __forceinline__ float cm_curve(const float *t, float v)
{
    const uint32_t u = __float_as_uint(v);
    int k = 0;
    float fr = v * 0x1p64f;
    if (u >= XGPU_CM_CURVE_U0) { k = min((int)((u - XGPU_CM_CURVE_U0) >> 18) + 1, XGPU_CM_CURVE_SIZE - 2); fr = (float)(int)(u & 0x3FFFFu) * 0x1p-18f; }
    const float t0 = t[k], t1 = t[k + 1];
    return t0 + fr * (t1 - t0);
}
__device__ __forceinline__ float cm_dot(const float *m, float r, float g, float b) { return (m[0] * r + m[1] * g) + m[2] * b; }
__device__ __forceinline__ float cm_clip01(float v) { return fminf(v > 0.f ? v : 0.f, 1.f); }      // -0 and NaN -> +0

// the tables in LDS: lin[n_lin], then tone and encode (XGPU_CM_CURVE_SIZE each) where the transform has them
__device__ __forceinline__ void cm_fill_lds(const CmOutArgs &a, float *lds)
{
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int i = tid; i < a.n_lin; i += 256) lds[i] = a.lin[i];
    float *d = lds + a.n_lin;
    if (a.tone) { for (int i = tid; i < XGPU_CM_CURVE_SIZE; i += 256) d[i] = a.tone[i]; d += XGPU_CM_CURVE_SIZE; }
    if (a.enc) for (int i = tid; i < XGPU_CM_CURVE_SIZE; i += 256) d[i] = a.enc[i];
    __syncthreads();
}

template <int DT> struct CmConv {
__device__ static __forceinline__ void apply(const RgbOutArgs &a0, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const CmOutArgs &a = static_cast<const CmOutArgs &>(a0);
    extern __shared__ float cm_lds[];
    const float *lin = cm_lds, *tone = cm_lds + a.n_lin, *enc = cm_lds + a.n_lin + (a.tone ? XGPU_CM_CURVE_SIZE : 0);      // cm_fill_lds's layout
    // the integer R'G'B' of k_output_rgb's U16 form: the code at the coding depth
    const int yy = y - a.yo, u = cb - a.co, v = cr - a.co;
    const int ty = a.coef[0] * yy + (1 << (a.shift - 1));
    const float e0 = lin[min(max((ty + a.coef[1] * v) >> a.shift, 0), a.maxv)];
    const float e1 = lin[min(max((ty + a.coef[2] * u + a.coef[3] * v) >> a.shift, 0), a.maxv)];
    const float e2 = lin[min(max((ty + a.coef[4] * u) >> a.shift, 0), a.maxv)];
    float p[3] = { e0, e1, e2 };
    if (a.use_matrix) {
        #pragma unroll
        for (int c = 0; c < 3; c++) p[c] = cm_dot(a.m + 3 * c, e0, e1, e2);
    }
    float s = a.scale;
    if (a.tone) {      // g(Y) / Y: the division is IEEE (correctly rounded); Y = 0 is black, whatever the gain
        const float yl = cm_clip01(cm_dot(a.luma, e0, e1, e2));
        s = yl > 0.f ? cm_curve(tone, yl) / yl : 0.f;
    }
    uint32_t o[3];
    #pragma unroll
    for (int c = 0; c < 3; c++) {
        float q = cm_clip01(p[c] * s);
        if (a.enc) q = cm_curve(enc, q);
        o[c] = OutT<DT>::is_float ? fbits<DT>(q) : (uint32_t)__float2int_rn(q * a.outmax);
    }
    r = o[0]; g = o[1]; b = o[2];
}
};

template <int LAYOUT, int DT, int UP>
__global__ __launch_bounds__(256) void k_output_cm(const CmOutArgs a)
{
    extern __shared__ float cm_lds[];
    cm_fill_lds(a, cm_lds);      // (every thread of the workgroup, before the lanes outside the picture leave)
    output_three_channels<LAYOUT == XGPU_OUT_RGB_PLANAR, DT, UP, CmConv<DT>>(a);
}

struct CmKernels {
    template <bool PLANAR, int DT, int UP> static void launch(const RgbOutArgs &a0, dim3 grid, hipStream_t s)
    {
        const CmOutArgs &a = static_cast<const CmOutArgs &>(a0);      // launch_three_channels hands the reference through
        const size_t lds = sizeof(float) * (a.n_lin + (a.tone ? XGPU_CM_CURVE_SIZE : 0) + (a.enc ? XGPU_CM_CURVE_SIZE : 0));      // at most 32.8 KB
        hipLaunchKernelGGL((k_output_cm<PLANAR ? XGPU_OUT_RGB_PLANAR : XGPU_OUT_RGB_INTERLEAVED, DT, UP>), grid, dim3(64, 4), lds, s, a);
    }
};

void launch_output_cm(const CmOutArgs &a, int layout, int dtype, int upsample, hipStream_t s)
{
    launch_three_channels<CmKernels>(a, layout == XGPU_OUT_RGB_PLANAR, dtype, upsample, s);
}
