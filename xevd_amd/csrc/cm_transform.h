// cm_transform.h - the colour transform of one pixel as the kernels that apply it run it (k_output_cm.hip at full size, k_output_scaled_cm.hip behind the scaled
// outputs' filter): the R'G'B' code of the fixed-point path at the coding depth -> linear light (one table lookup per channel) -> destination primaries (3x3) ->
// tone curve or scale, clip -> destination transfer characteristic (an interpolated table lookup per channel) -> the output dtype.  The arithmetic is the contract
// of INTEGRATION.md section 8b and tests/colour_cm_ref.py restates it bit for bit, so: no powf / exp2f / log2f, every float32 multiply and add rounded on its own
// (the files that include this header switch contraction into FMA off first), tables made by the host in double precision (xgpu_colour.hip).
#pragma once
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

// the tables in LDS, copied by a workgroup of 64 x 4: lin[n_lin], then tone and encode (XGPU_CM_CURVE_SIZE each) where the transform has them
__device__ __forceinline__ void cm_fill_lds(const CmParams &a, float *lds)
{
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int i = tid; i < a.n_lin; i += 256) lds[i] = a.lin[i];
    float *d = lds + a.n_lin;
    if (a.tone) { for (int i = tid; i < XGPU_CM_CURVE_SIZE; i += 256) d[i] = a.tone[i]; d += XGPU_CM_CURVE_SIZE; }
    if (a.enc) for (int i = tid; i < XGPU_CM_CURVE_SIZE; i += 256) d[i] = a.enc[i];
    __syncthreads();
}

// one pixel: (Y, Cb, Cr) at the coding depth -> the bits of three elements of dtype DT in R, G, B order.  a: the matrix of the U16 form; p: the transform;
// t: where its tables are read - in LDS (cm_fill_lds's layout: cm_lds_tables) or in global memory (p.lin, p.tone, p.enc themselves)
struct CmTables { const float *lin, *tone, *enc; };
__device__ __forceinline__ CmTables cm_lds_tables(const CmParams &p, const float *lds)
{
    return { lds, lds + p.n_lin, lds + p.n_lin + (p.tone ? XGPU_CM_CURVE_SIZE : 0) };
}
// the two halves of cm_apply.  k_output_scaled_lin.hip runs them apart, with its filter between them.
// cm_linearise: (Y, Cb, Cr) at the coding depth -> linear light of the source primaries, R, G, B
__device__ __forceinline__ void cm_linearise(const RgbOutArgs &a, const float *lin, int y, int cb, int cr, float &e0, float &e1, float &e2)
{
    // the integer R'G'B' of k_output_rgb's U16 form: the code at the coding depth
    const int yy = y - a.yo, u = cb - a.co, v = cr - a.co;
    const int ty = a.coef[0] * yy + (1 << (a.shift - 1));
    e0 = lin[min(max((ty + a.coef[1] * v) >> a.shift, 0), a.maxv)];
    e1 = lin[min(max((ty + a.coef[2] * u + a.coef[3] * v) >> a.shift, 0), a.maxv)];
    e2 = lin[min(max((ty + a.coef[4] * u) >> a.shift, 0), a.maxv)];
}
// cm_from_linear: linear light of the source primaries -> the bits of three elements of dtype DT (t.lin is not read)
template <int DT>
__device__ __forceinline__ void cm_from_linear(const CmParams &p, const CmTables &t, float e0, float e1, float e2, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const float *tone = t.tone, *enc = t.enc;
    float q3[3] = { e0, e1, e2 };
    if (p.use_matrix) {
        #pragma unroll
        for (int c = 0; c < 3; c++) q3[c] = cm_dot(p.m + 3 * c, e0, e1, e2);
    }
    float s = p.scale;
    if (p.tone) {      // g(Y) / Y: the division is IEEE (correctly rounded); Y = 0 is black, whatever the gain
        const float yl = cm_clip01(cm_dot(p.luma, e0, e1, e2));
        s = yl > 0.f ? cm_curve(tone, yl) / yl : 0.f;
    }
    uint32_t o[3];
    #pragma unroll
    for (int c = 0; c < 3; c++) {
        float q = cm_clip01(q3[c] * s);
        if (p.enc) q = cm_curve(enc, q);
        o[c] = OutT<DT>::is_float ? fbits<DT>(q) : (uint32_t)__float2int_rn(q * p.outmax);
    }
    r = o[0]; g = o[1]; b = o[2];
}
template <int DT>
__device__ __forceinline__ void cm_apply(const RgbOutArgs &a, const CmParams &p, const CmTables &t, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    float e0, e1, e2;
    cm_linearise(a, t.lin, y, cb, cr, e0, e1, e2);
    cm_from_linear<DT>(p, t, e0, e1, e2, r, g, b);
}

// The CONV of three_channel_rows (output_common.h) with a transform, for the kernels at full size (k_output_cm, k_output_packed_rgb, k_output_dither_rgb): the
// arguments are a CmOutArgs handed through as its base, and the tables lie at the front of dynamic LDS - the kernel calls cm_fill_lds(a.cm, cm_lds) first, every
// thread of the workgroup, before the lanes outside the picture leave, and is launched with cm_lds_bytes.  The F32 instance gives the float32 q of every channel,
// before a code is made of it (the dither's).
template <int DT> struct CmConv {
__device__ static __forceinline__ void apply(const RgbOutArgs &a0, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const CmOutArgs &a = static_cast<const CmOutArgs &>(a0);
    extern __shared__ float cm_lds[];
    cm_apply<DT>(a, a.cm, cm_lds_tables(a.cm, cm_lds), y, cb, cr, r, g, b);
}
};
// the bytes of a transform's tables in LDS (cm_fill_lds's layout): at most 32.8 KB
static size_t cm_lds_bytes(const CmParams &p) { return sizeof(float) * ((size_t)p.n_lin + (p.tone ? XGPU_CM_CURVE_SIZE : 0) + (p.enc ? XGPU_CM_CURVE_SIZE : 0)); }
