// k_output_lut3d.hip - k_output_rgb and k_output_packed_rgb with a 3D LUT between the matrix and the store (xgpu_pic_output_device_lut3d / _packed_lut3d): the
// R'G'B' code of the fixed-point path at the coding depth -> a per-channel shaper table -> tetrahedral interpolation between four nodes of an n x n x n cube of
// uint16 triples -> the output dtype.  Load, clamp, DRA, upsampling and the stores are output_common.h's, untouched: output_three_channels for the RGB layouts,
// output_three_sinks - k_output_packed_rgb's body - for the packed ones; this file adds the CONV.  All of the arithmetic is unsigned 32-bit integer (INTEGRATION.md
// section 8q; tests/lut3d_ref.py restates it bit for bit): the weights of a cell sum to 65535, a node is at most 65535, so every sum stays below 2^32.
// The kernel is a gather behind a streaming read: 16 pixels per lane, per pixel three shaper reads and four 8-byte node records (R | G << 16, B | 0 << 16 - one
// load per vertex).  The shaper (6 KB at 10 bit, 24 KB at 12) is copied into LDS by every workgroup, the cube is read from global memory through L1 / L2 at every
// n: at 8K 10 bit the shaper in LDS is 1.1 - 1.3 times faster than in global memory on every picture, and a copy of the n = 17 cube in LDS next to it (39 KB, two
// workgroups per CU) is 1.2 times faster on a picture of random samples but 1.1 times slower on a smooth one, where neighbouring pixels share cells - what a
// decoded picture looks like (DESIGN.md section 5c has the measurements; the instances of the two forms that lost were dropped after them).
#pragma clang fp contract(off)
#include "output_common.h"

// x / 65535 for x <= 65535^2 + 32767 (nothing overflows: x + (x >> 16) + 1 < 2^32 there)
__device__ __forceinline__ uint32_t lut3d_div65535(uint32_t x) { return (x + (x >> 16) + 1) >> 16; }

// the shaper in LDS, copied by a workgroup of 64 x 4 in whole 16-byte groups (3 x 2^B uint16)
__device__ __forceinline__ void lut3d_fill_lds(const Lut3dOutArgs &a, uint4 *lds)
{
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int ns = (3 * (a.maxv + 1)) >> 3;
    for (int i = tid; i < ns; i += 256) lds[i] = ((const uint4 *)a.shaper)[i];
    __syncthreads();
}

// The CONV: one pixel's (Y, Cb, Cr) at the coding depth -> the bits of three elements of dtype DT in R, G, B order.  The shaper lies at the front of dynamic LDS
// (lut3d_fill_lds), the cube is a.cube.
template <int DT> struct Lut3dConv {
__device__ static __forceinline__ void apply(const RgbOutArgs &a0, int y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
    const Lut3dOutArgs &a = static_cast<const Lut3dOutArgs &>(a0);
    extern __shared__ uint4 lut3d_lds[];
    const uint16_t *sh = (const uint16_t *)lut3d_lds;
    const uint2 *cube = a.cube;

    // the integer R'G'B' of k_output_rgb's U16 form: the code at the coding depth (cm_linearise's)
    const int yy = y - a.yo, u = cb - a.co, v = cr - a.co;
    const int ty = a.coef[0] * yy + (1 << (a.shift - 1));
    const int c[3] = { min(max((ty + a.coef[1] * v) >> a.shift, 0), a.maxv), min(max((ty + a.coef[2] * u + a.coef[3] * v) >> a.shift, 0), a.maxv),
                       min(max((ty + a.coef[4] * u) >> a.shift, 0), a.maxv) };
    // the cell and the position inside it: f in [0, 65535], i <= n - 2, so that every vertex below is a node of the cube
    const uint32_t n = (uint32_t)a.n, nn = n * n, step[3] = { 1u, n, nn };
    uint32_t f[3], idx = 0;
    #pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t q = (uint32_t)sh[k * (a.maxv + 1) + c[k]] * (n - 1);
        const uint32_t i = min(lut3d_div65535(q), n - 2);
        f[k] = q - 65535u * i;
        idx += i * step[k];
    }
    // the tetrahedron: V1 steps on an axis of the largest f, V2 is V3 minus a step on an axis of the smallest; where two axes tie, the vertex that depends on the
    // choice has weight 0
    const uint32_t fa = max(max(f[0], f[1]), f[2]), fc = min(min(f[0], f[1]), f[2]), fb = f[0] + f[1] + f[2] - fa - fc;
    const uint32_t sa = f[0] == fa ? 1u : f[1] == fa ? n : nn;
    const uint32_t sc = f[2] == fc ? nn : f[1] == fc ? n : 1u;
    const uint32_t far = idx + 1u + n + nn;
    const uint2 v0 = cube[idx], v1 = cube[idx + sa], v2 = cube[far - sc], v3 = cube[far];
    const uint32_t w0 = 65535u - fa, w1 = fa - fb, w2 = fb - fc, w3 = fc;
    uint32_t o[3];
    o[0] = w0 * (v0.x & 0xFFFFu) + w1 * (v1.x & 0xFFFFu) + w2 * (v2.x & 0xFFFFu) + w3 * (v3.x & 0xFFFFu);
    o[1] = w0 * (v0.x >> 16) + w1 * (v1.x >> 16) + w2 * (v2.x >> 16) + w3 * (v3.x >> 16);
    o[2] = w0 * (v0.y & 0xFFFFu) + w1 * (v1.y & 0xFFFFu) + w2 * (v2.y & 0xFFFFu) + w3 * (v3.y & 0xFFFFu);
    #pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t val = lut3d_div65535(o[k] + 32767u);
        if (OutT<DT>::is_float) {
            float q = (float)val * (1.0f / 65535.0f);
            // The product is a float32 of its own before the dtype's rounding.  Left to itself the compiler makes the multiplication and the conversion to F16 one
            // mixed-precision instruction that rounds once, and v = 65519 (float32: exactly 1 - 2^-12, the middle of two halves) comes out as 0x3BFF, not 0x3C00.
            asm volatile("" : "+v"(q));
            o[k] = fbits<DT>(q);
        } else {
            o[k] = lut3d_div65535(val * a.dmax + 32767u);
        }
    }
    r = o[0]; g = o[1]; b = o[2];
}
};

static size_t lut3d_lds_bytes(const Lut3dOutArgs &a) { return (size_t)6 * (a.maxv + 1); }      // at most 24 KB

// ---- the two RGB layouts
template <int LAYOUT, int DT, int UP>
__global__ __launch_bounds__(256) void k_output_lut3d(const Lut3dOutArgs a)
{
    extern __shared__ uint4 lut3d_lds[];
    lut3d_fill_lds(a, lut3d_lds);      // (every thread of the workgroup, before the lanes outside the picture leave)
    output_three_channels<LAYOUT == XGPU_OUT_RGB_PLANAR, DT, UP, Lut3dConv<DT>>(a);
}

struct Lut3dKernels {
    template <bool PLANAR, int DT, int UP> static void launch(const RgbOutArgs &a0, dim3 grid, hipStream_t s)
    {
        const Lut3dOutArgs &a = static_cast<const Lut3dOutArgs &>(a0);      // launch_three_channels hands the reference through
        hipLaunchKernelGGL((k_output_lut3d<PLANAR ? XGPU_OUT_RGB_PLANAR : XGPU_OUT_RGB_INTERLEAVED, DT, UP>), grid, dim3(64, 4), lut3d_lds_bytes(a), s, a);
    }
};

void launch_output_lut3d(const Lut3dOutArgs &a, int layout, int dtype, int upsample, hipStream_t s)
{
    launch_three_channels<Lut3dKernels>(a, layout == XGPU_OUT_RGB_PLANAR, dtype, upsample, s);
}

// ---- the packed layouts: output_three_sinks' RGBA and 10:10:10:2 (RGBA in every dtype in one pass - the elements are the LUT rule's, not RgbConv's; 10:10:10:2
// is the U16 instance with dmax = 1023)
template <int SINK, int DT, int UP>
__global__ __launch_bounds__(256) void k_output_packed_lut3d(const Lut3dOutArgs a)
{
    extern __shared__ uint4 lut3d_lds[];
    lut3d_fill_lds(a, lut3d_lds);
    output_three_sinks<SINK, DT, UP, Lut3dConv<DT>>(a, a.alpha);
}

struct PackedLut3dKernels {
    template <int SINK, int DT, int UP> static void launch(const RgbOutArgs &a0, dim3 grid, hipStream_t s)
    {
        const Lut3dOutArgs &a = static_cast<const Lut3dOutArgs &>(a0);
        hipLaunchKernelGGL((k_output_packed_lut3d<SINK, DT, UP>), grid, dim3(64, 4), lut3d_lds_bytes(a), s, a);
    }
};

void launch_output_packed_lut3d(const Lut3dOutArgs &a, int layout, int dtype, int upsample, hipStream_t s)
{
    launch_three_packed<PackedLut3dKernels>(a, layout == XGPU_PACKED_RGB10A2, dtype, upsample, s);
}
