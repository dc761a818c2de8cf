// k_output_overlay.hip - the integer device outputs with a list of layers alpha-blended over the picture (xgpu_pic_output_device_overlaid,
// xgpu_pic_output_device_packed_overlaid): bitmaps in device memory (RGBA8, BGRA8, A8 coverage of one colour), boxes from the host and boxes a detector left in
// device memory, blended in the output's own code domain, integers only.  The contract is INTEGRATION.md section 8s; tests/overlay_ref.py restates it in numpy.
//
// k_output_overlay_rgb: k_output_packed_rgb's body, output_three_sinks (output_common.h) with RgbConv's / CmConv's integer instances, so a row's 3 x 8 elements are
// the plain call's bits when the finish step gets them; the finish step, which knows row and column, blends the layers over them.  The bgr swap follows it, so a
// layer's colour is swapped as the picture's is.
//
// k_output_overlay_semiplanar: a body of its own after output_semiplanar's (16 luma columns of two rows and 8 + 8 chroma samples per lane, the same loads,
// conversion and stores): all of the lane's samples are made first, at depth D and before P016's shift, then the layers are blended - luma per pixel, a chroma
// sample with the sum of the alphas of its four luma pixels -, then the stores.
//
// Uniform reject first.  A workgroup's tile is 512 x 8 pixels (1024 x 8 for the surfaces) and is known from blockIdx alone; the layers' rectangles are kernel
// arguments and the device boxes are read through the constant address space (k_overlay_prepare wrote them in an earlier launch on the same stream), so the
// loop over boxes and layers and its compare against the tile are scalar work, and a layer that misses the tile costs no vector instruction.  A tile no layer
// touches runs the plain call's conversion and stores and that loop.
//
// Bitmap reads are predicated per pixel: a byte (A8) or an aligned word (RGBA8 / BGRA8) of the bitmap is loaded only for a pixel (x, y) with x0 <= x < x1 and
// y0 <= y < y1 of the layer's own unclipped rectangle, from pix + (y - y0) * pitch + (x - x0) * bpp - an address inside row y - y0's width * bpp bytes, hence
// inside (height - 1) * pitch + width * bpp.  There is no vector load of a run and no tail: a lane whose run a layer's edge cuts, and a lane's pixels past the
// picture's width (which are computed and never stored), take the same per-pixel test, and a pixel outside the rectangle loads nothing.  The host has checked
// that the allocation holds those bytes.
//
// k_overlay_prepare: one thread per device box - the live count, the snap (overlay_rule.h), the palette entry by label - into the context's OvlBlock; a box that
// is skipped or misses the image is all zeros there, which no tile's compare accepts.
#pragma clang fp contract(off)
#include "cm_transform.h"
#include "overlay_rule.h"
#include <type_traits>

typedef const __attribute__((address_space(4))) OvlBlock *OvlBlockConst;

// every layer that touches the tile [tx0, tx1) x [ty0, ty1), device boxes first, in order: f(layer).  All of it is uniform over the workgroup.
template <class F>
__device__ __forceinline__ void ovl_for_tile(const OvlArgs &o, int tx0, int ty0, int tx1, int ty1, F &&f)
{
    const OvlBlockConst blk = (OvlBlockConst)o.boxes;
    const int cnt = o.boxes ? min(blk->count, XGPU_MAX_OVERLAY_BOXES) : 0;
    for (int t = 0; t < cnt + o.n; t++) {
        OvlLayer L;
        if (t < cnt) {
            L.x0 = blk->box[t].x0; L.y0 = blk->box[t].y0; L.x1 = blk->box[t].x1; L.y1 = blk->box[t].y1;
            L.kind = XGPU_OVL_BOX; L.opacity = 255; L.thickness = o.box_thickness;
            L.colour = blk->box[t].colour;
            L.fill = (L.colour & 0xFFFFFFu) | ((uint32_t)o.box_fill_alpha << 24);
            L.pitch = 0; L.pix = nullptr;
        } else {
            L = o.layer[t - cnt];
        }
        if (L.x0 >= tx1 || L.x1 <= tx0 || L.y0 >= ty1 || L.y1 <= ty0) continue;
        f(L);
    }
}

__device__ __forceinline__ uint32_t div255(uint32_t v) { return v / 255u; }

// layer L at pixel (x, y): its colour R | G << 8 | B << 16 and, in a, the effective alpha (0 outside the layer's rectangle).  The only loads of a bitmap.
__device__ __forceinline__ uint32_t ovl_sample(const OvlLayer &L, int x, int y, uint32_t &a)
{
    const bool in = x >= L.x0 && x < L.x1 && y >= L.y0 && y < L.y1;
    uint32_t c = L.colour, a8 = 0;
    if (L.kind == XGPU_OVL_BOX) {
        const int d = min(min(x - L.x0, L.x1 - 1 - x), min(y - L.y0, L.y1 - 1 - y));
        c = d < L.thickness ? L.colour : L.fill;
        a8 = c >> 24;
    } else if (L.kind == XGPU_OVL_A8) {
        uint32_t m = 0;
        if (in) m = L.pix[(size_t)(y - L.y0) * L.pitch + (size_t)(x - L.x0)];
        a8 = div255(m * (L.colour >> 24) + 127u);
    } else {
        uint32_t p = 0;
        if (in) p = *(const uint32_t *)(L.pix + (size_t)(y - L.y0) * L.pitch + (size_t)(x - L.x0) * 4);
        if (L.kind == XGPU_OVL_BGRA8) p = (p & 0xFF00FF00u) | ((p >> 16) & 0xFFu) | ((p & 0xFFu) << 16);
        c = p;
        a8 = p >> 24;
    }
    a = in ? div255(a8 * (uint32_t)L.opacity + 127u) : 0u;
    return c;
}

template <int SINK, int DT, int UP, bool CM>
__global__ __launch_bounds__(256) void k_output_overlay_rgb(const OverlayRgbArgs a)
{
    if (CM) {
        extern __shared__ float cm_lds[];
        cm_fill_lds(a.cm, cm_lds);                // (every thread of the workgroup, before the lanes outside the picture leave)
    }
    const int tx0 = blockIdx.x * 512, ty0 = blockIdx.y * 8;
    const uint32_t M = (uint32_t)a.ov.maxv;
    output_three_sinks<SINK, DT, UP, std::conditional_t<CM, CmConv<DT>, RgbConv<DT>>>(a, a.alpha, [&](int row, int x0, uint32_t (&ch)[3][8]) {
        ovl_for_tile(a.ov, tx0, ty0, tx0 + 512, ty0 + 8, [&](const OvlLayer &L) {
            #pragma unroll
            for (int m = 0; m < 8; m++) {
                uint32_t al;
                const uint32_t c = ovl_sample(L, x0 + m, row, al);
                #pragma unroll
                for (int k = 0; k < 3; k++) {
                    const uint32_t cd = div255(((c >> (8 * k)) & 0xFFu) * M + 127u);
                    // no branch on al and no clamp of v: RgbConv / CmConv hand over elements already clipped to [0, M], and with al == 0 the quotient
                    // (v * 255 + 127) / 255 is v itself for every v < 2^24 - the element stays the plain call's
                    ch[k][m] = div255(ch[k][m] * (255u - al) + cd * al + 127u);
                }
            }
        });
    });
}

// (integer dtypes only)
template <bool CM> struct OverlayRgbKernels {
    template <int SINK, int DT, int UP> static void launch(const RgbOutArgs &a0, dim3 grid, hipStream_t s)
    {
        const OverlayRgbArgs &a = static_cast<const OverlayRgbArgs &>(a0);      // the launchers hand the reference through
        if constexpr (!OutT<DT>::is_float)
            hipLaunchKernelGGL((k_output_overlay_rgb<SINK, DT, UP, CM>), grid, dim3(64, 4), CM ? cm_lds_bytes(a.cm) : 0, s, a);
    }
};
template <class K>
static void launch_overlay_rgb(const OverlayRgbArgs &a, int sink, int dtype, int upsample, hipStream_t s)
{
    if (sink == OUT_SINK_PLANAR)           launch_three_layout<K, OUT_SINK_PLANAR>(a, dtype, upsample, s);
    else if (sink == OUT_SINK_INTERLEAVED) launch_three_layout<K, OUT_SINK_INTERLEAVED>(a, dtype, upsample, s);
    else                                   launch_three_packed<K>(a, sink == OUT_SINK_RGB10A2, dtype, upsample, s);
}
void launch_output_overlay_rgb(const OverlayRgbArgs &a, int sink, int dtype, int upsample, bool cm, hipStream_t s)
{
    if (cm) launch_overlay_rgb<OverlayRgbKernels<true>>(a, sink, dtype, upsample, s);
    else    launch_overlay_rgb<OverlayRgbKernels<false>>(a, sink, dtype, upsample, s);
}

// the colour c (R | G << 8 | B << 16) as Y', Cb, Cr codes of depth D: the forward matrix of xgpu_overlay_coeffs
__device__ __forceinline__ void ovl_ycc(const OvlArgs &o, uint32_t c, int M, int (&ycc)[3])
{
    const int r = c & 0xFF, g = (c >> 8) & 0xFF, b = (c >> 16) & 0xFF;
    #pragma unroll
    for (int i = 0; i < 3; i++)
        ycc[i] = min(max(o.off[i] + ((o.m[3 * i] * r + o.m[3 * i + 1] * g + o.m[3 * i + 2] * b + (1 << (o.s - 1))) >> o.s), 0), M);
}

template <int DT>
__global__ __launch_bounds__(256) void k_output_overlay_semiplanar(const OverlaySemiArgs a)
{
    constexpr int SZ = OutT<DT>::size;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 16;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= a.w || i >= a.ch) return;
    const int n = min(16, a.w - x0);              // luma columns of this lane (even) = elements of its run of the interleaved chroma row
    const bool vec = a.aligned && n == 16;

    S16x8u ly[2][2];
    #pragma unroll
    for (int par = 0; par < 2; par++) {
        const int16_t *l = a.y + (size_t)(2 * i + par) * a.sy + x0;
        ly[par][0] = *(const S16x8u *)l;
        ly[par][1] = *(const S16x8u *)(l + 8);
    }
    const S16x8u cb = *(const S16x8u *)(a.u + (size_t)i * a.sc + (x0 >> 1));
    const S16x8u cr = *(const S16x8u *)(a.v + (size_t)i * a.sc + (x0 >> 1));

    // the plain call's samples at depth D, before the P016 shift: ec = Cb Cr interleaved, el = the two luma rows
    int ec[16], el[2][16];
    #pragma unroll
    for (int k = 0; k < 8; k++) {
        int b = cb.v[k], r = cr.v[k];
        if (a.dra) {                              // the factor of chroma column j comes from the unmapped luma sample (2i, 2j)
            const int luma = ly[0][k >> 2].v[(2 * k) & 7];
            b = dra1(a.dra, 1, b, luma);
            r = dra1(a.dra, 2, r, luma);
        }
        ec[2 * k]     = conv1(b, a.shift, a.maxv, a.out8);
        ec[2 * k + 1] = conv1(r, a.shift, a.maxv, a.out8);
    }
    #pragma unroll
    for (int par = 0; par < 2; par++) {
        #pragma unroll
        for (int m = 0; m < 16; m++) {
            int y = ly[par][m >> 3].v[m & 7];
            if (a.dra) y = dra1(a.dra, 0, y, 0);
            el[par][m] = conv1(y, a.shift, a.maxv, a.out8);
        }
    }

    const int M = a.maxv;
    const int tx0 = blockIdx.x * 1024, ty0 = blockIdx.y * 8;
    ovl_for_tile(a.ov, tx0, ty0, tx0 + 1024, ty0 + 8, [&](const OvlLayer &L) {
        // a box or a coverage mask has at most two colours, the same for every lane: they go through the matrix once per layer, as scalar work
        const bool two = L.kind == XGPU_OVL_BOX || L.kind == XGPU_OVL_A8;
        int yc[3] = { 0, 0, 0 }, yf[3] = { 0, 0, 0 };
        if (two) { ovl_ycc(a.ov, L.colour, M, yc); ovl_ycc(a.ov, L.fill, M, yf); }
        #pragma unroll
        for (int k = 0; k < 8; k++) {
            uint32_t A = 0, sb = 0, sr = 0;
            #pragma unroll
            for (int q = 0; q < 4; q++) {
                const int par = q >> 1, m = 2 * k + (q & 1);
                uint32_t al;
                const uint32_t c = ovl_sample(L, x0 + m, 2 * i + par, al);
                int ycc[3];
                if (two) {
                    #pragma unroll
                    for (int j = 0; j < 3; j++) ycc[j] = c == L.colour ? yc[j] : yf[j];      // (ovl_sample hands back `colour` or `fill` itself)
                } else {
                    ovl_ycc(a.ov, c, M, ycc);
                }
                if (al) el[par][m] = (int)div255((uint32_t)min(max(el[par][m], 0), M) * (255u - al) + (uint32_t)ycc[0] * al + 127u);
                A += al; sb += al * (uint32_t)ycc[1]; sr += al * (uint32_t)ycc[2];
            }
            if (A) {
                ec[2 * k]     = (int)(((uint32_t)min(max(ec[2 * k], 0), M) * (1020u - A) + sb + 510u) / 1020u);
                ec[2 * k + 1] = (int)(((uint32_t)min(max(ec[2 * k + 1], 0), M) * (1020u - A) + sr + 510u) / 1020u);
            }
        }
    });

    uint32_t e[16];
    #pragma unroll
    for (int m = 0; m < 16; m++) e[m] = (uint32_t)(uint16_t)(ec[m] << a.lsh);
    store_run<16, SZ>(a.dst + a.chroma_off + (size_t)i * a.pitch + (size_t)x0 * SZ, e, vec, n);
    #pragma unroll
    for (int par = 0; par < 2; par++) {
        #pragma unroll
        for (int m = 0; m < 16; m++) e[m] = (uint32_t)(uint16_t)(el[par][m] << a.lsh);
        store_run<16, SZ>(a.dst + (size_t)(2 * i + par) * a.pitch + (size_t)x0 * SZ, e, vec, n);
    }
}

void launch_output_overlay_semiplanar(const OverlaySemiArgs &a, int dtype, hipStream_t s)
{
    if (dtype == XGPU_OUT_U8) hipLaunchKernelGGL(k_output_overlay_semiplanar<XGPU_OUT_U8>, semiplanar_grid(a.w, a.ch), dim3(64, 4), 0, s, a);
    else                      hipLaunchKernelGGL(k_output_overlay_semiplanar<XGPU_OUT_U16>, semiplanar_grid(a.w, a.ch), dim3(64, 4), 0, s, a);
}

// one thread per device box (capacity <= XGPU_MAX_OVERLAY_BOXES = the workgroup: the host refuses more, and the test below keeps every store inside box[])
__global__ __launch_bounds__(XGPU_MAX_OVERLAY_BOXES) void k_overlay_prepare(const OvlPrepArgs a)
{
    const int i = threadIdx.x;
    int live = a.capacity;
    if (a.count) live = min(max(*a.count, 0), a.capacity);
    if (i == 0) { a.blk->count = live; a.blk->pad_[0] = a.blk->pad_[1] = a.blk->pad_[2] = 0; }
    if (i >= a.capacity || i >= XGPU_MAX_OVERLAY_BOXES) return;
    OvlBox b = { 0, 0, 0, 0, 0u };
    int r[4];
    if (i < live && ovl_snap_box(a.box_format, (const uint8_t *)a.boxes + (size_t)i * 16, r) && r[0] < a.pw && r[2] > 0 && r[1] < a.ph && r[3] > 0) {
        const int lab = a.labels ? a.labels[i] : 0;
        b.x0 = r[0]; b.y0 = r[1]; b.x1 = r[2]; b.y1 = r[3];
        b.colour = a.palette[((lab % a.n_palette) + a.n_palette) % a.n_palette];
    }
    a.blk->box[i] = b;
}

void launch_overlay_prepare(const OvlPrepArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_overlay_prepare, dim3(1), dim3(XGPU_MAX_OVERLAY_BOXES), 0, s, a);
}
