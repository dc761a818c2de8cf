// scale_taps.h - the integer constructions of the scaled outputs that the host and the device both run, each written once: one row of a tap table
// (xgpu_scale_taps on the host, k_rois_prepare on the device - INTEGRATION.md section 8d), the snapping of a box to an even rectangle inside the picture and the
// letterbox rule (xgpu_roi_snap / xgpu_roi_inner on the host, k_rois_prepare on the device - sections 8e, 8f).  Integers only but for the float32 steps of the
// F32 box format, each of which is exact.  No arrays: a row is made in two passes over its samples (its span and the sum of its numerators, then the weights),
// so that a lane of a kernel keeps it in registers.
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/xevd_hip.h"

#define XGPU_HD __host__ __device__ __forceinline__

// One axis of one plane (the notation of xgpu_scale.hip): n plane samples, subsampling s, siting h half luma samples, N destination samples of subsampling S and
// siting H half luma samples of the destination grid (S = 1, H = 0: a destination at luma resolution, xgpu_scale_taps), over D = 2 s N S.
struct ScaleAxis {
    int64_t n, s, h, N, S, H, D, F, reach;
    int     filter;
    int     kspan;      // the samples looked at from the first candidate of a row on: covers every sample within `reach` of the centre
    int     kw;         // no row is wider than this: floor(2 F / D) + 2
};

XGPU_HD int64_t scale_floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }      // b > 0

XGPU_HD void scale_axis_init(ScaleAxis &ax, int n_plane, int subsampling, int siting_half_luma, int n_dst, int filter, int dst_subsampling = 1,
                             int dst_siting_half_luma = 0)
{
    ax.n = n_plane; ax.s = subsampling; ax.h = siting_half_luma; ax.N = n_dst; ax.S = dst_subsampling; ax.H = dst_siting_half_luma; ax.filter = filter;
    ax.D = 2 * ax.s * ax.N * ax.S;
    ax.F = ax.D > 2 * ax.s * ax.S * ax.n ? ax.D : 2 * ax.s * ax.S * ax.n;
    // the samples that can have a positive weight: |i - c| < f (BILINEAR), |i - c| < (f + 1) / 2 (AREA) - one more on either side costs nothing
    ax.reach = filter == XGPU_SCALE_BILINEAR ? ax.F : (ax.F + ax.D + 1) / 2;
    // floor((C + reach) / D) + 1 - (floor((C - reach) / D) - 1) <= floor(2 reach / D) + 3 for every C
    ax.kspan = (int)(2 * ax.reach / ax.D) + 3;
    ax.kw = (int)(2 * ax.F / ax.D) + 2;
}

// the centre of destination sample o over D: C = (2 S o + H + 1) n s - (1 + h) N S
XGPU_HD int64_t scale_centre(const ScaleAxis &ax, int o) { return (2 * ax.S * (int64_t)o + ax.H + 1) * ax.n * ax.s - (1 + ax.h) * ax.N * ax.S; }

// the numerator u(i) of sample i in the row whose centre is C / D (<= 0: no weight)
XGPU_HD int64_t scale_tap_num(const ScaleAxis &ax, int64_t C, int64_t i)
{
    if (ax.filter == XGPU_SCALE_BILINEAR) {
        const int64_t t = i * ax.D - C;
        return ax.F - (t < 0 ? -t : t);
    }
    const int64_t a = (2 * i + 1) * ax.D, b = 2 * C + ax.F, c = (2 * i - 1) * ax.D, d = 2 * C - ax.F;
    return (a < b ? a : b) - (c > d ? c : d);
}

// Destination sample o: the first sample with a positive weight (*first), how many follow it contiguously (returned) and the sum of their numerators (*U).
// *U = 0: no sample of the plane lies under the window (a siting that moves the grid off the plane's end) - the nearest sample alone, with the whole weight.
XGPU_HD int scale_tap_span(const ScaleAxis &ax, int o, int32_t *first, int64_t *U)
{
    const int64_t C = scale_centre(ax, o);
    const int64_t l0 = scale_floor_div(C - ax.reach, ax.D) - 1;
    const int64_t lo = l0 > 0 ? l0 : 0, hi = l0 + ax.kspan < ax.n - 1 ? l0 + ax.kspan : ax.n - 1;
    int64_t i0 = 0, sum = 0;
    int cnt = 0;
    for (int64_t i = lo; i <= hi; i++) {
        const int64_t v = scale_tap_num(ax, C, i);
        if (v <= 0) { if (cnt == 0) continue; else break; }      // the positive weights are contiguous
        if (cnt == 0) i0 = i;
        cnt++;
        sum += v;
    }
    if (cnt == 0) {
        i0 = scale_floor_div(2 * C + ax.D, 2 * ax.D);
        i0 = i0 < 0 ? 0 : (i0 > ax.n - 1 ? ax.n - 1 : i0);
        cnt = 1;
    }
    *first = (int32_t)i0;
    *U = sum;
    return cnt;
}

// The weights of that row at q[k * step], k < cnt: q(i) = (2 u(i) 16384 + U) / (2 U), and 16384 - sum q goes to the largest q (the first of equals);
// zeros from cnt up to `width`.
XGPU_HD void scale_tap_weights(const ScaleAxis &ax, int o, int32_t first, int cnt, int64_t U, int16_t *q, size_t step, int width)
{
    const int64_t C = scale_centre(ax, o);
    int64_t sum = 0, bestv = 0;
    int best = 0;
    for (int k = 0; k < cnt; k++) {
        const int64_t v = U ? (2 * scale_tap_num(ax, C, first + k) * 16384 + U) / (2 * U) : 16384;
        q[(size_t)k * step] = (int16_t)v;
        sum += v;
        if (k == 0 || v > bestv) { best = k; bestv = v; }
    }
    q[(size_t)best * step] = (int16_t)(bestv + (16384 - sum));
    for (int k = cnt; k < width; k++) q[(size_t)k * step] = 0;
}

// one axis: n source samples to N destination samples is inside the limits of the scaled output (both counted in luma samples)
XGPU_HD bool scale_ratio_ok(int n, int N) { return N >= 2 && n <= 64 * (int64_t)N && N <= 8 * (int64_t)n; }

// the filtered part of a ws x hs rectangle inside a wd x hd image (xgpu_roi_inner)
XGPU_HD void roi_inner(int ws, int hs, int wd, int hd, int fit, int inner[4])
{
    int wi = wd, hi = hd;
    if (fit == XGPU_FIT_LETTERBOX) {
        if ((int64_t)ws * hd >= (int64_t)hs * wd) {
            const int64_t v = (2 * (int64_t)hs * wd + ws) / (2 * (int64_t)ws);
            hi = (int)(v < 2 ? 2 : (v > hd ? hd : v));
        } else {
            const int64_t v = (2 * (int64_t)ws * hd + hs) / (2 * (int64_t)hs);
            wi = (int)(v < 2 ? 2 : (v > wd ? wd : v));
        }
    }
    inner[0] = (wd - wi) >> 1; inner[1] = (hd - hi) >> 1; inner[2] = wi; inner[3] = hi;
}

// One axis of the snapping rule: [lo, hi) outward to even, then into 0 .. limit (even)
XGPU_HD void roi_snap_axis_i32(int p, int len, int limit, int *p0, int *p1)
{
    const int64_t a = (int64_t)p & ~(int64_t)1, b = ((int64_t)p + len + 1) & ~(int64_t)1;
    *p0 = (int)(a > 0 ? (a < limit ? a : limit) : 0);
    *p1 = (int)(b < limit ? (b > 0 ? b : 0) : limit);
}
XGPU_HD void roi_snap_axis_f32(float lo, float hi, int limit, int *p0, int *p1)
{
    const float top = 1048576.f;      // 2^20: beyond any picture, and every step below is exact in float32
    lo = fminf(fmaxf(lo, -top), top); hi = fminf(fmaxf(hi, -top), top);
    const int a = 2 * (int)floorf(lo * 0.5f), b = 2 * (int)ceilf(hi * 0.5f);
    *p0 = a > 0 ? (a < limit ? a : limit) : 0;
    *p1 = b < limit ? (b > 0 ? b : 0) : limit;
}
// a box of either format -> its status (XGPU_ROI_OK, _INVALID, _EMPTY) and, with XGPU_ROI_OK, the even rectangle inside pw x ph
XGPU_HD int roi_snap_box(int box_format, const void *box, int pw, int ph, xgpu_roi *used)
{
    int x0, x1, y0, y1;
    if (box_format == XGPU_BOX_XYXY_F32) {
        const float *b = (const float *)box;
        // finite: the exponent field is not all ones
        for (int k = 0; k < 4; k++) if (!(fabsf(b[k]) <= 3.402823466e38f)) return XGPU_ROI_INVALID;
        roi_snap_axis_f32(b[0], b[2], pw, &x0, &x1);
        roi_snap_axis_f32(b[1], b[3], ph, &y0, &y1);
    } else {
        const int *b = (const int *)box;
        roi_snap_axis_i32(b[0], b[2], pw, &x0, &x1);
        roi_snap_axis_i32(b[1], b[3], ph, &y0, &y1);
    }
    if (x1 - x0 < 2 || y1 - y0 < 2) return XGPU_ROI_EMPTY;
    used->x = x0; used->y = y0; used->width = x1 - x0; used->height = y1 - y0;
    return XGPU_ROI_OK;
}
