// xgpu_resample.hip - the tap tables of the bicubic resize (xgpu_resample_taps).  Host only, and integers only, like xgpu_scale.hip, whose
// notation this keeps: one axis of one plane, n plane samples, subsampling s, siting d = h / 2 luma samples, N destination samples, over D = 2 s N
//   c(o) = C / D with C = (2 o + 1) n s - (1 + h) N,      f = F / D with F = antialias ? max(D, 2 s n) : D.
// Sample i lies in the row of o when |i - c| < 2 f, that is t = |i D - C| < 2 F, and its weight is k(t / F) with k the BC-spline.  With B = b / 12 and C = c / 12
// (every kernel offered has such b, c) 72 F^3 k is a polynomial in t and F with integer coefficients:
//   t < F         (144 - 9 b - 6 c) t^3 + (-216 + 12 b + 6 c) t^2 F + (72 - 2 b) F^3
//   F <= t < 2 F  (-b - 6 c) t^3 + (6 b + 30 c) t^2 F + (-12 b - 48 c) t F^2 + (8 b + 24 c) F^3
// The factor 1 / (72 F^3) cancels in the normalisation: a row is its numerators u(i), of either sign, their sum U, and
//   q(i) = floor(u(i) 16384 / U + 1 / 2) = floor((2 u(i) 16384 + U) / (2 U));   16384 - sum q goes to the largest q (the first of equals).
// t^3 reaches 2^57 and the products pass int64, so the numerators are __int128.  tests/resample_ref.py restates the construction with fractions.Fraction.
#include "xgpu_internal.h"
#include <algorithm>
#include <vector>

typedef __int128 i128;
static i128 floor_div(i128 a, i128 b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }      // b > 0

int xgpu_resample_taps(int n_plane, int subsampling, int siting_half_luma, int n_dst, int kernel, int antialias, int32_t *first, int32_t *count, int16_t *w, int w_stride)
{
    static const int bc[3][2] = { { 0, 6 }, { 0, 9 }, { 4, 4 } };      // 12 B, 12 C of XGPU_RESAMPLE_CATMULL_ROM, _CUBIC_075, _MITCHELL
    const int64_t n = n_plane, s = subsampling, h = siting_half_luma, N = n_dst;
    if (n < 1 || n > 65536 || (s != 1 && s != 2) || h < 0 || h > 2 || kernel < 0 || kernel > 2 || (antialias & ~1) || !first || !count || (w && w_stride < 1))
        return XGPU_ERR_INVALID_ARGUMENT;
    // the limits of section 8d in luma samples
    if (N < 2 || N > 16384 || n * s > 64 * N || N > 8 * n * s) return XGPU_ERR_UNSUPPORTED;
    const int b = bc[kernel][0], c = bc[kernel][1];
    const i128 in3 = 144 - 9 * b - 6 * c, in2 = -216 + 12 * b + 6 * c, in0 = 72 - 2 * b;
    const i128 out3 = -b - 6 * c, out2 = 6 * b + 30 * c, out1 = -12 * b - 48 * c, out0 = 8 * b + 24 * c;
    const int64_t D = 2 * s * N, F = antialias ? std::max(D, 2 * s * n) : D;
    std::vector<i128> u;
    std::vector<int64_t> q;
    int widest = 0;
    for (int o = 0; o < n_dst; o++) {
        const int64_t C = (2 * (int64_t)o + 1) * n * s - (1 + h) * N;
        int64_t lo = (int64_t)floor_div(C - 2 * F, D) + 1, hi = -(int64_t)floor_div(-(C + 2 * F), D) - 1;      // C - 2 F < i D < C + 2 F
        lo = std::max<int64_t>(lo, 0); hi = std::min(hi, n - 1);
        u.clear();
        i128 U = 0;
        for (int64_t i = lo; i <= hi; i++) {
            const i128 t = i * D > C ? i * D - C : C - i * D, f = F;
            const i128 v = t < f ? (in3 * t + in2 * f) * t * t + in0 * f * f * f : ((out3 * t + out2 * f) * t + out1 * f * f) * t + out0 * f * f * f;
            u.push_back(v);
            U += v;
        }
        if (u.empty()) {      // no sample of the plane under the window: the nearest one, with the whole weight
            lo = std::min(std::max<int64_t>((int64_t)floor_div(2 * C + D, 2 * D), 0), n - 1);
            u.push_back(1);
            U = 1;
        }
        if (U <= 0) return XGPU_ERR_UNSUPPORTED;
        const int cnt = (int)u.size();
        q.resize(cnt);
        int64_t sum = 0, mag = 0;
        int best = 0;
        for (int k = 0; k < cnt; k++) {
            q[k] = (int64_t)floor_div(2 * u[k] * 16384 + U, 2 * U);
            sum += q[k];
            if (q[k] > q[best]) best = k;
        }
        q[best] += 16384 - sum;
        for (int k = 0; k < cnt; k++) mag += q[k] < 0 ? -q[k] : q[k];
        if (mag > 32768) return XGPU_ERR_UNSUPPORTED;
        first[o] = (int32_t)lo;
        count[o] = cnt;
        widest = std::max(widest, cnt);
        if (!w) continue;
        if (cnt > w_stride) return XGPU_ERR_INVALID_ARGUMENT;
        int16_t *row = w + (size_t)o * w_stride;
        for (int k = 0; k < w_stride; k++) row[k] = k < cnt ? (int16_t)q[k] : 0;
    }
    return widest;
}
