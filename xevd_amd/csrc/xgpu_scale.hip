// xgpu_scale.hip - the tap tables of the scaled device output (xgpu_scale_taps).  Host only, and integers only: every quantity of the
// contract is a fraction over one common denominator, so centres, widths, weights and their sum are int64 numerators and no float or double appears anywhere.
// tests/scale_ref.py restates the construction with fractions.Fraction; the two agree tap for tap.
//
// One axis of one plane: n plane samples, subsampling s (1 luma, 2 chroma), siting d = h / 2 luma samples (h = 0, 1, 2), N destination samples.
//   r = n s / N          f = max(1, r / s) = max(1, n / N)          c(o) = ((o + 1/2) r - 1/2 - d) / s
// Over the denominator D = 2 s N:   c(o) = C / D with C = (2 o + 1) n s - (1 + h) N,   f = F / D with F = max(D, 2 s n).
// xgpu_scale_taps_ex (the surface ladder, section 8l): the destination has a subsampling S and a siting H / 2 luma samples of its own grid -
//   r = n s / (N S)      f = max(1, r S / s) = max(1, n / N)        c(o) = ((S o + H / 2 + 1/2) r - 1/2 - d) / s
// over D = 2 s N S:   C = (2 S o + H + 1) n s - (1 + h) N S,   F = max(D, 2 s S n).  S = 1, H = 0 is the line above, term for term.
//   BILINEAR   w(i) = max(0, 1 - |i - c| / f)                              = max(0, F - |i D - C|) / F
//   AREA       w(i) = | [i - 1/2, i + 1/2] ^ [c - f / 2, c + f / 2] |      = max(0, min((2 i + 1) D, 2 C + F) - max((2 i - 1) D, 2 C - F)) / (2 D)
// The common factor of a row (1 / F, 1 / (2 D)) cancels in the normalisation: a row is its integer numerators u(i) > 0 over 0 <= i < n, their sum U, and
//   q(i) = floor(u(i) 16384 / U + 1 / 2) = (2 u(i) 16384 + U) / (2 U) in integers;   16384 - sum q goes to the largest q (the first of equals).
#include "xgpu_internal.h"
#include "scale_taps.h"
#include <algorithm>
#include <cstring>
#include <vector>

int xgpu_scale_taps_ex(int n_plane, int subsampling, int siting_half_luma, int n_dst, int dst_subsampling, int dst_siting_half_luma, int filter,
                       int32_t *first, int32_t *count, int16_t *w, int w_stride)
{
    const int64_t n = n_plane, s = subsampling, h = siting_half_luma, N = n_dst, S = dst_subsampling, H = dst_siting_half_luma;
    if (n < 1 || n > 65536 || (s != 1 && s != 2) || h < 0 || h > 2 || (S != 1 && S != 2) || H < 0 || H > 2 ||
        (filter != XGPU_SCALE_BILINEAR && filter != XGPU_SCALE_AREA) || !first || !count || (w && w_stride < 1))
        return XGPU_ERR_INVALID_ARGUMENT;
    // the limits of section 8d in luma samples: n s source and N S destination samples
    if (N < 1 || N * S < 2 || N > 16384 || n * s > 64 * N * S || N * S > 8 * n * s) return XGPU_ERR_UNSUPPORTED;
    // the row itself is scale_taps.h's, which k_rois_prepare runs on the device as well
    ScaleAxis ax;
    scale_axis_init(ax, n_plane, subsampling, siting_half_luma, n_dst, filter, dst_subsampling, dst_siting_half_luma);
    int widest = 0;
    for (int o = 0; o < n_dst; o++) {
        int64_t U;
        const int cnt = scale_tap_span(ax, o, &first[o], &U);
        count[o] = cnt;
        widest = std::max(widest, cnt);
        if (!w) continue;
        if (cnt > w_stride) return XGPU_ERR_INVALID_ARGUMENT;
        scale_tap_weights(ax, o, first[o], cnt, U, w + (size_t)o * w_stride, 1, w_stride);
    }
    return widest;
}
// the destination at luma resolution on the luma grid: S = 1, H = 0
int xgpu_scale_taps(int n_plane, int subsampling, int siting_half_luma, int n_dst, int filter, int32_t *first, int32_t *count, int16_t *w, int w_stride)
{
    return xgpu_scale_taps_ex(n_plane, subsampling, siting_half_luma, n_dst, 1, 0, filter, first, count, w, w_stride);
}

// The four tables of one (source size, destination size, filter, chroma_loc) as the block the kernels read (k_output_scaled.hip): per table first[], count[] and
// the weights - row by row for the vertical tables (0 luma rows, 1 chroma rows), transposed for the horizontal ones (2 luma columns, 3 chroma columns) -, every
// array at a multiple of 16 bytes.  It also measures what pass 2 stages in LDS: the widest span of the intermediate that 64 neighbouring destination columns
// reach, from an 8-sample-aligned start.  The kernel takes a workgroup's span from its first and last column, so the rows must move right monotonically: checked
// here, for every table it is given, before anything reaches the device.  x_off (the batched output's letterbox, k_output_rois.hip): the groups of 64 are those
// of an image in which column 0 of the tables is column x_off.
// `taps`: the builder of one table - xgpu_scale_taps with the filter bound (scale_build_tables), xgpu_resample_taps with kernel and antialias bound
// (resample_build_tables, section 8o: rows with weights of either sign, laid out and measured the same way).
template <class TAPS>
static int build_tables(int ws, int hs, int wd, int hd, int chroma_loc, std::vector<uint8_t> &blob, ScaleTabs &tb, int x_off, TAPS &&taps)
{
    static const int vsite[3] = { 1, 0, 2 };      // ChromaSampleLocType >> 1: centred, top, bottom - in half luma samples
    const int n[4] = { hs, hs >> 1, ws, ws >> 1 }, sub[4] = { 1, 2, 1, 2 }, site[4] = { 0, vsite[chroma_loc >> 1], 0, chroma_loc & 1 }, N[4] = { hd, hd, wd, wd };
    blob.clear();
    auto reserve = [&](size_t bytes) { const size_t off = (blob.size() + 15) & ~(size_t)15; blob.resize(off + bytes); return off; };
    std::vector<int32_t> first, count;
    std::vector<int16_t> w;
    for (int t = 0; t < 4; t++) {
        first.assign(N[t], 0); count.assign(N[t], 0);
        const int widest = taps(n[t], sub[t], site[t], N[t], first.data(), count.data(), (int16_t *)NULL, 0);
        if (widest < 0) return widest;
        w.assign((size_t)N[t] * widest, 0);
        const int rc = taps(n[t], sub[t], site[t], N[t], first.data(), count.data(), w.data(), widest);
        if (rc < 0) return rc;
        for (int o = 0; o < N[t]; o++) {
            if (first[o] < 0 || count[o] < 1 || first[o] + count[o] > n[t]) return XGPU_ERR_UNEXPECTED;
            if (o && (first[o] < first[o - 1] || first[o] + count[o] < first[o - 1] + count[o - 1])) return XGPU_ERR_UNEXPECTED;
        }
        tb.off_first[t] = reserve(sizeof(int32_t) * N[t]);
        memcpy(&blob[tb.off_first[t]], first.data(), sizeof(int32_t) * N[t]);
        tb.off_count[t] = reserve(sizeof(int32_t) * N[t]);
        memcpy(&blob[tb.off_count[t]], count.data(), sizeof(int32_t) * N[t]);
        tb.off_w[t] = reserve(sizeof(int16_t) * w.size());
        int16_t *dw = (int16_t *)&blob[tb.off_w[t]];
        if (t < 2) {
            memcpy(dw, w.data(), sizeof(int16_t) * w.size());
            tb.stride[t] = widest;
        } else {
            for (int o = 0; o < N[t]; o++) for (int k = 0; k < widest; k++) dw[(size_t)k * N[t] + o] = w[(size_t)o * widest + k];
            tb.stride[t] = N[t];
            int cap = 0;
            for (int g = -x_off; g < N[t]; g += 64) {      // the columns one workgroup filters: 64 from a multiple of 64 of the image the table's columns start x_off into
                const int ob = std::max(g, 0), ol = std::min(g + 63, N[t] - 1);
                if (ol >= ob) cap = std::max(cap, ((first[ol] + count[ol] + 7) & ~7) - (first[ob] & ~7));
            }
            (t == 2 ? tb.capy : tb.capc) = cap;
        }
    }
    return XGPU_OK;
}
int scale_build_tables(int ws, int hs, int wd, int hd, int filter, int chroma_loc, std::vector<uint8_t> &blob, ScaleTabs &tb, int x_off)
{
    return build_tables(ws, hs, wd, hd, chroma_loc, blob, tb, x_off, [filter](int n, int s, int h, int N, int32_t *first, int32_t *count, int16_t *w, int stride) {
        return xgpu_scale_taps(n, s, h, N, filter, first, count, w, stride); });
}
int resample_build_tables(int ws, int hs, int wd, int hd, int kernel, int antialias, int chroma_loc, std::vector<uint8_t> &blob, ScaleTabs &tb, int x_off)
{
    return build_tables(ws, hs, wd, hd, chroma_loc, blob, tb, x_off, [kernel, antialias](int n, int s, int h, int N, int32_t *first, int32_t *count, int16_t *w, int stride) {
        return xgpu_resample_taps(n, s, h, N, kernel, antialias, first, count, w, stride); });
}

// One table of the surface ladder (k_output_ladder.hip) behind what `blob` holds already: first[], count[] and the weights - row by row (a vertical table) or
// transposed (a horizontal one) -, every array at a multiple of 16 bytes.  For a horizontal table *cap is the widest span of the intermediate that `group`
// neighbouring destination columns reach, from an 8-sample-aligned start; the kernel takes a workgroup's span from its first and last column, so the rows must move
// right monotonically, which is checked here.
int scale_build_axis(int n, int s, int h, int N, int S, int H, int filter, bool transposed, int group, std::vector<uint8_t> &blob, ScaleAxisTab &t, int *cap)
{
    auto reserve = [&](size_t bytes) { const size_t off = (blob.size() + 15) & ~(size_t)15; blob.resize(off + bytes); return off; };
    std::vector<int32_t> first(N), count(N);
    const int widest = xgpu_scale_taps_ex(n, s, h, N, S, H, filter, first.data(), count.data(), NULL, 0);
    if (widest < 0) return widest;
    std::vector<int16_t> w((size_t)N * widest, 0);
    const int rc = xgpu_scale_taps_ex(n, s, h, N, S, H, filter, first.data(), count.data(), w.data(), widest);
    if (rc < 0) return rc;
    for (int o = 0; o < N; o++) {
        if (first[o] < 0 || count[o] < 1 || first[o] + count[o] > n) return XGPU_ERR_UNEXPECTED;
        if (o && (first[o] < first[o - 1] || first[o] + count[o] < first[o - 1] + count[o - 1])) return XGPU_ERR_UNEXPECTED;
    }
    t.first = reserve(sizeof(int32_t) * N);
    memcpy(&blob[t.first], first.data(), sizeof(int32_t) * N);
    t.count = reserve(sizeof(int32_t) * N);
    memcpy(&blob[t.count], count.data(), sizeof(int32_t) * N);
    t.w = reserve(sizeof(int16_t) * w.size());
    int16_t *dw = (int16_t *)&blob[t.w];
    if (!transposed) {
        memcpy(dw, w.data(), sizeof(int16_t) * w.size());
        t.stride = widest;
        return XGPU_OK;
    }
    for (int o = 0; o < N; o++) for (int k = 0; k < widest; k++) dw[(size_t)k * N + o] = w[(size_t)o * widest + k];
    t.stride = N;
    int c = 0;
    for (int g = 0; g < N; g += group) {
        const int ol = std::min(g + group - 1, N - 1);
        c = std::max(c, ((first[ol] + count[ol] + 7) & ~7) - (first[g] & ~7));
    }
    *cap = c;
    return XGPU_OK;
}
