// scale_taps_ex_check.cc - xgpu_scale_taps_ex over the grid of tests/test_output_ladder_format.py as a stand-alone host program, for a run under the host's
// sanitizers: it is linked with xevd_amd/csrc/xgpu_scale.hip alone and touches no GPU.  Every table goes into heap arrays of exactly the size the contract asks
// for, so a write past a row, a table or the first / count arrays is a report.  It also checks what a sanitizer cannot: every row sums to 16384, has no negative
// weight, stays inside the plane, and S = 1, D = 0 gives xgpu_scale_taps' arrays.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/scale_taps_ex_check.cc xevd_amd/csrc/xgpu_scale.hip -o scale_taps_ex_check && ./scale_taps_ex_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/xevd_hip.h"

static long long tables = 0, rows = 0;

static int fail(const char *what, int n, int s, int d, int N, int S, int D, int filter)
{
    fprintf(stderr, "FAILED: %s at n %d s %d d %d N %d S %d D %d filter %d\n", what, n, s, d, N, S, D, filter);
    return 1;
}

static int one(int n, int s, int d, int N, int S, int D, int filter)
{
    std::vector<int32_t> first(N), count(N);
    const int widest = xgpu_scale_taps_ex(n, s, d, N, S, D, filter, first.data(), count.data(), NULL, 0);
    if (widest < 1 || widest > 131) return fail("widest row", n, s, d, N, S, D, filter);
    std::vector<int16_t> w((size_t)N * widest, -1);
    if (xgpu_scale_taps_ex(n, s, d, N, S, D, filter, first.data(), count.data(), w.data(), widest) != widest) return fail("second call", n, s, d, N, S, D, filter);
    for (int o = 0; o < N; o++) {
        if (first[o] < 0 || count[o] < 1 || count[o] > widest || first[o] + count[o] > n) return fail("span", n, s, d, N, S, D, filter);
        int sum = 0;
        for (int k = 0; k < widest; k++) {
            const int q = w[(size_t)o * widest + k];
            if (q < 0 || (k >= count[o] && q != 0)) return fail("weight", n, s, d, N, S, D, filter);
            sum += q;
        }
        if (sum != 16384) return fail("sum", n, s, d, N, S, D, filter);
    }
    if (S == 1 && D == 0) {
        std::vector<int32_t> f2(N), c2(N);
        std::vector<int16_t> w2((size_t)N * widest, -1);
        if (xgpu_scale_taps(n, s, d, N, filter, f2.data(), c2.data(), w2.data(), widest) != widest || f2 != first || c2 != count || w2 != w)
            return fail("xgpu_scale_taps", n, s, d, N, S, D, filter);
    }
    tables++; rows += N;
    return 0;
}

int main()
{
    static const int planes[] = { 2, 9, 37, 148, 296 };
    static const int ratio[][2] = { { 1, 64 }, { 1, 33 }, { 10, 37 }, { 1, 2 }, { 1, 1 }, { 3, 2 }, { 8, 1 } };      // destination samples per source sample
    for (int n : planes) for (const auto &r : ratio) for (int sub = 1; sub <= 2; sub++) {
        const int s = sub, S = sub;
        const int N = (int)(((long long)n * r[0] + r[1] - 1) / r[1]);      // rounded up: never below the 1 / 64 limit
        const bool inside = N >= 1 && N * S >= 2 && (long long)n * s <= 64LL * N * S && (long long)N * S <= 8LL * n * s;
        for (int d = 0; d < 3; d++) for (int D = 0; D < 3; D++) for (int filter = 0; filter < 2; filter++) {
            if (!inside) {
                int32_t f0[1], c0[1];
                if (xgpu_scale_taps_ex(n, s, d, N, S, D, filter, f0, c0, NULL, 0) != XGPU_ERR_UNSUPPORTED) return fail("limit", n, s, d, N, S, D, filter);
                continue;
            }
            if (one(n, s, d, N, S, D, filter)) return 1;
            if (S == 2 && D == 0 && one(n, s, d, N * 2 <= 16384 && N * 2 <= 8 * n * s ? N * 2 : N, 1, 0, filter)) return 1;      // the luma-resolution table of the same plane
        }
    }
    // a row narrower than the table asks for is refused, not overrun
    int32_t f[4], c[4];
    int16_t w[4];
    if (xgpu_scale_taps_ex(64, 2, 0, 4, 2, 0, XGPU_SCALE_BILINEAR, f, c, w, 1) != XGPU_ERR_INVALID_ARGUMENT) return fail("narrow stride", 64, 2, 0, 4, 2, 0, 0);
    printf("scale_taps_ex_check: %lld tables, %lld rows: ok\n", tables, rows);
    return 0;
}
