// k_stats.hip - what is in one picture, from one pass over the slot (xgpu_pic_stats): per component the census (n, sum, sum of squares, minimum, maximum), a
// histogram and two percentiles of it; optionally the histogram of max(R', G', B') at luma resolution and the light level it implies.  The picture is only read.
// The contract is INTEGRATION.md section 8i; tests/stats_ref.py restates it in numpy, bit for bit.
//
// Three kernels on one stream, behind a memset of the context's accumulation block:
//   k_stats         the cropped plane of every component cut into tiles of 64x32 samples, numbered plane after plane, as k_compare has them; at most 1024
//                   workgroups of 256 lanes walk the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  A lane loads 8 samples of a row - 16 bytes when the plane's cropped base and
//                   pitch are multiples of 16, element by element otherwise and at the plane's right edge -, keeps the census in registers and counts the
//                   samples' bins in an LDS histogram.
//   k_stats_light   the same walk over groups of 64 lanes x 4 chroma rows of k_output_rgb's lanes: three_channel_rows and RgbConv<XGPU_OUT_U16> of
//                   output_common.h - the code of xgpu_pic_output_device itself, not a restatement - make the R'G'B' codes of 8 pixels of two luma rows, and their
//                   largest goes to an LDS histogram of 2^B bins.
//   k_stats_finish  one workgroup: adds the workgroups' rows of partial sums, copies the accumulation block to the caller's histogram, finds the percentiles
//                   with a parallel scan and computes light_sum in the contract's order.  It writes every field of the result with plain stores.
//   LDS histogram   atomicAdd, whose cost depends on the content: a flat picture sends every lane to one bin.  So (1) a lane merges equal neighbours among its
//                   8 samples into one add of the run length, (2) a wave whose samples all fall in one bin makes one add of their number, and (3) with fewer
//                   than 4096 bins the lanes of a wave spread over up to 64 copies of the histogram (4096 words of LDS in all), summed at the flush.
//   flush           when a workgroup moves on to the next plane and at its end: one row of census sums per component into the context's block (no atomics: a row
//                   has one writer), and the LDS bins - bin b by lane b mod 256, so a wave adds to contiguous words - with one integer global atomic per
//                   non-zero bin into the accumulation block.  Integer adds do not depend on the order.  Nothing is added to the caller's memory: k_stats_finish
//                   copies the block there, which is how the caller clears nothing.
// light_sum is binary64 with every operation rounded on its own: contraction is off for this file, and the division is the correctly rounded one the compiler
// emits without fast-math.
#pragma clang fp contract(off)
#include "output_common.h"
#include <algorithm>

namespace {
constexpr int TW = 64, TH = 32;                    // the tile of the plane pass: one group of 8 samples per lane
constexpr int MAX_COPIES = 64;                     // of an LDS histogram: one per lane of a wave at most

struct StAcc {
    unsigned long long n, sum, sq;
    uint32_t mn, mx;
    __device__ void reset() { n = sum = sq = 0; mn = ~0u; mx = 0; }
};
}

__device__ __forceinline__ int st_copies(int nbins) { return min(STATS_MAX_BINS / nbins, MAX_COPIES); }      // a power of two
__device__ __forceinline__ unsigned long long st_shfl64(unsigned long long v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}

// The bins of a lane's `cnt` (0 .. 8) adjacent samples into the LDS histogram h0 (copy 0; hc: the lane's copy).  Called by all 64 lanes of a wave together.
__device__ __forceinline__ void st_hist_add(uint32_t *h0, uint32_t *hc, const uint32_t (&bin)[8], int cnt)
{
    const unsigned long long act = __ballot(cnt > 0);
    if (!act) return;      // (uniform)
    bool single = true;
    #pragma unroll
    for (int m = 1; m < 8; m++) single &= m >= cnt || bin[m] == bin[0];
    const uint32_t bw = (uint32_t)__shfl((int)bin[0], __ffsll((long long)act) - 1);
    if (!__ballot(cnt > 0 && (!single || bin[0] != bw))) {      // every sample of the wave in one bin: one add
        uint32_t tot = 0;      // the sum of cnt (<= 8) over the wave, bit by bit: four votes instead of a chain of shuffles
        #pragma unroll
        for (int k = 0; k < 4; k++) tot += (uint32_t)__popcll(__ballot((cnt >> k) & 1)) << k;
        if ((threadIdx.x & 63) == 0) atomicAdd(&h0[bw], tot);
        return;
    }
    if (cnt > 0) {      // one add per run of equal neighbours
        uint32_t rb = bin[0], run = 1;
        #pragma unroll
        for (int m = 1; m < 8; m++) {
            if (m < cnt) {
                if (bin[m] == rb) run++;
                else { atomicAdd(&hc[rb], run); rb = bin[m]; run = 1; }
            }
        }
        atomicAdd(&hc[rb], run);
    }
}
// the workgroup's LDS histogram (copies x nbins) added to acc[nbins] and cleared
__device__ __forceinline__ void st_hist_flush(uint32_t *h, int nbins, int copies, uint32_t *acc)
{
    __syncthreads();      // every add of the workgroup has arrived
    for (int b = threadIdx.x; b < nbins; b += 256) {
        uint32_t tot = 0;
        for (int k = 0; k < copies; k++) { tot += h[k * nbins + b]; h[k * nbins + b] = 0; }
        if (tot) atomicAdd(&acc[b], tot);
    }
    __syncthreads();      // cleared before the next add
}

// the workgroup's sums: wave, LDS, and the totals in lane 0 of wave 0 (the other lanes' acc is undefined afterwards)
__device__ __forceinline__ void st_reduce(StAcc &acc, unsigned long long (*red)[3], uint32_t (*red_mm)[2])
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        acc.n += st_shfl64(acc.n, d); acc.sum += st_shfl64(acc.sum, d); acc.sq += st_shfl64(acc.sq, d);
        acc.mn = min(acc.mn, (uint32_t)__shfl_down((int)acc.mn, d));
        acc.mx = max(acc.mx, (uint32_t)__shfl_down((int)acc.mx, d));
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();      // the previous reduction has been read
    if ((threadIdx.x & 63) == 0) { red[wave][0] = acc.n; red[wave][1] = acc.sum; red[wave][2] = acc.sq; red_mm[wave][0] = acc.mn; red_mm[wave][1] = acc.mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        acc.reset();
        for (int k = 0; k < 4; k++) {
            acc.n += red[k][0]; acc.sum += red[k][1]; acc.sq += red[k][2];
            acc.mn = min(acc.mn, red_mm[k][0]); acc.mx = max(acc.mx, red_mm[k][1]);
        }
    }
}
__device__ __forceinline__ void st_store_part(unsigned long long *p, const StAcc &acc)
{
    p[0] = acc.n; p[1] = acc.sum; p[2] = acc.sq; p[3] = acc.mn; p[4] = acc.mx; p[5] = p[6] = p[7] = 0;
}

__global__ __launch_bounds__(256) void k_stats(const StatsArgs a)
{
    __shared__ uint32_t s_hist[STATS_MAX_BINS];
    __shared__ unsigned long long red[4][3];
    __shared__ uint32_t red_mm[4][2];
    const int tid = threadIdx.x;
    const int nbins = a.hist_bits ? 1 << a.hist_bits : 0, copies = nbins ? st_copies(nbins) : 1, shift = a.bd - a.hist_bits;
    for (int i = tid; i < nbins * copies; i += 256) s_hist[i] = 0;
    __syncthreads();
    uint32_t *hc = s_hist + (tid & (copies - 1)) * nbins;

    StAcc acc;
    acc.reset();
    int cur = -1, seen = 0;
    for (int t = blockIdx.x; t < a.tile_first[3]; t += gridDim.x) {
        const int c = t >= a.tile_first[2] ? 2 : t >= a.tile_first[1] ? 1 : 0;
        if (c != cur) {      // (uniform: the tile is the workgroup's)
            if (cur >= 0) {
                st_reduce(acc, red, red_mm);
                if (tid == 0) st_store_part(a.part + ((size_t)blockIdx.x * 3 + cur) * STATS_PART_WORDS, acc);
                acc.reset();
                if (nbins) st_hist_flush(s_hist, nbins, copies, a.acc + cur * nbins);
            }
            cur = c;
            seen |= 1 << c;
        }
        const int tl = t - a.tile_first[c];
        const int gx0 = (tl % a.tiles_x[c]) * TW + (tid & 7) * 8, gy = (tl / a.tiles_x[c]) * TH + (tid >> 3);
        const int nvalid = gy < a.h[c] ? min(8, max(a.w[c] - gx0, 0)) : 0;      // the lane's samples in the plane
        uint32_t v[8];
        #pragma unroll
        for (int m = 0; m < 8; m++) v[m] = 0;
        if (nvalid > 0) {
            const uint16_t *p = a.a[c] + (size_t)gy * a.sa[c] + gx0;
            if (a.vec[c] && nvalid == 8) {
                const uint4 q = *(const uint4 *)p;
                v[0] = q.x & 0xFFFFu; v[1] = q.x >> 16; v[2] = q.y & 0xFFFFu; v[3] = q.y >> 16; v[4] = q.z & 0xFFFFu; v[5] = q.z >> 16; v[6] = q.w & 0xFFFFu; v[7] = q.w >> 16;
            } else {
                #pragma unroll
                for (int m = 0; m < 8; m++) if (m < nvalid) v[m] = p[m];
            }
            uint32_t s = 0, mn = ~0u, mx = 0;
            unsigned long long sq = 0;
            #pragma unroll
            for (int m = 0; m < 8; m++) {      // (the samples past nvalid are 0: they add nothing, and the minimum leaves them out)
                s += v[m];
                sq += (unsigned long long)(uint32_t)__umul24(v[m], v[m]);      // the full-rate 24-bit multiply; 65535^2 < 2^32 (HIP declares the result int)
                mx = max(mx, v[m]);
                mn = min(mn, m < nvalid ? v[m] : ~0u);
            }
            acc.n += (unsigned long long)nvalid; acc.sum += s; acc.sq += sq;
            acc.mn = min(acc.mn, mn); acc.mx = max(acc.mx, mx);
        }
        if (nbins) {      // (uniform; all lanes call)
            uint32_t bin[8];
            #pragma unroll
            for (int m = 0; m < 8; m++) bin[m] = min(v[m] >> shift, (uint32_t)(nbins - 1));
            st_hist_add(s_hist, hc, bin, nvalid);
        }
    }
    if (cur >= 0) {
        st_reduce(acc, red, red_mm);
        if (tid == 0) st_store_part(a.part + ((size_t)blockIdx.x * 3 + cur) * STATS_PART_WORDS, acc);
        if (nbins) st_hist_flush(s_hist, nbins, copies, a.acc + cur * nbins);
    }
    if (tid == 0) {      // the components this workgroup had no tile of: rows that add nothing
        acc.reset();
        for (int c = 0; c < 3; c++) if (!((seen >> c) & 1)) st_store_part(a.part + ((size_t)blockIdx.x * 3 + c) * STATS_PART_WORDS, acc);
    }
}

// groups of 64 lanes x 4 chroma rows of the cropped picture, as k_output_rgb's workgroups have them
__host__ __device__ __forceinline__ int st_light_groups_x(int w) { return ((w + 7) / 8 + 63) / 64; }
__host__ __device__ __forceinline__ int st_light_groups(int w, int ch) { return st_light_groups_x(w) * ((ch + 3) / 4); }

template <int UP>
__global__ __launch_bounds__(256) void k_stats_light(const StatsArgs a)
{
    __shared__ uint32_t s_hist[STATS_MAX_BINS];
    const int tid = threadIdx.x;
    const int nbins = 1 << a.bd, copies = st_copies(nbins);
    for (int i = tid; i < nbins * copies; i += 256) s_hist[i] = 0;
    __syncthreads();
    uint32_t *hc = s_hist + (tid & (copies - 1)) * nbins;
    const RgbOutArgs &r = a.rgb;
    const int gx = st_light_groups_x(r.w), groups = st_light_groups(r.w, r.ch);
    for (int t = blockIdx.x; t < groups; t += gridDim.x) {
        const int x0 = ((t % gx) * 64 + (tid & 63)) * 8, i = (t / gx) * 4 + (tid >> 6);
        const bool in = x0 < r.w && i < r.ch;
        const int n = in ? min(8, r.w - x0) : 0;      // pixels of this lane in the row (even)
        uint32_t m0[8], m1[8];
        #pragma unroll
        for (int m = 0; m < 8; m++) m0[m] = m1[m] = 0;
        if (in)
            three_channel_rows<UP, RgbConv<XGPU_OUT_U16>>(r, x0, i, [&](int row, uint32_t (&ch)[3][8]) {
                #pragma unroll
                for (int m = 0; m < 8; m++) {
                    const uint32_t v = max(ch[0][m], max(ch[1][m], ch[2][m]));
                    if (row & 1) m1[m] = v; else m0[m] = v;
                }
            });
        st_hist_add(s_hist, hc, m0, n);      // (all lanes call)
        st_hist_add(s_hist, hc, m1, n);
    }
    st_hist_flush(s_hist, nbins, copies, a.acc + (a.hist_bits ? 3 << a.hist_bits : 0));
}

// One histogram of nbins bins at src: copied to dst (the caller's) and to s_h, and for each of the np percentiles p[q] (1/10000) the smallest bin b with
// cum(b) * 10000 >= max(p[q] * n, 1), n the sum of the bins (> 0), into found[q].  Returns n.  All 256 lanes call; s_h and found are complete at the return.
__device__ __forceinline__ uint32_t st_scan(const uint32_t *src, uint32_t *dst, int nbins, const int *p, int np, uint32_t *s_h, uint32_t *s_wave, uint32_t *found)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();      // s_h, s_wave and found of the previous histogram have been read
    if (tid < 3) found[tid] = 0;
    for (int i = tid; i < nbins; i += 256) { const uint32_t v = src[i]; dst[i] = v; s_h[i] = v; }
    __syncthreads();
    const int chunk = (nbins + 255) / 256, b0 = min(tid * chunk, nbins), b1 = min(b0 + chunk, nbins);      // consecutive bins per lane
    uint32_t loc = 0;
    for (int b = b0; b < b1; b++) loc += s_h[b];
    uint32_t incl = loc;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t excl = incl - loc, n = 0;
    for (int k = 0; k < 4; k++) { if (k < wave) excl += s_wave[k]; n += s_wave[k]; }
    for (int q = 0; q < np; q++) {
        const unsigned long long t = (unsigned long long)p[q] * n;
        const unsigned long long need = ((t ? t : 1) + 9999) / 10000;      // cum * 10000 >= t  <=>  cum >= ceil(t / 10000); 1 <= need <= n
        if (excl < need && need <= (unsigned long long)excl + loc) {      // (one lane: cum does not decrease)
            uint32_t cum = excl;
            for (int b = b0; b < b1; b++) {
                cum += s_h[b];
                if (cum >= need) { found[q] = (uint32_t)b; break; }
            }
        }
    }
    __syncthreads();
    return n;
}

// the rows of the n_wg workgroups and the accumulation block into the result and the caller's histogram: one workgroup, every field written with a plain store
__global__ __launch_bounds__(256) void k_stats_finish(const StatsArgs a, int n_wg)
{
    __shared__ uint32_t s_h[STATS_MAX_BINS];
    __shared__ unsigned long long red[4][3];
    __shared__ uint32_t red_mm[4][2];
    __shared__ uint32_t s_wave[4], s_found[3];
    __shared__ double s_part[64];
    const int tid = threadIdx.x;
    xgpu_stats_result *res = a.res;
    StAcc acc[3];
    #pragma unroll
    for (int c = 0; c < 3; c++) acc[c].reset();
    for (int g = tid; g < n_wg; g += 256) {      // a workgroup's three rows lie side by side: one round of loads per workgroup
        const unsigned long long *p = a.part + (size_t)g * 3 * STATS_PART_WORDS;
        #pragma unroll
        for (int c = 0; c < 3; c++, p += STATS_PART_WORDS) {
            acc[c].n += p[0]; acc[c].sum += p[1]; acc[c].sq += p[2];
            acc[c].mn = min(acc[c].mn, (uint32_t)p[3]); acc[c].mx = max(acc[c].mx, (uint32_t)p[4]);
        }
    }
    #pragma unroll
    for (int c = 0; c < 3; c++) {
        st_reduce(acc[c], red, red_mm);
        if (tid == 0) { res->n[c] = acc[c].n; res->sum[c] = acc[c].sum; res->sum_sq[c] = acc[c].sq; res->min[c] = acc[c].mn; res->max[c] = acc[c].mx; }
    }
    const int nbins = a.hist_bits ? 1 << a.hist_bits : 0, shift = a.bd - a.hist_bits;
    for (int c = 0; c < 3; c++) {
        if (nbins) st_scan(a.acc + c * nbins, a.hist + c * nbins, nbins, a.pctl_e4, 2, s_h, s_wave, s_found);      // (uniform)
        if (tid == 0) { res->pctl[c][0] = nbins ? s_found[0] << shift : 0; res->pctl[c][1] = nbins ? s_found[1] << shift : 0; }
    }
    if (!a.light) {
        if (tid == 0) {
            res->light_n = 0; res->light_sum = 0.0; res->light_mean = 0.0;
            res->light_max_code = res->light_pctl_code[0] = res->light_pctl_code[1] = res->reserved = 0;
            res->light_max = res->light_pctl[0] = res->light_pctl[1] = res->reserved2 = 0.f;
        }
        return;
    }
    const int nl = 1 << a.bd;
    const int pl[3] = { a.pctl_e4[0], a.pctl_e4[1], 10000 };      // the highest occupied code is the percentile 10000
    const uint32_t n = st_scan(a.acc + 3 * nbins, a.hist + 3 * nbins, nl, pl, 3, s_h, s_wave, s_found);
    if (tid < 64) {      // the contract's order: 64 partial sums over k = l, l + 64, ... ascending, then added left to right
        double part = 0.0;
        #pragma unroll 4
        for (int k = tid; k < nl; k += 64) part = part + (double)s_h[k] * (double)a.lin[k];
        s_part[tid] = part;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = s_part[0];
        for (int l = 1; l < 64; l++) sum = sum + s_part[l];
        res->light_n = n; res->light_sum = sum; res->light_mean = sum / (double)n;
        res->light_max_code = s_found[2]; res->light_pctl_code[0] = s_found[0]; res->light_pctl_code[1] = s_found[1]; res->reserved = 0;
        res->light_max = a.lin[s_found[2]]; res->light_pctl[0] = a.lin[s_found[0]]; res->light_pctl[1] = a.lin[s_found[1]]; res->reserved2 = 0.f;
    }
}

void launch_stats(const StatsArgs &a, hipStream_t s)
{
    const size_t words = (a.hist_bits ? (size_t)3 << a.hist_bits : 0) + (a.light ? (size_t)1 << a.bd : 0);
    if (words) (void)hipMemsetAsync(a.acc, 0, words * sizeof(uint32_t), s);
    const int n = std::min(a.tile_first[3], STATS_MAX_WORKGROUPS);
    hipLaunchKernelGGL(k_stats, dim3((unsigned)n), dim3(256), 0, s, a);
    if (a.light) {
        const dim3 grid((unsigned)std::min(st_light_groups(a.rgb.w, a.rgb.ch), STATS_MAX_WORKGROUPS));
        if (a.upsample == XGPU_UPSAMPLE_NEAREST) hipLaunchKernelGGL(k_stats_light<XGPU_UPSAMPLE_NEAREST>, grid, dim3(256), 0, s, a);
        else                                     hipLaunchKernelGGL(k_stats_light<XGPU_UPSAMPLE_LINEAR>, grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_stats_finish, dim3(1), dim3(256), 0, s, a, n);
}
