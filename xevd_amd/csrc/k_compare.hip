// k_compare.hip - a picture against a reference in one pass over both (xgpu_pic_compare): per component the census of the differences (n, sse, n_diff,
// max_abs, first_diff), the exact integer SSIM and - optionally - the SSE of every 16x16 luma / 8x8 chroma block.  Both pictures are only read.  The contract
// is INTEGRATION.md section 8h; tests/metrics_ref.py restates it in numpy, bit for bit.
//
// One launch for the three planes.  The cropped plane of every component is cut into tiles of 64x32 samples, numbered plane after plane; a workgroup of 256
// lanes walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... and keeps its sums in registers, so that a picture of any size ends in a few thousand partial sums.
//   ownership   a sample belongs to the tile it lies in; an SSIM window to the tile that holds its top-left 4x4 block; a map block to the tile it lies in (the
//               tile's origin is a multiple of every block size).  So nothing is counted twice and nothing is missed, whatever w and h are.
//   loads       a lane loads 8 samples of a row of either picture - 16 bytes when the plane's cropped base and pitch are multiples of 16 (a byte reference:
//               8), element by element otherwise and at the plane's right edge - and takes the census of them.  With SSIM the tile's 4-sample right and
//               bottom halo is loaded as well and everything goes to LDS; samples outside the plane are staged as 0 and used by no window.
//   SSIM        one lane per 4x4 block of the staged 68x36 samples sums a, r, a^2 + r^2 and a r (the last two in 64 bits: a sample may be any 16-bit
//               pattern); one lane per window adds four of them and quantises the window's SSIM.  That arithmetic is binary64 with every operation rounded
//               on its own: contraction is off for this file, and the division is the correctly rounded one the compiler emits without fast-math.
//   reduction   inside the wave by shuffles, across the four waves in LDS, then one row of sums per workgroup and component in a block of the context's - when
//               the workgroup moves on to the next plane and at its end.  k_compare_finish, one workgroup queued behind on the same stream, adds the rows and
//               writes every field of the result with plain stores.  (One atomic per field and workgroup on the result itself was measured first: 43 000
//               atomics on two cache lines cost 7 ns each, 190 - 330 us for an 8K picture whose samples take 32 us to read - DESIGN 5c.)  All sums are
//               integers: the result does not depend on the order.  The map's blocks are summed in LDS and stored by their one owner: nothing to clear.
#pragma clang fp contract(off)
#include "xgpu_internal.h"
#include <stddef.h>
#include <algorithm>

namespace {
constexpr int TW = 64, TH = 32;                    // the tile
constexpr int LW = 72, LH = 36;                    // what is staged: the tile and its halo, a row padded to 9 groups of 8 samples
constexpr int NBX = 17, NBY = 9, NB = NBX * NBY;   // its 4x4 blocks
constexpr int N_CORE = 8 * TH;                     // groups of 8 samples in the tile: one per lane
constexpr int N_GROUPS = N_CORE + TH + 4 * 9;      // ... the right halo (4 samples per row) and the 4 rows below
constexpr int MAX_WORKGROUPS = 2048;

struct CmpAcc {
    unsigned long long n, sse, nd, first, win;
    long long q;
    uint32_t mx;
    __device__ void reset() { n = sse = nd = win = 0; first = ~0ull; q = 0; mx = 0; }
};
}

__device__ __forceinline__ void cmp_unpack16(uint32_t lo, uint32_t hi, uint32_t *v) { v[0] = lo & 0xFFFFu; v[1] = lo >> 16; v[2] = hi & 0xFFFFu; v[3] = hi >> 16; }
__device__ __forceinline__ void cmp_unpack8(uint32_t q, uint32_t *v) { v[0] = q & 0xFFu; v[1] = (q >> 8) & 0xFFu; v[2] = (q >> 16) & 0xFFu; v[3] = q >> 24; }

// cnt (8, or 4 in the right halo) samples of a row from p on, of which the first nvalid (>= 1) are the plane's: the others read as 0 and are not loaded
__device__ __forceinline__ void cmp_load16(const uint16_t *p, int cnt, int nvalid, bool vec, uint32_t (&v)[8])
{
    #pragma unroll
    for (int k = 0; k < 8; k++) v[k] = 0;
    if (vec && nvalid == 8) {
        const uint4 q = *(const uint4 *)p;
        cmp_unpack16(q.x, q.y, v); cmp_unpack16(q.z, q.w, v + 4);
    } else if (vec && cnt == 4 && nvalid == 4) {
        const uint2 q = *(const uint2 *)p;
        cmp_unpack16(q.x, q.y, v);
    } else {
        #pragma unroll
        for (int k = 0; k < 8; k++) if (k < nvalid) v[k] = p[k];
    }
}
__device__ __forceinline__ void cmp_load8(const uint8_t *p, int cnt, int nvalid, bool vec, uint32_t (&v)[8])
{
    #pragma unroll
    for (int k = 0; k < 8; k++) v[k] = 0;
    if (vec && nvalid == 8) {
        const uint2 q = *(const uint2 *)p;
        cmp_unpack8(q.x, v); cmp_unpack8(q.y, v + 4);
    } else if (vec && cnt == 4 && nvalid == 4) {
        cmp_unpack8(*(const uint32_t *)p, v);
    } else {
        #pragma unroll
        for (int k = 0; k < 8; k++) if (k < nvalid) v[k] = p[k];
    }
}

__device__ __forceinline__ unsigned long long cmp_shfl64(unsigned long long v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}

// the workgroup's sums: wave, LDS, and the totals in lane 0 of wave 0 (the other lanes' acc is undefined afterwards)
__device__ __forceinline__ void cmp_reduce(CmpAcc &acc, unsigned long long (*red)[6], uint32_t *red_mx)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        acc.n += cmp_shfl64(acc.n, d); acc.sse += cmp_shfl64(acc.sse, d); acc.nd += cmp_shfl64(acc.nd, d); acc.win += cmp_shfl64(acc.win, d);
        acc.q += (long long)cmp_shfl64((unsigned long long)acc.q, d);
        const unsigned long long f = cmp_shfl64(acc.first, d);
        acc.first = f < acc.first ? f : acc.first;
        acc.mx = max(acc.mx, (uint32_t)__shfl_down((int)acc.mx, d));
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();      // the previous reduction has been read
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = acc.n; red[wave][1] = acc.sse; red[wave][2] = acc.nd; red[wave][3] = acc.first; red[wave][4] = acc.win; red[wave][5] = (unsigned long long)acc.q;
        red_mx[wave] = acc.mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        acc.reset();
        for (int k = 0; k < 4; k++) {
            acc.n += red[k][0]; acc.sse += red[k][1]; acc.nd += red[k][2]; acc.first = red[k][3] < acc.first ? red[k][3] : acc.first; acc.win += red[k][4];
            acc.q += (long long)red[k][5];
            acc.mx = max(acc.mx, red_mx[k]);
        }
    }
}
__device__ __forceinline__ void cmp_store_part(unsigned long long *p, const CmpAcc &acc)
{
    p[0] = acc.n; p[1] = acc.sse; p[2] = acc.nd; p[3] = acc.first; p[4] = acc.win; p[5] = (unsigned long long)acc.q; p[6] = acc.mx; p[7] = 0;
}
// the workgroup's sums of component c into its row of the partial sums; lane 0 writes all of them, so a row is written once
__device__ __forceinline__ void cmp_flush(const CompareArgs &a, int c, CmpAcc &acc, unsigned long long (*red)[6], uint32_t *red_mx)
{
    cmp_reduce(acc, red, red_mx);
    if (threadIdx.x == 0) cmp_store_part(a.part + ((size_t)blockIdx.x * 3 + c) * CMP_PART_WORDS, acc);
    acc.reset();
}

__global__ __launch_bounds__(256) void k_compare(const CompareArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_a[LH][LW];
    __shared__ __attribute__((aligned(16))) uint16_t s_r[LH][LW];
    __shared__ uint32_t b_s1[NB], b_s2[NB];
    __shared__ unsigned long long b_ss[NB], b_s12[NB];
    __shared__ unsigned long long s_map[2][32];      // the tile's map blocks, [row][8]; two sets: a tile's is stored and cleared while the next tile's fills
    __shared__ unsigned long long red[4][6];
    __shared__ uint32_t red_mx[4];
    const int tid = threadIdx.x;
    if (tid < 64) s_map[tid >> 5][tid & 31] = 0;
    __syncthreads();

    CmpAcc acc;
    acc.reset();
    int cur = -1, it = 0, seen = 0;
    for (int t = blockIdx.x; t < a.tile_first[3]; t += gridDim.x, it++) {
        const int c = t >= a.tile_first[2] ? 2 : t >= a.tile_first[1] ? 1 : 0;
        if (c != cur) {      // (uniform: the tile is the workgroup's)
            if (cur >= 0) cmp_flush(a, cur, acc, red, red_mx);
            cur = c;
            seen |= 1 << c;
        }
        const int tl = t - a.tile_first[c];
        const int tx0 = (tl % a.tiles_x[c]) * TW, ty0 = (tl / a.tiles_x[c]) * TH;
        const int w = a.w[c], h = a.h[c];
        const uint16_t *pa = a.a[c];
        const uint8_t *pr = a.r[c];
        const size_t sa = (size_t)a.sa[c], spr = a.pr[c];
        const bool va = a.vec_a[c] != 0, vr = a.vec_r[c] != 0;
        unsigned long long *mp = s_map[it & 1];
        const int bsh = c ? 3 : 4;      // log2 of the map's block in this plane

        // ---- load, census, stage
        const int n_groups = a.ssim ? N_GROUPS : N_CORE;
        for (int k = tid; k < n_groups; k += 256) {
            int ry, cx, cnt = 8;
            if (k < N_CORE) { ry = k >> 3; cx = k & 7; }
            else if (k < N_CORE + TH) { ry = k - N_CORE; cx = 8; cnt = 4; }
            else { const int j = k - N_CORE - TH; ry = TH + j / 9; cx = j % 9; if (cx == 8) cnt = 4; }
            const int gx0 = tx0 + cx * 8, gy = ty0 + ry;
            const int nvalid = gy < h ? min(cnt, max(w - gx0, 0)) : 0;
            uint32_t xa[8], xr[8];
            if (nvalid > 0) {
                cmp_load16(pa + (size_t)gy * sa + gx0, cnt, nvalid, va, xa);
                if (a.r8) cmp_load8(pr + (size_t)gy * spr + gx0, cnt, nvalid, vr, xr);
                else      cmp_load16((const uint16_t *)(pr + (size_t)gy * spr) + gx0, cnt, nvalid, vr, xr);
            } else {
                #pragma unroll
                for (int m = 0; m < 8; m++) xa[m] = xr[m] = 0;
            }
            if (a.ssim) {
                *(uint4 *)&s_a[ry][cx * 8] = make_uint4(xa[0] | xa[1] << 16, xa[2] | xa[3] << 16, xa[4] | xa[5] << 16, xa[6] | xa[7] << 16);
                *(uint4 *)&s_r[ry][cx * 8] = make_uint4(xr[0] | xr[1] << 16, xr[2] | xr[3] << 16, xr[4] | xr[5] << 16, xr[6] | xr[7] << 16);
            }
            if (k < N_CORE && nvalid > 0) {      // the samples this tile owns (those past nvalid are 0 in both)
                unsigned long long s = 0;
                uint32_t nd = 0, mx = 0;
                int fk = 8;
                #pragma unroll
                for (int m = 7; m >= 0; m--) {
                    const int d = (int)xa[m] - (int)xr[m];
                    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
                    s += (unsigned long long)(ad * ad);      // 65535^2 < 2^32
                    if (ad) { nd++; fk = m; }
                    mx = max(mx, ad);
                }
                acc.n += (unsigned long long)nvalid;
                if (nd) {
                    acc.sse += s; acc.nd += nd; acc.mx = max(acc.mx, mx);
                    const unsigned long long key = ((unsigned long long)(uint32_t)gy << 32) | (uint32_t)(gx0 + fk);
                    acc.first = key < acc.first ? key : acc.first;
                    if (a.block_map) atomicAdd(&mp[(ry >> bsh) * 8 + ((cx * 8) >> bsh)], s);
                }
            }
        }
        if (a.ssim || a.block_map) __syncthreads();

        // ---- the tile's map blocks: stored by their one owner, and cleared for the tile after the next
        if (a.block_map && tid < 32) {
            const int bx = tid & 7, by = tid >> 3;
            const int gbx = (tx0 >> bsh) + bx, gby = (ty0 >> bsh) + by;
            if (bx < (TW >> bsh) && by < (TH >> bsh) && gbx < a.mw && gby < a.mh) a.map[((size_t)c * a.mh + gby) * a.mw + gbx] = mp[tid];
            mp[tid] = 0;
        }
        if (!a.ssim) continue;

        // ---- sums of the 4x4 blocks
        if (tid < NB) {
            const int bx = tid % NBX, by = tid / NBX;
            uint32_t s1 = 0, s2 = 0;
            unsigned long long ss = 0, s12 = 0;
            #pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const uint2 qa = *(const uint2 *)&s_a[by * 4 + rr][bx * 4], qr = *(const uint2 *)&s_r[by * 4 + rr][bx * 4];
                uint32_t ea[4], er[4];
                cmp_unpack16(qa.x, qa.y, ea); cmp_unpack16(qr.x, qr.y, er);
                #pragma unroll
                for (int m = 0; m < 4; m++) {
                    s1 += ea[m]; s2 += er[m];
                    ss += (unsigned long long)(ea[m] * ea[m]) + (unsigned long long)(er[m] * er[m]);
                    s12 += (unsigned long long)(ea[m] * er[m]);
                }
            }
            b_s1[tid] = s1; b_s2[tid] = s2; b_ss[tid] = ss; b_s12[tid] = s12;
        }
        __syncthreads();

        // ---- the windows whose top-left block is the tile's
        if (tid < 128) {
            const int bi = tid & 15, bj = tid >> 4;
            if ((tx0 >> 2) + bi < (w >> 2) - 1 && (ty0 >> 2) + bj < (h >> 2) - 1) {
                const int b0 = bj * NBX + bi;
                const long long s1 = (long long)b_s1[b0] + b_s1[b0 + 1] + b_s1[b0 + NBX] + b_s1[b0 + NBX + 1];
                const long long s2 = (long long)b_s2[b0] + b_s2[b0 + 1] + b_s2[b0 + NBX] + b_s2[b0 + NBX + 1];
                const long long ss = (long long)(b_ss[b0] + b_ss[b0 + 1] + b_ss[b0 + NBX] + b_ss[b0 + NBX + 1]);
                const long long s12 = (long long)(b_s12[b0] + b_s12[b0 + 1] + b_s12[b0 + NBX] + b_s12[b0 + NBX + 1]);
                const long long vars = 64 * ss - s1 * s1 - s2 * s2, cov = 64 * s12 - s1 * s2;      // below 2^46 in magnitude
                const double num = (double)(2 * s1 * s2 + a.c1) * (double)(2 * cov + a.c2);
                const double den = (double)(s1 * s1 + s2 * s2 + a.c1) * (double)(vars + a.c2);
                acc.q += (long long)__builtin_floor(num / den * 1073741824.0 + 0.5);
                acc.win++;
            }
        }
    }
    if (cur >= 0) cmp_flush(a, cur, acc, red, red_mx);
    if (tid == 0) {      // the components this workgroup had no tile of: rows that add nothing
        acc.reset();
        for (int c = 0; c < 3; c++) if (!((seen >> c) & 1)) cmp_store_part(a.part + ((size_t)blockIdx.x * 3 + c) * CMP_PART_WORDS, acc);
    }
}

// the rows of the n workgroups into the result: one workgroup, every field written with a plain store
__global__ __launch_bounds__(256) void k_compare_finish(const unsigned long long *part, int n, xgpu_compare_result *res)
{
    __shared__ unsigned long long red[4][6];
    __shared__ uint32_t red_mx[4];
    for (int c = 0; c < 3; c++) {
        CmpAcc acc;
        acc.reset();
        for (int g = threadIdx.x; g < n; g += 256) {
            const unsigned long long *p = part + ((size_t)g * 3 + c) * CMP_PART_WORDS;
            acc.n += p[0]; acc.sse += p[1]; acc.nd += p[2]; acc.first = p[3] < acc.first ? p[3] : acc.first; acc.win += p[4]; acc.q += (long long)p[5];
            acc.mx = max(acc.mx, (uint32_t)p[6]);
        }
        cmp_reduce(acc, red, red_mx);
        if (threadIdx.x == 0) {
            res->n[c] = acc.n; res->sse[c] = acc.sse; res->n_diff[c] = acc.nd; res->first_diff[c] = acc.first; res->max_abs[c] = acc.mx;
            res->ssim_windows[c] = acc.win; res->ssim_q30[c] = acc.q;
            if (c == 0) res->reserved = 0;
        }
    }
}

int compare_workgroups(int tiles) { return std::min(tiles, MAX_WORKGROUPS); }
void launch_compare(const CompareArgs &a, hipStream_t s)
{
    const int n = compare_workgroups(a.tile_first[3]);
    hipLaunchKernelGGL(k_compare, dim3((unsigned)n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_compare_finish, dim3(1), dim3(256), 0, s, a.part, n, a.res);
}
