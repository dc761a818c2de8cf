// itdq_body.h - the device side of the residual pass (dequantisation + inverse transforms of one 256-thread work item), shared by k_itdq.hip (the pass as
// a launch of its own) and k_intra.hip (k_intra_itdq: the NEXT picture's residual pass rides in the workgroups of this picture's data-flow intra launch).
// The transform matrices are constant memory of the including translation unit: each unit uploads its own copy (upload_transform_tables_tu).
// What is restated and how it is mapped: see the header of k_itdq.hip.
#pragma once
#include "xgpu_internal.h"
#include <type_traits>

typedef short v2s __attribute__((ext_vector_type(2)));

// transform matrices xevd_tbl_tm2..64 packed as row pairs: entry [k2][n] = (tm[2*k2][n], tm[2*k2+1][n]) as two s16;
// filled by the host from the closed form (xgpu_api.hip: init_transform_tables).  Offsets: N*N/2 dwords per size.
static __constant__ uint32_t k_tmp[2730];
__host__ __device__ constexpr int tmp_base(int log2n) { return log2n == 1 ? 0 : log2n == 2 ? 2 : log2n == 3 ? 10 : log2n == 4 ? 42 : log2n == 5 ? 170 : 682; }

// ATS matrices, same packing, [type DST7=0 / DCT8=1][size 4,8,16,32]: offsets 8, 32, 128, 512 dwords per size.
// The 4-point entries hold the 4x4 matrices equivalent to the reference's factorised kernels (xevdm_itdq.c:163-190, 284-312).
static __constant__ uint32_t k_atsp[2][680];
__host__ __device__ constexpr int atsp_base(int log2n) { return log2n == 2 ? 0 : log2n == 3 ? 8 : log2n == 4 ? 40 : 168; }

static void upload_transform_tables_tu(const int *tm, const int16_t *ats, hipStream_t s)      // this translation unit's copy of the tables
{
    // ats: [type DST7=0/DCT8=1][log2n 2..5] row-major s16 matrices M[k][n] back to back (16+64+256+1024 per type)
    static uint32_t apk[2][680];
    for (int t = 0; t < 2; t++) {
        int src = 0;
        for (int l = 2; l <= 5; l++) {
            const int N = 1 << l, dst = atsp_base(l);
            for (int k2 = 0; k2 < N / 2; k2++)
                for (int n = 0; n < N; n++)
                    apk[t][dst + k2 * N + n] = (uint32_t)(uint16_t)ats[t * 1360 + src + (2 * k2) * N + n] |
                                               ((uint32_t)(uint16_t)ats[t * 1360 + src + (2 * k2 + 1) * N + n] << 16);
            src += N * N;
        }
    }
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(k_atsp), apk, sizeof(apk), 0, hipMemcpyHostToDevice, s);
    // tm: int32 row-major matrices 2,4,..,64 back to back (5460 entries)
    static uint32_t packed[2730];
    int src = 0;
    for (int l = 1; l <= 6; l++) {
        const int N = 1 << l, dst = tmp_base(l);
        for (int k2 = 0; k2 < N / 2; k2++)
            for (int n = 0; n < N; n++)
                packed[dst + k2 * N + n] = (uint32_t)(uint16_t)(int16_t)tm[src + (2 * k2) * N + n] |
                                           ((uint32_t)(uint16_t)(int16_t)tm[src + (2 * k2 + 1) * N + n] << 16);
        src += N * N;
    }
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(k_tmp), packed, sizeof(packed), 0, hipMemcpyHostToDevice, s);
    (void)hipStreamSynchronize(s);
}

__device__ __forceinline__ int clip16(int v) { return min(max(v, -32768), 32767); }
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, a), __builtin_bit_cast(v2s, b), c, false);
}
// a * b + c of two factors inside s24, full rate (the compiler's own choice for __mul24 + add here was the quarter-rate v_mad_u64_u32)
__device__ __forceinline__ int mad24(int a, int b, int c)
{
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t pack16(int lo, int hi) { return (uint32_t)(uint16_t)lo | ((uint32_t)hi << 16); }

// geometry of a size class, shared with the host-side batch builder (xgpu_builder.hip)
__host__ __device__ constexpr int itdq_group(int lw, int lh)
{
    const int W = 1 << lw, H = 1 << lh;
    const int l1 = W * (H > 16 ? H / 16 : 1), l2 = H * (W > 16 ? W / 16 : 1);
    return 256 / (l1 > l2 ? l1 : l2);
}

#define ITDQ_PLANES_DWORDS 4608  // max over size classes of 2 planes x G*H*(W/2+1) dwords (16x16: 2*2304)
#define ITDQ_LDS_DWORDS (ITDQ_PLANES_DWORDS + 2048)   // + 4096 dequantised s16 coefficients
#define ITDQ_MAX_G 32            // TBs per work item of the LDS form (4x8, 8x4, 8x8; the classes up to 16 samples keep up to 128 TBs in registers: itdq_small)
#define ITDQ_TB_DWORDS (4 * ITDQ_MAX_G)               // per TB: row-pair mask, column-pair mask, the two dwords of its record

// Vector tuples a lane may sit out of loading (mc_filters.h: gload*_if): the value stays one register tuple from the load to its first use, so the place where the lane's
// branch joins the wave again needs no copy that would wait for the load; a lane that sat out keeps whatever the registers held and never looks at them.
typedef uint32_t itq_v2 __attribute__((ext_vector_type(2)));
typedef uint32_t itq_v4 __attribute__((ext_vector_type(4)));
typedef itq_v2 __attribute__((aligned(4))) itq_v2_u;
typedef itq_v4 __attribute__((aligned(2))) itq_v4_u;
typedef itq_v2 __attribute__((aligned(2))) itq_v2_s;
template <typename T> __device__ __forceinline__ T itq_any() { T v; asm volatile("" : "=v"(v)); return v; }
static_assert(sizeof(TbRec) == 8, "a TbRec is fetched as one 8-byte load: off | log2w, log2h, qp, log2s");
__device__ __forceinline__ void itq_rec_if(itq_v2 &v, const TbRec *p, bool on) { if (on) v = *(const itq_v2_u *)p; }
__device__ __forceinline__ int rec_qp(itq_v2 r) { return (int)((r.y >> 16) & 0xFF); }
__device__ __forceinline__ int rec_log2s(itq_v2 r) { return (int)(r.y >> 24); }

// Dequantisation of one coefficient (xevd_dquant, xevd_itdq.c:480-492; shift / offset :511-515; scale tables xevd_tbl.c:255-256: {..,72} with tool_iqt, {..,71} without):
// clip16((c * mul + offset) >> shift), mul = scale[qp % 6] << (qp / 6), times 181 for a class with odd LW + LH, shift = bd - 9 + (LW + LH) / 2 (+ 8 when odd).
// Even classes, 32 bits: qp < 96 (xgpu_builder.hip) gives mul <= 72 << 15; with |c| held to cmax = 2^23 >> (qp / 6) - which no s16 value exceeds up to qp 53 -
// |c * mul| <= 72 * 2^23 < 2^30, so product + offset is exact in s32 and both factors fit v_mad_i32_i24.  A coefficient beyond cmax gives, held or not,
// |c * mul| >= 40 * 2^23 > 2^(15 + shift) for every shift <= 13 (bit depths to 16): the result is clipped to the same end of the s16 range either way.
// Odd classes keep the s64 form (c * 181 * mul needs 37 bits).
template <bool ODD, bool IQT>
struct ItdqScale {
    int mul, cmax, shift, offset;
    __device__ __forceinline__ ItdqScale(int qp, int bd, int lwh)
    {
        shift = bd - 9 + (lwh >> 1) + (ODD ? 8 : 0);
        offset = shift == 0 ? 0 : 1 << (shift - 1);
        const int q6 = (int)(((uint32_t)qp * 171u) >> 10), sidx = qp - 6 * q6;                      // qp / 6, qp % 6 for every u8
        constexpr uint64_t scale = 40ull | 45ull << 8 | 51ull << 16 | 57ull << 24 | 64ull << 32 | (uint64_t)(IQT ? 72 : 71) << 40;
        const int sbase = (int)((scale >> (8 * sidx)) & 0xFF);          // (a lookup: the ?: ladder was five nested divergent branches)
        mul = sbase << q6;
        cmax = (1 << 23) >> q6;
    }
    __device__ __forceinline__ int operator()(int c) const
    {
        if constexpr (!ODD) {
            const int held = min(max(c, -cmax), cmax);
            return clip16(mad24(held, mul, offset) >> shift);
        }
        const long long l = ((long long)(c * (ODD ? 181 : 1)) * mul + offset) >> shift;
        return (int)min(max(l, -32768ll), 32767ll);
    }
};

// OR of the masks of the TBs that the lanes of this wave belong to, lane t working on TB (t % (G * X)) / X: a run of min(G, max(1, 64 / X)) entries that starts at a
// multiple of its length - independent LDS reads of wave-uniform addresses, one wait (an OR over the lanes through six dependent ds_bpermute round trips stood here).  Entries from the item's
// count on were reset and never set.
template <int G, int LX>
__device__ __forceinline__ uint32_t wave_masks(const uint32_t *s_m, int t)
{
    constexpr int X = 1 << LX, PER = 64 / X > 1 ? 64 / X : 1, N = G < PER ? G : PER;
    const int p0 = __builtin_amdgcn_readfirstlane(((t & ~63) % (G * X)) >> LX);
    static_assert(G * X >= 64 ? (G % N == 0) : (64 % (G * X) == 0 && N == G), "the wave's TBs are entries [p0, p0 + N)");
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < N; i++) m |= s_m[p0 + i];
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
}

// A matrix row pair's entries for one walk step.  For a pair of items the values are pinned in scalar registers in front of the two items' products: each item's products
// stand behind a test of its own mask, and left alone the compiler sinks the scalar load into both branches - one load and one wait per item instead of one per row pair.
// (PIN: a pair, in a class whose chunk index is wave-uniform - elsewhere the entries are vector loads.)
template <int N, bool PIN>
__device__ __forceinline__ void itq_row(uint32_t (&rw)[N], const uint32_t *row)
{
#pragma unroll
    for (int n = 0; n < N; n++) rw[n] = row[n];
    if constexpr (PIN) {
#pragma unroll
        for (int n = 0; n < N; n++) asm volatile("" : "+s"(rw[n]));
    }
}

// wave-uniform matrix choice: DCT-II, or for ATS work items (4..32 only) DST-VII / DCT-VIII
template <int L>
__device__ __forceinline__ const uint32_t *itdq_matrix(int tr) { return (tr == TR_DCT2 || L < 2 || L > 5) ? k_tmp + tmp_base(L) : k_atsp[tr - 1] + atsp_base(L); }

// The classes with at most 16 samples (2x2 .. 4x4, 2x8, 8x2: a quarter of a picture's work items, a twelfth of its samples): TB p of the item on lane p, the whole block
// in registers - one load of its 8 / 16 / 32 contiguous bytes (log2s == log2w: only 64x64 sub-blocks keep a CU's stride), both stages as direct products with the
// wave-uniform matrix pairs as scalar operands, the intermediate rounded and clipped (or split hi * 2^15 + lo) exactly like the LDS form.  No LDS, no barrier; lanes and
// waves without a TB leave at once.
// itdq_small_tb: the products and the stores of one TB whose record and coefficients have arrived; itdq_small: the requests of the lane's TB of each of the NI items
// (one, or the two items of a pair: k_intra_itdq), all of them in flight before the first product.
template <int LW, int LH, bool IQT>
__device__ __forceinline__ void itdq_small_tb(const ItdqArgs &a, const itq_v2 rec, const uint32_t (&raw)[(1 << (LW + LH)) / 2], const uint32_t *tmh, const uint32_t *tmw, bool s16_mid)
{
    constexpr int W = 1 << LW, H = 1 << LH, S = W * H;
    const ItdqScale<(LW + LH) & 1, IQT> dq(rec_qp(rec), a.bd, LW + LH);
    int d[S];
#pragma unroll
    for (int i = 0; i < S / 2; i++) {
        d[2 * i] = 0; d[2 * i + 1] = 0;
        if (raw[i] != 0) { d[2 * i] = dq((int16_t)(raw[i] & 0xFFFF)); d[2 * i + 1] = dq((int16_t)(raw[i] >> 16)); }
    }
    // stage 1: columns j, pairs of coefficient rows; the results leave as the column pairs stage 2 multiplies
    uint32_t mh[H][W / 2], ml[H][W / 2];
#pragma unroll
    for (int jj = 0; jj < W / 2; jj++) {
        int acc[2][H];
#pragma unroll
        for (int e = 0; e < 2; e++) {
#pragma unroll
            for (int n = 0; n < H; n++) acc[e][n] = 0;
#pragma unroll
            for (int k2 = 0; k2 < H / 2; k2++) {
                const uint32_t vp = pack16(d[(2 * k2) * W + 2 * jj + e], d[(2 * k2 + 1) * W + 2 * jj + e]);
#pragma unroll
                for (int n = 0; n < H; n++) acc[e][n] = dot2(tmh[k2 * H + n], vp, acc[e][n]);
            }
        }
#pragma unroll
        for (int n = 0; n < H; n++) {
            if (s16_mid) mh[n][jj] = pack16(clip16((acc[0][n] + 64) >> 7), clip16((acc[1][n] + 64) >> 7));      // xevdm_itdq.c ITX_SHIFT1 = 7
            else if constexpr (!IQT) {
                mh[n][jj] = pack16(acc[0][n] >> 15, acc[1][n] >> 15);                                         // |acc| < 2^28 -> hi in s16 range
                ml[n][jj] = pack16(acc[0][n] & 0x7FFF, acc[1][n] & 0x7FFF);
            }
        }
    }
    // stage 2: rows
    const int shift2 = s16_mid ? 12 - (a.bd - 8) : 7 + 12 - (a.bd - 8);
    uint32_t out[S / 2];
#pragma unroll
    for (int r = 0; r < H; r++) {
        int res[W];
        if (s16_mid) {
            int s[W];
#pragma unroll
            for (int n = 0; n < W; n++) s[n] = 1 << (shift2 - 1);
#pragma unroll
            for (int k2 = 0; k2 < W / 2; k2++) {
#pragma unroll
                for (int n = 0; n < W; n++) s[n] = dot2(tmw[k2 * W + n], mh[r][k2], s[n]);
            }
#pragma unroll
            for (int n = 0; n < W; n++) res[n] = clip16(s[n] >> shift2);
        } else if constexpr (!IQT) {
            int sh[W], sl[W];
#pragma unroll
            for (int n = 0; n < W; n++) { sh[n] = 0; sl[n] = 0; }
#pragma unroll
            for (int k2 = 0; k2 < W / 2; k2++) {
#pragma unroll
                for (int n = 0; n < W; n++) { sh[n] = dot2(tmw[k2 * W + n], mh[r][k2], sh[n]); sl[n] = dot2(tmw[k2 * W + n], ml[r][k2], sl[n]); }
            }
            const long long add = 1ll << (shift2 - 1);
#pragma unroll
            for (int n = 0; n < W; n++) {
                const long long s = (long long)sh[n] * 32768 + sl[n] + add;     // == the reference's s64 sum + rounding offset
                res[n] = (int)min(max(s >> shift2, -32768ll), 32767ll);
            }
        }
#pragma unroll
        for (int n = 0; n < W; n += 2) out[(r * W + n) / 2] = pack16(res[n], res[n + 1]);
    }
    int16_t *dst = a.resid + rec.x;
    if constexpr (S == 4) { itq_v2 v; v.x = out[0]; v.y = out[1]; *(itq_v2_s *)dst = v; }
    else {
#pragma unroll
        for (int i = 0; i < S / 8; i++) {
            itq_v4 v; v.x = out[4 * i]; v.y = out[4 * i + 1]; v.z = out[4 * i + 2]; v.w = out[4 * i + 3];
            *(itq_v4_u *)(dst + 8 * i) = v;
        }
    }
}

template <int LW, int LH, bool IQT, int NI = 1>
__device__ __forceinline__ void itdq_small(const ItdqArgs &a, const TbWave (&wv)[NI], const int tid)
{
    constexpr int W = 1 << LW, H = 1 << LH, S = W * H;
    static_assert(S <= 16 && itdq_group(LW, LH) <= 256, "one TB per lane");
    static_assert(NI == 1 || NI == 2, "an item, or a pair of one class and one transform pair");
    const int p = tid;
    bool live[NI], any = false;
#pragma unroll
    for (int i = 0; i < NI; i++) { live[i] = p < wv[i].count; any |= live[i]; }
    if (!any) return;
    itq_v2 rec[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) { rec[i] = itq_any<itq_v2>(); itq_rec_if(rec[i], a.tbs + wv[i].first + p, live[i]); }
    const uint32_t *tmh = itdq_matrix<LH>(wv[0].tr_v), *tmw = itdq_matrix<LW>(wv[0].tr_h);
    const bool s16_mid = IQT || wv[0].tr_v != TR_DCT2 || wv[0].tr_h != TR_DCT2;
    constexpr int NV = S == 4 ? 1 : S / 8;
    typedef typename std::conditional<S == 4, itq_v2, itq_v4>::type cvec;
    cvec cv[NI][NV];
    if (NI > 1) __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0): both records, in front of both coefficient requests (see itdq_item)
#pragma unroll
    for (int i = 0; i < NI; i++) {
#pragma unroll
        for (int k = 0; k < NV; k++) cv[i][k] = itq_any<cvec>();
        if (live[i]) {
            if constexpr (S == 4) cv[i][0] = *(const itq_v2_s *)(a.coef + rec[i].x);
            else {
#pragma unroll
                for (int k = 0; k < NV; k++) cv[i][k] = *(const itq_v4_u *)(a.coef + rec[i].x + 8 * k);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NI; i++) {
        if (!live[i]) continue;
        uint32_t raw[S / 2];
#pragma unroll
        for (int k = 0; k < S / 2; k++) raw[k] = cv[i][k / (S == 4 ? 2 : 4)][k % (S == 4 ? 2 : 4)];
        itdq_small_tb<LW, LH, IQT>(a, rec[i], raw, tmh, tmw, s16_mid);
    }
}

// Sparsity masks (round 3): a coded block of a real stream holds a handful of non-zero coefficients at low frequencies.  Stage 0 records, per TB, which
// coefficient ROW pairs and COLUMN pairs hold a non-zero value (LDS atomic OR, only for the few non-zero dwords); stage 1 then walks only the set row
// pairs (union over the wave's TBs, a scalar bit loop - the matrix rows stay wave-uniform SGPR loads) and stage 2 only the set column pairs: a column
// without coefficients stays zero through the vertical transform.  The round-2 loop tested every row pair with an LDS read + ballot + branch - 32
// dependent LDS round trips per stage for a 64-point transform, which is what the kernel's time was (the arithmetic itself is a few dozen dot2).
// IQT: the sequence uses the 16-bit two-stage transforms (sps->tool_iqt) - every work item keeps a clipped s16 intermediate, so only ONE intermediate plane
// exists in LDS (17 KB instead of 27 KB per workgroup) and the 32-bit split path is not compiled in: more workgroups per CU for a kernel that is bound by the
// latency of its dependent loads, not by arithmetic.
// The item is its chain of dependent round trips, so the requests come first: the TB records of all the lane's units are asked for before the mask reset and its barrier,
// the coefficients of all units before the first dequantisation - two vector-memory waits between the item's first request and its first dot2.
// NI = 2 (k_intra_itdq's residual side): two items of one class and one transform pair as ONE double-width item, in lockstep - each stage runs over both, each item
// in its own LDS block (lds + i * ITDQ_ITEM_DWORDS) and its own per-TB arrays (s_tb + i * ITDQ_TB_DWORDS), the barriers and each matrix row pair's scalar load shared.
// Four load units per lane in flight instead of two at the same number of waves (profiles/residual_item_pairs.txt).  The masks stay per TB of each item: the walk over
// the row / column pairs takes the union of the two items' wave masks, and an item's products run only for the pairs of its own mask.
template <bool IQT> constexpr int itdq_item_dwords() { return IQT ? ITDQ_LDS_DWORDS - ITDQ_PLANES_DWORDS / 2 : ITDQ_LDS_DWORDS; }
template <int LW, int LH, bool IQT, int NI = 1>
__device__ __forceinline__ void itdq_item(const ItdqArgs &a, const TbWave (&wv)[NI], uint32_t *lds, uint32_t *s_tb, const int tid)
{
    static_assert(NI == 1 || NI == 2, "an item, or a pair of one class and one transform pair");
    constexpr int ITEM = itdq_item_dwords<IQT>();
    constexpr int W = 1 << LW, H = 1 << LH;
    constexpr int N1 = H > 16 ? 16 : H, C1 = H / N1;          // stage-1 outputs per lane, chunks
    constexpr int N2 = W > 16 ? 16 : W, C2 = W / N2;
    constexpr int G = itdq_group(LW, LH);
    constexpr int RS = W / 2 + 1;                              // LDS row stride in dwords (s16 pairs), odd
    constexpr int PLANE = G * H * RS;                          // dwords per intermediate plane
    constexpr bool UNI1 = (G * W) % 64 == 0, UNI2 = (G * H) % 64 == 0;
    static_assert(2 * PLANE <= ITDQ_PLANES_DWORDS && G * W * H <= 4096 && G <= ITDQ_MAX_G, "LDS budget");
    constexpr int PLANES_DWORDS = IQT ? ITDQ_PLANES_DWORDS / 2 : ITDQ_PLANES_DWORDS;
    constexpr bool RMASK = H >= 16, CMASK = W >= 16;          // shorter transforms: the masks would cost more than the 2..4 loop rounds they can save
    uint32_t *s_rm[NI], *s_cm[NI], *s_rec[NI];               // per TB: the two masks, its record (two dwords)
#pragma unroll
    for (int i = 0; i < NI; i++) { s_rm[i] = s_tb + i * ITDQ_TB_DWORDS; s_cm[i] = s_rm[i] + ITDQ_MAX_G; s_rec[i] = s_rm[i] + 2 * ITDQ_MAX_G; }
    const int t = tid;

    // ------------------------------------------------ stage 0: load + dequantise ---------------------------
    // all coefficients of the G blocks in one coalesced sweep, dequantised once (ItdqScale) and parked in LDS as s16.  A lane has one or two load units (8 samples;
    // 4 for 2x2): both units' records, then both units' coefficients are in flight together; a unit past the item's count forms no address.
    constexpr int S = W * H, UN = S >= 8 ? 8 : 4, NU = G * S / UN, NR = (NU + 255) / 256;
    typedef typename std::conditional<UN == 8, itq_v4, itq_v2>::type cvec;
    bool on[NI][NR];
    int up[NR], uo[NR];
    itq_v2 rec[NI][NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int u = t + 256 * r;
        up[r] = (u * UN) / S; uo[r] = (u * UN) % S;
#pragma unroll
        for (int i = 0; i < NI; i++) {
            on[i][r] = (NU % 256 == 0 || u < NU) && up[r] < wv[i].count;
            rec[i][r] = itq_any<itq_v2>();
            itq_rec_if(rec[i][r], a.tbs + wv[i].first + up[r], on[i][r]);
        }
    }
    if (RMASK || CMASK) {
        if (t < G) {
#pragma unroll
            for (int i = 0; i < NI; i++) { s_rm[i][t] = 0; s_cm[i][t] = 0; }
        }
        __syncthreads();
    }
    const uint32_t *tmh = itdq_matrix<LH>(wv[0].tr_v), *tmw = itdq_matrix<LW>(wv[0].tr_h);
    const bool s16_mid = IQT || wv[0].tr_v != TR_DCT2 || wv[0].tr_h != TR_DCT2;     // ATS keeps a clipped s16 intermediate like IQT (:406-421)
    asm volatile("" :: "s"(tmh), "s"(tmw));                    // the tables' addresses now, under the records' round trip, not in front of stage 1's first row
    cvec cv[NI][NR];
    // (a pair: every record here, for all lanes, before the first coefficient request.  Left to the requests' own branches, the wait for item B's record stood behind item
    //  A's coefficient request - a lane that sat that one out cannot tell how many loads are ahead of it, so the wait was for all of them: a third round trip per pair)
    if (NI > 1) __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
#pragma unroll
    for (int i = 0; i < NI; i++) {
#pragma unroll
        for (int r = 0; r < NR; r++) {
            cv[i][r] = itq_any<cvec>();
            if (on[i][r]) {
                // row-major TB with row stride 2^log2s (a sub-block of a >64 CU keeps the CU's stride, xevd_itdq.c:573-584)
                const int16_t *src = a.coef + rec[i][r].x + ((uo[r] >> LW) << rec_log2s(rec[i][r])) + (uo[r] & (W - 1));
                if constexpr (UN == 8) cv[i][r] = *(const itq_v4_u *)src; else cv[i][r] = *(const itq_v2_s *)src;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NI; i++) {
        uint32_t *ldsc = lds + i * ITEM + PLANES_DWORDS;       // dequantised coefficients, [p][row][col] s16
#pragma unroll
        for (int r = 0; r < NR; r++) {
            if (!on[i][r]) continue;
            const int p = up[r], o = uo[r];
            const ItdqScale<(LW + LH) & 1, IQT> dq(rec_qp(rec[i][r]), a.bd, LW + LH);
            if (o == 0) { s_rec[i][2 * p] = rec[i][r].x; s_rec[i][2 * p + 1] = rec[i][r].y; }      // for stage 2's lanes, which belong to other TBs than stage 0's: an LDS read, not a second fetch
            uint32_t raw[UN / 2];
#pragma unroll
            for (int k = 0; k < UN / 2; k++) raw[k] = cv[i][r][k];
#pragma unroll
            for (int k = 0; k < UN / 2; k++) {
                if (raw[k] == 0) continue;
                raw[k] = pack16(dq((int16_t)(raw[k] & 0xFFFF)), dq((int16_t)(raw[k] >> 16)));
                if (RMASK) atomicOr(&s_rm[i][p], 1u << ((o + 2 * k) >> (LW + 1)));                  // row pair of this dword
                if (CMASK) atomicOr(&s_cm[i][p], 1u << (((o + 2 * k) & (W - 1)) >> 1));              // column pair
            }
#pragma unroll
            for (int k = 0; k < UN / 2; k++) ldsc[(p * S + o) / 2 + k] = raw[k];
        }
    }
    __syncthreads();

    // ------------------------------------------------ stage 1: columns ------------------------------------
    uint32_t rows1[NI], rows1_any = 0;
#pragma unroll
    for (int i = 0; i < NI; i++) { rows1[i] = RMASK ? wave_masks<G, LW>(s_rm[i], t) : 0u; rows1_any |= rows1[i]; }
    if (t < G * W * C1) {
        const int idx = t % (G * W);
        int chunk = t / (G * W);
        if (UNI1) chunk = __builtin_amdgcn_readfirstlane(chunk);
        const int p = idx >> LW, j = idx & (W - 1);
        bool valid[NI];
        uint32_t vmask[NI];
        const int16_t *src[NI];
        int acc[NI][N1];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            valid[i] = p < wv[i].count;
            vmask[i] = valid[i] ? 0xFFFFFFFFu : 0u;           // the LDS reads are unconditional (a TB past the count holds whatever was there): no branch with a wait of its own around them
            src[i] = (const int16_t *)(lds + i * ITEM + PLANES_DWORDS) + p * (W * H) + j;
#pragma unroll
            for (int n = 0; n < N1; n++) acc[i][n] = 0;
        }
        if (RMASK) {
            for (uint32_t m = rows1_any; m; m &= m - 1) {      // the row pairs that hold a coefficient in one of this wave's TBs (of either item)
                const int k2 = __builtin_ctz(m);
                uint32_t vp[NI];
#pragma unroll
                for (int i = 0; i < NI; i++) vp[i] = pack16(src[i][(2 * k2) * W], src[i][(2 * k2 + 1) * W]) & vmask[i];
                uint32_t row[N1];
                itq_row<N1, (NI > 1 && UNI1)>(row, tmh + k2 * H + chunk * N1);
#pragma unroll
                for (int i = 0; i < NI; i++) {
                    if (NI > 1 && !((rows1[i] >> k2) & 1)) continue;      // the other item's row pair: nothing of this item's lies there
#pragma unroll
                    for (int n = 0; n < N1; n++) acc[i][n] = dot2(row[n], vp[i], acc[i][n]);
                }
            }
        } else {
            for (int k2 = 0; k2 < H / 2; k2++) {
                uint32_t vp[NI];
                bool go[NI], any = false;
#pragma unroll
                for (int i = 0; i < NI; i++) {
                    vp[i] = pack16(src[i][(2 * k2) * W], src[i][(2 * k2 + 1) * W]) & vmask[i];
                    go[i] = __ballot(vp[i] != 0) != 0;
                    any |= go[i];
                }
                if (!any) continue;                                // both coefficient rows zero across this wave
                uint32_t row[N1];
                itq_row<N1, (NI > 1 && UNI1)>(row, tmh + k2 * H + chunk * N1);
#pragma unroll
                for (int i = 0; i < NI; i++) {
                    if (NI > 1 && !go[i]) continue;
#pragma unroll
                    for (int n = 0; n < N1; n++) acc[i][n] = dot2(row[n], vp[i], acc[i][n]);
                }
            }
        }
        // transposed store: element [p][row = chunk*N1+n][col = j] - only columns stage 2 will read (its column pair holds a coefficient)
        const int base = (p * H + chunk * N1) * (2 * RS) + j;
#pragma unroll
        for (int i = 0; i < NI; i++) {
            int16_t *ldsh = (int16_t *)(lds + i * ITEM);       // plane 0: hi (or the IQT intermediate), plane 1: lo
            int16_t *ldsl = (int16_t *)(lds + i * ITEM + PLANE);
            if (CMASK && !(valid[i] && ((s_cm[i][p] >> (j >> 1)) & 1))) {
            } else if (s16_mid) {
#pragma unroll
                for (int n = 0; n < N1; n++) ldsh[base + n * (2 * RS)] = (int16_t)clip16((acc[i][n] + 64) >> 7);   // xevdm_itdq.c ITX_SHIFT1 = 7
            } else {
#pragma unroll
                for (int n = 0; n < N1; n++) {
                    ldsh[base + n * (2 * RS)] = (int16_t)(acc[i][n] >> 15);          // |acc| < 2^28 -> hi in s16 range
                    ldsl[base + n * (2 * RS)] = (int16_t)(acc[i][n] & 0x7FFF);
                }
            }
        }
    }
    __syncthreads();

    // ------------------------------------------------ stage 2: rows ---------------------------------------
    uint32_t cols2[NI], cols2_any = 0;
#pragma unroll
    for (int i = 0; i < NI; i++) { cols2[i] = CMASK ? wave_masks<G, LH>(s_cm[i], t) : 0u; cols2_any |= cols2[i]; }
    if (t < G * H * C2) {
        const int idx = t % (G * H);
        int chunk = t / (G * H);
        if (UNI2) chunk = __builtin_amdgcn_readfirstlane(chunk);
        const int p = idx >> LH, r = idx & (H - 1);
        bool live[NI], any_live = false;
#pragma unroll
        for (int i = 0; i < NI; i++) { live[i] = p < wv[i].count; any_live |= live[i]; }
        if (!any_live) return;
        // a column pair outside this TB's own mask was not written by stage 1 (it may be set for another TB of the wave): reads as zero.  (A pair's lane whose TB only
        // one of the two items has runs the other item's products on zeros and stores nothing for it.)
        uint32_t own[NI];
        itq_v2 tb[NI];
        const uint32_t *inh[NI], *inl[NI];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            own[i] = CMASK ? s_cm[i][p] : 0xFFFFFFFFu;
            if (NI > 1 && !live[i]) own[i] = 0;
            tb[i].x = s_rec[i][2 * p]; tb[i].y = s_rec[i][2 * p + 1];
            inh[i] = lds + i * ITEM + (p * H + r) * RS;
            inl[i] = inh[i] + PLANE;
        }
        const int shift2 = s16_mid ? 12 - (a.bd - 8) : 7 + 12 - (a.bd - 8);
        int res[NI][N2];
        if (s16_mid) {
            int s[NI][N2];
#pragma unroll
            for (int i = 0; i < NI; i++)
#pragma unroll
                for (int n = 0; n < N2; n++) s[i][n] = 1 << (shift2 - 1);
            if (CMASK) {
                for (uint32_t m = cols2_any; m; m &= m - 1) {
                    const int k2 = __builtin_ctz(m);
                    uint32_t vp[NI];
#pragma unroll
                    for (int i = 0; i < NI; i++) vp[i] = inh[i][k2] & (0u - ((own[i] >> k2) & 1));
                    uint32_t row[N2];
                    itq_row<N2, (NI > 1 && UNI2)>(row, tmw + k2 * W + chunk * N2);
#pragma unroll
                    for (int i = 0; i < NI; i++) {
                        if (NI > 1 && !((cols2[i] >> k2) & 1)) continue;      // the other item's column pair
#pragma unroll
                        for (int n = 0; n < N2; n++) s[i][n] = dot2(row[n], vp[i], s[i][n]);
                    }
                }
            } else {
                for (int k2 = 0; k2 < W / 2; k2++) {
                    uint32_t vp[NI];
                    bool go[NI], any = false;
#pragma unroll
                    for (int i = 0; i < NI; i++) {
                        vp[i] = inh[i][k2] & (0u - ((own[i] >> k2) & 1));      // (own is all ones here, but for a lane of a pair whose TB this item does not have)
                        go[i] = __ballot(vp[i] != 0) != 0;
                        any |= go[i];
                    }
                    if (!any) continue;
                    uint32_t row[N2];
                    itq_row<N2, (NI > 1 && UNI2)>(row, tmw + k2 * W + chunk * N2);
#pragma unroll
                    for (int i = 0; i < NI; i++) {
                        if (NI > 1 && !go[i]) continue;
#pragma unroll
                        for (int n = 0; n < N2; n++) s[i][n] = dot2(row[n], vp[i], s[i][n]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NI; i++)
#pragma unroll
                for (int n = 0; n < N2; n++) res[i][n] = clip16(s[i][n] >> shift2);
        } else {
            int sh[NI][N2], sl[NI][N2];
#pragma unroll
            for (int i = 0; i < NI; i++)
#pragma unroll
                for (int n = 0; n < N2; n++) { sh[i][n] = 0; sl[i][n] = 0; }
            if (CMASK) {
                for (uint32_t m = cols2_any; m; m &= m - 1) {
                    const int k2 = __builtin_ctz(m);
                    const uint32_t *row = tmw + k2 * W + chunk * N2;
#pragma unroll
                    for (int i = 0; i < NI; i++) {
                        const uint32_t mine = 0u - ((own[i] >> k2) & 1);
                        const uint32_t vh = inh[i][k2] & mine, vl = inl[i][k2] & mine;
#pragma unroll
                        for (int n = 0; n < N2; n++) { sh[i][n] = dot2(row[n], vh, sh[i][n]); sl[i][n] = dot2(row[n], vl, sl[i][n]); }
                    }
                }
            } else {
                for (int k2 = 0; k2 < W / 2; k2++) {
                    uint32_t vh[NI], vl[NI], nz = 0;
#pragma unroll
                    for (int i = 0; i < NI; i++) {
                        const uint32_t mine = 0u - ((own[i] >> k2) & 1);
                        vh[i] = inh[i][k2] & mine; vl[i] = inl[i][k2] & mine;
                        nz |= vh[i] | vl[i];
                    }
                    if (__ballot(nz != 0) == 0) continue;
                    const uint32_t *row = tmw + k2 * W + chunk * N2;
#pragma unroll
                    for (int i = 0; i < NI; i++)
#pragma unroll
                        for (int n = 0; n < N2; n++) { sh[i][n] = dot2(row[n], vh[i], sh[i][n]); sl[i][n] = dot2(row[n], vl[i], sl[i][n]); }
                }
            }
            const long long add = 1ll << (shift2 - 1);
#pragma unroll
            for (int i = 0; i < NI; i++)
#pragma unroll
                for (int n = 0; n < N2; n++) {
                    const long long s = (long long)sh[i][n] * 32768 + sl[i][n] + add;     // == the reference's s64 sum + rounding offset
                    res[i][n] = (int)min(max(s >> shift2, -32768ll), 32767ll);
                }
        }
#pragma unroll
        for (int i = 0; i < NI; i++) {
            if (NI > 1 && !live[i]) continue;
            int16_t *out = a.resid + tb[i].x + (r << rec_log2s(tb[i])) + chunk * N2;
            if constexpr (N2 >= 8) {
#pragma unroll
                for (int n = 0; n < N2; n += 8) {
                    uint4 v;
                    v.x = pack16(res[i][n + 0], res[i][n + 1]);
                    v.y = pack16(res[i][n + 2], res[i][n + 3]);
                    v.z = pack16(res[i][n + 4], res[i][n + 5]);
                    v.w = pack16(res[i][n + 6], res[i][n + 7]);
                    *(uint4 *)(out + n) = v;
                }
            } else if constexpr (N2 == 4) {
                uint2 v;
                v.x = pack16(res[i][0], res[i][1]);
                v.y = pack16(res[i][2], res[i][3]);
                *(uint2 *)out = v;
            } else {
                *(uint32_t *)out = pack16(res[i][0], res[i][1]);
            }
        }
    }
}

// one work item; lds = ITDQ_LDS_DWORDS dwords (IQT: minus half the planes), s_tb = ITDQ_TB_DWORDS dwords; all 256 threads of the workgroup call it
template <bool IQT>
__device__ __forceinline__ void itdq_dispatch(const ItdqArgs &a, int wi, uint32_t *lds, uint32_t *s_tb)
{
    // the record as three scalar loads (its u16 / u8 fields one by one came as vector loads + v_readfirstlane: a vector round trip in front of everything)
    static_assert(sizeof(TbWave) == 12 && alignof(TbWave) == 4, "TbWave is read as three dwords");
    const uint32_t *w = (const uint32_t *)(a.waves + wi);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    TbWave wv[1];
    wv[0].first = w0; wv[0].count = (uint16_t)(w1 & 0xFFFF); wv[0].log2w = (uint8_t)(w1 >> 16); wv[0].log2h = (uint8_t)(w1 >> 24); wv[0].tr_v = (uint8_t)w2; wv[0].tr_h = (uint8_t)(w2 >> 8);
#define CASE(lw, lh) case (lw) * 8 + (lh): if constexpr ((lw) + (lh) <= 4) itdq_small<lw, lh, IQT>(a, wv, threadIdx.x); else itdq_item<lw, lh, IQT>(a, wv, lds, s_tb, threadIdx.x); break;
#define ROW(lw) CASE(lw, 1) CASE(lw, 2) CASE(lw, 3) CASE(lw, 4) CASE(lw, 5) CASE(lw, 6)
    switch (wv[0].log2w * 8 + wv[0].log2h) {
        ROW(1) ROW(2) ROW(3) ROW(4) ROW(5) ROW(6)
        default: break;
    }
#undef ROW
#undef CASE
}

// Two adjacent entries of the item list, waves[e0] and [e0 + 1], in one workgroup (n = 2; n = 1: the entry e0 alone, in the single form): as one double-width item where they have the same class and the same transform
// pair (the class-sorted list makes that the rule), else - and for an odd last entry - the single form, one entry after the other, each in its own LDS block.  Every entry
// is done exactly once.  lds = 2 x itdq_item_dwords<IQT>() dwords, s_tb = 2 x ITDQ_TB_DWORDS; all 256 threads of the workgroup call it.
template <bool IQT>
__device__ __forceinline__ void itdq_dispatch_pair(const ItdqArgs &a, int e0, int n, uint32_t *lds, uint32_t *s_tb)
{
    // both records as scalar loads together (an odd last entry reads itself twice: no address past the list)
    const bool two = n == 2 && e0 + 1 < a.n_waves;
    const uint32_t *w = (const uint32_t *)(a.waves + e0), *x = (const uint32_t *)(a.waves + e0 + (two ? 1 : 0));
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], x0 = x[0], x1 = x[1], x2 = x[2];
    TbWave wv[2];
    wv[0].first = w0; wv[0].count = (uint16_t)(w1 & 0xFFFF); wv[0].log2w = (uint8_t)(w1 >> 16); wv[0].log2h = (uint8_t)(w1 >> 24); wv[0].tr_v = (uint8_t)w2; wv[0].tr_h = (uint8_t)(w2 >> 8);
    wv[1].first = x0; wv[1].count = (uint16_t)(x1 & 0xFFFF); wv[1].log2w = (uint8_t)(x1 >> 16); wv[1].log2h = (uint8_t)(x1 >> 24); wv[1].tr_v = (uint8_t)x2; wv[1].tr_h = (uint8_t)(x2 >> 8);
#define ROW(lw) CASE(lw, 1) CASE(lw, 2) CASE(lw, 3) CASE(lw, 4) CASE(lw, 5) CASE(lw, 6)
    if (two && (w1 >> 16) == (x1 >> 16) && (w2 & 0xFFFFu) == (x2 & 0xFFFFu)) {
#define CASE(lw, lh) case (lw) * 8 + (lh): if constexpr ((lw) + (lh) <= 4) itdq_small<lw, lh, IQT, 2>(a, wv, threadIdx.x); else itdq_item<lw, lh, IQT, 2>(a, wv, lds, s_tb, threadIdx.x); break;
        switch (wv[0].log2w * 8 + wv[0].log2h) {
            ROW(1) ROW(2) ROW(3) ROW(4) ROW(5) ROW(6)
            default: break;
        }
#undef CASE
        return;
    }
#pragma unroll 1
    for (int k = 0; k < (two ? 2 : 1); k++) {
        TbWave one[1];
        one[0] = k ? wv[1] : wv[0];
        // (the lane's index behind a fence: left visible, everything the 36 classes derive from it is invariant in this loop and gets hoisted in front of it - 250 VGPRs)
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
        __builtin_assume(t >= 0 && t < 256);
        uint32_t *lds_k = lds + k * itdq_item_dwords<IQT>(), *s_tb_k = s_tb + k * ITDQ_TB_DWORDS;
#define CASE(lw, lh) case (lw) * 8 + (lh): if constexpr ((lw) + (lh) <= 4) itdq_small<lw, lh, IQT>(a, one, t); else itdq_item<lw, lh, IQT>(a, one, lds_k, s_tb_k, t); break;
        switch (one[0].log2w * 8 + one[0].log2h) {
            ROW(1) ROW(2) ROW(3) ROW(4) ROW(5) ROW(6)
            default: break;
        }
#undef CASE
    }
#undef ROW
}
