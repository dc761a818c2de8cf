// xgpu_dither.hip - the dither side of the C ABI of include/xevd_hip.h that is not an output call: the host-only constructors of the Bayer and the blue-noise
// matrix and of the per-picture phase (integers only, so that every host makes the same matrix; tests/dither_ref.py restates them) and the matrix handles of a
// context.  The output calls that read a handle are xgpu_output.hip's; the kernels are k_output_dither.hip; the contract is INTEGRATION.md section 8r.
#include "xgpu_host.h"
#include <vector>

int xgpu_dither_bayer(int log2n, uint16_t *rank)
{
    if (!rank) return XGPU_ERR_INVALID_ARGUMENT;
    if (log2n < 1 || log2n > 7) return XGPU_ERR_UNSUPPORTED;
    const int n = 1 << log2n;
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++) {
            int r = 0;
            for (int b = 0; b < log2n; b++) {
                const int hi = 2 * (log2n - 1 - b);
                r |= (((x ^ y) >> b) & 1) << (hi + 1);
                r |= ((y >> b) & 1) << hi;
            }
            rank[y * n + x] = (uint16_t)r;
        }
    return XGPU_OK;
}

// floor(2^20 * exp(-d2 / 4.5) + 0.5) for d2 = dx^2 + dy^2, |dx|, |dy| <= 6: the Gaussian of sigma^2 = 2.25 the void filling adds around every filled cell
static const int32_t BLUE_GAUSS[73] = {
    1048576, 839634, 672326, 538357, 431082, 345184, 276402, 221325, 177223, 141909, 113632, 90989, 72859, 58341, 46716, 37407, 29953, 23985, 19205, 15378,
    12314, 9860, 7896, 6322, 5062, 4054, 3246, 2599, 2081, 1667, 1334, 1069, 856, 685, 549, 439, 352, 282, 226, 181, 145, 116, 93, 74, 59, 48, 38, 31, 24, 20,
    16, 13, 10, 8, 6, 5, 4, 3, 3, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 };

int xgpu_dither_blue(int log2n, uint32_t seed, uint16_t *rank)
{
    if (!rank) return XGPU_ERR_INVALID_ARGUMENT;
    if (log2n < 2 || log2n > 7) return XGPU_ERR_UNSUPPORTED;
    const int n = 1 << log2n, nn = n * n;
    // tie: Fisher-Yates from the back with a 64-bit linear congruential generator (Knuth's MMIX constants), the high bits of the state
    std::vector<int64_t> key(nn);      // E * n^2 + tie of an unfilled cell, INT64_MAX of a filled one
    std::vector<int32_t> tie(nn);
    for (int i = 0; i < nn; i++) tie[i] = i;
    uint64_t s = seed;
    for (int i = nn - 1; i > 0; i--) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const int j = (int)((s >> 33) % (uint64_t)(i + 1));
        std::swap(tie[i], tie[j]);
    }
    for (int i = 0; i < nn; i++) key[i] = tie[i];
    for (int r = 0; r < nn; r++) {
        int best = 0;
        for (int i = 1; i < nn; i++) if (key[i] < key[best]) best = i;      // the keys of unfilled cells are distinct: E * n^2 + a permutation below n^2
        rank[best] = (uint16_t)r;
        key[best] = INT64_MAX;
        const int by = best >> log2n, bx = best & (n - 1);
        for (int dy = -6; dy <= 6; dy++)
            for (int dx = -6; dx <= 6; dx++) {
                const int i = (((by + dy) & (n - 1)) << log2n) | ((bx + dx) & (n - 1));
                if (key[i] != INT64_MAX) key[i] += (int64_t)BLUE_GAUSS[dx * dx + dy * dy] * nn;
            }
    }
    return XGPU_OK;
}

static bool pow2_upto128(int v) { return v >= 1 && v <= 128 && !(v & (v - 1)); }

int xgpu_dither_phase(uint32_t index, int mw, int mh, int *px, int *py)
{
    if (!px || !py || !pow2_upto128(mw) || !pow2_upto128(mh)) return XGPU_ERR_INVALID_ARGUMENT;
    *px = (int)(((uint32_t)(index * 0x9E3779B1u) >> 16) & (uint32_t)(mw - 1));
    *py = (int)(((uint32_t)(index * 0x85EBCA6Bu) >> 16) & (uint32_t)(mh - 1));
    return XGPU_OK;
}

// One matrix on the device is one block of mh extended rows (DitherSlot).  Made on the host, copied with a blocking hipMemcpy: when the call returns the ranks
// are there, and no stream has to order anything against the upload.
int xgpu_dither_create(xgpu_ctx *c, int mw, int mh, int k, const uint16_t *rank, int *handle)
{
    ARGCHK(c, c != NULL); ARGCHK(c, rank != NULL); ARGCHK(c, handle != NULL);
    *handle = -1;
    if (!pow2_upto128(mw) || !pow2_upto128(mh) || k < 1 || k > 14) {
        snprintf(c->err, sizeof(c->err), "dither_create: %d x %d ranks of %d bits; sides are powers of two in 1 .. 128, 1 <= k <= 14", mw, mh, k);
        return XGPU_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < mw * mh; i++)
        if (rank[i] >> k) { snprintf(c->err, sizeof(c->err), "dither_create: rank %d at %d is not below 2^%d", rank[i], i, k); return XGPU_ERR_INVALID_ARGUMENT; }
    int h = 0;
    while (h < XGPU_MAX_DITHER && c->dither[h].d) h++;
    if (h == XGPU_MAX_DITHER) { snprintf(c->err, sizeof(c->err), "dither_create: all %d handles of the context are in use", XGPU_MAX_DITHER); return XGPU_ERR_OUT_OF_MEMORY; }
    const int stride = mw + 16;
    std::vector<uint16_t> blk((size_t)stride * mh);
    for (int y = 0; y < mh; y++)
        for (int x = 0; x < stride; x++) blk[(size_t)y * stride + x] = rank[y * mw + (x & (mw - 1))];
    HIPCHK(c, hipSetDevice(c->sp.device));
    uint16_t *d = NULL;
    const size_t bytes = blk.size() * sizeof(uint16_t);
    if (hipMalloc((void **)&d, bytes) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(c->err, sizeof(c->err), "dither_create: cannot allocate the %zu-byte matrix", bytes);
        return XGPU_ERR_OUT_OF_MEMORY;
    }
    if (hipMemcpy(d, blk.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(d);
        snprintf(c->err, sizeof(c->err), "dither_create: the upload failed");
        return XGPU_ERR_UNEXPECTED;
    }
    c->dither[h].d = d; c->dither[h].mw = mw; c->dither[h].mh = mh; c->dither[h].k = k;
    *handle = h;
    return XGPU_OK;
}
// Every call that read the matrix has ended in the context's stream (out_join), so waiting for that stream waits for all of them (xgpu_lut3d_destroy's ordering).
int xgpu_dither_destroy(xgpu_ctx *c, int handle)
{
    ARGCHK(c, c != NULL); ARGCHK(c, handle >= 0 && handle < XGPU_MAX_DITHER && c->dither[handle].d != NULL);
    HIPCHK(c, hipSetDevice(c->sp.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->dither[handle].d);
    c->dither[handle].d = NULL; c->dither[handle].mw = c->dither[handle].mh = c->dither[handle].k = 0;
    return XGPU_OK;
}
