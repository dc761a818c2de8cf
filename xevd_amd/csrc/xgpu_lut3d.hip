// xgpu_lut3d.hip - the 3D LUT side of the C ABI of include/xevd_hip.h that is not an output call: the host-only helpers that make the uint16 tables (double
// arithmetic with + - * / and floor only, so that every host makes the same table; tests/lut3d_ref.py restates them) and the LUT handles of a context.  The output
// calls that read a handle are xgpu_output.hip's; the kernel is k_output_lut3d.hip; the contract is INTEGRATION.md section 8q.
#include "xgpu_host.h"
#include <vector>

static bool lut3d_n_ok(int n) { return n >= 2 && n <= 65; }
// floor(clip(v, 0, 1) * 65535 + 0.5); NaN -> 0
static uint16_t lut3d_quant(double v)
{
    if (!(v > 0.0)) v = 0.0;
    if (v > 1.0) v = 1.0;
    return (uint16_t)floor(v * 65535.0 + 0.5);
}
int xgpu_lut3d_from_float(const float *rgb, int n, uint16_t *nodes)
{
    if (!rgb || !nodes) return XGPU_ERR_INVALID_ARGUMENT;
    if (!lut3d_n_ok(n)) return XGPU_ERR_UNSUPPORTED;
    const size_t cnt = (size_t)3 * n * n * n;
    for (size_t i = 0; i < cnt; i++) nodes[i] = lut3d_quant((double)rgb[i]);
    return XGPU_OK;
}
int xgpu_lut3d_identity(int n, uint16_t *nodes)
{
    if (!nodes) return XGPU_ERR_INVALID_ARGUMENT;
    if (!lut3d_n_ok(n)) return XGPU_ERR_UNSUPPORTED;
    uint16_t e[65];
    for (int i = 0; i < n; i++) e[i] = (uint16_t)((2u * 65535u * (unsigned)i + (unsigned)(n - 1)) / (2u * (unsigned)(n - 1)));
    size_t o = 0;
    for (int b = 0; b < n; b++)
        for (int g = 0; g < n; g++)
            for (int r = 0; r < n; r++) { nodes[o++] = e[r]; nodes[o++] = e[g]; nodes[o++] = e[b]; }
    return XGPU_OK;
}
int xgpu_lut3d_shaper(int bit_depth, const float *curve, int n_curve, const float in_min[3], const float in_max[3], uint16_t *out)
{
    if (bit_depth < 8 || bit_depth > 12 || !out || (curve && n_curve < 2)) return XGPU_ERR_INVALID_ARGUMENT;
    const int m = (1 << bit_depth) - 1;
    for (int k = 0; k < 3; k++) {
        const double lo = in_min ? (double)in_min[k] : 0.0, hi = in_max ? (double)in_max[k] : 1.0;
        if (!(hi > lo) || !(hi - lo <= 1.7e308)) return XGPU_ERR_INVALID_ARGUMENT;      // (NaN fails the first comparison, an infinite span the second)
        for (int c = 0; c <= m; c++) {
            double t = ((double)c / (double)m - lo) / (hi - lo);
            if (!(t > 0.0)) t = 0.0;
            if (t > 1.0) t = 1.0;
            if (curve) {
                const double u = t * (double)(n_curve - 1);
                const int j = std::min((int)floor(u), n_curve - 2);
                const double c0 = (double)curve[3 * j + k], c1 = (double)curve[3 * (j + 1) + k];
                t = c0 + (u - (double)j) * (c1 - c0);
            }
            out[(size_t)k * (m + 1) + c] = lut3d_quant(t);
        }
    }
    return XGPU_OK;
}

// One LUT on the device is one block: the shaper [3][2^B] at its start, the cube's n^3 records of 8 bytes (R | G << 16, B) behind it.  Made on the host, copied
// with a blocking hipMemcpy: when the call returns the tables are there, and no stream has to order anything against the upload.
int xgpu_lut3d_create(xgpu_ctx *c, int n, const uint16_t *nodes, const uint16_t *shaper, int *handle)
{
    ARGCHK(c, c != NULL); ARGCHK(c, nodes != NULL); ARGCHK(c, handle != NULL);
    *handle = -1;
    if (!lut3d_n_ok(n)) { snprintf(c->err, sizeof(c->err), "lut3d_create: %d nodes per axis, 2 .. 65 are supported", n); return XGPU_ERR_UNSUPPORTED; }
    int h = 0;
    while (h < XGPU_MAX_LUT3D && c->lut3d[h].d) h++;
    if (h == XGPU_MAX_LUT3D) { snprintf(c->err, sizeof(c->err), "lut3d_create: all %d handles of the context are in use", XGPU_MAX_LUT3D); return XGPU_ERR_OUT_OF_MEMORY; }
    const int bd = c->sp.bit_depth_luma;
    const size_t sb = lut3d_shaper_bytes(bd), nn = (size_t)n * n * n;
    std::vector<uint8_t> blk(sb + 8 * nn);
    uint16_t *hs = (uint16_t *)blk.data();
    if (shaper) memcpy(hs, shaper, sb);
    else (void)xgpu_lut3d_shaper(bd, NULL, 0, NULL, NULL, hs);
    uint16_t *hc = (uint16_t *)(blk.data() + sb);
    for (size_t i = 0; i < nn; i++) { hc[4 * i] = nodes[3 * i]; hc[4 * i + 1] = nodes[3 * i + 1]; hc[4 * i + 2] = nodes[3 * i + 2]; hc[4 * i + 3] = 0; }
    HIPCHK(c, hipSetDevice(c->sp.device));
    uint8_t *d = NULL;
    if (hipMalloc((void **)&d, blk.size()) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(c->err, sizeof(c->err), "lut3d_create: cannot allocate the %zu-byte tables", blk.size());
        return XGPU_ERR_OUT_OF_MEMORY;
    }
    if (hipMemcpy(d, blk.data(), blk.size(), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(d);
        snprintf(c->err, sizeof(c->err), "lut3d_create: the upload failed");
        return XGPU_ERR_UNEXPECTED;
    }
    c->lut3d[h].d = d; c->lut3d[h].n = n;
    *handle = h;
    return XGPU_OK;
}
// Every call that read the LUT has ended in the context's stream (out_join), so waiting for that stream waits for all of them - upload_dra's ordering, with
// the host waiting where the DRA upload queues behind.
int xgpu_lut3d_destroy(xgpu_ctx *c, int handle)
{
    ARGCHK(c, c != NULL); ARGCHK(c, handle >= 0 && handle < XGPU_MAX_LUT3D && c->lut3d[handle].d != NULL);
    HIPCHK(c, hipSetDevice(c->sp.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->lut3d[handle].d);
    c->lut3d[handle].d = NULL; c->lut3d[handle].n = 0;
    return XGPU_OK;
}
