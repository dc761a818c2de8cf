// Sweep of the host-only half of the picture comparison (development tool): xgpu_compare_check / xgpu_compare_ref_size / xgpu_compare_map_size over valid and
// hostile arguments - NULLs, negative and huge sizes, crops and pitches - against the rules of include/xevd_hip.h restated here, for a sanitizer build of the
// file they live in.  No device is touched.  The sanitized object is linked with the product library's other objects (after make -C xevd_amd/csrc):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined -c xevd_amd/csrc/xgpu_output.hip -o xgpu_output_san.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -c tests/tools/compare_check_sweep.cc -o compare_check_sweep.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o compare_check_sweep compare_check_sweep.o xgpu_output_san.o $(ls xevd_amd/csrc/*.o | grep -v xgpu_output.o)
//   ./compare_check_sweep          (prints the number of calls; exit status 1 on the first disagreement)
#include "../../include/xevd_hip.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

static size_t rule_ref_size(const xgpu_compare_ref &r, int w, int h)
{
    if (w <= 0 || h <= 0 || ((w | h) & 1) || r.kind != XGPU_CMP_REF_YUV420 || (r.dtype != XGPU_OUT_U8 && r.dtype != XGPU_OUT_U16)) return 0;
    const size_t es = r.dtype == XGPU_OUT_U8 ? 1 : 2;
    if (r.row_pitch % (2 * es) || (r.row_pitch && r.row_pitch < (size_t)w * es)) return 0;
    const size_t pitch = r.row_pitch ? r.row_pitch : (size_t)w * es;
    return (size_t)h * pitch + (size_t)(h - 1) * (pitch / 2) + (size_t)(w / 2) * es;
}
static bool rule_params(const xgpu_compare_params &p, int w, int h)
{
    if (w <= 0 || h <= 0 || ((w | h) & 1)) return false;
    for (int i = 0; i < 4; i++) if (p.crop[i] < 0 || (p.crop[i] & 1)) return false;
    if ((long long)p.crop[0] + p.crop[1] >= w || (long long)p.crop[2] + p.crop[3] >= h) return false;
    return (p.ssim == 0 || p.ssim == 1) && (p.block_map == 0 || p.block_map == 1);
}
static int rule_check(const xgpu_compare_ref &r, const xgpu_compare_params &p, int w, int h, int bd)
{
    if (!rule_params(p, w, h) || bd < 8 || bd > 12) return XGPU_ERR_INVALID_ARGUMENT;
    if (r.kind == XGPU_CMP_REF_PIC) return r.pic < 0 ? XGPU_ERR_INVALID_ARGUMENT : XGPU_OK;
    const size_t need = rule_ref_size(r, w, h);
    if (!need || (r.dtype == XGPU_OUT_U8 && bd != 8) || !r.d_yuv || r.size < need) return XGPU_ERR_INVALID_ARGUMENT;
    return XGPU_OK;
}

int main()
{
    static const int sizes[][2] = { { 8, 8 }, { 72, 40 }, { 200, 136 }, { 7680, 4320 }, { 16384, 16384 }, { 0, 8 }, { 8, -2 }, { 9, 8 }, { INT_MAX, 2 }, { INT_MAX - 1, INT_MAX - 1 }, { INT_MIN, INT_MIN } };
    static const int crops[][4] = { { 0, 0, 0, 0 }, { 2, 6, 4, 2 }, { 1, 0, 0, 0 }, { 0, 0, 0, -2 }, { 100, 100, 0, 0 }, { 0, 0, 60, 76 }, { INT_MAX - 1, INT_MAX - 1, 0, 0 }, { INT_MIN, 0, 0, 0 },
                                    { 0, 0, INT_MAX - 1, 2 } };
    static const size_t pitches[] = { 0, 2, 200, 202, 400, 402, 404, 15360, 15364, (size_t)1 << 40 };
    static const size_t avail[] = { 0, 1, 200 * 136 * 3 / 2, 200 * 136 * 3 - 1, 200 * 136 * 3, (size_t)1 << 40, ~(size_t)0 };
    static const int kinds[] = { XGPU_CMP_REF_PIC, XGPU_CMP_REF_YUV420, 2, -1, INT_MAX }, dtypes[] = { XGPU_OUT_U8, XGPU_OUT_U16, XGPU_OUT_F16, XGPU_OUT_F32, -1, INT_MIN };
    static const int flags[] = { 0, 1, 2, -1, INT_MIN }, depths[] = { 8, 10, 12, 7, 13, 0, INT_MAX };
    static char mem[16];
    long calls = 0;
    if (xgpu_compare_ref_size(NULL, 8, 8) || xgpu_compare_map_size(NULL, 8, 8) || xgpu_compare_check(NULL, NULL, 8, 8, 8) != XGPU_ERR_INVALID_ARGUMENT) { printf("NULL arguments accepted\n"); return 1; }
    for (const auto &sz : sizes) for (const auto &cr : crops) for (int ssim : flags) for (int bm : flags) {
        xgpu_compare_params p;
        for (int i = 0; i < 4; i++) p.crop[i] = cr[i];
        p.ssim = ssim; p.block_map = bm;
        const int w = sz[0], h = sz[1];
        size_t want = 0;
        if (rule_params(p, w, h) && bm) {
            const size_t cw = (size_t)w - cr[0] - cr[1], ch = (size_t)h - cr[2] - cr[3];
            want = 3 * ((ch + 15) / 16) * ((cw + 15) / 16) * 8;
        }
        const size_t got = xgpu_compare_map_size(&p, w, h);
        calls++;
        if (got != want) { printf("map_size %dx%d crop %d %d %d %d ssim %d map %d: %zu, expected %zu\n", w, h, cr[0], cr[1], cr[2], cr[3], ssim, bm, got, want); return 1; }
        if (!((ssim == 0 && bm == 0) || (ssim == 1 && bm == 1) || (ssim == 2 && bm == 0))) continue;      // the reference's sweep: under three of the flag pairs
        for (int kind : kinds) for (int dtype : dtypes) for (size_t pitch : pitches) for (size_t size : avail) for (int slot : { 0, -1, INT_MIN }) for (const void *ptr : { (const void *)mem, (const void *)NULL }) {
            xgpu_compare_ref r;
            r.kind = kind; r.pic = slot; r.d_yuv = ptr; r.size = size; r.dtype = dtype; r.row_pitch = pitch;
            const size_t rs = xgpu_compare_ref_size(&r, w, h);
            if (rs != rule_ref_size(r, w, h)) { printf("ref_size %dx%d kind %d dtype %d pitch %zu: %zu, expected %zu\n", w, h, kind, dtype, pitch, rs, rule_ref_size(r, w, h)); return 1; }
            for (int bd : depths) {
                const int rc = xgpu_compare_check(&r, &p, w, h, bd);
                calls += 2;
                if (rc != rule_check(r, p, w, h, bd)) {
                    printf("check %dx%d depth %d kind %d slot %d dtype %d pitch %zu size %zu ptr %p crop %d %d %d %d ssim %d map %d: %d, expected %d\n", w, h, bd, kind, slot, dtype, pitch,
                           size, ptr, cr[0], cr[1], cr[2], cr[3], ssim, bm, rc, rule_check(r, p, w, h, bd));
                    return 1;
                }
            }
        }
    }
    printf("%ld calls agree\n", calls);
    return 0;
}
