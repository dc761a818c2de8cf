// xgpu_api.hip - the C ABI of include/xevd_hip.h, part 1: context, device pictures, output, frame begin / end, HIP-event kernel timing.
// Host-side code only; kernels live in k_*.hip, the batch builder in xgpu_builder.hip, the launch sequencing in xgpu_launch.hip, the test shims in xgpu_shims.hip.
#include "xgpu_host.h"
#include "scale_taps.h"
#include <memory>

// xevd_tbl_qp_chroma_adjust_base (src_base/xevd_tbl.c:345-354): default Baseline chroma QP mapping.
// ... and xevd_tbl_qp_chroma_adjust_main (xevd_tbl.c:334-342): the default when sps->tool_iqt is on (xevdm.c:471-479)
static const int8_t k_chroma_qp_main[58] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
    29, 30, 31, 32, 33, 34, 35, 36, 37, 37, 38, 39, 40, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54 };
static const int8_t k_chroma_qp_base[58] = {
     0,  1,  2,  3,  4,  5,  6,  7,  8,  9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19,
    20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 29, 30, 31, 32, 32, 33, 33, 34, 34,
    35, 35, 36, 36, 36, 37, 37, 37, 38, 38, 39, 39, 40, 40, 40, 41, 41, 41 };


const char *xgpu_version(void) { return "xevd_amd 0.1 (gfx950)"; }
const char *xgpu_last_error(const xgpu_ctx *c) { return c ? c->err : "null ctx"; }

// ------------------------------------------------------------------------------------------------ timing
void time_begin(xgpu_ctx *c, int k, hipEvent_t *a, hipEvent_t *b)
{
    if (!c->timing) return;
    auto get = [&]() {
        hipEvent_t e;
        if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    };
    *a = get(); *b = get();
    (void)hipEventRecord(*a, c->stream);
    (void)k;
}
void time_end(xgpu_ctx *c, int k, hipEvent_t a, hipEvent_t b)
{
    if (!c->timing) return;
    (void)hipEventRecord(b, c->stream);
    c->ev_pending.push_back({ a, b, k });
}
int xgpu_timing_enable(xgpu_ctx *c, int on) { ARGCHK(c, c != NULL); c->timing = on; return XGPU_OK; }
int xgpu_timing_reset(xgpu_ctx *c)
{
    ARGCHK(c, c != NULL);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &e : c->ev_pending) { c->ev_pool.push_back(e.a); c->ev_pool.push_back(e.b); }
    c->ev_pending.clear();
    memset(c->t_ms, 0, sizeof(c->t_ms));
    memset(c->t_n, 0, sizeof(c->t_n));
    return XGPU_OK;
}
int xgpu_timing_get(xgpu_ctx *c, double ms[XGPU_K_COUNT], long long n[XGPU_K_COUNT])
{
    ARGCHK(c, c != NULL);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &e : c->ev_pending) {
        float t = 0;
        HIPCHK(c, hipEventElapsedTime(&t, e.a, e.b));
        c->t_ms[e.k] += t; c->t_n[e.k]++;
        c->ev_pool.push_back(e.a); c->ev_pool.push_back(e.b);
    }
    c->ev_pending.clear();
    for (int i = 0; i < XGPU_K_COUNT; i++) { ms[i] = c->t_ms[i]; n[i] = c->t_n[i]; }
    return XGPU_OK;
}

// ------------------------------------------------------------------------------------------------ lifetime
static void init_transform_tables(xgpu_ctx *c)
{
    // xevd_tbl_tm2..64 (src_base/xevd_tbl.c:89-243) = round(64*sqrt(2)*cos((2n+1)k*pi/2N)), row 0 = 64; checked
    // entry by entry against the reference's tables in tests/test_oracle_vs_ref.py (same closed form as the oracle)
    static int tm[5460];
    int o = 0;
    for (int l = 1; l <= 6; l++) {
        const int N = 1 << l;
        for (int k = 0; k < N; k++)
            for (int n = 0; n < N; n++) {
                const double v = k == 0 ? 64.0 : 64.0 * sqrt(2.0) * cos((2 * n + 1) * k * 3.14159265358979323846 / (2.0 * N));
                tm[o++] = (int)(v >= 0 ? floor(v + 0.5) : -floor(-v + 0.5));
            }
    }
    // ATS matrices exactly as xevdm_init_multi_tbl builds them in double precision (src_main/xevdm_itdq.c:81-119); the
    // 4-point kernels of the reference are factorised around three entries of the first row (:163-190, :284-312) -
    // the equivalent 4x4 matrices are stored instead.  Order: [DST7, DCT8][4, 8, 16, 32], M[k][n].
    static int16_t ats[2 * 1360];
    for (int t = 0; t < 2; t++) {
        int q = t * 1360;
        for (int l = 2; l <= 5; l++) {
            const int N = 1 << l;
            const double sc = sqrt((double)N) * 64;
            int16_t m[32 * 32];
            for (int k = 0; k < N; k++)
                for (int n = 0; n < N; n++) {
                    const double v = t == 0 ? sin(3.14159265358979323846 * (k + 0.5) * (n + 1) / (N + 0.5)) * sqrt(2.0 / (N + 0.5))
                                            : cos(3.14159265358979323846 * (k + 0.5) * (n + 0.5) / (N + 0.5)) * sqrt(2.0 / (N + 0.5));
                    m[k * N + n] = (int16_t)(sc * v + (v > 0 ? 0.5 : -0.5));
                }
            if (N == 4) {
                const int a = m[0], b = m[1], cc = m[2], d = m[3];
                const int e7[16] = { a, b, cc, b + a,  cc, cc, 0, -cc,  a + b, -a, -cc, b,  b, -(b + a), cc, -a };
                const int e8[16] = { d + cc, b, cc, d,  b, 0, -b, -b,  cc, -b, -d, d + cc,  d, -b, d + cc, -cc };
                for (int i = 0; i < 16; i++) m[i] = (int16_t)(t == 0 ? e7[i] : e8[i]);
            }
            for (int i = 0; i < N * N; i++) ats[q++] = m[i];
        }
    }
    upload_transform_tables(tm, ats, c->stream);
}

int xgpu_open(const xgpu_seq_params *sp, xgpu_ctx **out)
{
    if (!sp || !out) return XGPU_ERR_INVALID_ARGUMENT;
    *out = NULL;
    if (sp->chroma_format_idc != 1) return XGPU_ERR_UNSUPPORTED;
    if (sp->width <= 0 || sp->height <= 0 || (sp->width & 7) || (sp->height & 7)) return XGPU_ERR_INVALID_ARGUMENT;
    if (sp->bit_depth_luma < 8 || sp->bit_depth_luma > 12 || sp->bit_depth_chroma < 8 || sp->bit_depth_chroma > 12) return XGPU_ERR_UNSUPPORTED;
    if (sp->log2_ctu < 5 || sp->log2_ctu > 7) return XGPU_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || sp->device < 0 || sp->device >= ndev) return XGPU_ERR_UNEXPECTED;

    xgpu_ctx *c = new xgpu_ctx();
    c->sp = *sp;
    c->sp.chroma_qp_table[0] = c->sp.chroma_qp_table[1] = NULL;
    c->builder_threads = 1;
    c->err[0] = 0; c->timing = 0; c->have_frame = 0; c->side_pic = -1; c->d_maps = NULL; c->d_dra = NULL; c->d_cm = NULL; c->cm_tab = NULL; c->d_ctb_flag = NULL; c->stream = 0; c->up_stream = 0; c->down_stream = 0; c->side_stream = 0; c->after_inter = 0; c->have_after_inter = 0; c->where = 0; c->addb_pending = 0;
    c->fork_ev = c->join_ev = 0;
    c->intra_small_min = getenv("XEVD_HIP_INTRA_SMALL_MIN") ? std::max(1, atoi(getenv("XEVD_HIP_INTRA_SMALL_MIN"))) : 2048;      // (k_intra.hip: launch_intra; read per context, tests set 1)
    c->addb_scalar = getenv("XEVD_HIP_ADDB_SCALAR") != NULL;
    c->split_addb_alf = getenv("XEVD_HIP_SPLIT_ADDB_ALF") != NULL;      // measurement knob: ADDB and ALF as two kernels (the round-2 chain) instead of k_addb_alf
    for (int i = 0; i < 2; i++) { c->d_out[i] = NULL; c->out_caps[i] = 0; c->out_ready[i] = c->out_done[i] = 0; c->out_busy[i] = 0; }
    c->d_md5 = NULL; c->md5_ready = 0;
    c->odev_ev[0] = c->odev_ev[1] = 0;
    c->sc_tab = NULL; c->sc_tab_cap = 0; c->sc_mid = NULL; c->sc_mid_cap = 0;
    c->roi_blk = NULL; c->roi_blk_cap = 0;
    for (int i = 0; i < 6; i++) c->sc_key[i] = -1;
    c->out_next = 0;
    memset(c->t_ms, 0, sizeof(c->t_ms)); memset(c->t_n, 0, sizeof(c->t_n));
    // chroma QP mapping: caller table starts at qp = -6*(bdc-8); default = Baseline static table with the
    // identity extension below 0 (xevd_set_chroma_qp_tbl_loc, xevd_tbl.c:364-372)
    const int boff = 6 * (sp->bit_depth_chroma - 8);
    for (int t = 0; t < 2; t++)
        for (int q = -boff; q <= 57; q++)
            c->chroma_qp[t][q + boff] = sp->chroma_qp_table[t] ? sp->chroma_qp_table[t][q + boff] : (int8_t)(q < 0 ? q : (sp->tool_iqt ? k_chroma_qp_main[q] : k_chroma_qp_base[q]));

    auto fail = [&](int code) { xgpu_close(c); return code; };
    if (hipSetDevice(sp->device) != hipSuccess) return fail(XGPU_ERR_UNEXPECTED);
    // Host waits (hipEventSynchronize / hipStreamSynchronize) spin by default: a decoder thread that waits for a picture's download burns a whole CPU doing so, and on
    // a host with a CPU quota (the GPU boxes of this pool: cgroup cpu.max = 16 CPUs under 256 hardware threads) the spinning of several workers throttles the
    // parser threads next to them.  XEVD_HIP_BLOCKING_SYNC=1: the runtime sleeps on an interrupt instead (a few microseconds more latency per wait).
    static const bool blocking = getenv("XEVD_HIP_BLOCKING_SYNC") != NULL && atoi(getenv("XEVD_HIP_BLOCKING_SYNC")) != 0;
    if (blocking) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
    const unsigned ev_flags = hipEventDisableTiming | (blocking ? hipEventBlockingSync : 0);
    {
        // The runtime hands its hardware queues (four by default, GPU_MAX_HW_QUEUES) to the streams of a process in the order they are created.  Every context creates
        // four streams, so created in one fixed order the KERNEL streams of all contexts of a process shared one hardware queue, and the pictures of independent decoders ran
        // strictly one after the other (two contexts in one process: 2814 pictures/s at 8K against 2841 for one; 3087 - 3118 with the queues apart, 4K 7865 -> 11 300).  Every
        // other context creates its kernel stream LAST instead of first: the kernel streams alternate between the first and the fourth queue, the upload and download streams
        // of all contexts stay on the second and third - a picture's output copy never queues behind another decoder's kernels (rotating all four positions cost the host-bound
        // many-stream decode 4 %; stream priority classes changed nothing) -, and the rarely used side stream shares with the other parity's kernels.
        // XEVD_HIP_NO_QUEUE_ROTATION=1: the fixed order (A/B measurements).
        static std::atomic<int> n_ctx(0);
        static const bool no_rot = getenv("XEVD_HIP_NO_QUEUE_ROTATION") != NULL;
        const bool swap = !no_rot && (n_ctx.fetch_add(1) & 1);
        hipStream_t *const order[4] = { swap ? &c->side_stream : &c->stream, &c->up_stream, &c->down_stream, swap ? &c->stream : &c->side_stream };
        for (int i = 0; i < 4; i++)
            if (hipStreamCreateWithFlags(order[i], hipStreamNonBlocking) != hipSuccess) return fail(XGPU_ERR_UNEXPECTED);
    }
    if (hipEventCreateWithFlags(&c->after_inter, hipEventDisableTiming) != hipSuccess) return fail(XGPU_ERR_UNEXPECTED);
    if (hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming) != hipSuccess) return fail(XGPU_ERR_UNEXPECTED);
    for (int i = 0; i < 2; i++)
        if (hipEventCreateWithFlags(&c->out_ready[i], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->out_done[i], ev_flags) != hipSuccess)
            return fail(XGPU_ERR_UNEXPECTED);

    c->w_scu = sp->width >> 2; c->h_scu = sp->height >> 2;
    const int ctu = 1 << sp->log2_ctu;
    c->w_ctu = (sp->width + ctu - 1) / ctu; c->h_ctu = (sp->height + ctu - 1) / ctu;
    c->s_l = align_up(XGPU_MARGIN_L + sp->width + XGPU_PAD_L, 64);
    c->s_c = align_up(XGPU_MARGIN_C + (sp->width >> 1) + XGPU_PAD_C, 64);
    c->rows_l = sp->height + 2 * XGPU_PAD_L;
    c->rows_c = (sp->height >> 1) + 2 * XGPU_PAD_C;
    c->off_u = (size_t)c->s_l * c->rows_l;
    c->off_v = c->off_u + (size_t)c->s_c * c->rows_c;
    c->pic_elems = c->off_v + (size_t)c->s_c * c->rows_c + 64;   // +64: slack for the 16-byte window over-read of the last row

    if (hipMalloc((void **)&c->d_maps, sizeof(ScuRec) * (size_t)c->w_scu * c->h_scu) != hipSuccess) return fail(XGPU_ERR_OUT_OF_MEMORY);
    if (hipMemsetAsync(c->d_maps, 0, sizeof(ScuRec) * (size_t)c->w_scu * c->h_scu, c->stream) != hipSuccess) return fail(XGPU_ERR_UNEXPECTED);
    if (hipMalloc((void **)&c->d_ctb_flag, (size_t)c->w_ctu * c->h_ctu + 16) != hipSuccess) return fail(XGPU_ERR_OUT_OF_MEMORY);
    init_transform_tables(c);
    // slot 0 of `pics` is the private scratch picture of the deblocking passes
    c->pics.resize(1 + std::max(1, std::min(sp->max_pics, 34)));
    for (auto &p : c->pics) { p.base = NULL; p.used = 0; }
    {
        DevPic &p = c->pics[0];
        if (hipMalloc((void **)&p.base, c->pic_elems * sizeof(int16_t)) != hipSuccess) return fail(XGPU_ERR_OUT_OF_MEMORY);
        (void)hipMemsetAsync(p.base, 0, c->pic_elems * sizeof(int16_t), c->stream);
        p.s_l = c->s_l; p.s_c = c->s_c; p.used = 1;
        p.y = p.base + (size_t)XGPU_PAD_L * c->s_l + XGPU_MARGIN_L;
        p.u = p.base + c->off_u + (size_t)XGPU_PAD_C * c->s_c + XGPU_MARGIN_C;
        p.v = p.base + c->off_v + (size_t)XGPU_PAD_C * c->s_c + XGPU_MARGIN_C;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(XGPU_ERR_UNEXPECTED);
    *out = c;
    return XGPU_OK;
}

void xgpu_close(xgpu_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->sp.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
    if (c->down_stream) (void)hipStreamSynchronize(c->down_stream);
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
    for (auto &p : c->pics) if (p.base) (void)hipFree(p.base);
    if (c->d_maps) (void)hipFree(c->d_maps);
    for (BatchBlock &k : c->pool) { (void)hipFree(k.d_base); (void)hipHostFree(k.h_stage); (void)hipEventDestroy(k.uploaded); (void)hipEventDestroy(k.done); (void)hipEventDestroy(k.itdq_done); if (k.d_chroma) (void)hipFree(k.d_chroma); }
    for (auto &h : c->pinned) (void)hipHostFree(h.p);
    c->pinned.clear();
    c->pool.clear();
    if (c->d_md5) (void)hipFree(c->d_md5);
    if (c->md5_ready) (void)hipEventDestroy(c->md5_ready);
    for (int i = 0; i < 2; i++) if (c->odev_ev[i]) (void)hipEventDestroy(c->odev_ev[i]);
    for (int i = 0; i < 2; i++) { if (c->d_out[i]) (void)hipFree(c->d_out[i]); if (c->out_ready[i]) (void)hipEventDestroy(c->out_ready[i]); if (c->out_done[i]) (void)hipEventDestroy(c->out_done[i]); }
    if (c->d_dra) (void)hipFree(c->d_dra);
    if (c->d_cm) (void)hipFree(c->d_cm);
    delete c->cm_tab;
    if (c->sc_tab) (void)hipFree(c->sc_tab);
    if (c->sc_mid) (void)hipFree(c->sc_mid);
    if (c->roi_blk) (void)hipFree(c->roi_blk);
    if (c->d_ctb_flag) (void)hipFree(c->d_ctb_flag);
    for (auto &e : c->ev_pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto &e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
    if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    if (c->after_inter) (void)hipEventDestroy(c->after_inter);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->join_ev) (void)hipEventDestroy(c->join_ev);
    delete c;
}

int xgpu_sync(xgpu_ctx *c)
{
    ARGCHK(c, c != NULL);
    HIPCHK(c, hipStreamSynchronize(c->up_stream));
    HIPCHK(c, hipStreamSynchronize(c->side_stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->down_stream));
    return XGPU_OK;
}

// pinned host memory for the arrays a batch points at: xgpu_batch_create sends a coefficient arena inside such a range straight from the caller's buffer
int xgpu_host_alloc(xgpu_ctx *c, size_t bytes, void **out)
{
    ARGCHK(c, c != NULL); ARGCHK(c, out != NULL && bytes > 0);
    *out = NULL;
    HIPCHK(c, hipSetDevice(c->sp.device));
    void *p = NULL;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { snprintf(c->err, sizeof(c->err), "host_alloc: cannot pin %zu bytes", bytes); return XGPU_ERR_OUT_OF_MEMORY; }
    std::lock_guard<std::mutex> g(c->pool_mu);
    c->pinned.push_back({ (uint8_t *)p, bytes });
    *out = p;
    return XGPU_OK;
}
void xgpu_host_free(xgpu_ctx *c, void *p)
{
    if (!c || !p) return;
    std::lock_guard<std::mutex> g(c->pool_mu);
    for (size_t i = 0; i < c->pinned.size(); i++)
        if (c->pinned[i].p == (uint8_t *)p) { (void)hipHostFree(p); c->pinned.erase(c->pinned.begin() + (long)i); return; }
}

// ------------------------------------------------------------------------------------------------ pictures

int xgpu_pic_alloc(xgpu_ctx *c)
{
    ARGCHK(c, c != NULL);
    HIPCHK(c, hipSetDevice(c->sp.device));
    for (size_t i = 1; i < c->pics.size(); i++) {
        DevPic &p = c->pics[i];
        if (p.used) continue;
        if (!p.base) {
            if (hipMalloc((void **)&p.base, c->pic_elems * sizeof(int16_t)) != hipSuccess) {
                snprintf(c->err, sizeof(c->err), "hipMalloc of a %zu-byte picture failed", c->pic_elems * sizeof(int16_t));
                return XGPU_ERR_OUT_OF_MEMORY;
            }
            HIPCHK(c, hipMemsetAsync(p.base, 0, c->pic_elems * sizeof(int16_t), c->stream));
        }
        p.s_l = c->s_l; p.s_c = c->s_c;
        p.y = p.base + (size_t)XGPU_PAD_L * c->s_l + XGPU_MARGIN_L;
        p.u = p.base + c->off_u + (size_t)XGPU_PAD_C * c->s_c + XGPU_MARGIN_C;
        p.v = p.base + c->off_v + (size_t)XGPU_PAD_C * c->s_c + XGPU_MARGIN_C;
        p.used = 1;
        return (int)i - 1;
    }
    snprintf(c->err, sizeof(c->err), "no free picture slot (max_pics=%d)", c->sp.max_pics);
    return XGPU_ERR_OUT_OF_MEMORY;
}

int xgpu_pic_free(xgpu_ctx *c, int pic)
{
    ARGCHK(c, c != NULL);
    ARGCHK(c, valid_pic(c, pic));
    dpic(c, pic).used = 0;          // memory is kept for reuse (a DPB recycles its buffers, xevd_picman.c)
    return XGPU_OK;
}

static int copy_planes(xgpu_ctx *c, int pic, int16_t *y, int s_y, int16_t *u, int16_t *v, int s_c, int ext_l, int ext_c, bool up)
{
    // ext_*: how many samples of padding around the active area take part (0 = active area only)
    DevPic &p = dpic(c, pic);
    int16_t *host[3] = { y, u, v };
    int16_t *dev[3] = { p.y, p.u, p.v };
    for (int i = 0; i < 3; i++) {
        if (!host[i]) continue;                           // a plane the caller did not ask for (xgpu_pic_download_padded with luma only)
        const int e = i ? ext_c : ext_l, hs = i ? s_c : s_y, ds = i ? p.s_c : p.s_l;
        const int w = (i ? c->sp.width >> 1 : c->sp.width) + 2 * e, h = (i ? c->sp.height >> 1 : c->sp.height) + 2 * e;
        int16_t *d = dev[i] - (size_t)e * ds - e;
        if (up) HIPCHK(c, hipMemcpy2DAsync(d, ds * 2, host[i], hs * 2, w * 2, h, hipMemcpyHostToDevice, c->stream));
        else    HIPCHK(c, hipMemcpy2DAsync(host[i], hs * 2, d, ds * 2, w * 2, h, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return XGPU_OK;
}

int xgpu_pic_upload(xgpu_ctx *c, int pic, const int16_t *y, int s_y, const int16_t *u, const int16_t *v, int s_c)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, y && u && v && s_y >= c->sp.width && s_c >= c->sp.width / 2);
    return copy_planes(c, pic, (int16_t *)y, s_y, (int16_t *)u, (int16_t *)v, s_c, 0, 0, true);
}
int xgpu_pic_download(xgpu_ctx *c, int pic, int16_t *y, int s_y, int16_t *u, int16_t *v, int s_c)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, y && u && v && s_y >= c->sp.width && s_c >= c->sp.width / 2);
    return copy_planes(c, pic, y, s_y, u, v, s_c, 0, 0, false);
}
int xgpu_pic_download_padded(xgpu_ctx *c, int pic, int16_t *by, int16_t *bu, int16_t *bv)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, by && (bu != NULL) == (bv != NULL));
    return copy_planes(c, pic, by, c->sp.width + 2 * XGPU_PAD_L, bu, bv, (c->sp.width >> 1) + 2 * XGPU_PAD_C, XGPU_PAD_L, XGPU_PAD_C, false);
}
int xgpu_pic_upload_padded(xgpu_ctx *c, int pic, const int16_t *by, const int16_t *bu, const int16_t *bv)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, by && bu && bv);
    return copy_planes(c, pic, (int16_t *)by, c->sp.width + 2 * XGPU_PAD_L, (int16_t *)bu, (int16_t *)bv,
                       (c->sp.width >> 1) + 2 * XGPU_PAD_C, XGPU_PAD_L, XGPU_PAD_C, true);
}

static bool valid_output(const xgpu_ctx *c, int out_bd, int cl, int cr, int ct, int cb)
{
    return out_bd >= 8 && out_bd <= 16 && cl >= 0 && cr >= 0 && ct >= 0 && cb >= 0 && !((cl | cr | ct | cb) & 1) &&
           cl + cr < c->sp.width && ct + cb < c->sp.height;
}
size_t xgpu_pic_output_size(const xgpu_ctx *c, int out_bit_depth, int crop_l, int crop_r, int crop_t, int crop_b)
{
    if (!c || !valid_output(c, out_bit_depth, crop_l, crop_r, crop_t, crop_b)) return 0;
    const size_t w = c->sp.width - crop_l - crop_r, h = c->sp.height - crop_t - crop_b;
    return (w * h + 2 * (w >> 1) * (h >> 1)) * (out_bit_depth == 8 ? 1 : 2);
}
static int upload_dra(xgpu_ctx *c, const xgpu_dra_luts *dra)      // the inverse-mapping tables behind the picture's kernels on their stream
{
    ARGCHK(c, dra->luma_inv_scale_lut && dra->chroma_inv_scale_lut[0] && dra->chroma_inv_scale_lut[1]);
    ARGCHK(c, c->sp.bit_depth_luma <= 10);                         // the tables have 1024 entries (DRA_LUT_MAXSIZE)
    if (!c->d_dra && hipMalloc((void **)&c->d_dra, sizeof(int32_t) * 3 * 1024) != hipSuccess) { snprintf(c->err, sizeof(c->err), "pic_output: cannot allocate the DRA tables"); return XGPU_ERR_OUT_OF_MEMORY; }
    const int32_t *src[3] = { dra->luma_inv_scale_lut, dra->chroma_inv_scale_lut[0], dra->chroma_inv_scale_lut[1] };
    for (int i = 0; i < 3; i++) HIPCHK(c, hipMemcpyAsync(c->d_dra + 1024 * i, src[i], sizeof(int32_t) * 1024, hipMemcpyHostToDevice, c->stream));
    return XGPU_OK;
}
int xgpu_pic_output_async(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, int out_bit_depth, int crop_l, int crop_r, int crop_t, int crop_b, void *dst, size_t dst_size,
                          int *ticket)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, dst != NULL && ticket != NULL);
    ARGCHK(c, valid_output(c, out_bit_depth, crop_l, crop_r, crop_t, crop_b));
    const size_t need = xgpu_pic_output_size(c, out_bit_depth, crop_l, crop_r, crop_t, crop_b);
    ARGCHK(c, dst_size >= need);
    const int k = c->out_next;
    if (c->out_busy[k]) { HIPCHK(c, hipEventSynchronize(c->out_done[k])); c->out_busy[k] = 0; }      // two outputs in flight at most
    if (c->out_caps[k] < need) {
        if (c->d_out[k]) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->d_out[k]); c->d_out[k] = NULL; c->out_caps[k] = 0; }
        if (hipMalloc((void **)&c->d_out[k], need) != hipSuccess) { snprintf(c->err, sizeof(c->err), "pic_output: cannot allocate the %zu-byte staging buffer", need); return XGPU_ERR_OUT_OF_MEMORY; }
        c->out_caps[k] = need;
    }
    if (dra) { const int rc = upload_dra(c, dra); if (rc < 0) return rc; }
    // conversion + packing behind the picture's kernels on their stream; the copy to the host on the download stream behind an event, so it
    // overlaps the kernels of the next picture
    launch_output(c, dpic(c, pic), dra ? c->d_dra : NULL, out_bit_depth, crop_l, crop_r, crop_t, crop_b, c->d_out[k]);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->out_ready[k], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->down_stream, c->out_ready[k], 0));
    HIPCHK(c, hipMemcpyAsync(dst, c->d_out[k], need, hipMemcpyDeviceToHost, c->down_stream));
    HIPCHK(c, hipEventRecord(c->out_done[k], c->down_stream));
    c->out_busy[k] = 1;
    c->out_next = k ^ 1;
    *ticket = k;
    return XGPU_OK;
}
int xgpu_pic_output_wait(xgpu_ctx *c, int ticket)
{
    ARGCHK(c, c != NULL); ARGCHK(c, ticket == 0 || ticket == 1);
    if (c->out_busy[ticket]) { HIPCHK(c, hipEventSynchronize(c->out_done[ticket])); c->out_busy[ticket] = 0; }
    return XGPU_OK;
}
int xgpu_pic_output(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, int out_bit_depth, int crop_l, int crop_r, int crop_t, int crop_b, void *dst, size_t dst_size)
{
    int ticket = 0;
    const int rc = xgpu_pic_output_async(c, pic, dra, out_bit_depth, crop_l, crop_r, crop_t, crop_b, dst, dst_size, &ticket);
    return rc < 0 ? rc : xgpu_pic_output_wait(c, ticket);
}

// ------------------------------------------------------------------------------------------------ output into device memory
// Kr, Kb of the supported H.273 MatrixCoefficients code points; false for the others (0 identity, 2 unspecified, 10 constant luminance, ...)
static bool matrix_kr_kb(int m, double *kr, double *kb)
{
    switch (m) {
    case 1: *kr = 0.2126; *kb = 0.0722; return true;      // BT.709
    case 4: *kr = 0.30;   *kb = 0.11;   return true;      // FCC
    case 5: case 6: *kr = 0.299; *kb = 0.114; return true;      // BT.601 (625 / 525)
    case 7: *kr = 0.212;  *kb = 0.087;  return true;      // SMPTE 240M
    case 9: *kr = 0.2627; *kb = 0.0593; return true;      // BT.2020 non-constant luminance
    default: return false;
    }
}
static int elem_size(int dtype) { return dtype == XGPU_OUT_U8 ? 1 : dtype == XGPU_OUT_F32 ? 4 : 2; }
static bool is_rgb(int layout) { return layout == XGPU_OUT_RGB_PLANAR || layout == XGPU_OUT_RGB_INTERLEAVED; }
static bool is_yuv444(int layout) { return layout == XGPU_OUT_YUV444_PLANAR || layout == XGPU_OUT_YUV444_INTERLEAVED; }
static bool is_semiplanar(int layout) { return layout == XGPU_OUT_NV12 || layout == XGPU_OUT_P016; }
// the depth D the samples of YUV420P / NV12 / P016 are converted to
static int sample_depth(const xgpu_output_format *f, int bd) { return f->out_bit_depth ? f->out_bit_depth : bd; }
// the format alone (no picture size): 0 or a negative code, `why` says which field
static int check_format(const xgpu_output_format *f, int bd, const char **why)
{
    *why = "format is NULL";
    if (!f) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "crop offsets must be even and >= 0";
    for (int i = 0; i < 4; i++) if (f->crop[i] < 0 || (f->crop[i] & 1)) return XGPU_ERR_INVALID_ARGUMENT;
    if (f->layout == XGPU_OUT_YUV420P) {
        const int obd = sample_depth(f, bd);
        *why = "YUV420P: out_bit_depth 8..16 with dtype U8 at 8 bit, U16 above, tight rows";
        if (obd < 8 || obd > 16 || f->dtype != (obd == 8 ? XGPU_OUT_U8 : XGPU_OUT_U16) || f->row_pitch != 0) return XGPU_ERR_INVALID_ARGUMENT;
        return XGPU_OK;
    }
    if (is_semiplanar(f->layout)) {
        const int obd = sample_depth(f, bd);
        if (f->layout == XGPU_OUT_NV12) {
            *why = "NV12: dtype U8 with out_bit_depth 8, or U16 with out_bit_depth 9..16 (0 = a coding depth above 8)";
            if (f->dtype == XGPU_OUT_U8 ? f->out_bit_depth != 8 : (f->dtype != XGPU_OUT_U16 || obd < 9 || obd > 16)) return XGPU_ERR_INVALID_ARGUMENT;
        } else {
            *why = "P016: dtype U16 with out_bit_depth 8..16 (0 = the coding depth)";
            if (f->dtype != XGPU_OUT_U16 || obd < 8 || obd > 16) return XGPU_ERR_INVALID_ARGUMENT;
        }
        *why = "NV12 / P016: bgr must be 0, row_pitch a multiple of the element size";
        if (f->bgr || f->row_pitch % (size_t)elem_size(f->dtype)) return XGPU_ERR_INVALID_ARGUMENT;
        return XGPU_OK;
    }
    *why = "layout must be one of XGPU_OUT_YUV420P .. XGPU_OUT_YUV444_INTERLEAVED";
    if (!is_rgb(f->layout) && !is_yuv444(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "dtype must be one of XGPU_OUT_U8 .. XGPU_OUT_F32";
    if (f->dtype < XGPU_OUT_U8 || f->dtype > XGPU_OUT_F32) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "RGB / YUV444: out_bit_depth must be 0 or the coding depth";
    if (f->out_bit_depth != 0 && f->out_bit_depth != bd) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "bgr, full_range: 0 or 1 (bgr: RGB layouts only); chroma_loc 0..5; upsample XGPU_UPSAMPLE_NEAREST or _LINEAR; row_pitch a multiple of the element size";
    if ((f->bgr | f->full_range) & ~1 || (f->bgr && !is_rgb(f->layout)) || f->chroma_loc < 0 || f->chroma_loc > 5 ||
        (f->upsample != XGPU_UPSAMPLE_NEAREST && f->upsample != XGPU_UPSAMPLE_LINEAR) || f->row_pitch % (size_t)elem_size(f->dtype))
        return XGPU_ERR_INVALID_ARGUMENT;
    if (is_yuv444(f->layout)) return XGPU_OK;      // no matrix
    double kr, kb;
    *why = "matrix: supported MatrixCoefficients are 1, 4, 5, 6, 7 and 9";
    if (!matrix_kr_kb(f->matrix, &kr, &kb)) return XGPU_ERR_UNSUPPORTED;
    return XGPU_OK;
}
// luma offset and the luma / chroma excursions at coding depth bd
static void range_terms(int bd, int full_range, int *yo, double *yr, double *cr)
{
    *yo = full_range ? 0 : 16 << (bd - 8);
    *yr = full_range ? (double)((1 << bd) - 1) : (double)(219 << (bd - 8));
    *cr = full_range ? (double)((1 << bd) - 1) : (double)(224 << (bd - 8));
}
int xgpu_output_coeffs(const xgpu_output_format *f, int bit_depth, int32_t coef[5], int *shift, float fcoef[5])
{
    const char *why;
    if (bit_depth < 8 || bit_depth > 12 || !coef || !shift || !fcoef) return XGPU_ERR_INVALID_ARGUMENT;
    const int rc = check_format(f, bit_depth, &why);
    if (rc < 0) return rc;
    if (!is_rgb(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
    double kr, kb, yr, cr;
    int yo;
    matrix_kr_kb(f->matrix, &kr, &kb);
    const double kg = 1.0 - kr - kb;
    range_terms(bit_depth, f->full_range, &yo, &yr, &cr);
    // the same expressions, term for term, as tests/colour_ref.py (a different order of the double operations could round differently)
    auto terms = [&](double m, double sc, double t[5]) {
        t[0] = m / yr * sc;
        t[1] = 2.0 * (1.0 - kr) * m / cr * sc;
        t[2] = -(2.0 * kb * (1.0 - kb) / kg * m / cr * sc);
        t[3] = -(2.0 * kr * (1.0 - kr) / kg * m / cr * sc);
        t[4] = 2.0 * (1.0 - kb) * m / cr * sc;
    };
    double t[5];
    terms(1.0, 1.0, t);
    for (int i = 0; i < 5; i++) fcoef[i] = (float)t[i];
    if (f->dtype != XGPU_OUT_U8 && f->dtype != XGPU_OUT_U16) {
        for (int i = 0; i < 5; i++) coef[i] = 0;
        *shift = 0;
        return XGPU_OK;
    }
    const int d = f->dtype == XGPU_OUT_U8 ? 8 : bit_depth, sh = 27 - d;
    terms((double)((1 << d) - 1), (double)(1 << sh), t);
    for (int i = 0; i < 5; i++) coef[i] = (int32_t)round(t[i]);      // half away from zero; cgu and cgv are negated rounded magnitudes
    *shift = sh;
    return XGPU_OK;
}
static size_t format_size(const xgpu_output_format *f, int width, int height, int bd, const char **why)
{
    *why = "picture size or bit depth out of range";
    if (width <= 0 || height <= 0 || ((width | height) & 1) || bd < 8 || bd > 12) return 0;
    if (check_format(f, bd, why) < 0) return 0;
    *why = "crop leaves no picture";
    if (f->crop[0] + f->crop[1] >= width || f->crop[2] + f->crop[3] >= height) return 0;
    const size_t w = width - f->crop[0] - f->crop[1], h = height - f->crop[2] - f->crop[3], es = elem_size(f->dtype);
    if (f->layout == XGPU_OUT_YUV420P) return (w * h + 2 * (w >> 1) * (h >> 1)) * es;      // xgpu_pic_output_size
    const bool interleaved = f->layout == XGPU_OUT_RGB_INTERLEAVED || f->layout == XGPU_OUT_YUV444_INTERLEAVED;
    const size_t row = interleaved ? 3 * w * es : w * es;
    const size_t pitch = f->row_pitch ? f->row_pitch : row;
    *why = "row_pitch is shorter than a row";
    if (pitch < row) return 0;
    const size_t rows = is_semiplanar(f->layout) ? h + h / 2 : (interleaved ? h : 3 * h);
    return (rows - 1) * pitch + row;      // the last row need not be followed by a pitch's worth of bytes
}
size_t xgpu_output_format_size(const xgpu_output_format *f, int width, int height, int bit_depth)
{
    const char *why;
    return format_size(f, width, height, bit_depth, &why);
}
static size_t device_size(const xgpu_ctx *c, const xgpu_output_format *f, const char **why)
{
    return format_size(f, c->sp.width, c->sp.height, c->sp.bit_depth_luma, why);
}
size_t xgpu_pic_output_device_size(const xgpu_ctx *c, const xgpu_output_format *f)
{
    return c ? xgpu_output_format_size(f, c->sp.width, c->sp.height, c->sp.bit_depth_luma) : 0;
}
// the colour transform's tables on the device: the host copy is kept with the (cm, depth) it was made for, and made and uploaded again - on `s`, the stream the
// kernel runs on, which is behind every earlier reader of d_cm - only when they differ.  (cm_tab, cm_key, cm_bd) name what d_cm holds: they are set only once
// every copy of a new set has been queued, and cleared before the first one, so a call that returns early never leaves a key without its tables.
// The copies read pageable host memory (as upload_dra's do): hipMemcpyAsync stages such a source before it returns, so the host tables may be freed or replaced
// by the next call without waiting for the stream.
static const size_t CM_TONE_OFF = 4096, CM_ENC_OFF = 4096 + XGPU_CM_CURVE_SIZE, CM_FLOATS = 4096 + 2 * XGPU_CM_CURVE_SIZE;
static bool cm_cached(const xgpu_ctx *c, const xgpu_colour_transform *cm, int bd)
{
    const xgpu_colour_transform &k = c->cm_key;
    return c->cm_tab && c->cm_bd == bd && k.src_primaries == cm->src_primaries && k.src_transfer == cm->src_transfer && k.dst_primaries == cm->dst_primaries &&
           k.dst_transfer == cm->dst_transfer && k.tone_map == cm->tone_map && k.src_peak == cm->src_peak && k.dst_peak == cm->dst_peak && k.linear_scale == cm->linear_scale;
}
static int upload_cm(xgpu_ctx *c, const xgpu_colour_tables_t *t, hipStream_t s)
{
    HIPCHK(c, hipMemcpyAsync(c->d_cm, t->lin, sizeof(float) * t->n_lin, hipMemcpyHostToDevice, s));
    if (t->use_tone) HIPCHK(c, hipMemcpyAsync(c->d_cm + CM_TONE_OFF, t->tone, sizeof(t->tone), hipMemcpyHostToDevice, s));
    if (t->use_encode) HIPCHK(c, hipMemcpyAsync(c->d_cm + CM_ENC_OFF, t->encode, sizeof(t->encode), hipMemcpyHostToDevice, s));
    return XGPU_OK;
}
// the destination of an output into device memory must be device memory of this context's device, and the allocation must hold `need` bytes from d_dst on
static int check_device_dst(xgpu_ctx *c, const char *what, void *d_dst, size_t need)
{
    HIPCHK(c, hipSetDevice(c->sp.device));
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    const hipError_t pe = hipPointerGetAttributes(&at, d_dst);
    if (pe != hipSuccess) (void)hipGetLastError();      // an unknown (host) pointer: not an error of the runtime's state
    void *base = NULL;
    size_t range = 0;
    const bool dev = pe == hipSuccess && at.type == hipMemoryTypeDevice && at.device == c->sp.device;
    if (dev && hipMemGetAddressRange(&base, &range, d_dst) != hipSuccess) { (void)hipGetLastError(); base = NULL; }
    if (!dev || !base || (uint8_t *)d_dst + need > (uint8_t *)base + range) {
        snprintf(c->err, sizeof(c->err), "%s: %p is not %zu bytes of device memory on device %d", what, d_dst, need, c->sp.device);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    return XGPU_OK;
}
static int output_device(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream);
int xgpu_pic_output_device(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, void *d_dst, size_t dst_size, void *stream)
{
    return output_device(c, pic, dra, f, NULL, d_dst, dst_size, stream);
}
int xgpu_pic_output_device_cm(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream)
{
    return output_device(c, pic, dra, f, cm, d_dst, dst_size, stream);
}
static int output_device(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const char *why = "";
    const size_t need = device_size(c, f, &why);
    if (need == 0) {
        snprintf(c->err, sizeof(c->err), "pic_output_device: invalid format: %s", why);
        return f && is_rgb(f->layout) && check_format(f, c->sp.bit_depth_luma, &why) == XGPU_ERR_UNSUPPORTED ? XGPU_ERR_UNSUPPORTED : XGPU_ERR_INVALID_ARGUMENT;
    }
    const size_t es = f->layout == XGPU_OUT_YUV420P ? 1 : (size_t)elem_size(f->dtype);
    if (dst_size < need || ((uintptr_t)d_dst % es)) {
        snprintf(c->err, sizeof(c->err), "pic_output_device: destination of %zu bytes at %p, the format needs %zu bytes aligned to %zu", dst_size, d_dst, need, es);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    { const int rc = check_device_dst(c, "pic_output_device", d_dst, need); if (rc < 0) return rc; }
    std::unique_ptr<xgpu_colour_tables_t> cm_new;      // a new set of tables: made here, before anything is queued; uploaded and committed below
    if (cm) {
        const int bd = c->sp.bit_depth_luma;
        if (!is_rgb(f->layout)) { snprintf(c->err, sizeof(c->err), "pic_output_device_cm: a colour transform needs one of the RGB layouts"); return XGPU_ERR_INVALID_ARGUMENT; }
        if (!cm_cached(c, cm, bd)) {
            cm_new.reset(new (std::nothrow) xgpu_colour_tables_t);
            const int rc = cm_new ? xgpu_colour_tables(f, cm, bd, cm_new.get()) : XGPU_ERR_OUT_OF_MEMORY;
            if (rc < 0) {
                snprintf(c->err, sizeof(c->err), "pic_output_device_cm: transform %d/%d -> %d/%d (primaries / transfer) is not supported or its parameters are invalid",
                         cm->src_primaries, cm->src_transfer, cm->dst_primaries, cm->dst_transfer);
                return rc;
            }
            if (!c->d_cm && hipMalloc((void **)&c->d_cm, sizeof(float) * CM_FLOATS) != hipSuccess) { snprintf(c->err, sizeof(c->err), "pic_output_device_cm: cannot allocate the tables"); return XGPU_ERR_OUT_OF_MEMORY; }
        }
    }
    if (dra) { const int rc = upload_dra(c, dra); if (rc < 0) return rc; }
    hipStream_t s = c->stream;
    if (stream) {
        for (int i = 0; i < 2; i++)
            if (!c->odev_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->odev_ev[i], hipEventDisableTiming));
        s = (hipStream_t)stream;
        HIPCHK(c, hipEventRecord(c->odev_ev[0], c->stream));      // the picture's kernels (and the DRA tables) -> the caller's stream
        HIPCHK(c, hipStreamWaitEvent(s, c->odev_ev[0], 0));
    }
    if (cm_new) {      // behind the wait above: after every kernel that read the previous tables
        delete c->cm_tab;
        c->cm_tab = NULL;      // d_cm is about to change: no key names it until all of the new set is queued
        const int rc = upload_cm(c, cm_new.get(), s);
        if (rc < 0) return rc;
        c->cm_tab = cm_new.release(); c->cm_key = *cm; c->cm_bd = c->sp.bit_depth_luma;
    }
    const int *cr = f->crop;
    const DevPic &p = dpic(c, pic);
    const int bd = c->sp.bit_depth_luma;
    const int w = c->sp.width - cr[0] - cr[1], h = c->sp.height - cr[2] - cr[3];
    const int16_t *sy = p.y + (size_t)cr[2] * p.s_l + cr[0];      // first sample of the cropped area of every plane
    const int16_t *su = p.u + (size_t)(cr[2] >> 1) * p.s_c + (cr[0] >> 1), *sv = p.v + (size_t)(cr[2] >> 1) * p.s_c + (cr[0] >> 1);
    if (f->layout == XGPU_OUT_YUV420P) {
        launch_output(c, p, dra ? c->d_dra : NULL, sample_depth(f, bd), cr[0], cr[1], cr[2], cr[3], (uint8_t *)d_dst, false, s);
    } else if (is_semiplanar(f->layout)) {
        SemiPlanarArgs a;
        memset(&a, 0, sizeof(a));
        const int obd = sample_depth(f, bd);
        a.y = sy; a.u = su; a.v = sv;
        a.sy = p.s_l; a.sc = p.s_c;
        a.w = w; a.ch = h >> 1;
        a.dst = (uint8_t *)d_dst;
        a.pitch = f->row_pitch ? f->row_pitch : (size_t)w * es;
        a.chroma_off = a.pitch * h;
        a.aligned = (((uintptr_t)d_dst | a.pitch | a.chroma_off) & 15) == 0;
        a.shift = bd - obd; a.out8 = obd == 8; a.maxv = (1 << obd) - 1;      // launch_output's conversion
        a.lsh = f->layout == XGPU_OUT_P016 ? 16 - obd : 0;
        a.dra = dra ? c->d_dra : NULL;
        launch_output_semiplanar(a, f->dtype, s);
    } else {
        RgbOutArgs a;
        memset(&a, 0, sizeof(a));
        const bool planar = f->layout == XGPU_OUT_RGB_PLANAR || f->layout == XGPU_OUT_YUV444_PLANAR;
        a.y = sy; a.u = su; a.v = sv;
        a.sy = p.s_l; a.sc = p.s_c;
        a.w = w; a.h = h;
        a.cw = a.w >> 1; a.ch = a.h >> 1;
        a.dst = (uint8_t *)d_dst;
        a.pitch = f->row_pitch ? f->row_pitch : (size_t)a.w * es * (planar ? 1 : 3);
        a.plane = a.pitch * a.h;
        a.aligned = (((uintptr_t)d_dst | a.pitch | a.plane) & 15) == 0;
        a.bgr = f->bgr;
        double yr, crr;
        range_terms(bd, f->full_range, &a.yo, &yr, &crr);
        a.co = 1 << (bd - 1);
        // ChromaSampleLocType: horizontally co-sited (0, 2, 4) / centred (1, 3, 5); vertically centred (0, 1), top (2, 3), bottom (4, 5)
        static const int ve[3][2] = { { 1, 3 }, { 0, 4 }, { 2, 2 } }, vo[3][2] = { { 3, 1 }, { 2, 2 }, { 4, 0 } };
        a.hc = f->chroma_loc & 1;
        a.ve[0] = ve[f->chroma_loc >> 1][0]; a.ve[1] = ve[f->chroma_loc >> 1][1];
        a.vo[0] = vo[f->chroma_loc >> 1][0]; a.vo[1] = vo[f->chroma_loc >> 1][1];
        a.dra = dra ? c->d_dra : NULL;
        if (cm) {
            CmOutArgs ca;
            static_cast<RgbOutArgs &>(ca) = a;
            xgpu_output_format f16 = *f;
            f16.dtype = XGPU_OUT_U16;      // the code at the coding depth feeds the transform, whatever the output dtype
            f16.row_pitch = 0;             // (the caller's pitch counts the caller's elements, not 16-bit ones)
            (void)xgpu_output_coeffs(&f16, bd, ca.coef, &ca.shift, ca.fcoef);
            ca.maxv = (1 << bd) - 1;
            const xgpu_colour_tables_t &t = *c->cm_tab;
            ca.lin = c->d_cm; ca.tone = t.use_tone ? c->d_cm + CM_TONE_OFF : NULL; ca.enc = t.use_encode ? c->d_cm + CM_ENC_OFF : NULL;
            ca.n_lin = t.n_lin; ca.use_matrix = t.use_matrix;
            memcpy(ca.m, t.matrix, sizeof(ca.m)); memcpy(ca.luma, t.luma, sizeof(ca.luma));
            ca.scale = t.scale;
            ca.outmax = f->dtype == XGPU_OUT_U8 ? 255.f : (float)((1 << bd) - 1);
            launch_output_cm(ca, f->layout, f->dtype, f->upsample, s);
        } else if (is_rgb(f->layout)) {
            (void)xgpu_output_coeffs(f, bd, a.coef, &a.shift, a.fcoef);
            a.maxv = f->dtype == XGPU_OUT_U8 ? 255 : (1 << bd) - 1;
            launch_output_rgb(a, f->layout, f->dtype, f->upsample, s);
        } else {
            a.shift = bd - 8;
            a.fcoef[0] = (float)(1.0 / yr); a.fcoef[1] = (float)(1.0 / crr);      // rounded once from double
            launch_output_yuv444(a, f->layout, f->dtype, f->upsample, s);
        }
    }
    HIPCHK(c, hipGetLastError());
    if (stream) {
        HIPCHK(c, hipEventRecord(c->odev_ev[1], s));      // the context's stream does not touch the slot or the DRA tables before the kernel is done
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->odev_ev[1], 0));
    }
    return XGPU_OK;
}

// ------------------------------------------------------------------------------------------------ scaled output into device memory
// format and scale parameters for a picture of width x height at depth bd: the bytes the destination needs, or 0 with *rc = the code and `why`
// the part that does not look at the ratio of source and destination: what the batched output (section 8e) shares
static bool scaled_params_ok(const xgpu_output_format *f, const xgpu_scale_params *sc, int width, int height, int bd, int *rc, const char **why)
{
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    *why = "format or scale parameters are NULL";
    if (!f || !sc) return false;
    *why = "picture size or bit depth out of range";
    if (width <= 0 || height <= 0 || ((width | height) & 1) || bd < 8 || bd > 12) return false;
    *why = "scaled output: layout must be XGPU_OUT_RGB_PLANAR / _INTERLEAVED or XGPU_OUT_YUV444_PLANAR / _INTERLEAVED";
    if (!is_rgb(f->layout) && !is_yuv444(f->layout)) return false;
    const int frc = check_format(f, bd, why);
    if (frc < 0) { *rc = frc; return false; }
    *why = "crop leaves no picture";
    if (f->crop[0] + f->crop[1] >= width || f->crop[2] + f->crop[3] >= height) return false;
    *why = "filter must be XGPU_SCALE_BILINEAR or XGPU_SCALE_AREA, normalize 0 or 1";
    if ((sc->filter != XGPU_SCALE_BILINEAR && sc->filter != XGPU_SCALE_AREA) || (sc->normalize & ~1)) return false;
    if (sc->normalize) {
        *why = "normalize needs a float dtype and finite mean / inv_std";
        if (f->dtype == XGPU_OUT_U8 || f->dtype == XGPU_OUT_U16) return false;
        for (int k = 0; k < 3; k++) if (!std::isfinite(sc->mean[k]) || !std::isfinite(sc->inv_std[k])) return false;
    }
    *rc = XGPU_ERR_UNSUPPORTED;
    *why = "destination size: 2..16384 per axis, between 1/64 and 8 times the source's";
    if (sc->width < 2 || sc->width > 16384 || sc->height < 2 || sc->height > 16384) return false;
    *rc = XGPU_OK;
    return true;
}
// the bytes of one sc->width x sc->height image (the last row not padded), or 0
static size_t scaled_image_bytes(const xgpu_output_format *f, const xgpu_scale_params *sc, int *rc, const char **why)
{
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    const size_t w = sc->width, h = sc->height, es = elem_size(f->dtype);
    const bool interleaved = f->layout == XGPU_OUT_RGB_INTERLEAVED || f->layout == XGPU_OUT_YUV444_INTERLEAVED;
    const size_t row = interleaved ? 3 * w * es : w * es, pitch = f->row_pitch ? f->row_pitch : row;
    *why = "row_pitch is shorter than a row";
    if (pitch < row) return 0;
    *rc = XGPU_OK;
    return ((interleaved ? h : 3 * h) - 1) * pitch + row;
}
static size_t scaled_size(const xgpu_output_format *f, const xgpu_scale_params *sc, int width, int height, int bd, int *rc, const char **why)
{
    if (!scaled_params_ok(f, sc, width, height, bd, rc, why)) return 0;
    const int ws = width - f->crop[0] - f->crop[1], hs = height - f->crop[2] - f->crop[3];
    *rc = XGPU_ERR_UNSUPPORTED;
    *why = "destination size: 2..16384 per axis, between 1/64 and 8 times the source's";
    if (!scale_ratio_ok(ws, sc->width) || !scale_ratio_ok(hs, sc->height)) return 0;
    return scaled_image_bytes(f, sc, rc, why);
}
size_t xgpu_output_scaled_size(const xgpu_output_format *f, const xgpu_scale_params *sc, int width, int height, int bit_depth)
{
    int rc; const char *why;
    return scaled_size(f, sc, width, height, bit_depth, &rc, &why);
}
int xgpu_output_scaled_check(const xgpu_output_format *f, const xgpu_scale_params *sc, int width, int height, int bit_depth)
{
    int rc; const char *why;
    (void)scaled_size(f, sc, width, height, bit_depth, &rc, &why);
    return rc;
}
// what the scaled outputs (one image, section 8d; a batch of rectangles, section 8e) hand their kernels alike: the picture minus f->crop, the destination of one
// sc->width x sc->height image at d_dst, the conversion, the clip and the normalise
static void scaled_common_args(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, void *d_dst, ScaledOutArgs &a)
{
    const DevPic &p = dpic(c, pic);
    const int *cr = f->crop;
    const int bd = c->sp.bit_depth_luma;
    const size_t es = (size_t)elem_size(f->dtype);
    const bool planar = f->layout == XGPU_OUT_RGB_PLANAR || f->layout == XGPU_OUT_YUV444_PLANAR;
    a.y = p.y + (size_t)cr[2] * p.s_l + cr[0];
    a.u = p.u + (size_t)(cr[2] >> 1) * p.s_c + (cr[0] >> 1); a.v = p.v + (size_t)(cr[2] >> 1) * p.s_c + (cr[0] >> 1);
    a.sy = p.s_l; a.sc = p.s_c;
    a.dw = sc->width; a.dh = sc->height;
    a.dst = (uint8_t *)d_dst;
    a.pitch = f->row_pitch ? f->row_pitch : (size_t)sc->width * es * (planar ? 1 : 3);
    a.plane = a.pitch * sc->height;
    a.bgr = f->bgr;
    double yr, crr;
    range_terms(bd, f->full_range, &a.yo, &yr, &crr);
    a.co = 1 << (bd - 1);
    a.dra = dra ? c->d_dra : NULL;
    if (is_rgb(f->layout)) {
        (void)xgpu_output_coeffs(f, bd, a.coef, &a.shift, a.fcoef);
        a.maxv = f->dtype == XGPU_OUT_U8 ? 255 : (1 << bd) - 1;
    } else {
        a.shift = bd - 8;
        a.fcoef[0] = (float)(1.0 / yr); a.fcoef[1] = (float)(1.0 / crr);
    }
    a.smax = (1 << bd) - 1;
    a.normalize = sc->normalize;
    for (int k = 0; k < 3; k++) { a.mean[k] = sc->mean[k]; a.inv_std[k] = sc->inv_std[k]; }
}
int xgpu_pic_output_device_scaled(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, void *d_dst, size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const int bd = c->sp.bit_depth_luma;
    int src_rc; const char *why = "";
    const size_t need = scaled_size(f, sc, c->sp.width, c->sp.height, bd, &src_rc, &why);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "pic_output_device_scaled: %s", why); return src_rc; }
    const size_t es = (size_t)elem_size(f->dtype);
    if (dst_size < need || ((uintptr_t)d_dst % es)) {
        snprintf(c->err, sizeof(c->err), "pic_output_device_scaled: destination of %zu bytes at %p, the format needs %zu bytes aligned to %zu", dst_size, d_dst, need, es);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    if (dra) { ARGCHK(c, dra->luma_inv_scale_lut && dra->chroma_inv_scale_lut[0] && dra->chroma_inv_scale_lut[1]); ARGCHK(c, bd <= 10); }      // upload_dra's refusals, before anything is queued
    { const int rc = check_device_dst(c, "pic_output_device_scaled", d_dst, need); if (rc < 0) return rc; }
    const int *cr = f->crop;
    const int ws = c->sp.width - cr[0] - cr[1], hs = c->sp.height - cr[2] - cr[3], wd = sc->width, hd = sc->height;
    // the tap tables: made here, before anything is queued; uploaded and committed below (the protocol of the colour transform's tables)
    const int key[6] = { ws, hs, wd, hd, sc->filter, f->chroma_loc };
    const bool cached = c->sc_tab && !memcmp(key, c->sc_key, sizeof(key));
    std::vector<uint8_t> blob;
    ScaleTabs tb = c->sc_host;
    if (!cached) {
        const int rc = scale_build_tables(ws, hs, wd, hd, sc->filter, f->chroma_loc, blob, tb);
        if (rc < 0) { snprintf(c->err, sizeof(c->err), "pic_output_device_scaled: cannot make the tap tables for %dx%d -> %dx%d", ws, hs, wd, hd); return rc; }
    }
    // the context's two buffers, grown on demand.  hipFree waits for the device, so no kernel of an earlier call still reads what is freed; in steady state neither runs.
    const int mpy = (ws + 7) & ~7, mpc = ((ws >> 1) + 7) & ~7;
    const size_t mid_need = (size_t)hd * (mpy + 2 * mpc) * sizeof(uint16_t);
    if (c->sc_mid_cap < mid_need) {
        if (c->sc_mid) { (void)hipFree(c->sc_mid); c->sc_mid = NULL; c->sc_mid_cap = 0; }
        if (hipMalloc((void **)&c->sc_mid, mid_need) != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, sizeof(c->err), "pic_output_device_scaled: cannot allocate the %zu-byte intermediate", mid_need); return XGPU_ERR_OUT_OF_MEMORY; }
        c->sc_mid_cap = mid_need;
    }
    if (!cached && c->sc_tab_cap < blob.size()) {
        if (c->sc_tab) { (void)hipFree(c->sc_tab); c->sc_tab = NULL; c->sc_tab_cap = 0; c->sc_key[0] = -1; }
        if (hipMalloc((void **)&c->sc_tab, blob.size()) != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, sizeof(c->err), "pic_output_device_scaled: cannot allocate the tap tables"); return XGPU_ERR_OUT_OF_MEMORY; }
        c->sc_tab_cap = blob.size();
    }
    if (dra) { const int rc = upload_dra(c, dra); if (rc < 0) return rc; }
    hipStream_t s = c->stream;
    if (stream) {
        for (int i = 0; i < 2; i++)
            if (!c->odev_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->odev_ev[i], hipEventDisableTiming));
        s = (hipStream_t)stream;
        HIPCHK(c, hipEventRecord(c->odev_ev[0], c->stream));      // the picture's kernels, the DRA tables and every earlier output call (they all end in the context's stream) -> the caller's stream
        HIPCHK(c, hipStreamWaitEvent(s, c->odev_ev[0], 0));
    }
    if (!cached) {      // behind the wait above: after every kernel that read the previous tables
        c->sc_key[0] = -1;      // sc_tab is about to change: no key names it until the new block is queued
        HIPCHK(c, hipMemcpyAsync(c->sc_tab, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
        memcpy(c->sc_key, key, sizeof(key));
        c->sc_host = tb;
    }
    ScaledOutArgs a;
    memset(&a, 0, sizeof(a));
    scaled_common_args(c, pic, dra, f, sc, d_dst, a);
    a.w = ws; a.h = hs; a.cw = ws >> 1; a.ch = hs >> 1;
    ScaleTaps *taps[4] = { &a.yl, &a.yc, &a.xl, &a.xc };
    for (int t = 0; t < 4; t++) {
        taps[t]->first = (const int32_t *)(c->sc_tab + tb.off_first[t]); taps[t]->count = (const int32_t *)(c->sc_tab + tb.off_count[t]);
        taps[t]->w = (const int16_t *)(c->sc_tab + tb.off_w[t]); taps[t]->stride = tb.stride[t];
    }
    a.mid = c->sc_mid; a.mpy = mpy; a.mpc = mpc;
    a.capy = tb.capy; a.capc = tb.capc;
    launch_output_scaled(a, f->layout, f->dtype, s);
    HIPCHK(c, hipGetLastError());
    if (stream) {
        HIPCHK(c, hipEventRecord(c->odev_ev[1], s));      // the context's stream - and through it the next output call on any stream - does not touch the slot, the tables or the intermediate before the kernels are done
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->odev_ev[1], 0));
    }
    return XGPU_OK;
}

// ------------------------------------------------------------------------------------------------ regions of interest: a batch of scaled images
// (the letterbox rule itself is scale_taps.h's roi_inner: k_rois_prepare runs it on the device as well)
int xgpu_roi_inner(const xgpu_roi *r, const xgpu_scale_params *sc, int fit, int inner[4])
{
    if (!r || !sc || !inner || r->width < 1 || r->height < 1 || sc->width < 1 || sc->height < 1 || (fit != XGPU_FIT_STRETCH && fit != XGPU_FIT_LETTERBOX))
        return XGPU_ERR_INVALID_ARGUMENT;
    roi_inner(r->width, r->height, sc->width, sc->height, fit, inner);
    return XGPU_OK;
}
// the pad value (read_pad: the call reads it) and the batch stride of a call: the bytes between two images, or 0 with `why`
static size_t rois_pad_and_pitch(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, int bd, size_t image, bool read_pad, char *why)
{
    const bool is_int = f->dtype == XGPU_OUT_U8 || f->dtype == XGPU_OUT_U16;
    if (read_pad) {
        const float top = (float)((1 << (f->dtype == XGPU_OUT_U8 ? 8 : bd)) - 1);
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(rp->pad[k]) || (is_int && (rp->pad[k] < 0.f || rp->pad[k] > top || rp->pad[k] != std::floor(rp->pad[k])))) {
                snprintf(why, 160, "pad[%d]: a finite value, for the integer dtypes an integer in 0..%d", k, (int)top);
                return 0;
            }
    }
    const size_t es = (size_t)elem_size(f->dtype);
    const bool interleaved = f->layout == XGPU_OUT_RGB_INTERLEAVED || f->layout == XGPU_OUT_YUV444_INTERLEAVED;
    const size_t row = (interleaved ? 3 : 1) * (size_t)sc->width * es;
    const size_t tight = (size_t)(interleaved ? 1 : 3) * sc->height * (f->row_pitch ? f->row_pitch : row);
    if (rp->image_pitch && (rp->image_pitch % es || rp->image_pitch < image)) {
        snprintf(why, 160, "image_pitch %zu: 0, or a multiple of the %zu-byte element not below the %zu bytes of one image", rp->image_pitch, es, image);
        return 0;
    }
    return rp->image_pitch ? rp->image_pitch : tight;
}
// The whole of a call's argument checks, without a device: the bytes the destination needs, or 0 with *rc = the code, `why` (a buffer of 160 bytes) and *bad =
// the rectangle it names (-1: none).  image_pitch / mid_bytes (may be NULL): the bytes between two images, and the intermediate of the call - the sum over the
// rectangles of Hi * (align8(Ws) + 2 * align8(Ws / 2)) * 2.
static const size_t ROIS_MID_LIMIT = (size_t)512 << 20;
static size_t rois_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi *rois, int n, int width, int height, int bd,
                        int *rc, char *why, int *bad, size_t *image_pitch, size_t *mid_bytes)
{
    const char *w0 = "";
    *bad = -1;
    if (!scaled_params_ok(f, sc, width, height, bd, rc, &w0)) { snprintf(why, 160, "%s", w0); return 0; }
    const size_t image = scaled_image_bytes(f, sc, rc, &w0);
    if (image == 0) { snprintf(why, 160, "%s", w0); return 0; }
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    if (!rp || !rois) { snprintf(why, 160, "roi parameters or rectangles are NULL"); return 0; }
    if (n < 1 || n > XGPU_MAX_ROIS) { snprintf(why, 160, "n_rois %d outside 1..%d", n, XGPU_MAX_ROIS); return 0; }
    if (rp->fit != XGPU_FIT_STRETCH && rp->fit != XGPU_FIT_LETTERBOX) { snprintf(why, 160, "fit must be XGPU_FIT_STRETCH or XGPU_FIT_LETTERBOX"); return 0; }
    const size_t ip = rois_pad_and_pitch(f, sc, rp, bd, image, rp->fit == XGPU_FIT_LETTERBOX, why);
    if (ip == 0) return 0;
    const int ws_all = width - f->crop[0] - f->crop[1], hs_all = height - f->crop[2] - f->crop[3];
    size_t mid = 0;
    for (int i = 0; i < n; i++) {
        const xgpu_roi &r = rois[i];
        *bad = i;
        *rc = XGPU_ERR_INVALID_ARGUMENT;
        if ((r.x | r.y | r.width | r.height) & 1) { snprintf(why, 160, "roi %d: (%d, %d, %d, %d) is not even", i, r.x, r.y, r.width, r.height); return 0; }
        if (r.x < 0 || r.y < 0 || r.width < 2 || r.height < 2 || r.x > ws_all - r.width || r.y > hs_all - r.height) {
            snprintf(why, 160, "roi %d: (%d, %d, %d, %d) is not inside the %d x %d picture minus the crop", i, r.x, r.y, r.width, r.height, ws_all, hs_all);
            return 0;
        }
        int in[4];
        roi_inner(r.width, r.height, sc->width, sc->height, rp->fit, in);
        *rc = XGPU_ERR_UNSUPPORTED;
        if (!scale_ratio_ok(r.width, in[2]) || !scale_ratio_ok(r.height, in[3])) {
            snprintf(why, 160, "roi %d: %d x %d to %d x %d is outside 1/64 .. 8 times per axis", i, r.width, r.height, in[2], in[3]);
            return 0;
        }
        mid += (size_t)in[3] * (((r.width + 7) & ~7) + 2 * (((r.width >> 1) + 7) & ~7)) * sizeof(uint16_t);
        if (mid > ROIS_MID_LIMIT) { snprintf(why, 160, "roi %d: the intermediate of the call passes 512 MiB here", i); return 0; }
    }
    *bad = -1;
    *rc = XGPU_OK;
    if (image_pitch) *image_pitch = ip;
    if (mid_bytes) *mid_bytes = mid;
    return (size_t)(n - 1) * ip + image;
}
int xgpu_output_rois_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois, int width, int height,
                           int bit_depth, int *bad_index)
{
    int rc, bad; char why[160];
    (void)rois_size(f, sc, rp, rois, n_rois, width, height, bit_depth, &rc, why, &bad, NULL, NULL);
    if (bad_index) *bad_index = bad;
    return rc;
}
size_t xgpu_output_rois_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois, int width, int height,
                             int bit_depth)
{
    int rc, bad; char why[160];
    return rois_size(f, sc, rp, rois, n_rois, width, height, bit_depth, &rc, why, &bad, NULL, NULL);
}
int xgpu_pic_output_device_rois(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp,
                                const xgpu_roi *rois, int n, void *d_dst, size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const int bd = c->sp.bit_depth_luma;
    int src_rc, bad; char why[160];
    size_t image_pitch = 0, mid_need = 0;
    const size_t need = rois_size(f, sc, rp, rois, n, c->sp.width, c->sp.height, bd, &src_rc, why, &bad, &image_pitch, &mid_need);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "pic_output_device_rois: %s", why); return src_rc; }
    const size_t es = (size_t)elem_size(f->dtype);
    if (dst_size < need || ((uintptr_t)d_dst % es)) {
        snprintf(c->err, sizeof(c->err), "pic_output_device_rois: destination of %zu bytes at %p, the %d images need %zu bytes aligned to %zu", dst_size, d_dst, n, need, es);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    if (dra) { ARGCHK(c, dra->luma_inv_scale_lut && dra->chroma_inv_scale_lut[0] && dra->chroma_inv_scale_lut[1]); ARGCHK(c, bd <= 10); }      // upload_dra's refusals, before anything is queued
    { const int rc = check_device_dst(c, "pic_output_device_rois", d_dst, need); if (rc < 0) return rc; }
    // the descriptor block, made here, before anything is queued: n records, then one set of tap tables per distinct (source size, inner size)
    const int wd = sc->width, hd = sc->height;
    std::vector<uint8_t> blk((size_t)n * sizeof(RoiDesc)), blob;
    struct Set { int ws, hs, wi, hi; ScaleTabs tb; size_t base; };
    std::vector<Set> sets;
    int capy = 0, capc = 0, max_w = 0, max_ih = 0;
    size_t mid = 0;
    for (int i = 0; i < n; i++) {
        const xgpu_roi &r = rois[i];
        int in[4];
        roi_inner(r.width, r.height, wd, hd, rp->fit, in);
        size_t k = 0;
        while (k < sets.size() && !(sets[k].ws == r.width && sets[k].hs == r.height && sets[k].wi == in[2] && sets[k].hi == in[3])) k++;
        if (k == sets.size()) {
            Set st = { r.width, r.height, in[2], in[3], {}, (blk.size() + 15) & ~(size_t)15 };
            const int rc = scale_build_tables(r.width, r.height, in[2], in[3], sc->filter, f->chroma_loc, blob, st.tb, in[0]);
            if (rc < 0) { snprintf(c->err, sizeof(c->err), "pic_output_device_rois: roi %d: cannot make the tap tables for %dx%d -> %dx%d", i, r.width, r.height, in[2], in[3]); return rc; }
            if (st.base + blob.size() > 0xFFFFFFFFu) { snprintf(c->err, sizeof(c->err), "pic_output_device_rois: roi %d: the tap tables of the call pass 4 GiB here", i); return XGPU_ERR_UNSUPPORTED; }
            blk.resize(st.base + blob.size());
            memcpy(&blk[st.base], blob.data(), blob.size());
            sets.push_back(st);
        }
        const Set &st = sets[k];
        RoiDesc d;
        memset(&d, 0, sizeof(d));
        d.dst = (uint64_t)i * image_pitch;
        d.x = r.x; d.y = r.y; d.w = r.width; d.h = r.height;
        d.ix = in[0]; d.iy = in[1]; d.iw = in[2]; d.ih = in[3];
        d.mid = (uint32_t)(mid / sizeof(uint16_t));
        d.mpy = (r.width + 7) & ~7; d.mpc = ((r.width >> 1) + 7) & ~7;
        mid += (size_t)in[3] * (d.mpy + 2 * d.mpc) * sizeof(uint16_t);
        for (int t = 0; t < 4; t++) {
            d.first[t] = (uint32_t)(st.base + st.tb.off_first[t]); d.count[t] = (uint32_t)(st.base + st.tb.off_count[t]); d.wt[t] = (uint32_t)(st.base + st.tb.off_w[t]);
            d.stride[t] = st.tb.stride[t];
        }
        memcpy(&blk[(size_t)i * sizeof(RoiDesc)], &d, sizeof(d));
        capy = std::max(capy, st.tb.capy); capc = std::max(capc, st.tb.capc);
        max_w = std::max(max_w, r.width); max_ih = std::max(max_ih, in[3]);
    }
    // the context's two buffers, grown on demand.  hipFree waits for the device, so no kernel of an earlier call still reads what is freed; in steady state neither runs.
    if (c->sc_mid_cap < mid_need) {
        if (c->sc_mid) { (void)hipFree(c->sc_mid); c->sc_mid = NULL; c->sc_mid_cap = 0; }
        if (hipMalloc((void **)&c->sc_mid, mid_need) != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, sizeof(c->err), "pic_output_device_rois: cannot allocate the %zu-byte intermediate", mid_need); return XGPU_ERR_OUT_OF_MEMORY; }
        c->sc_mid_cap = mid_need;
    }
    if (c->roi_blk_cap < blk.size()) {
        if (c->roi_blk) { (void)hipFree(c->roi_blk); c->roi_blk = NULL; c->roi_blk_cap = 0; }
        const size_t cap = blk.size() + blk.size() / 2;      // some room: a batch of boxes changes its tables' size from call to call
        if (hipMalloc((void **)&c->roi_blk, cap) != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, sizeof(c->err), "pic_output_device_rois: cannot allocate the %zu-byte descriptor block", cap); return XGPU_ERR_OUT_OF_MEMORY; }
        c->roi_blk_cap = cap;
    }
    if (dra) { const int rc = upload_dra(c, dra); if (rc < 0) return rc; }
    hipStream_t s = c->stream;
    if (stream) {
        for (int i = 0; i < 2; i++)
            if (!c->odev_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->odev_ev[i], hipEventDisableTiming));
        s = (hipStream_t)stream;
        HIPCHK(c, hipEventRecord(c->odev_ev[0], c->stream));      // the picture's kernels, the DRA tables and every earlier output call (they all end in the context's stream) -> the caller's stream
        HIPCHK(c, hipStreamWaitEvent(s, c->odev_ev[0], 0));
    }
    // behind the wait above: after every kernel that read the previous block.  (Pageable host memory: staged before the call returns, as the DRA tables are.)
    HIPCHK(c, hipMemcpyAsync(c->roi_blk, blk.data(), blk.size(), hipMemcpyHostToDevice, s));
    RoisOutArgs a;
    memset(&a, 0, sizeof(a));
    scaled_common_args(c, pic, dra, f, sc, d_dst, a);
    a.mid = c->sc_mid;
    a.capy = capy; a.capc = capc;
    a.blk = c->roi_blk; a.n = n;
    for (int k = 0; k < 3; k++) a.padv[k] = rp->fit == XGPU_FIT_LETTERBOX ? rp->pad[k] : 0.f;
    launch_output_rois(a, f->layout, f->dtype, max_w, max_ih, s);
    HIPCHK(c, hipGetLastError());
    if (stream) {
        HIPCHK(c, hipEventRecord(c->odev_ev[1], s));      // the context's stream - and through it the next output call on any stream - does not touch the slot, the block or the intermediate before the kernels are done
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->odev_ev[1], 0));
    }
    return XGPU_OK;
}

// ------------------------------------------------------------------------------------------------ regions of interest from boxes in device memory
int xgpu_roi_snap(int box_format, const void *box, int pic_w, int pic_h, xgpu_roi *used)
{
    if ((box_format != XGPU_BOX_XYWH_I32 && box_format != XGPU_BOX_XYXY_F32) || !box || !used || pic_w < 2 || pic_h < 2 || ((pic_w | pic_h) & 1))
        return XGPU_ERR_INVALID_ARGUMENT;
    memset(used, 0, sizeof(*used));
    return roi_snap_box(box_format, box, pic_w, pic_h, used);
}
// What the host-box call derives from its rectangles, from the bounds alone: the slot of tap tables and of the intermediate every box gets, the block, and the
// span of the intermediate pass 2 stages per row.
//   tables    table t of a box has N <= Nmax rows (Nmax = sc->height for the vertical tables, sc->width for the horizontal ones) over n <= Mn plane samples
//             (Mh, Mh / 2, Mw, Mw / 2), each row kw = floor(2 max(1, n / N)) + 2 weights wide (scale_taps.h): N kw <= max(2 N, 2 n) + 2 N <= 2 Mn + 4 Nmax.
//   LDS span  64 neighbouring columns ob .. ol of a table of ratio r = n / N, window f = max(1, r): the first sample of ob lies above c(ob) - f, the last of ol
//             below c(ol) + f, and c(ol) - c(ob) <= 63 r, so they span less than 63 r + 2 f + 1 samples, 14 more with the start rounded down and the end rounded
//             up to 8: at most 65 r + 17 with r >= 1 (for r < 1, 63 r + 2 + 15 is below it too).  r is at most 64 / s by the ratio limit and at most Mn / 2
//             (N >= 2); stretched, N = sc->width exactly, so r <= Mn / sc->width.  And no span leaves the plane: at most align8(Mn).
//             k_rois_prepare measures every box against this and refuses (XGPU_ROI_TOO_LARGE) what would not fit.
struct RoisDevLayout { uint32_t off_first[4], off_count[4], off_w[4]; size_t slot, tab, blk, mid_slot; int capy, capc; };
static int rois_span_bound(int mn, int sub, int wd, bool stretch)
{
    const int64_t general = 65 * std::max<int64_t>(1, std::min<int64_t>(64 / sub, (mn + 1) / 2)) + 19;
    const int64_t stretched = (65 * (int64_t)mn + wd - 1) / wd + 19;
    const int64_t b = stretch ? std::min(general, stretched) : general;
    return (int)std::max<int64_t>(8, std::min<int64_t>((b + 7) & ~(int64_t)7, (mn + 7) & ~7));
}
static void rois_dev_layout(const xgpu_scale_params *sc, int fit, int mw, int mh, int capacity, RoisDevLayout &L)
{
    const int mn[4] = { mh, mh >> 1, mw, mw >> 1 }, nmax[4] = { sc->height, sc->height, sc->width, sc->width };
    size_t off = 0;
    auto reserve = [&](size_t bytes) { const size_t at = off; off = (off + bytes + 15) & ~(size_t)15; return (uint32_t)at; };
    for (int t = 0; t < 4; t++) {
        L.off_first[t] = reserve(sizeof(int32_t) * nmax[t]);
        L.off_count[t] = reserve(sizeof(int32_t) * nmax[t]);
        L.off_w[t] = reserve(sizeof(int16_t) * (2 * (size_t)mn[t] + 4 * (size_t)nmax[t]));
    }
    L.slot = off;
    L.tab = (size_t)capacity * sizeof(RoiDesc);
    L.blk = L.tab + (size_t)capacity * L.slot;
    L.mid_slot = (size_t)sc->height * (((mw + 7) & ~7) + 2 * (((mw >> 1) + 7) & ~7));      // samples
    L.capy = rois_span_bound(mw, 1, sc->width, fit == XGPU_FIT_STRETCH);
    L.capc = rois_span_bound(mw >> 1, 2, sc->width, fit == XGPU_FIT_STRETCH);
}
// the call's argument checks, without a device: the bytes the destination needs, or 0 with *rc and `why`; the bounds resolved (0: the picture minus the crop)
static size_t rois_dev_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi_bounds *bounds, int box_format,
                            int capacity, int width, int height, int bd, int *rc, char *why, size_t *image_pitch, int *mw, int *mh)
{
    const char *w0 = "";
    if (!scaled_params_ok(f, sc, width, height, bd, rc, &w0)) { snprintf(why, 160, "%s", w0); return 0; }
    const size_t image = scaled_image_bytes(f, sc, rc, &w0);
    if (image == 0) { snprintf(why, 160, "%s", w0); return 0; }
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    if (!rp || !bounds) { snprintf(why, 160, "roi parameters or bounds are NULL"); return 0; }
    if (capacity < 1 || capacity > XGPU_MAX_ROIS) { snprintf(why, 160, "capacity %d outside 1..%d", capacity, XGPU_MAX_ROIS); return 0; }
    if (rp->fit != XGPU_FIT_STRETCH && rp->fit != XGPU_FIT_LETTERBOX) { snprintf(why, 160, "fit must be XGPU_FIT_STRETCH or XGPU_FIT_LETTERBOX"); return 0; }
    if (box_format != XGPU_BOX_XYWH_I32 && box_format != XGPU_BOX_XYXY_F32) { snprintf(why, 160, "box_format must be XGPU_BOX_XYWH_I32 or XGPU_BOX_XYXY_F32"); return 0; }
    const size_t ip = rois_pad_and_pitch(f, sc, rp, bd, image, true, why);      // a refused box is all pad, whatever the fit
    if (ip == 0) return 0;
    const int pw = width - f->crop[0] - f->crop[1], ph = height - f->crop[2] - f->crop[3];
    if (bounds->max_width < 0 || bounds->max_height < 0 || bounds->max_width > pw || bounds->max_height > ph) {
        snprintf(why, 160, "bounds %d x %d: 0 or at most the %d x %d picture minus the crop", bounds->max_width, bounds->max_height, pw, ph);
        return 0;
    }
    *mw = bounds->max_width ? bounds->max_width : pw; *mh = bounds->max_height ? bounds->max_height : ph;
    RoisDevLayout L;
    rois_dev_layout(sc, rp->fit, *mw, *mh, capacity, L);
    *rc = XGPU_ERR_UNSUPPORTED;
    if ((size_t)capacity * L.mid_slot * sizeof(uint16_t) > ROIS_MID_LIMIT) {
        snprintf(why, 160, "%d boxes of up to %d columns to %d rows: the intermediate of the call passes 512 MiB", capacity, *mw, sc->height);
        return 0;
    }
    if (L.blk > 0xFFFFFFFFu) { snprintf(why, 160, "the tap tables of %d boxes of up to %d x %d pass 4 GiB", capacity, *mw, *mh); return 0; }
    *rc = XGPU_OK;
    if (image_pitch) *image_pitch = ip;
    return (size_t)(capacity - 1) * ip + image;
}
int xgpu_output_rois_dev_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi_bounds *bounds, int box_format,
                               int capacity, int width, int height, int bit_depth)
{
    int rc, mw, mh; char why[160];
    (void)rois_dev_size(f, sc, rp, bounds, box_format, capacity, width, height, bit_depth, &rc, why, NULL, &mw, &mh);
    return rc;
}
size_t xgpu_output_rois_dev_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi_bounds *bounds, int box_format,
                                 int capacity, int width, int height, int bit_depth)
{
    int rc, mw, mh; char why[160];
    return rois_dev_size(f, sc, rp, bounds, box_format, capacity, width, height, bit_depth, &rc, why, NULL, &mw, &mh);
}
int xgpu_pic_output_device_rois_dev(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp,
                                    const xgpu_roi_bounds *bounds, int box_format, const void *d_boxes, int capacity, const int *d_count, xgpu_roi_result *d_results,
                                    void *d_dst, size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL); ARGCHK(c, d_boxes != NULL);
    const int bd = c->sp.bit_depth_luma;
    int src_rc, mw = 0, mh = 0; char why[160];
    size_t image_pitch = 0;
    const size_t need = rois_dev_size(f, sc, rp, bounds, box_format, capacity, c->sp.width, c->sp.height, bd, &src_rc, why, &image_pitch, &mw, &mh);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "pic_output_device_rois_dev: %s", why); return src_rc; }
    const size_t es = (size_t)elem_size(f->dtype);
    if (dst_size < need || ((uintptr_t)d_dst % es)) {
        snprintf(c->err, sizeof(c->err), "pic_output_device_rois_dev: destination of %zu bytes at %p, the %d images need %zu bytes aligned to %zu", dst_size, d_dst, capacity, need, es);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    if (dra) { ARGCHK(c, dra->luma_inv_scale_lut && dra->chroma_inv_scale_lut[0] && dra->chroma_inv_scale_lut[1]); ARGCHK(c, bd <= 10); }      // upload_dra's refusals, before anything is queued
    { const int rc = check_device_dst(c, "pic_output_device_rois_dev", d_dst, need); if (rc < 0) return rc; }
    // the boxes, the count and the results are device memory of 4-byte words as well - the host never reads them
    { const int rc = check_device_dst(c, "pic_output_device_rois_dev (boxes)", const_cast<void *>(d_boxes), (size_t)capacity * 16); if (rc < 0) return rc; }
    if (d_count) { const int rc = check_device_dst(c, "pic_output_device_rois_dev (count)", const_cast<int *>(d_count), sizeof(int)); if (rc < 0) return rc; }
    if (d_results) { const int rc = check_device_dst(c, "pic_output_device_rois_dev (results)", d_results, (size_t)capacity * sizeof(xgpu_roi_result)); if (rc < 0) return rc; }
    if (((uintptr_t)d_boxes | (uintptr_t)d_count | (uintptr_t)d_results) & 3) {
        snprintf(c->err, sizeof(c->err), "pic_output_device_rois_dev: boxes, count and results must be aligned to 4 bytes");
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    RoisDevLayout L;
    rois_dev_layout(sc, rp->fit, mw, mh, capacity, L);
    // the context's two buffers, grown on demand (section 8e's): sized from the bounds and the capacity, so a steady stream of calls never grows them
    const size_t mid_need = (size_t)capacity * L.mid_slot * sizeof(uint16_t);
    if (c->sc_mid_cap < mid_need) {
        if (c->sc_mid) { (void)hipFree(c->sc_mid); c->sc_mid = NULL; c->sc_mid_cap = 0; }
        if (hipMalloc((void **)&c->sc_mid, mid_need) != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, sizeof(c->err), "pic_output_device_rois_dev: cannot allocate the %zu-byte intermediate", mid_need); return XGPU_ERR_OUT_OF_MEMORY; }
        c->sc_mid_cap = mid_need;
    }
    if (c->roi_blk_cap < L.blk) {
        if (c->roi_blk) { (void)hipFree(c->roi_blk); c->roi_blk = NULL; c->roi_blk_cap = 0; }
        if (hipMalloc((void **)&c->roi_blk, L.blk) != hipSuccess) { (void)hipGetLastError(); snprintf(c->err, sizeof(c->err), "pic_output_device_rois_dev: cannot allocate the %zu-byte descriptor block", L.blk); return XGPU_ERR_OUT_OF_MEMORY; }
        c->roi_blk_cap = L.blk;
    }
    if (dra) { const int rc = upload_dra(c, dra); if (rc < 0) return rc; }
    hipStream_t s = c->stream;
    if (stream) {
        for (int i = 0; i < 2; i++)
            if (!c->odev_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->odev_ev[i], hipEventDisableTiming));
        s = (hipStream_t)stream;
        HIPCHK(c, hipEventRecord(c->odev_ev[0], c->stream));      // the picture's kernels, the DRA tables and every earlier output call (they all end in the context's stream) -> the caller's stream
        HIPCHK(c, hipStreamWaitEvent(s, c->odev_ev[0], 0));
    }
    // behind the wait above: after every kernel that read the previous block
    RoisPrepArgs p;
    memset(&p, 0, sizeof(p));
    p.blk = c->roi_blk; p.boxes = d_boxes; p.count = d_count; p.results = d_results;
    p.capacity = capacity; p.box_format = box_format;
    p.pw = c->sp.width - f->crop[0] - f->crop[1]; p.ph = c->sp.height - f->crop[2] - f->crop[3]; p.mw = mw; p.mh = mh;
    p.wd = sc->width; p.hd = sc->height; p.fit = rp->fit; p.filter = sc->filter; p.chroma_loc = f->chroma_loc;
    p.capy = L.capy; p.capc = L.capc;
    p.image_pitch = image_pitch;
    p.tab = (uint32_t)L.tab; p.slot = (uint32_t)L.slot; p.mid_slot = (uint32_t)L.mid_slot;
    for (int t = 0; t < 4; t++) { p.off_first[t] = L.off_first[t]; p.off_count[t] = L.off_count[t]; p.off_w[t] = L.off_w[t]; }
    launch_rois_prepare(p, s);
    RoisOutArgs a;
    memset(&a, 0, sizeof(a));
    scaled_common_args(c, pic, dra, f, sc, d_dst, a);
    a.mid = c->sc_mid;
    a.capy = L.capy; a.capc = L.capc;
    a.blk = c->roi_blk; a.n = capacity;
    for (int k = 0; k < 3; k++) a.padv[k] = rp->pad[k];
    launch_output_rois(a, f->layout, f->dtype, mw, sc->height, s);
    HIPCHK(c, hipGetLastError());
    if (stream) {
        HIPCHK(c, hipEventRecord(c->odev_ev[1], s));      // the context's stream - and through it the next output call on any stream - does not touch the slot, the block or the intermediate before the kernels are done
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->odev_ev[1], 0));
    }
    return XGPU_OK;
}

// ------------------------------------------------------------------------------------------------ coding side information of the picture decoded last
// the format alone and the size it needs for a picture of width x height; 0: invalid, `why` says which field
static size_t side_size(const xgpu_side_format *f, int width, int height, const char **why)
{
    *why = "format is NULL";
    if (!f) return 0;
    *why = "picture size must be positive multiples of 8";
    if (width <= 0 || height <= 0 || ((width | height) & 7)) return 0;
    *why = "crop offsets must be even and >= 0";
    for (int i = 0; i < 4; i++) if (f->crop[i] < 0 || (f->crop[i] & 1)) return 0;
    if (f->layout == XGPU_SIDE_BLOCKS) {
        *why = "BLOCKS: dtype XGPU_OUT_U16 (int16 planes), no crop, row_pitch a multiple of 2 and at least a row";
        if (f->dtype != XGPU_OUT_U16 || f->crop[0] || f->crop[1] || f->crop[2] || f->crop[3] || (f->row_pitch & 1)) return 0;
        const size_t w_scu = width >> 2, h_scu = height >> 2, row = w_scu * 2, pitch = f->row_pitch ? f->row_pitch : row;
        if (pitch < row) return 0;
        return (9 * h_scu - 1) * pitch + row;
    }
    *why = "layout must be XGPU_SIDE_BLOCKS, XGPU_SIDE_FLOW_PLANAR or XGPU_SIDE_FLOW_INTERLEAVED";
    if (f->layout != XGPU_SIDE_FLOW_PLANAR && f->layout != XGPU_SIDE_FLOW_INTERLEAVED) return 0;
    *why = "FLOW: dtype XGPU_OUT_F16 or XGPU_OUT_F32, lists 1..3, per_poc 0 or 1, row_pitch a multiple of the element size";
    if ((f->dtype != XGPU_OUT_F16 && f->dtype != XGPU_OUT_F32) || f->lists < 1 || f->lists > 3 || (f->per_poc & ~1)) return 0;
    const size_t es = (size_t)elem_size(f->dtype), ch = f->lists == 3 ? 4 : 2;
    if (f->row_pitch % es) return 0;
    *why = "crop leaves no picture";
    if (f->crop[0] + f->crop[1] >= width || f->crop[2] + f->crop[3] >= height) return 0;
    const size_t w = width - f->crop[0] - f->crop[1], h = height - f->crop[2] - f->crop[3];
    const bool planar = f->layout == XGPU_SIDE_FLOW_PLANAR;
    const size_t row = (planar ? w : ch * w) * es, pitch = f->row_pitch ? f->row_pitch : row;
    *why = "row_pitch is shorter than a row";
    if (pitch < row) return 0;
    return ((planar ? ch * h : h) - 1) * pitch + row;
}
size_t xgpu_side_info_size(const xgpu_side_format *f, int width, int height)
{
    const char *why;
    return side_size(f, width, height, &why);
}
// The SCU map is per context: it holds the side information of the picture whose xgpu_frame_end came last (c->side_pic) until the next xgpu_frame_begin -
// the next picture's k_inter overwrites it.  Checks first, then the order of output_device: on a caller's stream the kernel runs behind the picture's kernels
// (the side stream of k_affine / k_dmvr has been joined by then) and the context's stream waits for it before the next k_inter may write the map.
int xgpu_frame_side_info(xgpu_ctx *c, int pic, const xgpu_side_format *f, void *d_dst, size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, d_dst != NULL);
    if (c->have_frame || c->side_pic < 0 || pic != c->side_pic || !valid_pic(c, pic)) {
        snprintf(c->err, sizeof(c->err), "frame_side_info: slot %d is not the picture decoded last (%s): the SCU map belongs to the picture whose xgpu_frame_end came last, until the next xgpu_frame_begin",
                 pic, c->have_frame ? "a frame is open" : c->side_pic < 0 ? "no picture yet" : "another slot");
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    const char *why = "";
    const size_t need = side_size(f, c->sp.width, c->sp.height, &why);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "frame_side_info: invalid format: %s", why); return XGPU_ERR_INVALID_ARGUMENT; }
    const size_t es = (size_t)elem_size(f->dtype);
    if (dst_size < need || ((uintptr_t)d_dst % es)) {
        snprintf(c->err, sizeof(c->err), "frame_side_info: destination of %zu bytes at %p, the format needs %zu bytes aligned to %zu", dst_size, d_dst, need, es);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    { const int rc = check_device_dst(c, "frame_side_info", d_dst, need); if (rc < 0) return rc; }
    hipStream_t s = c->stream;
    if (stream) {
        for (int i = 0; i < 2; i++)
            if (!c->odev_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->odev_ev[i], hipEventDisableTiming));
        s = (hipStream_t)stream;
        HIPCHK(c, hipEventRecord(c->odev_ev[0], c->stream));      // the picture's kernels -> the caller's stream
        HIPCHK(c, hipStreamWaitEvent(s, c->odev_ev[0], 0));
    }
    SideArgs a;
    memset(&a, 0, sizeof(a));
    a.maps = c->d_maps; a.w_scu = c->w_scu; a.h_scu = c->h_scu;
    a.dst = (uint8_t *)d_dst;
    a.poc = c->fp.poc;
    for (int l = 0; l < 2; l++)
        for (int i = 0; i < XGPU_MAX_REFS; i++) a.refp_poc[i][l] = i < c->fp.num_refp[l] ? c->fp.refp_poc[i][l] : c->fp.poc;      // (an index past the list: distance 0)
    if (f->layout == XGPU_SIDE_BLOCKS) {
        a.pitch = f->row_pitch ? f->row_pitch : (size_t)c->w_scu * 2;
        a.plane = a.pitch * c->h_scu;
        a.aligned = (((uintptr_t)d_dst | a.pitch | a.plane) & 15) == 0;
        launch_side_blocks(a, s);
    } else {
        const bool planar = f->layout == XGPU_SIDE_FLOW_PLANAR;
        const int n_lists = f->lists == 3 ? 2 : 1;
        a.w = c->sp.width - f->crop[0] - f->crop[1]; a.h = c->sp.height - f->crop[2] - f->crop[3];
        a.crop_l = f->crop[0]; a.crop_t = f->crop[2];
        a.list0 = f->lists == 2 ? 1 : 0; a.per_poc = f->per_poc;
        a.pitch = f->row_pitch ? f->row_pitch : (size_t)a.w * es * (planar ? 1 : 2 * n_lists);
        a.plane = a.pitch * a.h;
        a.aligned = (((uintptr_t)d_dst | a.pitch | a.plane) & 15) == 0;
        launch_side_flow(a, planar, f->dtype, n_lists, s);
    }
    HIPCHK(c, hipGetLastError());
    if (stream) {
        HIPCHK(c, hipEventRecord(c->odev_ev[1], s));      // the context's stream does not let the next picture's k_inter write the map before the kernel is done
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->odev_ev[1], 0));
    }
    return XGPU_OK;
}

// ------------------------------------------------------------------------------------------------ the residual of a batch as picture-shaped planes
// the format alone and the size it needs for a picture of width x height; 0: invalid, `why` says which field
static size_t resid_size(const xgpu_resid_format *f, int width, int height, const char **why)
{
    *why = "format is NULL";
    if (!f) return 0;
    *why = "picture size must be positive multiples of 8";
    if (width <= 0 || height <= 0 || ((width | height) & 7)) return 0;
    *why = "crop offsets must be even and >= 0";
    for (int i = 0; i < 4; i++) if (f->crop[i] < 0 || (f->crop[i] & 1)) return 0;
    if (f->layout == XGPU_RESID_ENERGY) {
        *why = "ENERGY: dtype XGPU_OUT_F32, no crop, row_pitch a multiple of 4 and at least a row";
        if (f->dtype != XGPU_OUT_F32 || f->crop[0] || f->crop[1] || f->crop[2] || f->crop[3] || (f->row_pitch & 3)) return 0;
        const size_t w_scu = width >> 2, h_scu = height >> 2, row = w_scu * 4, pitch = f->row_pitch ? f->row_pitch : row;
        if (pitch < row) return 0;
        return (3 * h_scu - 1) * pitch + row;
    }
    *why = "layout must be XGPU_RESID_YUV420, XGPU_RESID_444_PLANAR, XGPU_RESID_444_INTERLEAVED or XGPU_RESID_ENERGY";
    if (f->layout != XGPU_RESID_YUV420 && f->layout != XGPU_RESID_444_PLANAR && f->layout != XGPU_RESID_444_INTERLEAVED) return 0;
    *why = "crop leaves no picture";
    if (f->crop[0] + f->crop[1] >= width || f->crop[2] + f->crop[3] >= height) return 0;
    const size_t w = width - f->crop[0] - f->crop[1], h = height - f->crop[2] - f->crop[3];
    if (f->layout == XGPU_RESID_YUV420) {
        *why = "YUV420: dtype XGPU_OUT_U16 (int16 planes), row_pitch a multiple of 4 (the chroma pitch is half of it) and at least a row";
        if (f->dtype != XGPU_OUT_U16 || (f->row_pitch & 3)) return 0;
        const size_t row = w * 2, pitch = f->row_pitch ? f->row_pitch : row;
        if (pitch < row) return 0;
        return h * pitch + (h - 1) * (pitch / 2) + row / 2;      // Y: h rows; Cb, Cr: h / 2 rows of pitch / 2 each, the last one tight
    }
    *why = "444: dtype XGPU_OUT_U16, XGPU_OUT_F16 or XGPU_OUT_F32, row_pitch a multiple of the element size";
    if (f->dtype != XGPU_OUT_U16 && f->dtype != XGPU_OUT_F16 && f->dtype != XGPU_OUT_F32) return 0;
    const size_t es = (size_t)elem_size(f->dtype);
    if (f->row_pitch % es) return 0;
    const bool planar = f->layout == XGPU_RESID_444_PLANAR;
    const size_t row = (planar ? w : 3 * w) * es, pitch = f->row_pitch ? f->row_pitch : row;
    *why = "row_pitch is shorter than a row";
    if (pitch < row) return 0;
    return ((planar ? 3 * h : h) - 1) * pitch + row;
}
size_t xgpu_resid_size(const xgpu_resid_format *f, int width, int height)
{
    const char *why;
    return resid_size(f, width, height, &why);
}
// The arena belongs to the batch: it holds the residual from the batch's residual pass (k_itdq, or the pass that rode in the previous picture's k_intra_itdq)
// until the batch is destroyed.  Checks first, then the order of output_device.  The pass ran on the context's stream - or, after xgpu_batch_prepare, on the
// side stream, and blk.itdq_done says when - so the kernel starts behind an event of the context's stream (and behind itdq_done), and the context's stream
// waits for the kernel: xgpu_batch_destroy records blk.done there, so a block that goes back to the pool is not refilled under the kernel.
int xgpu_batch_residual(xgpu_ctx *c, xgpu_dbatch *db, const xgpu_resid_format *f, void *d_dst, size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, db != NULL); ARGCHK(c, d_dst != NULL);
    if (!db->used && !db->prepared) {
        snprintf(c->err, sizeof(c->err), "batch_residual: the residual pass of this batch has not been queued: call xgpu_batch_recon(_ahead) of it, xgpu_batch_prepare, or pass it as `next` of xgpu_batch_recon_ahead first");
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    const char *why = "";
    const size_t need = resid_size(f, c->sp.width, c->sp.height, &why);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "batch_residual: invalid format: %s", why); return XGPU_ERR_INVALID_ARGUMENT; }
    const size_t es = (size_t)elem_size(f->dtype);
    if (dst_size < need || ((uintptr_t)d_dst % es)) {
        snprintf(c->err, sizeof(c->err), "batch_residual: destination of %zu bytes at %p, the format needs %zu bytes aligned to %zu", dst_size, d_dst, need, es);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    { const int rc = check_device_dst(c, "batch_residual", d_dst, need); if (rc < 0) return rc; }
    hipStream_t s = c->stream;
    if (stream) {
        for (int i = 0; i < 2; i++)
            if (!c->odev_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->odev_ev[i], hipEventDisableTiming));
        s = (hipStream_t)stream;
        HIPCHK(c, hipEventRecord(c->odev_ev[0], c->stream));      // the residual pass (and the batch's upload, which the context's stream has waited for) -> the caller's stream
        HIPCHK(c, hipStreamWaitEvent(s, c->odev_ev[0], 0));
    }
    if (db->prepared == 1) HIPCHK(c, hipStreamWaitEvent(s, db->blk.itdq_done, 0));      // the pass is on the side stream (behind the upload)
    ResidArgs a;
    memset(&a, 0, sizeof(a));
    a.owner = db->d_owner; a.cus = db->d_cus; a.resid = db->d_resid; a.w_scu = c->w_scu; a.h_scu = c->h_scu;
    a.chroma_cus = db->d_chroma_cus; a.n_chroma_cus = db->n_chroma_cus;
    a.dst = (uint8_t *)d_dst;
    a.scale[0] = 1.0f / (float)(1 << c->sp.bit_depth_luma); a.scale[1] = a.scale[2] = 1.0f / (float)(1 << c->sp.bit_depth_chroma);
    a.w = c->sp.width - f->crop[0] - f->crop[1]; a.h = c->sp.height - f->crop[2] - f->crop[3];
    a.crop_l = f->crop[0]; a.crop_t = f->crop[2];
    if (f->layout == XGPU_RESID_ENERGY) {
        a.pitch = f->row_pitch ? f->row_pitch : (size_t)c->w_scu * 4;
        a.plane = a.pitch * c->h_scu;
        a.aligned = (((uintptr_t)d_dst | a.pitch | a.plane) & 15) == 0;
    } else if (f->layout == XGPU_RESID_YUV420) {
        a.pitch = f->row_pitch ? f->row_pitch : (size_t)a.w * 2;
        a.pitch_c = a.pitch / 2;
        a.off_c[0] = a.pitch * a.h; a.off_c[1] = a.off_c[0] + a.pitch_c * (a.h / 2);
        a.aligned = (((uintptr_t)d_dst | a.pitch) & 15) == 0;      // then the chroma rows (8-byte stores) start at multiples of 8
    } else {
        a.pitch = f->row_pitch ? f->row_pitch : (size_t)a.w * es * (f->layout == XGPU_RESID_444_PLANAR ? 1 : 3);
        a.plane = a.pitch * a.h;
        a.aligned = (((uintptr_t)d_dst | a.pitch | a.plane) & 15) == 0;
    }
    launch_residual(a, f->layout, f->dtype, s);
    HIPCHK(c, hipGetLastError());
    if (stream) {
        HIPCHK(c, hipEventRecord(c->odev_ev[1], s));      // the context's stream - where xgpu_batch_destroy records blk.done - does not pass the kernel
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->odev_ev[1], 0));
    }
    return XGPU_OK;
}

// The picture signature on the device (k_md5.hip): the planes packed as the signature's message behind the picture's kernels (k_output, samples as they are), the three
// chains on the transfer stream - the kernel stream is free for the next picture while they run -, 48 bytes to the host.  Blocking.
int xgpu_pic_md5(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, uint8_t digest[3][16])
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, digest != NULL);
    const int w = c->sp.width, h = c->sp.height;
    const size_t need = ((size_t)w * h + 2 * (size_t)(w >> 1) * (h >> 1)) * 2;
    if (!c->d_md5) {
        if (!c->md5_ready) HIPCHK(c, hipEventCreateWithFlags(&c->md5_ready, hipEventDisableTiming));      // the event first: d_md5 != NULL means both exist
        if (hipMalloc((void **)&c->d_md5, need + 64) != hipSuccess) { c->d_md5 = NULL; snprintf(c->err, sizeof(c->err), "pic_md5: cannot allocate the %zu-byte message buffer", need + 64); return XGPU_ERR_OUT_OF_MEMORY; }
    }
    if (dra) { const int rc = upload_dra(c, dra); if (rc < 0) return rc; }
    uint32_t *d_digest = (uint32_t *)(c->d_md5 + ((need + 15) & ~(size_t)15));
    launch_output(c, dpic(c, pic), dra ? c->d_dra : NULL, c->sp.bit_depth_luma, 0, 0, 0, 0, c->d_md5, true);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->md5_ready, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->down_stream, c->md5_ready, 0));
    launch_md5(c, c->down_stream, c->d_md5, w, h, d_digest);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(digest, d_digest, 48, hipMemcpyDeviceToHost, c->down_stream));
    HIPCHK(c, hipStreamSynchronize(c->down_stream));
    return XGPU_OK;
}

// ------------------------------------------------------------------------------------------------ per picture
// ADDB deblocking directly followed by ALF: xgpu_deblock only prepares its arguments and xgpu_alf launches k_addb_alf, which deblocks the 72 x 72 region around

int xgpu_frame_begin(xgpu_ctx *c, const xgpu_frame_params *fp)
{
    ARGCHK(c, c != NULL); ARGCHK(c, fp != NULL); ARGCHK(c, valid_pic(c, fp->pic));
    for (int l = 0; l < 2; l++) {
        ARGCHK(c, fp->num_refp[l] >= 0 && fp->num_refp[l] <= XGPU_MAX_REFS);
        for (int i = 0; i < fp->num_refp[l]; i++) ARGCHK(c, valid_pic(c, fp->refp_pic[i][l]));
    }
    c->fp = *fp;
    c->have_frame = 1;
    c->side_pic = -1;      // the map is about to be overwritten
    c->where = 0;
    c->pad_done = 0;
    c->addb_pending = 0;
    c->order_rl = 0;
    return XGPU_OK;
}

int xgpu_frame_end(xgpu_ctx *c)
{
    ARGCHK(c, c != NULL);
    const int was_open = c->have_frame;
    c->have_frame = 0;
    c->side_pic = -1;
    if (c->where != 0 || c->addb_pending) {
        c->addb_pending = 0;
        snprintf(c->err, sizeof(c->err), "frame_end: the in-loop filters announced in xgpu_frame_params (deblock_on=%d alf_on=%d) were not all run",
                 c->fp.deblock_on, c->fp.alf_on);
        c->where = 0;
        return XGPU_ERR_UNEXPECTED;
    }
    if (was_open) c->side_pic = c->fp.pic;      // the SCU map now holds this picture's side information (xgpu_frame_side_info)
    return XGPU_OK;
}
