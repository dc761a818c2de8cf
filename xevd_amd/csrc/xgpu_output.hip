// xgpu_output.hip - the C ABI of include/xevd_hip.h, part 2: the outputs into device memory - the picture as it is, colour-managed, as a packed display surface, through a 3D LUT, dithered, scaled, as a batch of regions of
// interest (rectangles from the host or boxes in device memory), of affine maps or of coordinate grids, as a ladder of scaled video surfaces, the coding side information, the residual, the comparison with a reference and the statistics
// of one picture - and their argument checks without a device.
// Every entry point is the same skeleton: check the format -> check_dst -> (check_dra; tables, made on the host) -> grow a context buffer -> out_fork -> fill an args struct ->
// launch -> out_join.  Host-side code only; the kernels live in k_output*.hip, k_side_info.hip, k_residual.hip, k_compare.hip and k_stats.hip.
#include "xgpu_host.h"
#include "scale_taps.h"
#include <memory>

#define TRY(expr) do { const int rc_ = (expr); if (rc_ < 0) return rc_; } while (0)

// ------------------------------------------------------------------------------------------------ what the entry points share
// The ordering contract of every output into device memory.  The kernels of a call run on `stream`, the caller's (NULL: the context's stream, where nothing needs
// ordering).  out_fork makes that stream wait for an event of the context's stream: the picture's kernels, the uploads of upload_dra and - because out_join ends
// every earlier call there - every earlier output call are done before anything this call queues starts.  out_join makes the context's stream wait for the call's
// last kernel.  So every output call ends in the context's stream, whichever stream it ran on, and the next call - on any stream - starts behind it: what a call
// reads or rewrites that is the context's and not the call's (the DRA, colour and tap tables, the intermediate, the descriptor block, the SCU map, a batch's arena)
// is never written under a running kernel, neither by the next output call nor by the context's own next kernels.  Everything a call rewrites is therefore queued
// between the two, on *s.
static int out_fork(xgpu_ctx *c, void *stream, hipStream_t *s)
{
    *s = c->stream;
    if (!stream) return XGPU_OK;
    for (int i = 0; i < 2; i++)
        if (!c->odev_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->odev_ev[i], hipEventDisableTiming));
    *s = (hipStream_t)stream;
    HIPCHK(c, hipEventRecord(c->odev_ev[0], c->stream));
    HIPCHK(c, hipStreamWaitEvent(*s, c->odev_ev[0], 0));
    return XGPU_OK;
}
static int out_join(xgpu_ctx *c, void *stream, hipStream_t s)
{
    HIPCHK(c, hipGetLastError());      // of the launches between the two
    if (!stream) return XGPU_OK;
    HIPCHK(c, hipEventRecord(c->odev_ev[1], s));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->odev_ev[1], 0));
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
// The destination of entry point `who`: dst_size bytes at d_dst must hold the `need` bytes of the call, aligned to the element (es bytes) ...
static int check_dst_fits(xgpu_ctx *c, const char *who, void *d_dst, size_t dst_size, size_t need, size_t es)
{
    if (dst_size < need || ((uintptr_t)d_dst % es)) {
        snprintf(c->err, sizeof(c->err), "%s: destination of %zu bytes at %p, the call needs %zu bytes aligned to %zu", who, dst_size, d_dst, need, es);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    return XGPU_OK;
}
// ... in device memory of this device.  (The scaled outputs refuse their DRA tables between the two, so they call the two halves themselves.)
static int check_dst(xgpu_ctx *c, const char *who, void *d_dst, size_t dst_size, size_t need, size_t es)
{
    TRY(check_dst_fits(c, who, d_dst, dst_size, need, es));
    return check_device_dst(c, who, d_dst, need);
}
// A buffer of the context, grown on demand to `need` bytes (and `room` more, once it has to grow).  hipFree waits for the device, so no kernel of an earlier call
// still reads what is freed; in steady state neither runs.
template <class T> static int grow(xgpu_ctx *c, const char *who, T **ptr, size_t *cap, size_t need, const char *what, size_t room = 0)
{
    if (*cap >= need) return XGPU_OK;
    if (*ptr) { (void)hipFree(*ptr); *ptr = NULL; *cap = 0; }
    if (hipMalloc((void **)ptr, need + room) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(c->err, sizeof(c->err), "%s: cannot allocate the %zu-byte %s", who, need + room, what);
        return XGPU_ERR_OUT_OF_MEMORY;
    }
    *cap = need + room;
    return XGPU_OK;
}
// n rows of `row` bytes in a destination: the bytes between two of them (row_pitch, 0: tight) and the bytes they span - the last row need not be followed by a
// pitch's worth of bytes -, 0 for a pitch shorter than a row
struct Rows { size_t pitch, total; };
static Rows rows_of(size_t row, size_t n, size_t row_pitch)
{
    const size_t pitch = row_pitch ? row_pitch : row;
    return { pitch, pitch < row ? 0 : (n - 1) * pitch + row };
}
static bool aligned16(uintptr_t bits) { return (bits & 15) == 0; }      // every address and distance or-ed into `bits` allows 16-byte vector stores
// ... and the same rows in an args struct: the pitch, the distance between two planes of `rows` rows (SemiPlanarArgs: to its chroma plane) and whether all allow vector stores
template <class A> static void fill_rows(A &a, void *d_dst, size_t row, size_t rows, size_t row_pitch, size_t A::*plane = &A::plane)
{
    a.pitch = rows_of(row, rows, row_pitch).pitch;
    a.*plane = a.pitch * rows;
    a.aligned = aligned16((uintptr_t)d_dst | a.pitch | a.*plane);
}
// crop (left, right, top, bottom): even and >= 0, and - where the caller knows the picture (width > 0) - leaving some of it
static bool crop_ok(const int crop[4], int width, int height, const char **why)
{
    *why = "crop offsets must be even and >= 0";
    for (int i = 0; i < 4; i++) if (crop[i] < 0 || (crop[i] & 1)) return false;
    *why = "crop leaves no picture";
    return width <= 0 || ((long long)crop[0] + crop[1] < width && (long long)crop[2] + crop[3] < height);
}
// first sample of the cropped area of every plane
static void cropped_planes(const DevPic &p, const int crop[4], const int16_t **y, const int16_t **u, const int16_t **v)
{
    const size_t oc = (size_t)(crop[2] >> 1) * p.s_c + (crop[0] >> 1);
    *y = p.y + (size_t)crop[2] * p.s_l + crop[0];
    *u = p.u + oc; *v = p.v + oc;
}
template <class T> static T align8(T v) { return (v + 7) & ~(T)7; }
// the samples of one row of the scaled outputs' intermediate for a source ws wide: a luma row and two chroma rows, each a multiple of 8 (k_output_scaled.hip)
static size_t mid_row_samples(int ws) { return (size_t)align8(ws) + 2 * (size_t)align8(ws >> 1); }

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
static bool is_interleaved(int layout) { return layout == XGPU_OUT_RGB_INTERLEAVED || layout == XGPU_OUT_YUV444_INTERLEAVED; }
// a w x h image of three channels in an RGB / YUV444 layout: h rows of 3 w elements, or three planes of h rows of w
static size_t image_row(const xgpu_output_format *f, size_t w) { return (is_interleaved(f->layout) ? 3 : 1) * w * elem_size(f->dtype); }
static size_t image_rows(const xgpu_output_format *f, size_t h) { return (is_interleaved(f->layout) ? 1 : 3) * h; }
// the depth D the samples of YUV420P / NV12 / P016 are converted to
static int sample_depth(const xgpu_output_format *f, int bd) { return f->out_bit_depth ? f->out_bit_depth : bd; }
// the format alone (no picture size): 0 or a negative code, `why` says which field
static int check_format(const xgpu_output_format *f, int bd, const char **why)
{
    *why = "format is NULL";
    if (!f) return XGPU_ERR_INVALID_ARGUMENT;
    if (!crop_ok(f->crop, 0, 0, why)) return XGPU_ERR_INVALID_ARGUMENT;
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
// the matrix of a supported `matrix` at coding depth bd: fcoef = the float32 coefficients (2^D - 1 = 1) and, for integer elements of depth d (0: none - zeros),
// coef = round(k * (2^d - 1) / range * 2^S) with S = 27 - d
static void matrix_coeffs(int matrix, int full_range, int bit_depth, int d, int32_t coef[5], int *shift, float fcoef[5])
{
    double kr, kb, yr, cr;
    int yo;
    matrix_kr_kb(matrix, &kr, &kb);
    const double kg = 1.0 - kr - kb;
    range_terms(bit_depth, full_range, &yo, &yr, &cr);
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
    if (!d) {
        for (int i = 0; i < 5; i++) coef[i] = 0;
        *shift = 0;
        return;
    }
    const int sh = 27 - d;
    terms((double)((1 << d) - 1), (double)(1 << sh), t);
    for (int i = 0; i < 5; i++) coef[i] = (int32_t)round(t[i]);      // half away from zero; cgu and cgv are negated rounded magnitudes
    *shift = sh;
}
int xgpu_output_coeffs(const xgpu_output_format *f, int bit_depth, int32_t coef[5], int *shift, float fcoef[5])
{
    const char *why;
    if (bit_depth < 8 || bit_depth > 12 || !coef || !shift || !fcoef) return XGPU_ERR_INVALID_ARGUMENT;
    const int rc = check_format(f, bit_depth, &why);
    if (rc < 0) return rc;
    if (!is_rgb(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
    matrix_coeffs(f->matrix, f->full_range, bit_depth, f->dtype == XGPU_OUT_U8 ? 8 : f->dtype == XGPU_OUT_U16 ? bit_depth : 0, coef, shift, fcoef);
    return XGPU_OK;
}
// 0 with *rc = the code and `why`, or the bytes the destination needs.  At a valid depth the format's own refusal comes first: a matrix that is not supported is
// XGPU_ERR_UNSUPPORTED whatever the picture's size.
static size_t format_size(const xgpu_output_format *f, int width, int height, int bd, int *rc, const char **why)
{
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    *why = "picture size or bit depth out of range";
    if (bd < 8 || bd > 12) return 0;
    const char *fwhy;
    const int frc = check_format(f, bd, &fwhy);
    if (frc == XGPU_ERR_UNSUPPORTED) *rc = frc;
    if (width <= 0 || height <= 0 || ((width | height) & 1)) return 0;
    if (frc < 0) { *why = fwhy; return 0; }
    if (!crop_ok(f->crop, width, height, why)) return 0;
    const size_t w = width - f->crop[0] - f->crop[1], h = height - f->crop[2] - f->crop[3];
    *why = "row_pitch is shorter than a row";
    const size_t total = f->layout == XGPU_OUT_YUV420P ? (w * h + 2 * (w >> 1) * (h >> 1)) * elem_size(f->dtype) :      // xgpu_pic_output_size
                         is_semiplanar(f->layout) ? rows_of(w * elem_size(f->dtype), h + h / 2, f->row_pitch).total :
                                                    rows_of(image_row(f, w), image_rows(f, h), f->row_pitch).total;
    if (total) *rc = XGPU_OK;
    return total;
}
size_t xgpu_output_format_size(const xgpu_output_format *f, int width, int height, int bit_depth)
{
    int rc; const char *why;
    return format_size(f, width, height, bit_depth, &rc, &why);
}
size_t xgpu_pic_output_device_size(const xgpu_ctx *c, const xgpu_output_format *f)
{
    int rc; const char *why;
    return c ? format_size(f, c->sp.width, c->sp.height, c->sp.bit_depth_luma, &rc, &why) : 0;
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
// What every call with a transform does with these tables, in three steps (xgpu_pic_output_device_cm and the scaled calls of section 8m share the cache).
// cm_prepare, before anything is queued: the layout must be RGB; a transform the cache does not hold is made into cm_new, or refused with xgpu_colour_tables' code.
static int cm_prepare(xgpu_ctx *c, const char *who, const xgpu_output_format *f, const xgpu_colour_transform *cm, std::unique_ptr<xgpu_colour_tables_t> &cm_new)
{
    const int bd = c->sp.bit_depth_luma;
    if (!is_rgb(f->layout)) { snprintf(c->err, sizeof(c->err), "%s: a colour transform needs one of the RGB layouts", who); return XGPU_ERR_INVALID_ARGUMENT; }
    if (cm_cached(c, cm, bd)) return XGPU_OK;
    cm_new.reset(new (std::nothrow) xgpu_colour_tables_t);
    const int rc = cm_new ? xgpu_colour_tables(f, cm, bd, cm_new.get()) : XGPU_ERR_OUT_OF_MEMORY;
    if (rc < 0) {
        snprintf(c->err, sizeof(c->err), "%s: transform %d/%d -> %d/%d (primaries / transfer) is not supported or its parameters are invalid", who,
                 cm->src_primaries, cm->src_transfer, cm->dst_primaries, cm->dst_transfer);
        return rc;
    }
    if (!c->d_cm && hipMalloc((void **)&c->d_cm, sizeof(float) * CM_FLOATS) != hipSuccess) { snprintf(c->err, sizeof(c->err), "%s: cannot allocate the tables", who); return XGPU_ERR_OUT_OF_MEMORY; }
    return XGPU_OK;
}
// what a _check entry ends in: the layout, then whether the transform's tables would build (cm_prepare's order), without a device
static int cm_dry_run(const xgpu_output_format *f, const xgpu_colour_transform *cm, int bit_depth)
{
    if (!is_rgb(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
    std::unique_ptr<xgpu_colour_tables_t> t(new (std::nothrow) xgpu_colour_tables_t);
    return t ? xgpu_colour_tables(f, cm, bit_depth, t.get()) : XGPU_ERR_OUT_OF_MEMORY;
}
// cm_commit, behind the fork - after every kernel that read the previous tables: a new set is uploaded on `s` and named by the key
static int cm_commit(xgpu_ctx *c, const xgpu_colour_transform *cm, std::unique_ptr<xgpu_colour_tables_t> &cm_new, hipStream_t s)
{
    if (!cm_new) return XGPU_OK;
    delete c->cm_tab;
    c->cm_tab = NULL;      // d_cm is about to change: no key names it until all of the new set is queued
    TRY(upload_cm(c, cm_new.get(), s));
    c->cm_tab = cm_new.release(); c->cm_key = *cm; c->cm_bd = c->sp.bit_depth_luma;
    return XGPU_OK;
}
// fill_cm: the matrix of the U16 form in `a` (the code at the coding depth feeds the transform, whatever the output dtype) and the transform of tables `t` in `p`
static void fill_cm(xgpu_ctx *c, const xgpu_output_format *f, const xgpu_colour_tables_t &t, RgbOutArgs &a, CmParams &p)
{
    const int bd = c->sp.bit_depth_luma;
    xgpu_output_format f16 = *f;
    f16.dtype = XGPU_OUT_U16;
    f16.row_pitch = 0;             // (the caller's pitch counts the caller's elements, not 16-bit ones)
    (void)xgpu_output_coeffs(&f16, bd, a.coef, &a.shift, a.fcoef);
    a.maxv = (1 << bd) - 1;
    p.lin = c->d_cm; p.tone = t.use_tone ? c->d_cm + CM_TONE_OFF : NULL; p.enc = t.use_encode ? c->d_cm + CM_ENC_OFF : NULL;
    p.n_lin = t.n_lin; p.use_matrix = t.use_matrix;
    memcpy(p.m, t.matrix, sizeof(p.m)); memcpy(p.luma, t.luma, sizeof(p.luma));
    p.scale = t.scale;
    p.outmax = f->dtype == XGPU_OUT_U8 ? 255.f : (float)((1 << bd) - 1);
}
// the conversion of an RGB or YUV444 layout at the context's coding depth: range terms, matrix (RGB) or scales (YUV444: no matrix, coef / maxv stay zero), the DRA tables
static void fill_conversion(xgpu_ctx *c, const xgpu_dra_luts *dra, const xgpu_output_format *f, RgbOutArgs &a)
{
    const int bd = c->sp.bit_depth_luma;
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
        a.fcoef[0] = (float)(1.0 / yr); a.fcoef[1] = (float)(1.0 / crr);      // rounded once from double
    }
}
// ChromaSampleLocType: horizontally co-sited (0, 2, 4) / centred (1, 3, 5); vertically centred (0, 1), top (2, 3), bottom (4, 5)
static void fill_siting(int chroma_loc, RgbOutArgs &a)
{
    static const int ve[3][2] = { { 1, 3 }, { 0, 4 }, { 2, 2 } }, vo[3][2] = { { 3, 1 }, { 2, 2 }, { 4, 0 } };
    a.hc = chroma_loc & 1;
    a.ve[0] = ve[chroma_loc >> 1][0]; a.ve[1] = ve[chroma_loc >> 1][1];
    a.vo[0] = vo[chroma_loc >> 1][0]; a.vo[1] = vo[chroma_loc >> 1][1];
}
// the source of the cropped picture `pic`, its size and where it goes; the destination's rows are the caller's to fill
static void fill_source(xgpu_ctx *c, int pic, const int crop[4], void *d_dst, RgbOutArgs &a)
{
    const DevPic &p = dpic(c, pic);
    cropped_planes(p, crop, &a.y, &a.u, &a.v);
    a.sy = p.s_l; a.sc = p.s_c;
    a.w = c->sp.width - crop[0] - crop[1]; a.h = c->sp.height - crop[2] - crop[3];
    a.cw = a.w >> 1; a.ch = a.h >> 1;
    a.dst = (uint8_t *)d_dst;
}
// all of an NV12 / P016 call's arguments: source, rows and launch_output's conversion at depth D
static void fill_semiplanar(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, void *d_dst, SemiPlanarArgs &a)
{
    const DevPic &p = dpic(c, pic);
    const int bd = c->sp.bit_depth_luma, obd = sample_depth(f, bd);
    const int w = c->sp.width - f->crop[0] - f->crop[1], h = c->sp.height - f->crop[2] - f->crop[3];
    cropped_planes(p, f->crop, &a.y, &a.u, &a.v);
    a.sy = p.s_l; a.sc = p.s_c;
    a.w = w; a.ch = h >> 1;
    a.dst = (uint8_t *)d_dst;
    fill_rows(a, d_dst, (size_t)w * elem_size(f->dtype), h, f->row_pitch, &SemiPlanarArgs::chroma_off);
    a.shift = bd - obd; a.out8 = obd == 8; a.maxv = (1 << obd) - 1;
    a.lsh = f->layout == XGPU_OUT_P016 ? 16 - obd : 0;
    a.dra = dra ? c->d_dra : NULL;
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
    int rc;
    const size_t need = format_size(f, c->sp.width, c->sp.height, c->sp.bit_depth_luma, &rc, &why);
    if (need == 0) {
        snprintf(c->err, sizeof(c->err), "pic_output_device: invalid format: %s", why);
        return rc;
    }
    const size_t es = f->layout == XGPU_OUT_YUV420P ? 1 : (size_t)elem_size(f->dtype);
    TRY(check_dst(c, "pic_output_device", d_dst, dst_size, need, es));
    std::unique_ptr<xgpu_colour_tables_t> cm_new;      // a new set of tables: made here, before anything is queued; uploaded and committed below
    if (cm) TRY(cm_prepare(c, "pic_output_device_cm", f, cm, cm_new));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    TRY(cm_commit(c, cm, cm_new, s));
    const int *cr = f->crop;
    if (f->layout == XGPU_OUT_YUV420P) {
        launch_output(c, dpic(c, pic), dra ? c->d_dra : NULL, sample_depth(f, c->sp.bit_depth_luma), cr[0], cr[1], cr[2], cr[3], (uint8_t *)d_dst, false, s);
    } else if (is_semiplanar(f->layout)) {
        SemiPlanarArgs a;
        memset(&a, 0, sizeof(a));
        fill_semiplanar(c, pic, dra, f, d_dst, a);
        launch_output_semiplanar(a, f->dtype, s);
    } else {
        RgbOutArgs a;
        memset(&a, 0, sizeof(a));
        fill_source(c, pic, cr, d_dst, a);
        fill_rows(a, d_dst, image_row(f, a.w), a.h, f->row_pitch);
        fill_conversion(c, dra, f, a);
        fill_siting(f->chroma_loc, a);
        if (cm) {
            CmOutArgs ca;
            static_cast<RgbOutArgs &>(ca) = a;
            fill_cm(c, f, *c->cm_tab, ca, ca.cm);
            launch_output_cm(ca, f->layout, f->dtype, f->upsample, s);
        } else if (is_rgb(f->layout)) {
            launch_output_rgb(a, f->layout, f->dtype, f->upsample, s);
        } else {
            launch_output_yuv444(a, f->layout, f->dtype, f->upsample, s);
        }
    }
    return out_join(c, stream, s);      // the slot, the DRA and the colour tables
}

// ------------------------------------------------------------------------------------------------ packed display surfaces
static bool is_packed_rgb(int layout) { return layout == XGPU_PACKED_RGBA || layout == XGPU_PACKED_RGB10A2; }
static bool is_packed_422(int layout) { return layout == XGPU_PACKED_YUYV || layout == XGPU_PACKED_UYVY; }
// the element of a packed layout's rows and pitch (10:10:10:2: the word) and the bytes of a row of w pixels
static size_t packed_elem_size(const xgpu_packed_format *f) { return f->layout == XGPU_PACKED_RGB10A2 ? 4 : (size_t)elem_size(f->dtype); }
static size_t packed_row(const xgpu_packed_format *f, size_t w) { return f->layout == XGPU_PACKED_RGB10A2 ? 4 * w : (is_packed_422(f->layout) ? 2 : 4) * w * elem_size(f->dtype); }
// the depth D of the 4:2:2 samples
static int packed_depth(const xgpu_packed_format *f, int bd) { return f->out_bit_depth ? f->out_bit_depth : bd; }
// the format alone (no picture size): 0 or a negative code, `why` says which field
static int check_packed_format(const xgpu_packed_format *f, int bd, const char **why)
{
    *why = "format is NULL";
    if (!f) return XGPU_ERR_INVALID_ARGUMENT;
    if (!crop_ok(f->crop, 0, 0, why)) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "layout must be one of XGPU_PACKED_RGBA .. XGPU_PACKED_UYVY";
    if (!is_packed_rgb(f->layout) && !is_packed_422(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "chroma_loc 0..5; upsample XGPU_UPSAMPLE_NEAREST or _LINEAR";
    if (f->chroma_loc < 0 || f->chroma_loc > 5 || (f->upsample != XGPU_UPSAMPLE_NEAREST && f->upsample != XGPU_UPSAMPLE_LINEAR)) return XGPU_ERR_INVALID_ARGUMENT;
    if (is_packed_422(f->layout)) {
        const int obd = packed_depth(f, bd);
        *why = "YUYV / UYVY: dtype U8 with out_bit_depth 8, or U16 with out_bit_depth 8..16 (0 = the coding depth)";
        if (f->dtype == XGPU_OUT_U8 ? f->out_bit_depth != 8 : (f->dtype != XGPU_OUT_U16 || obd < 8 || obd > 16)) return XGPU_ERR_INVALID_ARGUMENT;
        *why = "YUYV / UYVY: bgr must be 0, row_pitch a multiple of the element size";
        if (f->bgr || f->row_pitch % packed_elem_size(f)) return XGPU_ERR_INVALID_ARGUMENT;
        return XGPU_OK;
    }
    if (f->layout == XGPU_PACKED_RGBA) {
        *why = "RGBA: dtype must be one of XGPU_OUT_U8 .. XGPU_OUT_F32";
        if (f->dtype < XGPU_OUT_U8 || f->dtype > XGPU_OUT_F32) return XGPU_ERR_INVALID_ARGUMENT;
        *why = "RGBA: out_bit_depth must be 0 or the coding depth";
        if (f->out_bit_depth != 0 && f->out_bit_depth != bd) return XGPU_ERR_INVALID_ARGUMENT;
    } else {
        *why = "RGB10A2: dtype and out_bit_depth must be 0";
        if (f->dtype != 0 || f->out_bit_depth != 0) return XGPU_ERR_INVALID_ARGUMENT;
    }
    *why = "bgr, full_range: 0 or 1; row_pitch a multiple of the element size (RGB10A2: of 4)";
    if ((f->bgr | f->full_range) & ~1 || f->row_pitch % packed_elem_size(f)) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "alpha must be finite and in [0, 1]";
    if (!(f->alpha >= 0.f && f->alpha <= 1.f)) return XGPU_ERR_INVALID_ARGUMENT;      // (a NaN fails both comparisons)
    double kr, kb;
    *why = "matrix: supported MatrixCoefficients are 1, 4, 5, 6, 7 and 9";
    if (!matrix_kr_kb(f->matrix, &kr, &kb)) return XGPU_ERR_UNSUPPORTED;
    return XGPU_OK;
}
// 0 with *rc = the code and `why`, or the bytes the destination needs
static size_t packed_size(const xgpu_packed_format *f, int width, int height, int bd, int *rc, const char **why)
{
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    *why = "picture size or bit depth out of range";
    if (width <= 0 || height <= 0 || ((width | height) & 1) || bd < 8 || bd > 12) return 0;
    if ((*rc = check_packed_format(f, bd, why)) < 0) return 0;
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    if (!crop_ok(f->crop, width, height, why)) return 0;
    const size_t w = width - f->crop[0] - f->crop[1], h = height - f->crop[2] - f->crop[3];
    *why = "row_pitch is shorter than a row";
    const size_t total = rows_of(packed_row(f, w), h, f->row_pitch).total;
    if (total) *rc = XGPU_OK;
    return total;
}
size_t xgpu_output_packed_size(const xgpu_packed_format *f, int width, int height, int bit_depth)
{
    int rc; const char *why;
    return packed_size(f, width, height, bit_depth, &rc, &why);
}
// the RGB format whose three elements the packed RGB layouts write (RGB10A2: the U16 form, whose code at the coding depth feeds a transform)
static xgpu_output_format packed_rgb_format(const xgpu_packed_format *f)
{
    xgpu_output_format r;
    memset(&r, 0, sizeof(r));
    r.layout = XGPU_OUT_RGB_INTERLEAVED; r.bgr = f->bgr;
    r.dtype = f->layout == XGPU_PACKED_RGB10A2 ? XGPU_OUT_U16 : f->dtype;
    r.matrix = f->matrix; r.full_range = f->full_range; r.chroma_loc = f->chroma_loc; r.upsample = f->upsample;
    memcpy(r.crop, f->crop, sizeof(r.crop));
    return r;
}
// the plain call's checks and codes first, then the layout and the transform (cm_prepare's order)
int xgpu_output_packed_check(const xgpu_packed_format *f, const xgpu_colour_transform *cm, int width, int height, int bit_depth)
{
    int rc; const char *why;
    (void)packed_size(f, width, height, bit_depth, &rc, &why);
    if (rc < 0 || !cm) return rc;
    if (!is_packed_rgb(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
    const xgpu_output_format rf = packed_rgb_format(f);
    return cm_dry_run(&rf, cm, bit_depth);
}
// The A element.  RGBA: floor(alpha * (2^D - 1) + 0.5) in double for the integer dtypes (D = 8 for U8, else the coding depth), the float32 bits of alpha for the
// float dtypes (the kernel rounds them to the dtype); RGB10A2: floor(alpha * 3 + 0.5)
static uint32_t packed_alpha_code(const xgpu_packed_format *f, int bd)
{
    if (f->layout == XGPU_PACKED_RGBA && f->dtype != XGPU_OUT_U8 && f->dtype != XGPU_OUT_U16) {
        uint32_t bits;
        memcpy(&bits, &f->alpha, sizeof(bits));
        return bits;
    }
    const int d = f->layout == XGPU_PACKED_RGB10A2 ? 2 : f->dtype == XGPU_OUT_U8 ? 8 : bd;
    return (uint32_t)floor((double)f->alpha * (double)((1 << d) - 1) + 0.5);
}
// The matrix of the packed RGB layouts without a transform.  RGBA: xgpu_output_coeffs' of the dtype.  RGB10A2: D = 10, S = 17 whatever the coding depth B.  Its sums
// fit int32 for B = 8 .. 12 and samples in 0 .. 2^B - 1: cy * (Y - yo) <= 1023 * 2^17 * (2^B - 1 - yo) / yr <= 1023 * 2^17 * 239 / 219 < 2^28, one chroma term
// <= 2 (1 - k) * 1023 * 2^17 * 2^(B-1) / cr <= 1.8814 * 1023 * 2^17 * 128 / 224 < 2^28 (full range: 128 / 255), G's two chroma terms together less than that, and
// the rounding term 2^16: every sum is below 2^29 + 2^16 in magnitude.
int xgpu_output_packed_coeffs(const xgpu_packed_format *f, int bit_depth, int32_t coef[5], int *shift, float fcoef[5], uint32_t *alpha_code)
{
    const char *why;
    if (bit_depth < 8 || bit_depth > 12 || !coef || !shift || !fcoef || !alpha_code) return XGPU_ERR_INVALID_ARGUMENT;
    const int rc = check_packed_format(f, bit_depth, &why);
    if (rc < 0) return rc;
    if (!is_packed_rgb(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
    const int d = f->layout == XGPU_PACKED_RGB10A2 ? 10 : f->dtype == XGPU_OUT_U8 ? 8 : f->dtype == XGPU_OUT_U16 ? bit_depth : 0;
    matrix_coeffs(f->matrix, f->full_range, bit_depth, d, coef, shift, fcoef);
    *alpha_code = packed_alpha_code(f, bit_depth);
    return XGPU_OK;
}
// the conversion of the packed RGB layouts (rf: packed_rgb_format's): range terms, DRA, the A element and the matrix - with a transform (the context's tables,
// committed) the U16 form's and the transform, else that of the store's depth; 10:10:10:2 stores D = 10 whatever the coding depth
static void fill_packed_rgb(xgpu_ctx *c, const xgpu_dra_luts *dra, const xgpu_packed_format *f, const xgpu_output_format *rf, bool cm, PackedRgbArgs &a)
{
    const int bd = c->sp.bit_depth_luma;
    fill_conversion(c, dra, rf, a);
    a.alpha = packed_alpha_code(f, bd);
    if (cm) {
        fill_cm(c, rf, *c->cm_tab, a, a.cm);
        if (f->layout == XGPU_PACKED_RGB10A2) a.cm.outmax = 1023.f;
    } else if (f->layout == XGPU_PACKED_RGB10A2) {
        matrix_coeffs(f->matrix, f->full_range, bd, 10, a.coef, &a.shift, a.fcoef);
        a.maxv = 1023;
    }
}
int xgpu_pic_output_device_packed(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_packed_format *f, const xgpu_colour_transform *cm, void *d_dst,
                                  size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const char *why = "";
    int rc;
    const int bd = c->sp.bit_depth_luma;
    const size_t need = packed_size(f, c->sp.width, c->sp.height, bd, &rc, &why);
    if (need == 0) {
        snprintf(c->err, sizeof(c->err), "pic_output_device_packed: invalid format: %s", why);
        return rc;
    }
    if (cm && !is_packed_rgb(f->layout)) {
        snprintf(c->err, sizeof(c->err), "pic_output_device_packed: a colour transform needs XGPU_PACKED_RGBA or XGPU_PACKED_RGB10A2");
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    TRY(check_dst(c, "pic_output_device_packed", d_dst, dst_size, need, packed_elem_size(f)));
    const xgpu_output_format rf = packed_rgb_format(f);      // (read by the RGB layouts only)
    std::unique_ptr<xgpu_colour_tables_t> cm_new;      // a new set of tables: made here, before anything is queued; uploaded and committed below
    if (cm) TRY(cm_prepare(c, "pic_output_device_packed", &rf, cm, cm_new));
    const int w = c->sp.width - f->crop[0] - f->crop[1], h = c->sp.height - f->crop[2] - f->crop[3];
    // RGBA in a float dtype without a transform: k_output_rgb's own interleaved image in the context's intermediate, then the copy that adds A (k_output_packed.hip
    // says why).  Its rows hold a multiple of 8 pixels and are a multiple of 16 bytes apart, so that the copy loads whole vectors.
    const bool two_pass = f->layout == XGPU_PACKED_RGBA && !cm && f->dtype != XGPU_OUT_U8 && f->dtype != XGPU_OUT_U16;
    const size_t mid_pitch = two_pass ? ((size_t)3 * align8(w) * elem_size(f->dtype) + 15) & ~(size_t)15 : 0;
    if (two_pass) TRY(grow(c, "pic_output_device_packed", &c->sc_mid, &c->sc_mid_cap, mid_pitch * h, "intermediate"));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    TRY(cm_commit(c, cm, cm_new, s));
    auto source_and_rows = [&](RgbOutArgs &a) {
        fill_source(c, pic, f->crop, d_dst, a);
        fill_rows(a, d_dst, packed_row(f, w), h, f->row_pitch);
        fill_siting(f->chroma_loc, a);
    };
    if (is_packed_422(f->layout)) {
        Packed422Args a;
        memset(&a, 0, sizeof(a));
        source_and_rows(a);
        const int obd = packed_depth(f, bd);
        a.cshift = bd - obd; a.out8 = obd == 8; a.cmax = (1 << obd) - 1;      // launch_output's conversion
        a.lsh = f->dtype == XGPU_OUT_U16 ? 16 - obd : 0;
        a.dra = dra ? c->d_dra : NULL;
        launch_output_packed_422(a, f->dtype, f->layout == XGPU_PACKED_UYVY, f->upsample, s);
    } else {
        PackedRgbArgs a;
        memset(&a, 0, sizeof(a));
        source_and_rows(a);
        fill_packed_rgb(c, dra, f, &rf, cm != NULL, a);
        if (two_pass) {
            RgbOutArgs r = a;      // the source, the conversion and the siting; the destination is the intermediate
            r.dst = (uint8_t *)c->sc_mid;
            fill_rows(r, r.dst, image_row(&rf, w), h, mid_pitch);
            launch_output_rgb(r, XGPU_OUT_RGB_INTERLEAVED, f->dtype, f->upsample, s);
            launch_packed_rgba_from_rgb(a, f->dtype, r.dst, mid_pitch, s);
        } else {
            launch_output_packed_rgb(a, f->layout, f->dtype, f->upsample, cm != NULL, s);
        }
    }
    return out_join(c, stream, s);      // the slot, the DRA and the colour tables
}

// ------------------------------------------------------------------------------------------------ 3D LUT output
// The format the plain call's checks see: U16 with out_bit_depth 16 - the 16-bit store only this call has - as out_bit_depth 0, which has the same size.
static xgpu_output_format lut3d_plain_format(const xgpu_output_format *f, bool *full16)
{
    xgpu_output_format g = *f;
    *full16 = is_rgb(f->layout) && f->dtype == XGPU_OUT_U16 && f->out_bit_depth == 16;
    if (*full16) g.out_bit_depth = 0;
    return g;
}
// the refusals of the RGB call up to the layout, without a device: 0 with *need = the bytes at d_dst, or the code and `why`
static int lut3d_rgb_check(const xgpu_output_format *f, int width, int height, int bd, size_t *need, bool *full16, const char **why)
{
    *why = "format is NULL";
    if (!f) return XGPU_ERR_INVALID_ARGUMENT;
    const xgpu_output_format g = lut3d_plain_format(f, full16);
    int rc;
    *need = format_size(&g, width, height, bd, &rc, why);
    if (*need == 0) return rc;
    *why = "a 3D LUT needs one of the RGB layouts";
    return is_rgb(g.layout) ? XGPU_OK : XGPU_ERR_INVALID_ARGUMENT;
}
static int lut3d_packed_check(const xgpu_packed_format *f, int width, int height, int bd, size_t *need, const char **why)
{
    int rc;
    *need = packed_size(f, width, height, bd, &rc, why);
    if (*need == 0) return rc;
    *why = "a 3D LUT needs XGPU_PACKED_RGBA or XGPU_PACKED_RGB10A2";
    return is_packed_rgb(f->layout) ? XGPU_OK : XGPU_ERR_INVALID_ARGUMENT;
}
int xgpu_output_lut3d_check(const xgpu_output_format *f, const xgpu_packed_format *pf, int n, int width, int height, int bit_depth)
{
    if ((f != NULL) == (pf != NULL)) return XGPU_ERR_INVALID_ARGUMENT;
    size_t need; bool full16; const char *why;
    const int rc = f ? lut3d_rgb_check(f, width, height, bit_depth, &need, &full16, &why) : lut3d_packed_check(pf, width, height, bit_depth, &need, &why);
    if (rc < 0) return rc;
    return n >= 2 && n <= 65 ? XGPU_OK : XGPU_ERR_UNSUPPORTED;
}
static const Lut3dSlot *lut3d_slot(xgpu_ctx *c, const char *who, int lut)
{
    if (lut >= 0 && lut < XGPU_MAX_LUT3D && c->lut3d[lut].d) return &c->lut3d[lut];
    snprintf(c->err, sizeof(c->err), "%s: %d names no 3D LUT of this context", who, lut);
    return NULL;
}
// the source, the matrix of the U16 form (the code at the coding depth feeds the shaper, whatever the output dtype), the siting and the LUT; the destination's rows
// are the caller's to fill
static void fill_lut3d(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *rf, const Lut3dSlot &l, void *d_dst, Lut3dOutArgs &a)
{
    memset(&a, 0, sizeof(a));
    fill_source(c, pic, rf->crop, d_dst, a);
    xgpu_output_format f16 = *rf;
    f16.dtype = XGPU_OUT_U16; f16.out_bit_depth = 0; f16.row_pitch = 0;
    fill_conversion(c, dra, &f16, a);      // bgr, range terms, DRA, coef / shift / maxv of the U16 form
    fill_siting(rf->chroma_loc, a);
    a.shaper = (const uint16_t *)l.d;
    a.cube = (const uint2 *)(l.d + lut3d_shaper_bytes(c->sp.bit_depth_luma));
    a.n = l.n;
}
int xgpu_pic_output_device_lut3d(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, int lut, void *d_dst, size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const char *why = "";
    const int bd = c->sp.bit_depth_luma;
    size_t need; bool full16;
    const int rc = lut3d_rgb_check(f, c->sp.width, c->sp.height, bd, &need, &full16, &why);
    if (rc < 0) { snprintf(c->err, sizeof(c->err), "pic_output_device_lut3d: invalid format: %s", why); return rc; }
    const Lut3dSlot *l = lut3d_slot(c, "pic_output_device_lut3d", lut);
    if (!l) return XGPU_ERR_INVALID_ARGUMENT;
    TRY(check_dst(c, "pic_output_device_lut3d", d_dst, dst_size, need, (size_t)elem_size(f->dtype)));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    Lut3dOutArgs a;
    fill_lut3d(c, pic, dra, f, *l, d_dst, a);
    fill_rows(a, d_dst, image_row(f, a.w), a.h, f->row_pitch);
    a.dmax = f->dtype == XGPU_OUT_U8 ? 255u : full16 ? 65535u : (1u << bd) - 1;
    launch_output_lut3d(a, f->layout, f->dtype, f->upsample, s);
    return out_join(c, stream, s);      // the slot, the DRA tables and the LUT
}
int xgpu_pic_output_device_packed_lut3d(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_packed_format *f, int lut, void *d_dst, size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const char *why = "";
    const int bd = c->sp.bit_depth_luma;
    size_t need;
    const int rc = lut3d_packed_check(f, c->sp.width, c->sp.height, bd, &need, &why);
    if (rc < 0) { snprintf(c->err, sizeof(c->err), "pic_output_device_packed_lut3d: invalid format: %s", why); return rc; }
    const Lut3dSlot *l = lut3d_slot(c, "pic_output_device_packed_lut3d", lut);
    if (!l) return XGPU_ERR_INVALID_ARGUMENT;
    TRY(check_dst(c, "pic_output_device_packed_lut3d", d_dst, dst_size, need, packed_elem_size(f)));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    const xgpu_output_format rf = packed_rgb_format(f);
    Lut3dOutArgs a;
    fill_lut3d(c, pic, dra, &rf, *l, d_dst, a);
    fill_rows(a, d_dst, packed_row(f, a.w), a.h, f->row_pitch);
    a.dmax = f->layout == XGPU_PACKED_RGB10A2 ? 1023u : f->dtype == XGPU_OUT_U8 ? 255u : (1u << bd) - 1;
    a.alpha = packed_alpha_code(f, bd);
    launch_output_packed_lut3d(a, f->layout, f->dtype, f->upsample, s);
    return out_join(c, stream, s);      // the slot, the DRA tables and the LUT
}

// ------------------------------------------------------------------------------------------------ dithered output
static bool is_int_dtype(int dtype) { return dtype == XGPU_OUT_U8 || dtype == XGPU_OUT_U16; }
// The refusals that look at the format and the transform alone, in the contract's order: the plain call's with its codes, a float dtype, a layout without a
// dithered form, a transform on a video surface, then the transform's own (as the plain call has them, for the layouts that take one).  0 with *need = the bytes
// at d_dst and *s_bits = S of the matrix path (0: a path without that bound), or the code and `why`.  No device is touched.
static int dither_format_check(const xgpu_output_format *f, const xgpu_packed_format *pf, const xgpu_colour_transform *cm, int width, int height, int bd,
                               size_t *need, int *s_bits, const char **why)
{
    *s_bits = 0;
    if (f) {
        int rc;
        *need = format_size(f, width, height, bd, &rc, why);
        if (*need == 0) return rc;
        *why = "a dithered output needs an integer dtype";
        if (!is_int_dtype(f->dtype)) return XGPU_ERR_UNSUPPORTED;
        *why = "a dithered output needs one of the RGB layouts, NV12 or P016";
        if (!is_rgb(f->layout) && !is_semiplanar(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
        *why = "a colour transform needs one of the RGB layouts";
        if (cm && !is_rgb(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
        if (is_rgb(f->layout) && !cm) *s_bits = 27 - (f->dtype == XGPU_OUT_U8 ? 8 : bd);
    } else {
        int rc;
        *need = packed_size(pf, width, height, bd, &rc, why);
        if (*need == 0) return rc;
        *why = "a dithered output needs an integer dtype";
        if (pf->layout == XGPU_PACKED_RGBA && !is_int_dtype(pf->dtype)) return XGPU_ERR_UNSUPPORTED;
        *why = "a dithered packed output needs XGPU_PACKED_RGBA or XGPU_PACKED_RGB10A2";
        if (!is_packed_rgb(pf->layout)) return XGPU_ERR_INVALID_ARGUMENT;
        if (!cm) *s_bits = 27 - (pf->layout == XGPU_PACKED_RGB10A2 ? 10 : pf->dtype == XGPU_OUT_U8 ? 8 : bd);
    }
    return XGPU_OK;
}
// the last refusal: the matrix itself, and k against S on the matrix path
static int dither_matrix_check(int mw, int mh, int k, int s_bits, const char **why)
{
    *why = "dither matrix: sides are powers of two in 1 .. 128, 1 <= k <= 14, and k <= S on the matrix path";
    auto side_ok = [](int v) { return v >= 1 && v <= 128 && !(v & (v - 1)); };
    return side_ok(mw) && side_ok(mh) && k >= 1 && k <= 14 && (!s_bits || k <= s_bits) ? XGPU_OK : XGPU_ERR_UNSUPPORTED;
}
int xgpu_output_dither_check(const xgpu_output_format *f, const xgpu_packed_format *pf, const xgpu_colour_transform *cm, int mw, int mh, int k, int width,
                             int height, int bit_depth)
{
    if ((f != NULL) == (pf != NULL)) return XGPU_ERR_INVALID_ARGUMENT;
    size_t need; int s_bits; const char *why;
    const int rc = dither_format_check(f, pf, cm, width, height, bit_depth, &need, &s_bits, &why);
    if (rc < 0) return rc;
    if (cm) {
        const xgpu_output_format rf = f ? *f : packed_rgb_format(pf);
        TRY(cm_dry_run(&rf, cm, bit_depth));
    }
    return dither_matrix_check(mw, mh, k, s_bits, &why);
}
// the refusals that look at the call's matrix: the handle, the phase, the matrix against the path; the matrix in `di`
static int dither_prepare(xgpu_ctx *c, const char *who, const xgpu_dither_params *dp, int s_bits, DitherArgs &di)
{
    if (!dp || dp->handle < 0 || dp->handle >= XGPU_MAX_DITHER || !c->dither[dp->handle].d) {
        snprintf(c->err, sizeof(c->err), "%s: %d names no dither matrix of this context", who, dp ? dp->handle : -1);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    const DitherSlot &sl = c->dither[dp->handle];
    if (dp->phase_x < 0 || dp->phase_x >= sl.mw || dp->phase_y < 0 || dp->phase_y >= sl.mh) {
        snprintf(c->err, sizeof(c->err), "%s: phase (%d, %d) lies outside the %d x %d matrix", who, dp->phase_x, dp->phase_y, sl.mw, sl.mh);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    const char *why;
    const int rc = dither_matrix_check(sl.mw, sl.mh, sl.k, s_bits, &why);
    if (rc < 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return rc; }
    di.tab = sl.d; di.stride = sl.mw + 16; di.mwm = sl.mw - 1; di.mhm = sl.mh - 1;
    di.px = dp->phase_x; di.py = dp->phase_y; di.k = sl.k;
    return XGPU_OK;
}
int xgpu_pic_output_device_dithered(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_colour_transform *cm,
                                    const xgpu_dither_params *dp, void *d_dst, size_t dst_size, void *stream)
{
    static const char who[] = "pic_output_device_dithered";
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const char *why = "format is NULL";
    const int bd = c->sp.bit_depth_luma;
    size_t need; int s_bits;
    const int rc = f ? dither_format_check(f, NULL, cm, c->sp.width, c->sp.height, bd, &need, &s_bits, &why) : XGPU_ERR_INVALID_ARGUMENT;
    if (rc < 0) { snprintf(c->err, sizeof(c->err), "%s: invalid format: %s", who, why); return rc; }
    std::unique_ptr<xgpu_colour_tables_t> cm_new;      // a new set of tables: made here, before anything is queued; uploaded and committed below
    if (cm) TRY(cm_prepare(c, who, f, cm, cm_new));
    DitherArgs di;
    TRY(dither_prepare(c, who, dp, s_bits, di));
    const size_t es = (size_t)elem_size(f->dtype);
    TRY(check_dst(c, who, d_dst, dst_size, need, es));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    TRY(cm_commit(c, cm, cm_new, s));
    if (is_semiplanar(f->layout)) {      // xgpu_pic_output_device's arguments, and the matrix
        DitherSemiArgs a;
        memset(&a, 0, sizeof(a));
        fill_semiplanar(c, pic, dra, f, d_dst, a);
        a.di = di;
        launch_output_dither_semiplanar(a, f->dtype, s);
    } else {
        DitherRgbArgs a;
        memset(&a, 0, sizeof(a));
        fill_source(c, pic, f->crop, d_dst, a);
        fill_rows(a, d_dst, image_row(f, a.w), a.h, f->row_pitch);
        fill_conversion(c, dra, f, a);
        fill_siting(f->chroma_loc, a);
        if (cm) fill_cm(c, f, *c->cm_tab, a, a.cm);
        a.di = di;
        launch_output_dither_rgb(a, f->layout == XGPU_OUT_RGB_PLANAR ? OUT_SINK_PLANAR : OUT_SINK_INTERLEAVED, f->dtype, f->upsample, cm != NULL, s);
    }
    return out_join(c, stream, s);      // the slot, the DRA and the colour tables, the matrix
}
int xgpu_pic_output_device_packed_dithered(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_packed_format *f, const xgpu_colour_transform *cm,
                                           const xgpu_dither_params *dp, void *d_dst, size_t dst_size, void *stream)
{
    static const char who[] = "pic_output_device_packed_dithered";
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const char *why = "";
    const int bd = c->sp.bit_depth_luma;
    size_t need; int s_bits;
    const int rc = dither_format_check(NULL, f, cm, c->sp.width, c->sp.height, bd, &need, &s_bits, &why);
    if (rc < 0) { snprintf(c->err, sizeof(c->err), "%s: invalid format: %s", who, why); return rc; }
    const xgpu_output_format rf = packed_rgb_format(f);
    std::unique_ptr<xgpu_colour_tables_t> cm_new;
    if (cm) TRY(cm_prepare(c, who, &rf, cm, cm_new));
    DitherArgs di;
    TRY(dither_prepare(c, who, dp, s_bits, di));
    TRY(check_dst(c, who, d_dst, dst_size, need, packed_elem_size(f)));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    TRY(cm_commit(c, cm, cm_new, s));
    DitherRgbArgs a;
    memset(&a, 0, sizeof(a));
    fill_source(c, pic, f->crop, d_dst, a);
    fill_rows(a, d_dst, packed_row(f, a.w), a.h, f->row_pitch);
    fill_siting(f->chroma_loc, a);
    fill_packed_rgb(c, dra, f, &rf, cm != NULL, a);      // xgpu_pic_output_device_packed's arguments
    a.di = di;
    launch_output_dither_rgb(a, f->layout == XGPU_PACKED_RGBA ? OUT_SINK_RGBA : OUT_SINK_RGB10A2, f->dtype, f->upsample, cm != NULL, s);
    return out_join(c, stream, s);      // the slot, the DRA and the colour tables, the matrix
}

// ------------------------------------------------------------------------------------------------ overlaid output
// The refusals that look at the format and the transform alone, in the contract's order: the plain call's with its codes, a float dtype, a layout without an
// overlaid form, a transform on a video surface, a video surface whose matrix / full_range give no forward matrix.  0 with *need = the bytes at d_dst and
// *maxv = M, or the code and `why`.  No device is touched.
static int overlay_format_check(const xgpu_output_format *f, const xgpu_packed_format *pf, const xgpu_colour_transform *cm, int width, int height, int bd,
                                size_t *need, int *maxv, const char **why)
{
    int rc;
    if (f) {
        *need = format_size(f, width, height, bd, &rc, why);
        if (*need == 0) return rc;
        *why = "an overlaid output needs an integer dtype";
        if (!is_int_dtype(f->dtype)) return XGPU_ERR_UNSUPPORTED;
        *why = "an overlaid output needs one of the RGB layouts, NV12 or P016";
        if (!is_rgb(f->layout) && !is_semiplanar(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
        *why = "a colour transform needs one of the RGB layouts";
        if (cm && !is_rgb(f->layout)) return XGPU_ERR_INVALID_ARGUMENT;
        if (is_semiplanar(f->layout)) {
            double kr, kb;
            *why = "NV12 / P016: full_range must be 0 or 1";
            if (f->full_range & ~1) return XGPU_ERR_INVALID_ARGUMENT;
            *why = "matrix: supported MatrixCoefficients are 1, 4, 5, 6, 7 and 9";
            if (!matrix_kr_kb(f->matrix, &kr, &kb)) return XGPU_ERR_UNSUPPORTED;
            *maxv = (1 << sample_depth(f, bd)) - 1;
        } else {
            *maxv = f->dtype == XGPU_OUT_U8 ? 255 : (1 << bd) - 1;
        }
    } else {
        *need = packed_size(pf, width, height, bd, &rc, why);
        if (*need == 0) return rc;
        *why = "an overlaid output needs an integer dtype";
        if (pf->layout == XGPU_PACKED_RGBA && !is_int_dtype(pf->dtype)) return XGPU_ERR_UNSUPPORTED;
        *why = "an overlaid packed output needs XGPU_PACKED_RGBA or XGPU_PACKED_RGB10A2";
        if (!is_packed_rgb(pf->layout)) return XGPU_ERR_INVALID_ARGUMENT;
        *maxv = pf->layout == XGPU_PACKED_RGB10A2 ? 1023 : pf->dtype == XGPU_OUT_U8 ? 255 : (1 << bd) - 1;
    }
    return XGPU_OK;
}
int xgpu_overlay_coeffs(const xgpu_output_format *f, int bit_depth, int32_t m[9], int32_t offsets[3], int *shift)
{
    const char *why;
    if (bit_depth < 8 || bit_depth > 12 || !m || !offsets || !shift) return XGPU_ERR_INVALID_ARGUMENT;
    const int rc = check_format(f, bit_depth, &why);
    if (rc < 0) return rc;
    if (!is_semiplanar(f->layout) || (f->full_range & ~1)) return XGPU_ERR_INVALID_ARGUMENT;
    double kr, kb;
    if (!matrix_kr_kb(f->matrix, &kr, &kb)) return XGPU_ERR_UNSUPPORTED;
    overlay_forward_matrix(kr, kb, f->full_range, sample_depth(f, bit_depth), m, offsets, shift);
    return XGPU_OK;
}
int xgpu_output_overlay_check(const xgpu_output_format *f, const xgpu_packed_format *pf, const xgpu_colour_transform *cm, const xgpu_overlay_layer *layers,
                              int n_layers, const xgpu_overlay_boxes *boxes, int width, int height, int bit_depth)
{
    if ((f != NULL) == (pf != NULL)) return XGPU_ERR_INVALID_ARGUMENT;
    size_t need; int maxv; const char *why;
    const int rc = overlay_format_check(f, pf, cm, width, height, bit_depth, &need, &maxv, &why);
    if (rc < 0) return rc;
    if (cm) {
        const xgpu_output_format rf = f ? *f : packed_rgb_format(pf);
        TRY(cm_dry_run(&rf, cm, bit_depth));
    }
    return overlay_layers_check(layers, n_layers, boxes, &why);
}
// the refusals that look at the call's layers and boxes: the arguments, then the memory behind every pointer; then the block of the device boxes
static int overlay_prepare(xgpu_ctx *c, const char *who, const xgpu_overlay_layer *layers, int n, const xgpu_overlay_boxes *boxes)
{
    const char *why;
    const int rc = overlay_layers_check(layers, n, boxes, &why);
    if (rc < 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return rc; }
    char what[96];      // which pointer a refusal is about: "<who>: the bitmap of layer 3", "<who>: d_boxes"
    for (int i = 0; i < n; i++)
        if (layers[i].kind != XGPU_OVL_BOX) {
            snprintf(what, sizeof(what), "%s: the bitmap of layer %d", who, i);
            TRY(check_device_dst(c, what, (void *)layers[i].d_pixels, overlay_layer_bytes(layers[i])));
        }
    if (boxes) {
        snprintf(what, sizeof(what), "%s: d_boxes", who);
        TRY(check_device_dst(c, what, (void *)boxes->d_boxes, (size_t)boxes->capacity * 16));
        snprintf(what, sizeof(what), "%s: d_count", who);
        if (boxes->d_count) TRY(check_device_dst(c, what, (void *)boxes->d_count, sizeof(int32_t)));
        snprintf(what, sizeof(what), "%s: d_labels", who);
        if (boxes->d_labels) TRY(check_device_dst(c, what, (void *)boxes->d_labels, (size_t)boxes->capacity * sizeof(int32_t)));
        TRY(grow(c, who, &c->ovl_blk, &c->ovl_blk_cap, sizeof(OvlBlock), "block of the device boxes"));
    }
    return XGPU_OK;
}
// behind the fork: the device boxes into the context's block, on the call's stream; the layers as the kernels read them
static void overlay_queue(xgpu_ctx *c, const xgpu_overlay_layer *layers, int n, const xgpu_overlay_boxes *boxes, int w, int h, int maxv, OvlArgs &o, hipStream_t s)
{
    if (boxes) {
        OvlPrepArgs p;
        overlay_fill_prepare(boxes, (OvlBlock *)c->ovl_blk, w, h, p);
        launch_overlay_prepare(p, s);
    }
    overlay_fill_args(layers, n, boxes, (const OvlBlock *)c->ovl_blk, maxv, o);
}
int xgpu_pic_output_device_overlaid(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_colour_transform *cm,
                                    const xgpu_overlay_layer *layers, int n_layers, const xgpu_overlay_boxes *boxes, void *d_dst, size_t dst_size, void *stream)
{
    static const char who[] = "pic_output_device_overlaid";
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const char *why = "format is NULL";
    const int bd = c->sp.bit_depth_luma;
    size_t need; int maxv;
    const int rc = f ? overlay_format_check(f, NULL, cm, c->sp.width, c->sp.height, bd, &need, &maxv, &why) : XGPU_ERR_INVALID_ARGUMENT;
    if (rc < 0) { snprintf(c->err, sizeof(c->err), "%s: invalid format: %s", who, why); return rc; }
    std::unique_ptr<xgpu_colour_tables_t> cm_new;      // a new set of tables: made here, before anything is queued; uploaded and committed below
    if (cm) TRY(cm_prepare(c, who, f, cm, cm_new));
    TRY(overlay_prepare(c, who, layers, n_layers, boxes));
    TRY(check_dst(c, who, d_dst, dst_size, need, (size_t)elem_size(f->dtype)));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    TRY(cm_commit(c, cm, cm_new, s));
    if (is_semiplanar(f->layout)) {      // xgpu_pic_output_device's arguments, and the layers
        OverlaySemiArgs a;
        memset(&a, 0, sizeof(a));
        fill_semiplanar(c, pic, dra, f, d_dst, a);
        overlay_queue(c, layers, n_layers, boxes, a.w, 2 * a.ch, maxv, a.ov, s);
        double kr, kb;
        matrix_kr_kb(f->matrix, &kr, &kb);
        overlay_forward_matrix(kr, kb, f->full_range, sample_depth(f, bd), a.ov.m, a.ov.off, &a.ov.s);
        launch_output_overlay_semiplanar(a, f->dtype, s);
    } else {
        OverlayRgbArgs a;
        memset(&a, 0, sizeof(a));
        fill_source(c, pic, f->crop, d_dst, a);
        fill_rows(a, d_dst, image_row(f, a.w), a.h, f->row_pitch);
        fill_conversion(c, dra, f, a);
        fill_siting(f->chroma_loc, a);
        if (cm) fill_cm(c, f, *c->cm_tab, a, a.cm);
        overlay_queue(c, layers, n_layers, boxes, a.w, a.h, maxv, a.ov, s);
        launch_output_overlay_rgb(a, f->layout == XGPU_OUT_RGB_PLANAR ? OUT_SINK_PLANAR : OUT_SINK_INTERLEAVED, f->dtype, f->upsample, cm != NULL, s);
    }
    return out_join(c, stream, s);      // the slot, the DRA and the colour tables, the block of the device boxes
}
int xgpu_pic_output_device_packed_overlaid(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_packed_format *f, const xgpu_colour_transform *cm,
                                           const xgpu_overlay_layer *layers, int n_layers, const xgpu_overlay_boxes *boxes, void *d_dst, size_t dst_size,
                                           void *stream)
{
    static const char who[] = "pic_output_device_packed_overlaid";
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    const char *why = "";
    const int bd = c->sp.bit_depth_luma;
    size_t need; int maxv;
    const int rc = overlay_format_check(NULL, f, cm, c->sp.width, c->sp.height, bd, &need, &maxv, &why);
    if (rc < 0) { snprintf(c->err, sizeof(c->err), "%s: invalid format: %s", who, why); return rc; }
    const xgpu_output_format rf = packed_rgb_format(f);
    std::unique_ptr<xgpu_colour_tables_t> cm_new;
    if (cm) TRY(cm_prepare(c, who, &rf, cm, cm_new));
    TRY(overlay_prepare(c, who, layers, n_layers, boxes));
    TRY(check_dst(c, who, d_dst, dst_size, need, packed_elem_size(f)));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    TRY(cm_commit(c, cm, cm_new, s));
    OverlayRgbArgs a;
    memset(&a, 0, sizeof(a));
    fill_source(c, pic, f->crop, d_dst, a);
    fill_rows(a, d_dst, packed_row(f, a.w), a.h, f->row_pitch);
    fill_siting(f->chroma_loc, a);
    fill_packed_rgb(c, dra, f, &rf, cm != NULL, a);      // xgpu_pic_output_device_packed's arguments
    overlay_queue(c, layers, n_layers, boxes, a.w, a.h, maxv, a.ov, s);
    launch_output_overlay_rgb(a, f->layout == XGPU_PACKED_RGBA ? OUT_SINK_RGBA : OUT_SINK_RGB10A2, f->dtype, f->upsample, cm != NULL, s);
    return out_join(c, stream, s);      // the slot, the DRA and the colour tables, the block of the device boxes
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
    if (!crop_ok(f->crop, width, height, why)) return false;
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
    const size_t bytes = rows_of(image_row(f, sc->width), image_rows(f, sc->height), f->row_pitch).total;
    *why = "row_pitch is shorter than a row";
    *rc = bytes ? XGPU_OK : XGPU_ERR_INVALID_ARGUMENT;
    return bytes;
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
    cropped_planes(p, f->crop, &a.y, &a.u, &a.v);
    a.sy = p.s_l; a.sc = p.s_c;
    a.dw = sc->width; a.dh = sc->height;
    a.dst = (uint8_t *)d_dst;
    fill_rows(a, d_dst, image_row(f, sc->width), sc->height, f->row_pitch);      // (`aligned` is not read: the scaled kernels store element by element)
    fill_conversion(c, dra, f, a);
    a.smax = (1 << c->sp.bit_depth_luma) - 1;
    a.normalize = sc->normalize;
    for (int k = 0; k < 3; k++) { a.mean[k] = sc->mean[k]; a.inv_std[k] = sc->inv_std[k]; }
}
static int output_scaled(xgpu_ctx *c, const char *who, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                         const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream, bool lin = false);
int xgpu_pic_output_device_scaled(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, void *d_dst, size_t dst_size, void *stream)
{
    return output_scaled(c, "pic_output_device_scaled", pic, dra, f, sc, NULL, d_dst, dst_size, stream);
}
int xgpu_pic_output_device_scaled_cm(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_colour_transform *cm,
                                     void *d_dst, size_t dst_size, void *stream)
{
    return output_scaled(c, "pic_output_device_scaled_cm", pic, dra, f, sc, cm, d_dst, dst_size, stream);
}
// the plain call's checks and codes first, then the layout and the transform (cm_prepare's order)
int xgpu_output_scaled_cm_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_colour_transform *cm, int width, int height, int bit_depth)
{
    const int rc = xgpu_output_scaled_check(f, sc, width, height, bit_depth);
    if (rc < 0 || !cm) return rc;
    return cm_dry_run(f, cm, bit_depth);
}
// the linear-light form's own refusals behind the plain call's (section 8n), without a device: the float32 intermediate, then a transform that is missing
static const size_t ROIS_MID_LIMIT = (size_t)512 << 20;
// the bytes of the intermediate of a ws-wide source with `rows` destination rows: 16-bit Y, Cb, Cr rows, or (lin) float32 R, G, B rows at luma width
static size_t intermediate_bytes(int ws, int rows, bool lin)
{
    return lin ? (size_t)3 * rows * align8(ws) * sizeof(float) : (size_t)rows * mid_row_samples(ws) * sizeof(uint16_t);
}
static int scaled_lin_refusal(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_colour_transform *cm, int width, const char **why)
{
    *why = "the float32 intermediate of the call passes 512 MiB";
    if (intermediate_bytes(width - f->crop[0] - f->crop[1], sc->height, true) > ROIS_MID_LIMIT) return XGPU_ERR_UNSUPPORTED;
    *why = "filtering in linear light needs a colour transform";
    return cm ? XGPU_OK : XGPU_ERR_INVALID_ARGUMENT;
}
int xgpu_pic_output_device_scaled_lin(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_colour_transform *cm,
                                      void *d_dst, size_t dst_size, void *stream)
{
    return output_scaled(c, "pic_output_device_scaled_lin", pic, dra, f, sc, cm, d_dst, dst_size, stream, true);
}
// the plain call's checks and codes first, then the intermediate, the missing transform, the layout and the transform (cm_prepare's order)
int xgpu_output_scaled_lin_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_colour_transform *cm, int width, int height, int bit_depth)
{
    int rc = xgpu_output_scaled_check(f, sc, width, height, bit_depth);
    if (rc < 0) return rc;
    const char *why;
    if ((rc = scaled_lin_refusal(f, sc, cm, width, &why)) < 0) return rc;
    return xgpu_output_scaled_cm_check(f, sc, cm, width, height, bit_depth);
}
static int output_scaled(xgpu_ctx *c, const char *who, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc,
                         const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream, bool lin)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    int src_rc; const char *why = "";
    const size_t need = scaled_size(f, sc, c->sp.width, c->sp.height, c->sp.bit_depth_luma, &src_rc, &why);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return src_rc; }
    if (lin && (src_rc = scaled_lin_refusal(f, sc, cm, c->sp.width, &why)) < 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return src_rc; }
    TRY(check_dst_fits(c, who, d_dst, dst_size, need, elem_size(f->dtype)));
    if (dra) TRY(check_dra(c, dra));      // upload_dra's refusals, before anything is queued
    TRY(check_device_dst(c, who, d_dst, need));
    const int *cr = f->crop;
    const int ws = c->sp.width - cr[0] - cr[1], hs = c->sp.height - cr[2] - cr[3], wd = sc->width, hd = sc->height;
    // the tap tables: made here, before anything is queued; uploaded and committed below (the protocol of the colour transform's tables)
    const int key[6] = { ws, hs, wd, hd, sc->filter, f->chroma_loc };
    const bool cached = c->sc_tab && !memcmp(key, c->sc_key, sizeof(key));
    std::vector<uint8_t> blob;
    ScaleTabs tb = c->sc_host;
    if (!cached) {
        const int rc = scale_build_tables(ws, hs, wd, hd, sc->filter, f->chroma_loc, blob, tb);
        if (rc < 0) { snprintf(c->err, sizeof(c->err), "%s: cannot make the tap tables for %dx%d -> %dx%d", who, ws, hs, wd, hd); return rc; }
    }
    if (lin && (size_t)3 * tb.capy * sizeof(float) > LIN_LDS_LIMIT) { snprintf(c->err, sizeof(c->err), "%s: a row's spans pass the LDS of one launch", who); return XGPU_ERR_UNEXPECTED; }
    TRY(grow(c, who, &c->sc_mid, &c->sc_mid_cap, intermediate_bytes(ws, hd, lin), "intermediate"));
    if (!cached && c->sc_tab_cap < blob.size()) {
        c->sc_key[0] = -1;      // no key names a block that is freed
        TRY(grow(c, who, &c->sc_tab, &c->sc_tab_cap, blob.size(), "block of tap tables"));
    }
    std::unique_ptr<xgpu_colour_tables_t> cm_new;
    if (cm) TRY(cm_prepare(c, who, f, cm, cm_new));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    TRY(cm_commit(c, cm, cm_new, s));
    if (!cached) {      // behind the fork: after every kernel that read the previous tables
        c->sc_key[0] = -1;      // sc_tab is about to change: no key names it until the new block is queued
        HIPCHK(c, hipMemcpyAsync(c->sc_tab, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
        memcpy(c->sc_key, key, sizeof(key));
        c->sc_host = tb;
    }
    ScaledCmOutArgs a;
    memset(&a, 0, sizeof(a));
    scaled_common_args(c, pic, dra, f, sc, d_dst, a);
    a.w = ws; a.h = hs; a.cw = ws >> 1; a.ch = hs >> 1;
    ScaleTaps *taps[4] = { &a.yl, &a.yc, &a.xl, &a.xc };
    for (int t = 0; t < 4; t++) {
        taps[t]->first = (const int32_t *)(c->sc_tab + tb.off_first[t]); taps[t]->count = (const int32_t *)(c->sc_tab + tb.off_count[t]);
        taps[t]->w = (const int16_t *)(c->sc_tab + tb.off_w[t]); taps[t]->stride = tb.stride[t];
    }
    a.mid = c->sc_mid; a.mpy = align8(ws); a.mpc = align8(ws >> 1);
    a.capy = tb.capy; a.capc = tb.capc;
    if (lin) {
        fill_siting(f->chroma_loc, a);
        fill_cm(c, f, *c->cm_tab, a, a.cm);
        launch_output_scaled_lin(a, f->layout, f->dtype, f->upsample, s);
    } else if (cm) {
        fill_cm(c, f, *c->cm_tab, a, a.cm);
        launch_output_scaled_cm(a, f->layout, f->dtype, s);
    } else {
        launch_output_scaled(a, f->layout, f->dtype, s);
    }
    return out_join(c, stream, s);      // the slot, the DRA, colour and tap tables, the intermediate
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
    if (rp->image_pitch && (rp->image_pitch % es || rp->image_pitch < image)) {
        snprintf(why, 160, "image_pitch %zu: 0, or a multiple of the %zu-byte element not below the %zu bytes of one image", rp->image_pitch, es, image);
        return 0;
    }
    return rp->image_pitch ? rp->image_pitch : image_rows(f, sc->height) * rows_of(image_row(f, sc->width), 1, f->row_pitch).pitch;      // tight: every row a pitch
}
// The whole of a call's argument checks, without a device: the bytes the destination needs, or 0 with *rc = the code, `why` (a buffer of 160 bytes) and *bad =
// the rectangle it names (-1: none).  image_pitch / mid_bytes (may be NULL): the bytes between two images, and the intermediate of the call - the sum over the
// rectangles of intermediate_bytes(Ws, Hi, lin) (lin: the form filtered in linear light).
static size_t rois_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi *rois, int n, int width, int height, int bd,
                        int *rc, char *why, int *bad, size_t *image_pitch, size_t *mid_bytes, bool lin = false)
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
        mid += intermediate_bytes(r.width, in[3], lin);
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
// The descriptor block of a call, made on the host: n records (image i lies i * image_pitch bytes into the destination, its intermediate behind those of the
// rectangles before it), then one set of tap tables per distinct (source size, inner size).  capy / capc: the widest spans of all sets; max_w / max_ih: the widest
// rectangle and the tallest inner part, which size the launch.
struct RoiBlock { std::vector<uint8_t> blk; int capy, capc, max_w, max_ih; };
static int build_roi_block(xgpu_ctx *c, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi *rois, int n, size_t image_pitch,
                           RoiBlock &b, bool lin = false,      // lin: the float32 intermediate of section 8n - RoiDesc::mid counts floats
                           const xgpu_resample_params *rs = NULL)      // the bicubic tables of section 8o instead of sc->filter's
{
    struct Set { int ws, hs, wi, hi; ScaleTabs tb; size_t base; };
    std::vector<Set> sets;
    std::vector<uint8_t> blob;
    b.blk.assign((size_t)n * sizeof(RoiDesc), 0);
    b.capy = b.capc = b.max_w = b.max_ih = 0;
    size_t mid = 0;
    for (int i = 0; i < n; i++) {
        const xgpu_roi &r = rois[i];
        int in[4];
        roi_inner(r.width, r.height, sc->width, sc->height, rp->fit, in);
        size_t k = 0;
        while (k < sets.size() && !(sets[k].ws == r.width && sets[k].hs == r.height && sets[k].wi == in[2] && sets[k].hi == in[3])) k++;
        if (k == sets.size()) {
            Set st = { r.width, r.height, in[2], in[3], {}, (b.blk.size() + 15) & ~(size_t)15 };
            const int rc = rs ? resample_build_tables(r.width, r.height, in[2], in[3], rs->kernel, rs->antialias, f->chroma_loc, blob, st.tb, in[0])
                              : scale_build_tables(r.width, r.height, in[2], in[3], sc->filter, f->chroma_loc, blob, st.tb, in[0]);
            if (rc < 0) { snprintf(c->err, sizeof(c->err), "pic_output_device_rois: roi %d: cannot make the tap tables for %dx%d -> %dx%d", i, r.width, r.height, in[2], in[3]); return rc; }
            if (st.base + blob.size() > 0xFFFFFFFFu) { snprintf(c->err, sizeof(c->err), "pic_output_device_rois: roi %d: the tap tables of the call pass 4 GiB here", i); return XGPU_ERR_UNSUPPORTED; }
            b.blk.resize(st.base + blob.size());
            memcpy(&b.blk[st.base], blob.data(), blob.size());
            sets.push_back(st);
        }
        const Set &st = sets[k];
        RoiDesc d;
        memset(&d, 0, sizeof(d));
        d.dst = (uint64_t)i * image_pitch;
        d.x = r.x; d.y = r.y; d.w = r.width; d.h = r.height;
        d.ix = in[0]; d.iy = in[1]; d.iw = in[2]; d.ih = in[3];
        d.mid = (uint32_t)(mid / (lin ? sizeof(float) : sizeof(uint16_t)));
        d.mpy = align8(r.width); d.mpc = align8(r.width >> 1);
        mid += intermediate_bytes(r.width, in[3], lin);
        for (int t = 0; t < 4; t++) {
            d.first[t] = (uint32_t)(st.base + st.tb.off_first[t]); d.count[t] = (uint32_t)(st.base + st.tb.off_count[t]); d.wt[t] = (uint32_t)(st.base + st.tb.off_w[t]);
            d.stride[t] = st.tb.stride[t];
        }
        memcpy(&b.blk[(size_t)i * sizeof(RoiDesc)], &d, sizeof(d));
        b.capy = std::max(b.capy, st.tb.capy); b.capc = std::max(b.capc, st.tb.capc);
        b.max_w = std::max(b.max_w, r.width); b.max_ih = std::max(b.max_ih, in[3]);
    }
    return XGPU_OK;
}
// the batch's fields of the kernels' arguments: the intermediate, the widest spans, the block (on the device at `blk`), the pad value of a letterboxed call
static void batch_args(xgpu_ctx *c, const RoiBlock &b, const uint8_t *blk, int n, const xgpu_roi_params *rp, RoisOutArgs &a)
{
    a.mid = c->sc_mid;
    a.capy = b.capy; a.capc = b.capc;
    a.blk = blk; a.n = n;
    for (int k = 0; k < 3; k++) a.padv[k] = rp->fit == XGPU_FIT_LETTERBOX ? rp->pad[k] : 0.f;
}
static int output_rois(xgpu_ctx *c, const char *who, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp,
                       const xgpu_roi *rois, int n, const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream, bool lin = false);
int xgpu_pic_output_device_rois(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp,
                                const xgpu_roi *rois, int n, void *d_dst, size_t dst_size, void *stream)
{
    return output_rois(c, "pic_output_device_rois", pic, dra, f, sc, rp, rois, n, NULL, d_dst, dst_size, stream);
}
int xgpu_pic_output_device_rois_cm(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp,
                                   const xgpu_roi *rois, int n, const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream)
{
    return output_rois(c, "pic_output_device_rois_cm", pic, dra, f, sc, rp, rois, n, cm, d_dst, dst_size, stream);
}
int xgpu_pic_output_device_rois_lin(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp,
                                    const xgpu_roi *rois, int n, const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream)
{
    return output_rois(c, "pic_output_device_rois_lin", pic, dra, f, sc, rp, rois, n, cm, d_dst, dst_size, stream, true);
}
// the plain batch's checks with the float32 intermediate in its 512 MiB rule (*bad_index as xgpu_output_rois_check sets it), then the single call's order
int xgpu_output_rois_lin_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois,
                               const xgpu_colour_transform *cm, int width, int height, int bit_depth, int *bad_index)
{
    int rc, bad; char why[160];
    (void)rois_size(f, sc, rp, rois, n_rois, width, height, bit_depth, &rc, why, &bad, NULL, NULL, true);
    if (bad_index) *bad_index = bad;
    if (rc < 0) return rc;
    return cm ? cm_dry_run(f, cm, bit_depth) : XGPU_ERR_INVALID_ARGUMENT;
}
static int output_rois(xgpu_ctx *c, const char *who, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_roi_params *rp,
                       const xgpu_roi *rois, int n, const xgpu_colour_transform *cm, void *d_dst, size_t dst_size, void *stream, bool lin)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    int src_rc, bad; char why[160];
    size_t image_pitch = 0, mid_need = 0;
    const size_t need = rois_size(f, sc, rp, rois, n, c->sp.width, c->sp.height, c->sp.bit_depth_luma, &src_rc, why, &bad, &image_pitch, &mid_need, lin);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return src_rc; }
    if (lin && !cm) { snprintf(c->err, sizeof(c->err), "%s: filtering in linear light needs a colour transform", who); return XGPU_ERR_INVALID_ARGUMENT; }
    TRY(check_dst_fits(c, who, d_dst, dst_size, need, elem_size(f->dtype)));
    if (dra) TRY(check_dra(c, dra));      // upload_dra's refusals, before anything is queued
    TRY(check_device_dst(c, who, d_dst, need));
    RoiBlock b;      // made here, before anything is queued
    TRY(build_roi_block(c, f, sc, rp, rois, n, image_pitch, b, lin));
    if (lin && (size_t)3 * b.capy * sizeof(float) > LIN_LDS_LIMIT) { snprintf(c->err, sizeof(c->err), "%s: a row's spans pass the LDS of one launch", who); return XGPU_ERR_UNEXPECTED; }
    TRY(grow(c, who, &c->sc_mid, &c->sc_mid_cap, mid_need, "intermediate"));
    TRY(grow(c, who, &c->roi_blk, &c->roi_blk_cap, b.blk.size(), "descriptor block", b.blk.size() / 2));      // some room: a batch of boxes changes its tables' size from call to call
    std::unique_ptr<xgpu_colour_tables_t> cm_new;
    if (cm) TRY(cm_prepare(c, who, f, cm, cm_new));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    TRY(cm_commit(c, cm, cm_new, s));
    // behind the fork: after every kernel that read the previous block.  (Pageable host memory: staged before the call returns, as the DRA tables are.)
    HIPCHK(c, hipMemcpyAsync(c->roi_blk, b.blk.data(), b.blk.size(), hipMemcpyHostToDevice, s));
    RoisCmOutArgs a;
    memset(&a, 0, sizeof(a));
    scaled_common_args(c, pic, dra, f, sc, d_dst, a);
    batch_args(c, b, c->roi_blk, n, rp, a);
    if (lin) {
        fill_siting(f->chroma_loc, a);
        fill_cm(c, f, *c->cm_tab, a, a.cm);
        launch_output_rois_lin(a, f->layout, f->dtype, f->upsample, b.max_w, b.max_ih, s);
    } else if (cm) {
        fill_cm(c, f, *c->cm_tab, a, a.cm);
        launch_output_rois_cm(a, f->layout, f->dtype, b.max_w, b.max_ih, s);
    } else {
        launch_output_rois(a, f->layout, f->dtype, b.max_w, b.max_ih, s);
    }
    return out_join(c, stream, s);      // the slot, the DRA and colour tables, the block and the intermediate
}

// ------------------------------------------------------------------------------------------------ bicubic resize of the two outputs above
// Everything but the two passes is the scaled output's, so the checks are its checks on the same shape: rs as xgpu_scale_params (the filter is not read by what
// runs behind this), or false for rs = NULL, an unknown kernel or an antialias that is not 0 / 1
static bool resample_as_scale(const xgpu_resample_params *rs, xgpu_scale_params *sc)
{
    if (!rs || rs->kernel < XGPU_RESAMPLE_CATMULL_ROM || rs->kernel > XGPU_RESAMPLE_MITCHELL || (rs->antialias & ~1)) return false;
    sc->width = rs->width; sc->height = rs->height; sc->filter = XGPU_SCALE_BILINEAR; sc->normalize = rs->normalize;
    for (int k = 0; k < 3; k++) { sc->mean[k] = rs->mean[k]; sc->inv_std[k] = rs->inv_std[k]; }
    return true;
}
size_t xgpu_output_resampled_size(const xgpu_output_format *f, const xgpu_resample_params *rs, int width, int height, int bit_depth)
{
    xgpu_scale_params sc;
    return resample_as_scale(rs, &sc) ? xgpu_output_scaled_size(f, &sc, width, height, bit_depth) : 0;
}
int xgpu_output_resampled_check(const xgpu_output_format *f, const xgpu_resample_params *rs, int width, int height, int bit_depth)
{
    xgpu_scale_params sc;
    return resample_as_scale(rs, &sc) ? xgpu_output_scaled_check(f, &sc, width, height, bit_depth) : XGPU_ERR_INVALID_ARGUMENT;
}
int xgpu_output_rois_resampled_check(const xgpu_output_format *f, const xgpu_resample_params *rs, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois,
                                     int width, int height, int bit_depth, int *bad_index)
{
    xgpu_scale_params sc;
    if (bad_index) *bad_index = -1;
    return resample_as_scale(rs, &sc) ? xgpu_output_rois_check(f, &sc, rp, rois, n_rois, width, height, bit_depth, bad_index) : XGPU_ERR_INVALID_ARGUMENT;
}
size_t xgpu_output_rois_resampled_size(const xgpu_output_format *f, const xgpu_resample_params *rs, const xgpu_roi_params *rp, const xgpu_roi *rois, int n_rois,
                                       int width, int height, int bit_depth)
{
    xgpu_scale_params sc;
    return resample_as_scale(rs, &sc) ? xgpu_output_rois_size(f, &sc, rp, rois, n_rois, width, height, bit_depth) : 0;
}
// Both calls.  batch = false: the single picture - the batch of one stretched rectangle, the picture minus f->crop -, whose block depends on nothing but
// rs_key = (source size, destination size, kernel, antialias, chroma_loc) and stays on the device (rs_blk) until another key comes; a batch's block is made per
// call and goes to roi_blk, as xgpu_pic_output_device_rois' does.  The intermediate is sc_mid.
static int output_resampled(xgpu_ctx *c, const char *who, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_resample_params *rs,
                            bool batch, const xgpu_roi_params *rp, const xgpu_roi *rois, int n, void *d_dst, size_t dst_size, void *stream)
{
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL);
    xgpu_scale_params sc;
    if (!resample_as_scale(rs, &sc)) {
        snprintf(c->err, sizeof(c->err), "%s: resample parameters: not NULL, kernel XGPU_RESAMPLE_CATMULL_ROM / _CUBIC_075 / _MITCHELL, antialias 0 or 1", who);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    int src_rc, bad; char why[160];
    size_t image_pitch = 0, mid_need = 0, need;
    if (batch) {
        need = rois_size(f, &sc, rp, rois, n, c->sp.width, c->sp.height, c->sp.bit_depth_luma, &src_rc, why, &bad, &image_pitch, &mid_need);
    } else {
        const char *w0 = "";
        need = scaled_size(f, &sc, c->sp.width, c->sp.height, c->sp.bit_depth_luma, &src_rc, &w0);
        snprintf(why, sizeof(why), "%s", w0);
    }
    if (need == 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return src_rc; }
    TRY(check_dst_fits(c, who, d_dst, dst_size, need, elem_size(f->dtype)));
    if (dra) TRY(check_dra(c, dra));      // upload_dra's refusals, before anything is queued
    TRY(check_device_dst(c, who, d_dst, need));
    const xgpu_roi whole = { 0, 0, c->sp.width - f->crop[0] - f->crop[1], c->sp.height - f->crop[2] - f->crop[3] };
    const xgpu_roi_params stretch = { XGPU_FIT_STRETCH, { 0.f, 0.f, 0.f }, 0 };
    if (!batch) { rp = &stretch; rois = &whole; n = 1; mid_need = intermediate_bytes(whole.width, sc.height, false); }
    const int key[7] = { whole.width, whole.height, sc.width, sc.height, rs->kernel, rs->antialias, f->chroma_loc };
    const bool cached = !batch && c->rs_blk && !memcmp(key, c->rs_key, sizeof(key));
    RoiBlock b;      // made here, before anything is queued
    if (cached) { b.capy = c->rs_capy; b.capc = c->rs_capc; b.max_w = whole.width; b.max_ih = sc.height; }
    else TRY(build_roi_block(c, f, &sc, rp, rois, n, image_pitch, b, false, rs));
    TRY(grow(c, who, &c->sc_mid, &c->sc_mid_cap, mid_need, "intermediate"));
    if (batch) {
        TRY(grow(c, who, &c->roi_blk, &c->roi_blk_cap, b.blk.size(), "descriptor block", b.blk.size() / 2));
    } else if (!cached && c->rs_blk_cap < b.blk.size()) {
        c->rs_key[0] = -1;      // no key names a block that is freed
        TRY(grow(c, who, &c->rs_blk, &c->rs_blk_cap, b.blk.size(), "block of tap tables"));
    }
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    uint8_t *blk = batch ? c->roi_blk : c->rs_blk;
    if (!cached) {      // behind the fork: after every kernel that read the previous block
        if (!batch) c->rs_key[0] = -1;      // rs_blk is about to change: no key names it until the new block is queued
        HIPCHK(c, hipMemcpyAsync(blk, b.blk.data(), b.blk.size(), hipMemcpyHostToDevice, s));
        if (!batch) { memcpy(c->rs_key, key, sizeof(key)); c->rs_capy = b.capy; c->rs_capc = b.capc; }
    }
    RoisOutArgs a;
    memset(&a, 0, sizeof(a));
    scaled_common_args(c, pic, dra, f, &sc, d_dst, a);
    batch_args(c, b, blk, n, rp, a);
    launch_output_resampled(a, f->layout, f->dtype, b.max_w, b.max_ih, s);
    return out_join(c, stream, s);      // the slot, the DRA tables, the block and the intermediate
}
int xgpu_pic_output_device_resampled(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_resample_params *rs, void *d_dst, size_t dst_size,
                                     void *stream)
{
    return output_resampled(c, "pic_output_device_resampled", pic, dra, f, rs, false, NULL, NULL, 0, d_dst, dst_size, stream);
}
int xgpu_pic_output_device_rois_resampled(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_resample_params *rs, const xgpu_roi_params *rp,
                                          const xgpu_roi *rois, int n, void *d_dst, size_t dst_size, void *stream)
{
    return output_resampled(c, "pic_output_device_rois_resampled", pic, dra, f, rs, true, rp, rois, n, d_dst, dst_size, stream);
}

// ------------------------------------------------------------------------------------------------ scaled video surfaces: a ladder of renditions
// ChromaSampleLocType -> the chroma grid's siting in half luma samples, horizontally and vertically (xgpu_scale_taps' siting_half_luma)
static void chroma_siting(int loc, int *dx, int *dy)
{
    static const int vsite[3] = { 1, 0, 2 };      // ChromaSampleLocType >> 1: centred, top, bottom
    *dx = loc & 1; *dy = vsite[loc >> 1];
}
static bool is_surface420(int layout) { return layout == XGPU_OUT_YUV420P || is_semiplanar(layout); }
// the bytes of one rung: xgpu_output_format_size of its layout at the rung's size with the rung's pitch, no crop
static size_t ladder_rung_size(const xgpu_output_format *f, int rw, int rh, size_t row_pitch, int bd, const char **why)
{
    *why = "format is NULL";
    if (!f) return 0;
    *why = "ladder: layout must be XGPU_OUT_YUV420P, XGPU_OUT_NV12 or XGPU_OUT_P016, bgr 0";
    if (!is_surface420(f->layout) || f->bgr) return 0;
    xgpu_output_format g = *f;
    g.row_pitch = row_pitch;
    for (int i = 0; i < 4; i++) g.crop[i] = 0;
    int rc;
    return format_size(&g, rw, rh, bd, &rc, why);
}
size_t xgpu_output_ladder_rung_size(const xgpu_output_format *f, int rung_width, int rung_height, size_t row_pitch, int bit_depth)
{
    const char *why;
    return ladder_rung_size(f, rung_width, rung_height, row_pitch, bit_depth, &why);
}
// the samples of one rung's intermediate for a source ws wide: hd luma rows, hd / 2 rows of either chroma plane
static size_t ladder_mid_samples(int ws, int hd) { return (size_t)hd * align8(ws) + 2 * (size_t)(hd >> 1) * align8(ws >> 1); }
// The whole of a call's argument checks but for the pointers, without a device: *rc = the code, `why` (160 bytes), *mid_bytes (may be NULL) the call's intermediate
static bool ladder_ok(const xgpu_output_format *f, const xgpu_ladder_params *lp, const xgpu_surface_rung *rungs, int n, int width, int height, int bd, int *rc, char *why,
                      size_t *mid_bytes)
{
    const char *w0 = "";
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    if (!f || !lp || !rungs) { snprintf(why, 160, "format, ladder parameters or rungs are NULL"); return false; }
    if (width <= 0 || height <= 0 || ((width | height) & 1) || bd < 8 || bd > 12) { snprintf(why, 160, "picture size or bit depth out of range"); return false; }
    if (!is_surface420(f->layout) || f->bgr) { snprintf(why, 160, "layout must be XGPU_OUT_YUV420P, XGPU_OUT_NV12 or XGPU_OUT_P016, bgr 0"); return false; }
    if (!crop_ok(f->crop, width, height, &w0)) { snprintf(why, 160, "%s", w0); return false; }
    if (f->chroma_loc < 0 || f->chroma_loc > 5 || lp->dst_chroma_loc < -1 || lp->dst_chroma_loc > 5) { snprintf(why, 160, "chroma_loc 0..5, dst_chroma_loc -1..5"); return false; }
    if (lp->filter != XGPU_SCALE_BILINEAR && lp->filter != XGPU_SCALE_AREA) { snprintf(why, 160, "filter must be XGPU_SCALE_BILINEAR or XGPU_SCALE_AREA"); return false; }
    if (n < 1 || n > XGPU_MAX_RUNGS) { snprintf(why, 160, "n %d outside 1..%d", n, XGPU_MAX_RUNGS); return false; }
    const int ws = width - f->crop[0] - f->crop[1], hs = height - f->crop[2] - f->crop[3];
    size_t mid = 0;
    for (int i = 0; i < n; i++) {
        const xgpu_surface_rung &r = rungs[i];
        *rc = XGPU_ERR_INVALID_ARGUMENT;
        if ((r.width | r.height) & 1) { snprintf(why, 160, "rung %d: %d x %d is not even", i, r.width, r.height); return false; }
        *rc = XGPU_ERR_UNSUPPORTED;
        if (r.width < 2 || r.width > 16384 || r.height < 2 || r.height > 16384 || !scale_ratio_ok(ws, r.width) || !scale_ratio_ok(hs, r.height)) {
            snprintf(why, 160, "rung %d: %d x %d from %d x %d: 2..16384 per axis, between 1/64 and 8 times the source's", i, r.width, r.height, ws, hs);
            return false;
        }
        *rc = XGPU_ERR_INVALID_ARGUMENT;
        const size_t need = ladder_rung_size(f, r.width, r.height, r.row_pitch, bd, &w0);
        if (need == 0) { snprintf(why, 160, "rung %d: %s", i, w0); return false; }
        if (r.dst_size < need) { snprintf(why, 160, "rung %d: destination of %zu bytes, the rung needs %zu", i, r.dst_size, need); return false; }
        *rc = XGPU_ERR_UNSUPPORTED;
        mid += ladder_mid_samples(ws, r.height) * sizeof(uint16_t);
        if (mid > ROIS_MID_LIMIT) { snprintf(why, 160, "rung %d: the intermediate of the call passes 512 MiB here", i); return false; }
    }
    if (mid_bytes) *mid_bytes = mid;
    *rc = XGPU_OK;
    return true;
}
int xgpu_output_ladder_check(const xgpu_output_format *f, const xgpu_ladder_params *lp, const xgpu_surface_rung *rungs, int n, int width, int height, int bit_depth)
{
    int rc; char why[160];
    (void)ladder_ok(f, lp, rungs, n, width, height, bit_depth, &rc, why, NULL);
    return rc;
}
// The tap tables of a call behind the room for its records: per rung the rows of luma and chroma (vertical pass) and their columns (horizontal pass, transposed).
// The room is 6 records per rung whatever the layout (3 vertical, up to 3 horizontal), so the tables of a key lie where they lay.
static const size_t LADDER_RECORDS = 6;
static int build_ladder_tables(int ws, int hs, const xgpu_surface_rung *rungs, int n, int filter, int src_loc, int dst_loc, std::vector<uint8_t> &blob,
                               std::vector<ScaleAxisTab> &tabs, int *cap)
{
    int dx, dy, Dx, Dy;
    chroma_siting(src_loc, &dx, &dy);
    chroma_siting(dst_loc, &Dx, &Dy);
    blob.assign((size_t)n * LADDER_RECORDS * sizeof(LadderDesc), 0);
    tabs.assign((size_t)4 * n, ScaleAxisTab());
    *cap = 8;
    for (int i = 0; i < n; i++) {
        const int wd = rungs[i].width, hd = rungs[i].height;
        int cy = 0, cc = 0;
        TRY(scale_build_axis(hs, 1, 0, hd, 1, 0, filter, false, 0, blob, tabs[4 * i], NULL));
        TRY(scale_build_axis(hs >> 1, 2, dy, hd >> 1, 2, Dy, filter, false, 0, blob, tabs[4 * i + 1], NULL));
        TRY(scale_build_axis(ws, 1, 0, wd, 1, 0, filter, true, 64 * LADDER_GROUP, blob, tabs[4 * i + 2], &cy));
        TRY(scale_build_axis(ws >> 1, 2, dx, wd >> 1, 2, Dx, filter, true, 64 * LADDER_GROUP, blob, tabs[4 * i + 3], &cc));
        *cap = std::max(*cap, std::max(cy, cc));
    }
    return blob.size() > 0xFFFFFFFFu ? XGPU_ERR_UNSUPPORTED : XGPU_OK;
}
int xgpu_pic_output_device_ladder(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_ladder_params *lp, const xgpu_surface_rung *rungs,
                                  int n, void *stream)
{
    static const char who[] = "pic_output_device_ladder";
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic));
    int src_rc; char why[160];
    size_t mid_need = 0;
    const int bd = c->sp.bit_depth_luma;
    if (!ladder_ok(f, lp, rungs, n, c->sp.width, c->sp.height, bd, &src_rc, why, &mid_need)) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return src_rc; }
    const size_t es = (size_t)elem_size(f->dtype);
    size_t need[XGPU_MAX_RUNGS];
    for (int i = 0; i < n; i++) {
        const char *w0;
        need[i] = ladder_rung_size(f, rungs[i].width, rungs[i].height, rungs[i].row_pitch, bd, &w0);
        if (!rungs[i].d_dst) { snprintf(c->err, sizeof(c->err), "%s: rung %d: the destination is NULL", who, i); return XGPU_ERR_INVALID_ARGUMENT; }
        TRY(check_dst_fits(c, who, rungs[i].d_dst, rungs[i].dst_size, need[i], es));
        for (int k = 0; k < i; k++) {
            const uintptr_t a0 = (uintptr_t)rungs[k].d_dst, b0 = (uintptr_t)rungs[i].d_dst;
            if (a0 < b0 + need[i] && b0 < a0 + need[k]) { snprintf(c->err, sizeof(c->err), "%s: rungs %d and %d overlap", who, k, i); return XGPU_ERR_INVALID_ARGUMENT; }
        }
    }
    if (dra) TRY(check_dra(c, dra));      // upload_dra's refusals, before anything is queued
    for (int i = 0; i < n; i++) TRY(check_device_dst(c, who, rungs[i].d_dst, need[i]));
    const int *cr = f->crop;
    const int ws = c->sp.width - cr[0] - cr[1], hs = c->sp.height - cr[2] - cr[3];
    const int dst_loc = lp->dst_chroma_loc < 0 ? f->chroma_loc : lp->dst_chroma_loc;
    // the tap tables: made here, before anything is queued; uploaded and committed below (the protocol of the scaled output's tables)
    std::vector<int> key = { ws, hs, lp->filter, f->chroma_loc, dst_loc, n };
    for (int i = 0; i < n; i++) { key.push_back(rungs[i].width); key.push_back(rungs[i].height); }
    const bool cached = c->lad_blk && key == c->lad_key;
    std::vector<uint8_t> blob;
    std::vector<ScaleAxisTab> tabs;
    int cap = c->lad_cap;
    if (!cached) {
        const int rc = build_ladder_tables(ws, hs, rungs, n, lp->filter, f->chroma_loc, dst_loc, blob, tabs, &cap);
        if (rc < 0) { snprintf(c->err, sizeof(c->err), "%s: cannot make the tap tables of the %d rungs from %dx%d", who, n, ws, hs); return rc; }
    }
    TRY(grow(c, who, &c->sc_mid, &c->sc_mid_cap, mid_need, "intermediate"));
    if (!cached && c->lad_blk_cap < blob.size()) {
        c->lad_key.clear();      // no key names a block that is freed
        TRY(grow(c, who, &c->lad_blk, &c->lad_blk_cap, blob.size(), "block of records and tap tables"));
    }
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    if (!cached) {      // behind the fork: after every kernel that read the previous block
        c->lad_key.clear();
        c->lad_host.swap(blob);
        c->lad_tabs.swap(tabs);
        c->lad_cap = cap;
    }
    // the records of this call: where the planes of every rung lie in the intermediate and in the destinations
    const bool pair = is_semiplanar(f->layout);
    const int nh = (pair ? 2 : 3) * n;
    LadderDesc *dv = (LadderDesc *)c->lad_host.data(), *dh = dv + 3 * n;
    memset(dv, 0, (size_t)n * LADDER_RECORDS * sizeof(LadderDesc));
    size_t mid = 0;
    int max_w = 0, max_h = 0;
    for (int i = 0; i < n; i++) {
        const int wd = rungs[i].width, hd = rungs[i].height;
        const ScaleAxisTab *t = &c->lad_tabs[4 * i];
        const size_t pitch = rungs[i].row_pitch ? rungs[i].row_pitch : (size_t)wd * es;      // of a luma row, and of a row of Cb Cr pairs
        uint32_t m[3];
        for (int p = 0; p < 3; p++) {
            LadderDesc &d = dv[3 * i + p];
            m[p] = d.mid[0] = (uint32_t)mid;
            d.mp = align8(p ? ws >> 1 : ws);
            d.plane = p; d.sw = p ? ws >> 1 : ws; d.rows = p ? hd >> 1 : hd;
            const ScaleAxisTab &v = t[p ? 1 : 0];
            d.first = (uint32_t)v.first; d.count = (uint32_t)v.count; d.wt = (uint32_t)v.w; d.stride = v.stride;
            mid += (size_t)d.rows * d.mp;
        }
        for (int p = 0; p < (pair ? 2 : 3); p++) {
            LadderDesc &d = dh[(pair ? 2 : 3) * i + p];
            d.mid[0] = m[p]; d.mid[1] = m[2];
            d.mp = align8(p ? ws >> 1 : ws);
            d.rows = p ? hd >> 1 : hd; d.cols = p ? wd >> 1 : wd;
            d.pair = pair && p;
            const ScaleAxisTab &h = t[p ? 3 : 2];
            d.first = (uint32_t)h.first; d.count = (uint32_t)h.count; d.wt = (uint32_t)h.w; d.stride = h.stride;
            // YUV420P: Y, then Cb, then Cr, tight; NV12 / P016: hd luma rows, then hd / 2 rows of pairs at the same pitch
            size_t off = 0;
            if (p) off = pair ? (size_t)hd * pitch : ((size_t)wd * hd + (size_t)(p - 1) * (wd >> 1) * (hd >> 1)) * es;
            d.dst = (uint64_t)((uintptr_t)rungs[i].d_dst + off);
            d.pitch = pair || !p ? pitch : (size_t)(wd >> 1) * es;
        }
        max_w = std::max(max_w, wd); max_h = std::max(max_h, hd);
    }
    // at most one upload: the whole block (new tables), the records alone, or - the same rungs into the same destinations again, a transcode's steady state -
    // nothing.  (Pageable host memory: staged before the call returns, as the DRA tables are.)
    const size_t rec_bytes = (size_t)n * LADDER_RECORDS * sizeof(LadderDesc);
    if (!cached || c->lad_sent.size() != rec_bytes || memcmp(c->lad_sent.data(), c->lad_host.data(), rec_bytes)) {
        c->lad_sent.clear();      // the block is about to change
        HIPCHK(c, hipMemcpyAsync(c->lad_blk, c->lad_host.data(), cached ? rec_bytes : c->lad_host.size(), hipMemcpyHostToDevice, s));
        c->lad_sent.assign(c->lad_host.begin(), c->lad_host.begin() + rec_bytes);
    }
    c->lad_key = key;
    LadderOutArgs a;
    memset(&a, 0, sizeof(a));
    cropped_planes(dpic(c, pic), cr, &a.y, &a.u, &a.v);
    a.sy = dpic(c, pic).s_l; a.sc = dpic(c, pic).s_c;
    a.dra = dra ? c->d_dra : NULL;
    a.smax = (1 << bd) - 1;
    a.mid = c->sc_mid;
    a.blk = c->lad_blk; a.n = n; a.nh = nh; a.cap = c->lad_cap;
    const int obd = sample_depth(f, bd);
    a.cshift = bd - obd; a.cout8 = obd == 8; a.cmaxv = (1 << obd) - 1;      // launch_output's conversion
    a.clsh = f->layout == XGPU_OUT_P016 ? 16 - obd : 0;
    launch_output_ladder(a, f->dtype, ws, max_h, max_w, max_h, s);
    return out_join(c, stream, s);      // the slot, the DRA tables, the block and the intermediate
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
    return (int)std::max<int64_t>(8, std::min<int64_t>(align8(b), align8(mn)));
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
    L.mid_slot = (size_t)sc->height * mid_row_samples(mw);      // samples
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
    static const char who[] = "pic_output_device_rois_dev";
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL); ARGCHK(c, d_boxes != NULL);
    int src_rc, mw = 0, mh = 0; char why[160];
    size_t image_pitch = 0;
    const size_t need = rois_dev_size(f, sc, rp, bounds, box_format, capacity, c->sp.width, c->sp.height, c->sp.bit_depth_luma, &src_rc, why, &image_pitch, &mw, &mh);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return src_rc; }
    TRY(check_dst_fits(c, who, d_dst, dst_size, need, elem_size(f->dtype)));
    if (dra) TRY(check_dra(c, dra));      // upload_dra's refusals, before anything is queued
    TRY(check_device_dst(c, who, d_dst, need));
    // the boxes, the count and the results are device memory of 4-byte words as well - the host never reads them
    TRY(check_device_dst(c, "pic_output_device_rois_dev (boxes)", const_cast<void *>(d_boxes), (size_t)capacity * 16));
    if (d_count) TRY(check_device_dst(c, "pic_output_device_rois_dev (count)", const_cast<int *>(d_count), sizeof(int)));
    if (d_results) TRY(check_device_dst(c, "pic_output_device_rois_dev (results)", d_results, (size_t)capacity * sizeof(xgpu_roi_result)));
    if (((uintptr_t)d_boxes | (uintptr_t)d_count | (uintptr_t)d_results) & 3) {
        snprintf(c->err, sizeof(c->err), "%s: boxes, count and results must be aligned to 4 bytes", who);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    RoisDevLayout L;
    rois_dev_layout(sc, rp->fit, mw, mh, capacity, L);
    // section 8e's two buffers, sized from the bounds and the capacity, so a steady stream of calls never grows them
    TRY(grow(c, who, &c->sc_mid, &c->sc_mid_cap, (size_t)capacity * L.mid_slot * sizeof(uint16_t), "intermediate"));
    TRY(grow(c, who, &c->roi_blk, &c->roi_blk_cap, L.blk, "descriptor block"));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    // behind the fork: after every kernel that read the previous block
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
    return out_join(c, stream, s);      // the slot, the DRA tables, the block and the intermediate
}

// ------------------------------------------------------------------------------------------------ warped regions of interest: a batch of affine maps
static const int64_t WARP_LIN_LIMIT = (int64_t)64 << 16, WARP_OFF_LIMIT = (int64_t)1 << 36;
static bool warp_map_ok(const xgpu_warp_map &m)
{
    for (int k = 0; k < 6; k++) {
        const int64_t lim = (k == 2 || k == 5) ? WARP_OFF_LIMIT : WARP_LIN_LIMIT;
        if (m.m[k] < -lim || m.m[k] > lim) return false;
    }
    return true;
}
int xgpu_warp_from_matrix(const double theta[6], xgpu_warp_map *out)
{
    #pragma clang fp contract(off)
    if (!theta || !out) return XGPU_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 6; k++) if (!std::isfinite(theta[k])) return XGPU_ERR_INVALID_ARGUMENT;
    double v[6];
    for (int r = 0; r < 2; r++) {
        const double *t = theta + 3 * r;
        v[3 * r] = t[0] * 65536.0;
        v[3 * r + 1] = t[1] * 65536.0;
        v[3 * r + 2] = ((t[0] + t[1]) * 0.5 + t[2] - 0.5) * 65536.0;
    }
    xgpu_warp_map m;
    for (int k = 0; k < 6; k++) {
        if (!std::isfinite(v[k]) || std::fabs(v[k]) > 1e15) return XGPU_ERR_INVALID_ARGUMENT;      // (llround of such a value is not defined; the limits are far below)
        m.m[k] = llround(v[k]);
    }
    if (!warp_map_ok(m)) return XGPU_ERR_INVALID_ARGUMENT;
    *out = m;
    return XGPU_OK;
}
int xgpu_warp_from_rotated_box(double cx, double cy, double w, double h, double angle_deg, int dst_w, int dst_h, xgpu_warp_map *out)
{
    #pragma clang fp contract(off)
    if (!out || dst_w < 1 || dst_h < 1 || !std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(w) || !std::isfinite(h) || !std::isfinite(angle_deg))
        return XGPU_ERR_INVALID_ARGUMENT;
    const double rad = angle_deg * (3.14159265358979323846 / 180.0), c = cos(rad), s = sin(rad);
    const double theta[6] = { w * c / dst_w, -h * s / dst_h, cx - (w * c - h * s) / 2, w * s / dst_w, h * c / dst_h, cy - (w * s + h * c) / 2 };
    return xgpu_warp_from_matrix(theta, out);
}
// The whole of a call's argument checks, without a device: the bytes the destination needs, or 0 with *rc = the code, `why` (160 bytes) and *bad = the map it
// names (-1: none).  maps = NULL: the maps are not looked at (device maps, which the host does not read; the size, which does not depend on them); dev_maps: the
// pad is read whatever the border
static size_t warp_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_warp_params *wp, const xgpu_warp_map *maps, bool dev_maps, int n, int width,
                        int height, int bd, int *rc, char *why, int *bad, size_t *image_pitch)
{
    const char *w0 = "";
    *bad = -1;
    if (!scaled_params_ok(f, sc, width, height, bd, rc, &w0)) { snprintf(why, 160, "%s", w0); return 0; }
    const size_t image = scaled_image_bytes(f, sc, rc, &w0);
    if (image == 0) { snprintf(why, 160, "%s", w0); return 0; }
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    if (sc->filter != XGPU_SCALE_BILINEAR) { snprintf(why, 160, "filter must be XGPU_SCALE_BILINEAR"); return 0; }
    if (!wp) { snprintf(why, 160, "warp parameters are NULL"); return 0; }
    if (n < 1 || n > XGPU_MAX_ROIS) { snprintf(why, 160, "n %d outside 1..%d", n, XGPU_MAX_ROIS); return 0; }
    if (wp->samples != 1 && wp->samples != 2 && wp->samples != 4) { snprintf(why, 160, "samples must be 1, 2 or 4"); return 0; }
    if (wp->border != XGPU_WARP_CLAMP && wp->border != XGPU_WARP_PAD) { snprintf(why, 160, "border must be XGPU_WARP_CLAMP or XGPU_WARP_PAD"); return 0; }
    xgpu_roi_params rp;      // the pad and the batch stride follow the rules of the regions of interest
    rp.fit = XGPU_FIT_STRETCH; rp.image_pitch = wp->image_pitch;
    for (int k = 0; k < 3; k++) rp.pad[k] = wp->pad[k];
    const size_t ip = rois_pad_and_pitch(f, sc, &rp, bd, image, wp->border == XGPU_WARP_PAD || dev_maps, why);
    if (ip == 0) return 0;
    if (maps)
        for (int i = 0; i < n; i++)
            if (!warp_map_ok(maps[i])) {
                *bad = i;
                snprintf(why, 160, "map %d: a coefficient outside |m[0,1,3,4]| <= 64 << 16, |m[2,5]| <= 1 << 36", i);
                return 0;
            }
    *rc = XGPU_OK;
    if (image_pitch) *image_pitch = ip;
    return (size_t)(n - 1) * ip + image;
}
int xgpu_output_warp_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_warp_params *wp, const xgpu_warp_map *maps, int n, int width, int height,
                           int bit_depth, int *bad_index)
{
    int rc, bad; char why[160];
    (void)warp_size(f, sc, wp, maps, maps == NULL, n, width, height, bit_depth, &rc, why, &bad, NULL);
    if (bad_index) *bad_index = bad;
    return rc;
}
size_t xgpu_output_warp_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_warp_params *wp, int n, int width, int height, int bit_depth)
{
    int rc, bad; char why[160];
    return warp_size(f, sc, wp, NULL, wp && wp->border == XGPU_WARP_PAD, n, width, height, bit_depth, &rc, why, &bad, NULL);
}
int xgpu_pic_output_device_warp(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_warp_params *wp,
                                const xgpu_warp_map *maps, int maps_on_device, int n, int32_t *d_status, void *d_dst, size_t dst_size, void *stream)
{
    static const char who[] = "pic_output_device_warp";
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL); ARGCHK(c, maps != NULL); ARGCHK(c, maps_on_device == 0 || maps_on_device == 1);
    int src_rc, bad; char why[160];
    size_t image_pitch = 0;
    const size_t need = warp_size(f, sc, wp, maps_on_device ? NULL : maps, maps_on_device != 0, n, c->sp.width, c->sp.height, c->sp.bit_depth_luma, &src_rc, why, &bad, &image_pitch);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return src_rc; }
    TRY(check_dst_fits(c, who, d_dst, dst_size, need, elem_size(f->dtype)));
    if (dra) TRY(check_dra(c, dra));      // upload_dra's refusals, before anything is queued
    TRY(check_device_dst(c, who, d_dst, need));
    const size_t maps_bytes = (size_t)n * sizeof(xgpu_warp_map);
    if (maps_on_device) {
        if ((uintptr_t)maps % 8 || (d_status && (uintptr_t)d_status % 4)) { snprintf(c->err, sizeof(c->err), "%s: maps or status in device memory are not aligned", who); return XGPU_ERR_INVALID_ARGUMENT; }
        TRY(check_device_dst(c, "pic_output_device_warp (maps)", const_cast<xgpu_warp_map *>(maps), maps_bytes));
        if (d_status) TRY(check_device_dst(c, "pic_output_device_warp (status)", d_status, (size_t)n * sizeof(int32_t)));
    } else {
        TRY(grow(c, who, &c->roi_blk, &c->roi_blk_cap, maps_bytes, "block of maps"));
    }
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    // behind the fork: after every kernel that read the previous block.  (Pageable host memory: staged before the call returns, as the DRA tables are.)
    if (!maps_on_device) HIPCHK(c, hipMemcpyAsync(c->roi_blk, maps, maps_bytes, hipMemcpyHostToDevice, s));
    WarpOutArgs a;
    memset(&a, 0, sizeof(a));
    scaled_common_args(c, pic, dra, f, sc, d_dst, a);
    a.w = c->sp.width - f->crop[0] - f->crop[1]; a.h = c->sp.height - f->crop[2] - f->crop[3]; a.cw = a.w >> 1; a.ch = a.h >> 1;
    a.maps = maps_on_device ? (const int64_t *)maps : (const int64_t *)c->roi_blk;
    a.status = maps_on_device ? d_status : NULL;
    a.n = n;
    a.ls = wp->samples == 4 ? 2 : wp->samples == 2 ? 1 : 0;
    a.border = wp->border;
    a.sh = f->chroma_loc & 1;
    a.sv = f->chroma_loc < 2 ? 1 : f->chroma_loc < 4 ? 0 : 2;
    for (int k = 0; k < 3; k++) a.padv[k] = (wp->border == XGPU_WARP_PAD || maps_on_device) ? wp->pad[k] : 0.f;
    a.image_pitch = image_pitch;
    launch_output_warp(a, f->layout, f->dtype, s);
    return out_join(c, stream, s);      // the slot, the DRA tables and the block of maps
}

// ------------------------------------------------------------------------------------------------ remapped output: a batch of coordinate grids in device memory
int xgpu_remap_grid_dims(int dst_w, int dst_h, int step_log2, int *gw, int *gh)
{
    if (dst_w < 1 || dst_h < 1 || step_log2 < 0 || step_log2 > 6) return XGPU_ERR_INVALID_ARGUMENT;
    if (gw) *gw = ((dst_w - 1) >> step_log2) + 1 + (step_log2 > 0);
    if (gh) *gh = ((dst_h - 1) >> step_log2) + 1 + (step_log2 > 0);
    return XGPU_OK;
}
// the bytes of one grid and (*pitch, may be NULL) between two; 0: refused, `why` (160 bytes) says which field
static size_t remap_grid_bytes(const xgpu_scale_params *sc, const xgpu_remap_params *rp, size_t *pitch, char *why)
{
    int gw, gh;
    if (!sc || !rp || sc->width < 1 || sc->height < 1 || xgpu_remap_grid_dims(sc->width, sc->height, rp->step_log2, &gw, &gh) < 0) {
        snprintf(why, 160, "step_log2 must be 0..6");
        return 0;
    }
    const size_t one = (size_t)gh * gw * 8;
    if (rp->grid_pitch && (rp->grid_pitch % 8 || rp->grid_pitch < one)) {
        snprintf(why, 160, "grid_pitch %zu: 0, or a multiple of 8 not below the %zu bytes of one grid of %d x %d nodes", rp->grid_pitch, one, gw, gh);
        return 0;
    }
    if (pitch) *pitch = rp->grid_pitch ? rp->grid_pitch : one;
    return one;
}
size_t xgpu_remap_grid_size(const xgpu_scale_params *sc, const xgpu_remap_params *rp, int n)
{
    char why[160]; size_t pitch = 0;
    if (n < 1 || n > XGPU_MAX_ROIS) return 0;
    const size_t one = remap_grid_bytes(sc, rp, &pitch, why);
    return one ? (size_t)(n - 1) * pitch + one : 0;
}
// The whole of a call's argument checks that need no device: the bytes the destination needs, or 0 with *rc = the code and `why` (160 bytes)
static size_t remap_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_remap_params *rp, int n, int width, int height, int bd, int *rc, char *why,
                         size_t *image_pitch)
{
    const char *w0 = "";
    if (!scaled_params_ok(f, sc, width, height, bd, rc, &w0)) { snprintf(why, 160, "%s", w0); return 0; }
    const size_t image = scaled_image_bytes(f, sc, rc, &w0);
    if (image == 0) { snprintf(why, 160, "%s", w0); return 0; }
    *rc = XGPU_ERR_INVALID_ARGUMENT;
    if (sc->filter != XGPU_SCALE_BILINEAR) { snprintf(why, 160, "filter must be XGPU_SCALE_BILINEAR"); return 0; }
    if (!rp) { snprintf(why, 160, "remap parameters are NULL"); return 0; }
    if (n < 1 || n > XGPU_MAX_ROIS) { snprintf(why, 160, "n %d outside 1..%d", n, XGPU_MAX_ROIS); return 0; }
    if (rp->grid_format != XGPU_GRID_Q16_I32 && rp->grid_format != XGPU_GRID_F32) { snprintf(why, 160, "grid_format must be XGPU_GRID_Q16_I32 or XGPU_GRID_F32"); return 0; }
    if (rp->samples != 1 && rp->samples != 2 && rp->samples != 4) { snprintf(why, 160, "samples must be 1, 2 or 4"); return 0; }
    if (rp->border != XGPU_WARP_CLAMP && rp->border != XGPU_WARP_PAD) { snprintf(why, 160, "border must be XGPU_WARP_CLAMP or XGPU_WARP_PAD"); return 0; }
    if (remap_grid_bytes(sc, rp, NULL, why) == 0) return 0;
    xgpu_roi_params roi;      // the pad and the batch stride follow the rules of the regions of interest; either grid format can carry invalid nodes: the pad is always read
    roi.fit = XGPU_FIT_STRETCH; roi.image_pitch = rp->image_pitch;
    for (int k = 0; k < 3; k++) roi.pad[k] = rp->pad[k];
    const size_t ip = rois_pad_and_pitch(f, sc, &roi, bd, image, true, why);
    if (ip == 0) return 0;
    *rc = XGPU_OK;
    if (image_pitch) *image_pitch = ip;
    return (size_t)(n - 1) * ip + image;
}
int xgpu_output_remap_check(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_remap_params *rp, int n, int width, int height, int bit_depth)
{
    int rc; char why[160];
    (void)remap_size(f, sc, rp, n, width, height, bit_depth, &rc, why, NULL);
    return rc;
}
size_t xgpu_output_remap_size(const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_remap_params *rp, int n, int width, int height, int bit_depth)
{
    int rc; char why[160];
    return remap_size(f, sc, rp, n, width, height, bit_depth, &rc, why, NULL);
}
// a helper's value in luma samples -> Q16: non-finite = invalid (INT32_MIN), else llround of the product clamped to +-INT32_MAX
static bool remap_q16(double x, double y, int32_t *node)
{
    #pragma clang fp contract(off)
    const double tx = x * 65536.0, ty = y * 65536.0;
    if (!std::isfinite(tx) || !std::isfinite(ty)) { node[0] = node[1] = INT32_MIN; return false; }
    node[0] = (int32_t)llround(std::min(std::max(tx, -2147483647.0), 2147483647.0));
    node[1] = (int32_t)llround(std::min(std::max(ty, -2147483647.0), 2147483647.0));
    return true;
}
int xgpu_remap_from_warp(const xgpu_warp_map *map, int dst_w, int dst_h, int step_log2, int32_t *grid)
{
    int gw, gh;
    if (!map || !grid || dst_w < 2 || dst_h < 2 || xgpu_remap_grid_dims(dst_w, dst_h, step_log2, &gw, &gh) < 0 || !warp_map_ok(*map)) return XGPU_ERR_INVALID_ARGUMENT;
    const int64_t *m = map->m;
    for (int j = 0; j < gh; j++)
        for (int i = 0; i < gw; i++) {      // exact in int64: |m| <= 2^36, the coordinates below 2^15
            const int64_t ox = (int64_t)i << step_log2, oy = (int64_t)j << step_log2;
            const int64_t x = m[0] * ox + m[1] * oy + m[2], y = m[3] * ox + m[4] * oy + m[5];
            grid[2 * ((size_t)j * gw + i)] = (int32_t)std::min<int64_t>(std::max<int64_t>(x, -INT32_MAX), INT32_MAX);
            grid[2 * ((size_t)j * gw + i) + 1] = (int32_t)std::min<int64_t>(std::max<int64_t>(y, -INT32_MAX), INT32_MAX);
        }
    return XGPU_OK;
}
int xgpu_remap_from_homography(const double h[9], int dst_w, int dst_h, int step_log2, int32_t *grid)
{
    #pragma clang fp contract(off)
    int gw, gh;
    if (!h || !grid || dst_w < 2 || dst_h < 2 || xgpu_remap_grid_dims(dst_w, dst_h, step_log2, &gw, &gh) < 0) return XGPU_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < gh; j++)
        for (int i = 0; i < gw; i++) {
            const double u = (double)((int64_t)i << step_log2) + 0.5, v = (double)((int64_t)j << step_log2) + 0.5;
            const double den = h[6] * u + h[7] * v + h[8];
            int32_t *node = grid + 2 * ((size_t)j * gw + i);
            if (!(den > 0.0)) { node[0] = node[1] = INT32_MIN; continue; }
            (void)remap_q16((h[0] * u + h[1] * v + h[2]) / den - 0.5, (h[3] * u + h[4] * v + h[5]) / den - 0.5, node);
        }
    return XGPU_OK;
}
int xgpu_remap_from_lens(const xgpu_remap_lens *l, int dst_w, int dst_h, int step_log2, int32_t *grid)
{
    #pragma clang fp contract(off)
    int gw, gh;
    if (!l || !grid || dst_w < 2 || dst_h < 2 || xgpu_remap_grid_dims(dst_w, dst_h, step_log2, &gw, &gh) < 0) return XGPU_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < gh; j++)
        for (int i = 0; i < gw; i++) {
            const double x = ((double)((int64_t)i << step_log2) - l->ncx) / l->nfx, y = ((double)((int64_t)j << step_log2) - l->ncy) / l->nfy;
            const double r2 = x * x + y * y;
            const double rad = 1.0 + r2 * (l->k1 + r2 * (l->k2 + r2 * l->k3));
            const double xd = x * rad + 2.0 * l->p1 * x * y + l->p2 * (r2 + 2.0 * x * x);
            const double yd = y * rad + l->p1 * (r2 + 2.0 * y * y) + 2.0 * l->p2 * x * y;
            (void)remap_q16(l->fx * xd + l->cx, l->fy * yd + l->cy, grid + 2 * ((size_t)j * gw + i));
        }
    return XGPU_OK;
}
int xgpu_pic_output_device_remap(xgpu_ctx *c, int pic, const xgpu_dra_luts *dra, const xgpu_output_format *f, const xgpu_scale_params *sc, const xgpu_remap_params *rp,
                                 const void *d_grid, size_t grid_size, int n, void *d_dst, size_t dst_size, void *stream)
{
    static const char who[] = "pic_output_device_remap";
    ARGCHK(c, c != NULL); ARGCHK(c, valid_pic(c, pic)); ARGCHK(c, d_dst != NULL); ARGCHK(c, d_grid != NULL);
    int src_rc; char why[160];
    size_t image_pitch = 0, grid_pitch = 0;
    const size_t need = remap_size(f, sc, rp, n, c->sp.width, c->sp.height, c->sp.bit_depth_luma, &src_rc, why, &image_pitch);
    if (need == 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return src_rc; }
    const size_t one_grid = remap_grid_bytes(sc, rp, &grid_pitch, why), grids = (size_t)(n - 1) * grid_pitch + one_grid;
    if (grid_size < grids || (uintptr_t)d_grid % 8) {
        snprintf(c->err, sizeof(c->err), "%s: grid of %zu bytes at %p, the call needs %zu bytes aligned to 8", who, grid_size, d_grid, grids);
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    TRY(check_dst_fits(c, who, d_dst, dst_size, need, elem_size(f->dtype)));
    if (dra) TRY(check_dra(c, dra));      // upload_dra's refusals, before anything is queued
    TRY(check_device_dst(c, who, d_dst, need));
    TRY(check_device_dst(c, "pic_output_device_remap (grid)", const_cast<void *>(d_grid), grids));
    if (dra) TRY(upload_dra(c, dra));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    RemapOutArgs a;
    memset(&a, 0, sizeof(a));
    scaled_common_args(c, pic, dra, f, sc, d_dst, a);
    a.w = c->sp.width - f->crop[0] - f->crop[1]; a.h = c->sp.height - f->crop[2] - f->crop[3]; a.cw = a.w >> 1; a.ch = a.h >> 1;
    a.grid = (const uint8_t *)d_grid;
    a.grid_pitch = grid_pitch;
    (void)xgpu_remap_grid_dims(sc->width, sc->height, rp->step_log2, &a.gw, &a.gh);
    a.k = rp->step_log2;
    a.f32 = rp->grid_format == XGPU_GRID_F32;
    a.n = n;
    a.ls = rp->samples == 4 ? 2 : rp->samples == 2 ? 1 : 0;
    a.border = rp->border;
    a.sh = f->chroma_loc & 1;
    a.sv = f->chroma_loc < 2 ? 1 : f->chroma_loc < 4 ? 0 : 2;
    for (int k = 0; k < 3; k++) a.padv[k] = rp->pad[k];
    a.image_pitch = image_pitch;
    launch_output_remap(a, f->layout, f->dtype, s);
    return out_join(c, stream, s);      // the slot and the DRA tables; the grid is the caller's, ordered by the caller's stream
}

// ------------------------------------------------------------------------------------------------ coding side information of the picture decoded last
// the format alone and the size it needs for a picture of width x height; 0: invalid, `why` says which field
static size_t side_size(const xgpu_side_format *f, int width, int height, const char **why)
{
    *why = "format is NULL";
    if (!f) return 0;
    *why = "picture size must be positive multiples of 8";
    if (width <= 0 || height <= 0 || ((width | height) & 7)) return 0;
    if (!crop_ok(f->crop, 0, 0, why)) return 0;
    if (f->layout == XGPU_SIDE_BLOCKS) {
        *why = "BLOCKS: dtype XGPU_OUT_U16 (int16 planes), no crop, row_pitch a multiple of 2 and at least a row";
        if (f->dtype != XGPU_OUT_U16 || f->crop[0] || f->crop[1] || f->crop[2] || f->crop[3] || (f->row_pitch & 1)) return 0;
        return rows_of((size_t)(width >> 2) * 2, 9 * (size_t)(height >> 2), f->row_pitch).total;
    }
    *why = "layout must be XGPU_SIDE_BLOCKS, XGPU_SIDE_FLOW_PLANAR or XGPU_SIDE_FLOW_INTERLEAVED";
    if (f->layout != XGPU_SIDE_FLOW_PLANAR && f->layout != XGPU_SIDE_FLOW_INTERLEAVED) return 0;
    *why = "FLOW: dtype XGPU_OUT_F16 or XGPU_OUT_F32, lists 1..3, per_poc 0 or 1, row_pitch a multiple of the element size";
    if ((f->dtype != XGPU_OUT_F16 && f->dtype != XGPU_OUT_F32) || f->lists < 1 || f->lists > 3 || (f->per_poc & ~1)) return 0;
    const size_t es = (size_t)elem_size(f->dtype), ch = f->lists == 3 ? 4 : 2;
    if (f->row_pitch % es) return 0;
    if (!crop_ok(f->crop, width, height, why)) return 0;
    const size_t w = width - f->crop[0] - f->crop[1], h = height - f->crop[2] - f->crop[3];
    const bool planar = f->layout == XGPU_SIDE_FLOW_PLANAR;
    *why = "row_pitch is shorter than a row";
    return rows_of((planar ? w : ch * w) * es, planar ? ch * h : h, f->row_pitch).total;
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
    TRY(check_dst(c, "frame_side_info", d_dst, dst_size, need, es));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    SideArgs a;
    memset(&a, 0, sizeof(a));
    a.maps = c->d_maps; a.w_scu = c->w_scu; a.h_scu = c->h_scu;
    a.dst = (uint8_t *)d_dst;
    a.poc = c->fp.poc;
    for (int l = 0; l < 2; l++)
        for (int i = 0; i < XGPU_MAX_REFS; i++) a.refp_poc[i][l] = i < c->fp.num_refp[l] ? c->fp.refp_poc[i][l] : c->fp.poc;      // (an index past the list: distance 0)
    if (f->layout == XGPU_SIDE_BLOCKS) {
        fill_rows(a, d_dst, (size_t)c->w_scu * 2, c->h_scu, f->row_pitch);
        launch_side_blocks(a, s);
    } else {
        const bool planar = f->layout == XGPU_SIDE_FLOW_PLANAR;
        const int n_lists = f->lists == 3 ? 2 : 1;
        a.w = c->sp.width - f->crop[0] - f->crop[1]; a.h = c->sp.height - f->crop[2] - f->crop[3];
        a.crop_l = f->crop[0]; a.crop_t = f->crop[2];
        a.list0 = f->lists == 2 ? 1 : 0; a.per_poc = f->per_poc;
        fill_rows(a, d_dst, (size_t)a.w * es * (planar ? 1 : 2 * n_lists), a.h, f->row_pitch);
        launch_side_flow(a, planar, f->dtype, n_lists, s);
    }
    return out_join(c, stream, s);      // the SCU map, before the next picture's k_inter writes it
}

// ------------------------------------------------------------------------------------------------ the residual of a batch as picture-shaped planes
// the format alone and the size it needs for a picture of width x height; 0: invalid, `why` says which field
static size_t resid_size(const xgpu_resid_format *f, int width, int height, const char **why)
{
    *why = "format is NULL";
    if (!f) return 0;
    *why = "picture size must be positive multiples of 8";
    if (width <= 0 || height <= 0 || ((width | height) & 7)) return 0;
    if (!crop_ok(f->crop, 0, 0, why)) return 0;
    if (f->layout == XGPU_RESID_ENERGY) {
        *why = "ENERGY: dtype XGPU_OUT_F32, no crop, row_pitch a multiple of 4 and at least a row";
        if (f->dtype != XGPU_OUT_F32 || f->crop[0] || f->crop[1] || f->crop[2] || f->crop[3] || (f->row_pitch & 3)) return 0;
        return rows_of((size_t)(width >> 2) * 4, 3 * (size_t)(height >> 2), f->row_pitch).total;
    }
    *why = "layout must be XGPU_RESID_YUV420, XGPU_RESID_444_PLANAR, XGPU_RESID_444_INTERLEAVED or XGPU_RESID_ENERGY";
    if (f->layout != XGPU_RESID_YUV420 && f->layout != XGPU_RESID_444_PLANAR && f->layout != XGPU_RESID_444_INTERLEAVED) return 0;
    if (!crop_ok(f->crop, width, height, why)) return 0;
    const size_t w = width - f->crop[0] - f->crop[1], h = height - f->crop[2] - f->crop[3];
    if (f->layout == XGPU_RESID_YUV420) {
        *why = "YUV420: dtype XGPU_OUT_U16 (int16 planes), row_pitch a multiple of 4 (the chroma pitch is half of it) and at least a row";
        if (f->dtype != XGPU_OUT_U16 || (f->row_pitch & 3)) return 0;
        const Rows y = rows_of(w * 2, h, f->row_pitch);
        if (!y.total) return 0;
        return h * y.pitch + rows_of(w, h, y.pitch / 2).total;      // Y: h rows of the pitch; Cb, Cr: h / 2 rows of half the pitch each, the last one tight
    }
    *why = "444: dtype XGPU_OUT_U16, XGPU_OUT_F16 or XGPU_OUT_F32, row_pitch a multiple of the element size";
    if (f->dtype != XGPU_OUT_U16 && f->dtype != XGPU_OUT_F16 && f->dtype != XGPU_OUT_F32) return 0;
    const size_t es = (size_t)elem_size(f->dtype);
    if (f->row_pitch % es) return 0;
    const bool planar = f->layout == XGPU_RESID_444_PLANAR;
    *why = "row_pitch is shorter than a row";
    return rows_of((planar ? w : 3 * w) * es, planar ? 3 * h : h, f->row_pitch).total;
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
    TRY(check_dst(c, "batch_residual", d_dst, dst_size, need, es));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));      // (the batch's upload is behind it too: the context's stream has waited for it)
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
        fill_rows(a, d_dst, (size_t)c->w_scu * 4, c->h_scu, f->row_pitch);
    } else if (f->layout == XGPU_RESID_YUV420) {
        a.pitch = rows_of((size_t)a.w * 2, a.h, f->row_pitch).pitch;
        a.pitch_c = a.pitch / 2;
        a.off_c[0] = a.pitch * a.h; a.off_c[1] = a.off_c[0] + a.pitch_c * (a.h / 2);
        a.aligned = aligned16((uintptr_t)d_dst | a.pitch);      // then the chroma rows (8-byte stores) start at multiples of 8
    } else {
        fill_rows(a, d_dst, (size_t)a.w * es * (f->layout == XGPU_RESID_444_PLANAR ? 1 : 3), a.h, f->row_pitch);
    }
    launch_residual(a, f->layout, f->dtype, s);
    return out_join(c, stream, s);      // the arena, before xgpu_batch_destroy's blk.done lets the block be refilled
}

// ------------------------------------------------------------------------------------------------ a picture against a reference
// the reference alone for a picture of width x height: the bytes it spans from d_yuv (the luma pitch in *pitch), or 0 with `why`
static size_t compare_ref_size(const xgpu_compare_ref *r, int width, int height, size_t *pitch, const char **why)
{
    *why = "reference is NULL";
    if (!r) return 0;
    *why = "picture size must be positive and even";
    if (width <= 0 || height <= 0 || ((width | height) & 1)) return 0;
    *why = "reference: kind must be XGPU_CMP_REF_PIC or XGPU_CMP_REF_YUV420";
    if (r->kind != XGPU_CMP_REF_YUV420) return 0;      // (a slot has no memory to size)
    *why = "reference: dtype must be XGPU_OUT_U8 or XGPU_OUT_U16";
    if (r->dtype != XGPU_OUT_U8 && r->dtype != XGPU_OUT_U16) return 0;
    const size_t es = (size_t)elem_size(r->dtype), w = width, h = height;
    *why = "reference: row_pitch must be a multiple of 2 elements and at least a row";
    if (r->row_pitch % (2 * es)) return 0;
    const Rows y = rows_of(w * es, h, r->row_pitch);
    if (!y.total) return 0;
    if (pitch) *pitch = y.pitch;
    return h * y.pitch + rows_of((w >> 1) * es, h, y.pitch / 2).total;      // Y: h rows of the pitch; Cb, Cr: h / 2 rows of half the pitch each, the last one tight
}
size_t xgpu_compare_ref_size(const xgpu_compare_ref *r, int width, int height)
{
    const char *why;
    return compare_ref_size(r, width, height, NULL, &why);
}
static bool compare_params_ok(const xgpu_compare_params *p, int width, int height, const char **why)
{
    *why = "parameters are NULL";
    if (!p) return false;
    *why = "picture size must be positive and even";
    if (width <= 0 || height <= 0 || ((width | height) & 1)) return false;
    if (!crop_ok(p->crop, width, height, why)) return false;
    *why = "ssim and block_map: 0 or 1";
    return !((p->ssim | p->block_map) & ~1);
}
size_t xgpu_compare_map_size(const xgpu_compare_params *p, int width, int height)
{
    const char *why;
    if (!compare_params_ok(p, width, height, &why) || !p->block_map) return 0;
    const size_t w = width - p->crop[0] - p->crop[1], h = height - p->crop[2] - p->crop[3];
    return 3 * ((h + 15) / 16) * ((w + 15) / 16) * sizeof(uint64_t);
}
static int compare_check(const xgpu_compare_ref *r, const xgpu_compare_params *p, int width, int height, int bd, const char **why)
{
    if (!compare_params_ok(p, width, height, why)) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "bit depth out of range";
    if (bd < 8 || bd > 12) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "reference is NULL";
    if (!r) return XGPU_ERR_INVALID_ARGUMENT;
    if (r->kind == XGPU_CMP_REF_PIC) {
        *why = "reference: the slot is negative";
        return r->pic < 0 ? XGPU_ERR_INVALID_ARGUMENT : XGPU_OK;
    }
    const size_t need = compare_ref_size(r, width, height, NULL, why);
    if (!need) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "reference: XGPU_OUT_U8 needs a coding depth of 8";
    if (r->dtype == XGPU_OUT_U8 && bd != 8) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "reference: d_yuv is NULL or size is below xgpu_compare_ref_size";
    if (!r->d_yuv || r->size < need) return XGPU_ERR_INVALID_ARGUMENT;
    return XGPU_OK;
}
int xgpu_compare_check(const xgpu_compare_ref *r, const xgpu_compare_params *p, int width, int height, int bit_depth)
{
    const char *why;
    return compare_check(r, p, width, height, bit_depth, &why);
}
// Checks first, then the order of output_device: on a caller's stream the kernels run behind the picture's kernels - and behind every earlier output call -,
// and the context's stream waits for them before the next picture may write either slot.
int xgpu_pic_compare(xgpu_ctx *c, int pic, const xgpu_compare_ref *ref, const xgpu_compare_params *p, xgpu_compare_result *d_result, uint64_t *d_map,
                     size_t map_size, void *stream)
{
    static const char who[] = "pic_compare";
    ARGCHK(c, c != NULL); ARGCHK(c, d_result != NULL);
    const char *why = "";
    const int bd = c->sp.bit_depth_luma;
    if (compare_check(ref, p, c->sp.width, c->sp.height, bd, &why) < 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return XGPU_ERR_INVALID_ARGUMENT; }
    const bool slot = ref->kind == XGPU_CMP_REF_PIC;
    if (c->have_frame || !valid_pic(c, pic) || (slot && !valid_pic(c, ref->pic))) {
        snprintf(c->err, sizeof(c->err), "%s: %s", who, c->have_frame ? "a frame is open: compare after xgpu_frame_end" : !valid_pic(c, pic) ? "the slot holds no picture"
                                                                                                                                  : "the reference slot holds no picture");
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    const size_t es = slot ? 2 : (size_t)elem_size(ref->dtype);
    size_t pitch = 0;
    if (!slot) {
        const size_t need = compare_ref_size(ref, c->sp.width, c->sp.height, &pitch, &why);
        TRY(check_dst(c, "pic_compare: reference", (void *)ref->d_yuv, ref->size, need, es));
    }
    TRY(check_dst(c, "pic_compare: result", d_result, sizeof(xgpu_compare_result), sizeof(xgpu_compare_result), 8));
    const size_t map_need = xgpu_compare_map_size(p, c->sp.width, c->sp.height);
    if (p->block_map) {
        ARGCHK(c, d_map != NULL);
        TRY(check_dst(c, "pic_compare: map", d_map, map_size, map_need, 8));
    }
    const int *cr = p->crop;
    const int w = c->sp.width - cr[0] - cr[1], h = c->sp.height - cr[2] - cr[3];
    const int all_tiles = ((w + 63) / 64) * ((h + 31) / 32) + 2 * (((w >> 1) + 63) / 64) * (((h >> 1) + 31) / 32);
    TRY(grow(c, who, &c->cmp_part, &c->cmp_part_cap, (size_t)compare_workgroups(all_tiles) * 3 * CMP_PART_WORDS * sizeof(unsigned long long), "block of partial sums"));
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    CompareArgs a;
    memset(&a, 0, sizeof(a));
    const int16_t *pl[3];
    const DevPic &dp = dpic(c, pic);
    cropped_planes(dp, cr, &pl[0], &pl[1], &pl[2]);
    if (slot) {
        const DevPic &rp = dpic(c, ref->pic);
        const int16_t *rl[3];
        cropped_planes(rp, cr, &rl[0], &rl[1], &rl[2]);
        for (int k = 0; k < 3; k++) { a.r[k] = (const uint8_t *)rl[k]; a.pr[k] = (size_t)(k ? rp.s_c : rp.s_l) * 2; }
    } else {
        const uint8_t *base = (const uint8_t *)ref->d_yuv;
        const size_t hh = c->sp.height, pc = pitch / 2;
        const size_t off_c = (size_t)(cr[2] >> 1) * pc + (size_t)(cr[0] >> 1) * es;
        a.r[0] = base + (size_t)cr[2] * pitch + (size_t)cr[0] * es;
        a.r[1] = base + hh * pitch + off_c;
        a.r[2] = base + hh * pitch + (hh / 2) * pc + off_c;
        a.pr[0] = pitch; a.pr[1] = a.pr[2] = pc;
        a.r8 = es == 1;
    }
    int tiles = 0;
    for (int k = 0; k < 3; k++) {
        a.a[k] = (const uint16_t *)pl[k]; a.sa[k] = k ? dp.s_c : dp.s_l;
        a.w[k] = k ? w >> 1 : w; a.h[k] = k ? h >> 1 : h;
        a.vec_a[k] = aligned16((uintptr_t)a.a[k] | ((size_t)a.sa[k] * 2));
        a.vec_r[k] = (((uintptr_t)a.r[k] | a.pr[k]) & (a.r8 ? 7 : 15)) == 0;
        a.tiles_x[k] = (a.w[k] + 63) / 64;
        a.tile_first[k] = tiles;
        tiles += a.tiles_x[k] * ((a.h[k] + 31) / 32);
    }
    a.tile_first[3] = tiles;
    a.ssim = p->ssim; a.block_map = p->block_map;
    const long long L = (1 << bd) - 1;
    a.c1 = (64 * L * L + 5000) / 10000; a.c2 = (9 * 64 * 63 * L * L + 5000) / 10000;
    a.part = c->cmp_part; a.res = d_result; a.map = d_map; a.mw = (w + 15) / 16; a.mh = (h + 15) / 16;
    launch_compare(a, s);
    return out_join(c, stream, s);      // both slots, before the next picture's kernels may write them; the partial sums, before the next call's
}

// ------------------------------------------------------------------------------------------------ the statistics of one picture
// the parameters at coding depth bd, without a picture size: 0 or a negative code - every XGPU_ERR_INVALID_ARGUMENT before XGPU_ERR_UNSUPPORTED -, `why` says which field
static int stats_params_check(const xgpu_stats_params *p, int bd, const char **why)
{
    *why = "parameters are NULL";
    if (!p) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "bit depth out of range";
    if (bd < 8 || bd > 12) return XGPU_ERR_INVALID_ARGUMENT;
    if (!crop_ok(p->crop, 0, 0, why)) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "hist_bits must be 0 or 4 .. the coding depth";
    if (p->hist_bits != 0 && (p->hist_bits < 4 || p->hist_bits > bd)) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "light: 0 or 1";
    if (p->light & ~1) return XGPU_ERR_INVALID_ARGUMENT;
    if (p->hist_bits || p->light) {
        *why = "pctl_e4: 0 .. 10000";
        for (int i = 0; i < 2; i++) if (p->pctl_e4[i] < 0 || p->pctl_e4[i] > 10000) return XGPU_ERR_INVALID_ARGUMENT;
    }
    if (!p->light) return XGPU_OK;
    *why = "light: full_range 0 or 1; chroma_loc 0..5; upsample XGPU_UPSAMPLE_NEAREST or _LINEAR";
    if ((p->full_range & ~1) || p->chroma_loc < 0 || p->chroma_loc > 5 || (p->upsample != XGPU_UPSAMPLE_NEAREST && p->upsample != XGPU_UPSAMPLE_LINEAR))
        return XGPU_ERR_INVALID_ARGUMENT;
    double kr, kb;
    *why = "light: matrix: supported MatrixCoefficients are 1, 4, 5, 6, 7 and 9";
    if (!matrix_kr_kb(p->matrix, &kr, &kb)) return XGPU_ERR_UNSUPPORTED;
    *why = "light: transfer: supported TransferCharacteristics are 1, 4, 5, 6, 8, 13, 14, 15, 16 and 18";
    if (!colour_transfer_supported(p->transfer)) return XGPU_ERR_UNSUPPORTED;
    return XGPU_OK;
}
static size_t stats_hist_size(const xgpu_stats_params *p, int bd)
{
    return ((p->hist_bits ? (size_t)3 << p->hist_bits : 0) + (p->light ? (size_t)1 << bd : 0)) * sizeof(uint32_t);
}
size_t xgpu_stats_hist_size(const xgpu_stats_params *p, int bit_depth)
{
    const char *why;
    return stats_params_check(p, bit_depth, &why) < 0 ? 0 : stats_hist_size(p, bit_depth);
}
static int stats_check(const xgpu_stats_params *p, int width, int height, int bd, const char **why)
{
    *why = "parameters are NULL";
    if (!p) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "picture size must be positive and even, width * height below 2^31";
    if (width <= 0 || height <= 0 || ((width | height) & 1) || (long long)width * height >= (1ll << 31)) return XGPU_ERR_INVALID_ARGUMENT;
    *why = "bit depth out of range";
    if (bd < 8 || bd > 12) return XGPU_ERR_INVALID_ARGUMENT;
    if (!crop_ok(p->crop, width, height, why)) return XGPU_ERR_INVALID_ARGUMENT;
    return stats_params_check(p, bd, why);
}
int xgpu_stats_check(const xgpu_stats_params *p, int width, int height, int bit_depth)
{
    const char *why;
    return stats_check(p, width, height, bit_depth, &why);
}
// Checks first, then the order of xgpu_pic_compare.  What the call rewrites of the context's - the accumulation block, the lin table, the partial sums - is
// queued between out_fork and out_join, behind every earlier call that read them.
int xgpu_pic_stats(xgpu_ctx *c, int pic, const xgpu_stats_params *p, xgpu_stats_result *d_result, uint32_t *d_hist, size_t hist_size, void *stream)
{
    static const char who[] = "pic_stats";
    ARGCHK(c, c != NULL); ARGCHK(c, d_result != NULL);
    const char *why = "";
    const int bd = c->sp.bit_depth_luma;
    const int rc = stats_check(p, c->sp.width, c->sp.height, bd, &why);
    if (rc < 0) { snprintf(c->err, sizeof(c->err), "%s: %s", who, why); return rc; }
    if (c->have_frame || !valid_pic(c, pic)) {
        snprintf(c->err, sizeof(c->err), "%s: %s", who, c->have_frame ? "a frame is open: take the statistics after xgpu_frame_end" : "the slot holds no picture");
        return XGPU_ERR_INVALID_ARGUMENT;
    }
    TRY(check_dst(c, "pic_stats: result", d_result, sizeof(xgpu_stats_result), sizeof(xgpu_stats_result), 8));
    const size_t hist_need = stats_hist_size(p, bd);
    if (hist_need) {
        ARGCHK(c, d_hist != NULL);
        TRY(check_dst(c, "pic_stats: histogram", d_hist, hist_size, hist_need, 4));
    }
    float lin[STATS_MAX_BINS];
    const bool new_lin = p->light && (c->stats_lin_tc != p->transfer || c->stats_lin_bd != bd);
    if (new_lin) TRY(xgpu_stats_lin(p->transfer, bd, lin));      // (cannot fail: the check has passed)
    if (!c->stats_blk && hipMalloc((void **)&c->stats_blk, STATS_BLK_BYTES) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(c->err, sizeof(c->err), "%s: cannot allocate the %zu-byte block of the context", who, (size_t)STATS_BLK_BYTES);
        return XGPU_ERR_OUT_OF_MEMORY;
    }
    hipStream_t s;
    TRY(out_fork(c, stream, &s));
    StatsArgs a;
    memset(&a, 0, sizeof(a));
    a.acc = (uint32_t *)c->stats_blk;
    a.lin = (const float *)(c->stats_blk + STATS_ACC_BYTES);
    a.part = (unsigned long long *)(c->stats_blk + STATS_ACC_BYTES + STATS_LIN_BYTES);
    if (new_lin) {      // behind the fork: after every kernel that read the previous table; no key names the table until the copy is queued (upload_cm's rule)
        c->stats_lin_tc = c->stats_lin_bd = -1;
        HIPCHK(c, hipMemcpyAsync(c->stats_blk + STATS_ACC_BYTES, lin, sizeof(float) << bd, hipMemcpyHostToDevice, s));
        c->stats_lin_tc = p->transfer; c->stats_lin_bd = bd;
    }
    const int *cr = p->crop;
    const int w = c->sp.width - cr[0] - cr[1], h = c->sp.height - cr[2] - cr[3];
    const DevPic &dp = dpic(c, pic);
    const int16_t *pl[3];
    cropped_planes(dp, cr, &pl[0], &pl[1], &pl[2]);
    int tiles = 0;
    for (int k = 0; k < 3; k++) {
        a.a[k] = (const uint16_t *)pl[k]; a.sa[k] = k ? dp.s_c : dp.s_l;
        a.w[k] = k ? w >> 1 : w; a.h[k] = k ? h >> 1 : h;
        a.vec[k] = aligned16((uintptr_t)a.a[k] | ((size_t)a.sa[k] * 2));
        a.tiles_x[k] = (a.w[k] + 63) / 64;
        a.tile_first[k] = tiles;
        tiles += a.tiles_x[k] * ((a.h[k] + 31) / 32);
    }
    a.tile_first[3] = tiles;
    a.bd = bd; a.hist_bits = p->hist_bits; a.pctl_e4[0] = p->pctl_e4[0]; a.pctl_e4[1] = p->pctl_e4[1];
    a.light = p->light;
    if (p->light) {      // the arguments of xgpu_pic_output_device for XGPU_OUT_RGB_PLANAR, XGPU_OUT_U16 without DRA
        xgpu_output_format f;
        memset(&f, 0, sizeof(f));
        f.layout = XGPU_OUT_RGB_PLANAR; f.dtype = XGPU_OUT_U16;
        f.matrix = p->matrix; f.full_range = p->full_range; f.chroma_loc = p->chroma_loc; f.upsample = p->upsample;
        RgbOutArgs &r = a.rgb;
        r.y = pl[0]; r.u = pl[1]; r.v = pl[2];
        r.sy = dp.s_l; r.sc = dp.s_c;
        r.w = w; r.h = h; r.cw = w >> 1; r.ch = h >> 1;
        fill_conversion(c, NULL, &f, r);
        fill_siting(p->chroma_loc, r);
        a.upsample = p->upsample;
    }
    a.res = d_result; a.hist = d_hist;
    launch_stats(a, s);
    return out_join(c, stream, s);      // the slot, before the next picture's kernels may write it; the context's block, before the next call's
}
