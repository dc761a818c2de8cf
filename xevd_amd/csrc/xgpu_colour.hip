// xgpu_colour.hip - host side of the colour-managed RGB output (xgpu_colour_tables, include/xevd_hip.h) and of the light level (xgpu_stats_lin): the transfer characteristics of H.273 / BT.2100,
// the primaries matrices from the H.273 chromaticities, the BT.2390 EETF and the tables k_output_cm.hip reads.  Everything in double precision, rounded
// to float32 once; no device code.  tests/colour_cm_ref.py states the same formulae in numpy float64 and compares entry by entry.
#include "xgpu_internal.h"
#include <cmath>

namespace {

// H.273 TransferCharacteristics 1 / 6 / 14 / 15 and 13: alpha, beta of the piecewise curves
constexpr double A709 = 1.09929682680944, B709 = 0.018053968510807;
constexpr double ASRGB = 1.055, BSRGB = 0.0031308;
// SMPTE ST 2084
constexpr double PQ_M1 = 2610.0 / 16384.0, PQ_M2 = 2523.0 / 4096.0 * 128.0, PQ_C1 = 3424.0 / 4096.0, PQ_C2 = 2413.0 / 4096.0 * 32.0, PQ_C3 = 2392.0 / 4096.0 * 32.0;
// BT.2100 HLG
constexpr double HLG_A = 0.17883277, HLG_B = 1.0 - 4.0 * HLG_A;
const double HLG_C = 0.5 - HLG_A * std::log(4.0 * HLG_A);

int transfer_class(int tc)      // the curve of a TransferCharacteristics code point; 0: not supported
{
    switch (tc) {
    case 1: case 6: case 14: case 15: return 1;
    case 4: case 5: case 8: case 13: case 16: case 18: return tc;
    default: return 0;
    }
}
// linear light v in [0, 1] -> the encoded value in [0, 1]
double tc_forward(int cls, double v)
{
    switch (cls) {
    case 1:  return v < B709 ? 4.5 * v : A709 * std::pow(v, 0.45) - (A709 - 1.0);
    case 4:  return std::pow(v, 1.0 / 2.2);
    case 5:  return std::pow(v, 1.0 / 2.8);
    case 13: return v < BSRGB ? 12.92 * v : ASRGB * std::pow(v, 1.0 / 2.4) - (ASRGB - 1.0);
    case 16: { const double p = std::pow(v, PQ_M1); return std::pow((PQ_C1 + PQ_C2 * p) / (1.0 + PQ_C3 * p), PQ_M2); }
    case 18: return v <= 1.0 / 12.0 ? std::sqrt(3.0 * v) : HLG_A * std::log(12.0 * v - HLG_B) + HLG_C;
    default: return v;
    }
}
// the encoded value e in [0, 1] -> linear light
double tc_inverse(int cls, double e)
{
    switch (cls) {
    case 1:  return e < 4.5 * B709 ? e / 4.5 : std::pow((e + (A709 - 1.0)) / A709, 1.0 / 0.45);
    case 4:  return std::pow(e, 2.2);
    case 5:  return std::pow(e, 2.8);
    case 13: return e < 12.92 * BSRGB ? e / 12.92 : std::pow((e + (ASRGB - 1.0)) / ASRGB, 2.4);
    case 16: { const double p = std::pow(e, 1.0 / PQ_M2); return std::pow(std::fmax(p - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * p), 1.0 / PQ_M1); }
    case 18: return e <= 0.5 ? e * e / 3.0 : (std::exp((e - HLG_C) / HLG_A) + HLG_B) / 12.0;
    default: return e;
    }
}

// chromaticities (xr, yr, xg, yg, xb, yb) of the supported ColourPrimaries; the white point of all of them is D65
const double *primaries_xy(int cp)
{
    static const double bt709[6] = { 0.640, 0.330, 0.300, 0.600, 0.150, 0.060 }, bt601_625[6] = { 0.640, 0.330, 0.290, 0.600, 0.150, 0.060 },
                        bt601_525[6] = { 0.630, 0.340, 0.310, 0.595, 0.155, 0.070 }, bt2020[6] = { 0.708, 0.292, 0.170, 0.797, 0.131, 0.046 },
                        p3d65[6] = { 0.680, 0.320, 0.265, 0.690, 0.150, 0.060 };
    switch (cp) {
    case 1: return bt709;
    case 5: return bt601_625;
    case 6: case 7: return bt601_525;
    case 9: return bt2020;
    case 12: return p3d65;
    default: return NULL;
    }
}
void inv3(const double m[9], double o[9])
{
    const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    o[0] = c0 / det; o[1] = (m[2] * m[7] - m[1] * m[8]) / det; o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    o[3] = c1 / det; o[4] = (m[0] * m[8] - m[2] * m[6]) / det; o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    o[6] = c2 / det; o[7] = (m[1] * m[6] - m[0] * m[7]) / det; o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}
// RGB -> XYZ of a set of primaries with white D65 (Y of white = 1)
void rgb_to_xyz(const double *xy, double m[9])
{
    const double xw = 0.3127, yw = 0.3290;
    double p[9], pi[9];
    for (int k = 0; k < 3; k++) { const double x = xy[2 * k], y = xy[2 * k + 1]; p[k] = x / y; p[3 + k] = 1.0; p[6 + k] = (1.0 - x - y) / y; }
    inv3(p, pi);
    const double w[3] = { xw / yw, 1.0, (1.0 - xw - yw) / yw };
    for (int k = 0; k < 3; k++) {
        const double s = pi[3 * k] * w[0] + pi[3 * k + 1] * w[1] + pi[3 * k + 2] * w[2];
        for (int r = 0; r < 3; r++) m[3 * r + k] = p[3 * r + k] * s;
    }
}

// Report BT.2390 section 5.4.1 with black levels 0: display luminance `l` (cd/m2) of a display of peak lw -> of one of peak lmax
double eetf(double l, double lw, double lmax)
{
    if (lmax >= lw) return l;      // nothing to compress; what exceeds the destination's range meets the clip of step 3
    const double pw = tc_forward(16, lw / 10000.0), max_lum = tc_forward(16, lmax / 10000.0) / pw, ks = 1.5 * max_lum - 0.5;
    const double e1 = std::fmin(tc_forward(16, l / 10000.0) / pw, 1.0);
    double e2 = e1;
    if (e1 >= ks) {
        const double t = (e1 - ks) / (1.0 - ks), t2 = t * t, t3 = t2 * t;
        e2 = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * max_lum;
    }
    return 10000.0 * tc_inverse(16, e2 * pw);
}
double default_peak(int cls) { return cls == 16 || cls == 18 ? 1000.0 : 100.0; }

struct ToneCurve {
    int src_cls;
    double src_peak, dst_peak, dst_white, gamma;
    // g(Y): source luminance y in [0, 1] -> the destination's linear light
    double g(double y) const
    {
        const double ld = src_cls == 16 ? 10000.0 * y : (src_cls == 18 ? src_peak * std::pow(y, gamma) : src_peak * y);
        return eetf(ld, src_peak, dst_peak) / dst_white;
    }
};

float curve_x(int j)      // the sample point of entry j + 1
{
    const uint32_t u = XGPU_CM_CURVE_U0 + ((uint32_t)j << 18);
    float x;
    memcpy(&x, &u, sizeof(x));
    return x;
}

// step 1's table at coding depth bd: linear light of the code k, k = 0 .. 2^bd - 1 (xgpu_colour_tables and xgpu_stats_lin: one construction)
void make_lin(int cls, int bit_depth, float *lin)
{
    const int n = 1 << bit_depth;
    const double maxv = (double)(n - 1);
    for (int k = 0; k < n; k++) lin[k] = (float)tc_inverse(cls, (double)k / maxv);
}

}      // namespace

bool colour_transfer_supported(int tc) { return transfer_class(tc) != 0; }
int xgpu_stats_lin(int transfer, int bit_depth, float lin[4096])
{
    if (!lin || bit_depth < 8 || bit_depth > 12) return XGPU_ERR_INVALID_ARGUMENT;
    const int cls = transfer_class(transfer);
    if (!cls) return XGPU_ERR_UNSUPPORTED;
    memset(lin, 0, sizeof(float) * 4096);
    make_lin(cls, bit_depth, lin);
    return XGPU_OK;
}

int xgpu_colour_tables(const xgpu_output_format *f, const xgpu_colour_transform *cm, int bit_depth, xgpu_colour_tables_t *out)
{
    if (!f || !cm || !out || bit_depth < 8 || bit_depth > 12) return XGPU_ERR_INVALID_ARGUMENT;
    if (f->layout != XGPU_OUT_RGB_PLANAR && f->layout != XGPU_OUT_RGB_INTERLEAVED) return XGPU_ERR_INVALID_ARGUMENT;
    int32_t coef[5];
    int shift;
    float fcoef[5];
    const int rc = xgpu_output_coeffs(f, bit_depth, coef, &shift, fcoef);      // the rest of the format
    if (rc < 0) return rc;
    const int sc = transfer_class(cm->src_transfer), dc = transfer_class(cm->dst_transfer);
    const double *sxy = primaries_xy(cm->src_primaries), *dxy = primaries_xy(cm->dst_primaries);
    if (!sc || !dc || !sxy || !dxy) return XGPU_ERR_UNSUPPORTED;
    if ((cm->tone_map & ~1) || !(cm->src_peak >= 0.f) || !(cm->dst_peak >= 0.f) || !(cm->linear_scale >= 0.f) ||
        !std::isfinite(cm->src_peak) || !std::isfinite(cm->dst_peak) || !std::isfinite(cm->linear_scale)) return XGPU_ERR_INVALID_ARGUMENT;
    if (cm->tone_map && dc == 18) return XGPU_ERR_UNSUPPORTED;

    memset(out, 0, sizeof(*out));
    out->n_lin = 1 << bit_depth;
    make_lin(sc, bit_depth, out->lin);

    double s2x[9], d2x[9], x2d[9];
    rgb_to_xyz(sxy, s2x);
    rgb_to_xyz(dxy, d2x);
    inv3(d2x, x2d);
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) out->matrix[3 * r + k] = (float)(x2d[3 * r] * s2x[k] + x2d[3 * r + 1] * s2x[3 + k] + x2d[3 * r + 2] * s2x[6 + k]);
    for (int k = 0; k < 3; k++) out->luma[k] = (float)s2x[3 + k];
    out->use_matrix = sxy != dxy;
    if (!out->use_matrix)
        for (int k = 0; k < 9; k++) out->matrix[k] = k % 4 == 0 ? 1.f : 0.f;

    out->scale = cm->linear_scale == 0.f ? 1.f : cm->linear_scale;
    out->use_tone = cm->tone_map;
    if (cm->tone_map) {
        ToneCurve t;
        t.src_cls = sc;
        t.src_peak = cm->src_peak == 0.f ? default_peak(sc) : (double)cm->src_peak;
        t.dst_peak = cm->dst_peak == 0.f ? default_peak(dc) : (double)cm->dst_peak;
        t.dst_white = dc == 16 ? 10000.0 : t.dst_peak;
        t.gamma = 1.2 + 0.42 * std::log10(t.src_peak / 1000.0);
        out->tone[0] = (float)t.g(0.0);
        for (int j = 0; j <= 2048; j++) out->tone[j + 1] = (float)t.g((double)curve_x(j));
        out->tone[XGPU_CM_CURVE_SIZE - 1] = out->tone[XGPU_CM_CURVE_SIZE - 2];
    }
    out->use_encode = dc != 8;
    if (out->use_encode) {
        out->encode[0] = (float)tc_forward(dc, 0.0);
        for (int j = 0; j <= 2048; j++) out->encode[j + 1] = (float)tc_forward(dc, (double)curve_x(j));
        out->encode[XGPU_CM_CURVE_SIZE - 1] = out->encode[XGPU_CM_CURVE_SIZE - 2];
    }
    return XGPU_OK;
}
