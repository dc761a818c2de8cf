// overlay_rule.h - the one rule of the overlaid output that the host and the device both run, written once: the snapping of a device box to the rectangle its
// frame is drawn on (xgpu_overlay_box_snap on the host, k_overlay_prepare on the device - INTEGRATION.md section 8s).  Integers but for the float32 steps of the
// F32 box format, each of which is exact.
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/xevd_hip.h"

#define OVL_HD __host__ __device__ __forceinline__
#define OVL_LIMIT (1 << 20)         // positions are clamped to +-2^20: beyond any picture, and every float32 step below is exact

OVL_HD int ovl_clamp_pos(long long v) { return (int)(v < -OVL_LIMIT ? -OVL_LIMIT : v > OVL_LIMIT ? OVL_LIMIT : v); }

// a box of either format -> true and the unclipped rectangle [r[0], r[2]) x [r[1], r[3]), or false: skipped
OVL_HD bool ovl_snap_box(int box_format, const void *box, int r[4])
{
    if (box_format == XGPU_BOX_XYXY_F32) {
        const float *b = (const float *)box;
        for (int k = 0; k < 4; k++) if (!(fabsf(b[k]) <= 3.402823466e38f)) return false;      // finite: the exponent field is not all ones
        const float top = (float)OVL_LIMIT;
        r[0] = (int)floorf(fminf(fmaxf(b[0], -top), top)); r[1] = (int)floorf(fminf(fmaxf(b[1], -top), top));
        r[2] = (int)ceilf(fminf(fmaxf(b[2], -top), top));  r[3] = (int)ceilf(fminf(fmaxf(b[3], -top), top));
    } else {
        const int *b = (const int *)box;
        if (b[2] < 1 || b[3] < 1) return false;
        r[0] = ovl_clamp_pos(b[0]); r[1] = ovl_clamp_pos(b[1]);
        r[2] = ovl_clamp_pos((long long)b[0] + b[2]); r[3] = ovl_clamp_pos((long long)b[1] + b[3]);
    }
    return r[2] > r[0] && r[3] > r[1];
}
