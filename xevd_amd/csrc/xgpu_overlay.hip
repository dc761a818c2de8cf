// xgpu_overlay.hip - the host side of the overlaid output that is not an entry point: the forward matrix of the NV12 / P016 blend, the snapping rule of a device
// box on the host, the checks of a call's layers and boxes that need no device, and the kernels' layer records.  The output calls are xgpu_output.hip's; the
// kernels are k_output_overlay.hip; the contract is INTEGRATION.md section 8s and tests/overlay_ref.py restates it.
#include "xgpu_host.h"
#include "overlay_rule.h"

// R'G'B' in 0 .. 255 -> Y', Cb, Cr codes of depth D: m[i][j] = round(k[i][j] * range_i / 255 * 2^S) with S = 28 - D, built in double - the same expressions,
// term for term, as tests/overlay_ref.py
void overlay_forward_matrix(double kr, double kb, int full_range, int d, int32_t m[9], int32_t off[3], int *shift)
{
    const double kg = 1.0 - kr - kb;
    const double k[9] = { kr, kg, kb,
                          -kr / (2.0 * (1.0 - kb)), -kg / (2.0 * (1.0 - kb)), 0.5,
                          0.5, -kg / (2.0 * (1.0 - kr)), -kb / (2.0 * (1.0 - kr)) };
    const int s = 28 - d;
    const double yr = full_range ? (double)((1 << d) - 1) : (double)(219 << (d - 8)), cr = full_range ? (double)((1 << d) - 1) : (double)(224 << (d - 8));
    for (int i = 0; i < 9; i++) m[i] = (int32_t)round(k[i] * (i < 3 ? yr : cr) / 255.0 * (double)(1 << s));      // half away from zero
    off[0] = full_range ? 0 : 16 << (d - 8);
    off[1] = off[2] = 1 << (d - 1);
    *shift = s;
}

int xgpu_overlay_box_snap(int box_format, const void *box, int rect[4])
{
    if ((box_format != XGPU_BOX_XYWH_I32 && box_format != XGPU_BOX_XYXY_F32) || !box || !rect) return XGPU_ERR_INVALID_ARGUMENT;
    int r[4];
    const bool live = ovl_snap_box(box_format, box, r);
    for (int k = 0; k < 4; k++) rect[k] = live ? r[k] : 0;
    return live ? 1 : 0;
}

static int layer_bpp(int kind) { return kind == XGPU_OVL_A8 ? 1 : 4; }

// the refusals of a call's layers and boxes that look at the arguments alone; 0 or XGPU_ERR_INVALID_ARGUMENT with `why`
int overlay_layers_check(const xgpu_overlay_layer *layers, int n, const xgpu_overlay_boxes *boxes, const char **why)
{
    *why = "0 .. XGPU_MAX_OVERLAY_LAYERS layers, the list not NULL";
    if (n < 0 || n > XGPU_MAX_OVERLAY_LAYERS || (n && !layers)) return XGPU_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++) {
        const xgpu_overlay_layer &l = layers[i];
        *why = "layer: kind must be one of XGPU_OVL_RGBA8 .. XGPU_OVL_BOX";
        if (l.kind < XGPU_OVL_RGBA8 || l.kind > XGPU_OVL_BOX) return XGPU_ERR_INVALID_ARGUMENT;
        *why = "layer: |x|, |y| <= 1 << 20, width and height 1 .. 16384, opacity 0 .. 255";
        if (l.x < -OVL_LIMIT || l.x > OVL_LIMIT || l.y < -OVL_LIMIT || l.y > OVL_LIMIT || l.width < 1 || l.width > 16384 || l.height < 1 || l.height > 16384 ||
            l.opacity < 0 || l.opacity > 255)
            return XGPU_ERR_INVALID_ARGUMENT;
        if (l.kind == XGPU_OVL_BOX) {
            *why = "layer: a box needs thickness >= 1";
            if (l.thickness < 1) return XGPU_ERR_INVALID_ARGUMENT;
            continue;
        }
        const size_t bpp = (size_t)layer_bpp(l.kind), row = (size_t)l.width * bpp;
        *why = "layer: a bitmap needs d_pixels, aligned to its pixel";
        if (!l.d_pixels || (uintptr_t)l.d_pixels % bpp) return XGPU_ERR_INVALID_ARGUMENT;
        *why = "layer: pitch is shorter than a row, not a multiple of the pixel, or above 2^31";
        if (l.pitch && (l.pitch < row || l.pitch % bpp || l.pitch > ((size_t)1 << 31))) return XGPU_ERR_INVALID_ARGUMENT;
    }
    if (boxes) {
        *why = "boxes: box_format XGPU_BOX_XYWH_I32 or XGPU_BOX_XYXY_F32, capacity 1 .. XGPU_MAX_OVERLAY_BOXES, n_palette 1 .. 16, thickness >= 1, fill_alpha 0 .. 255";
        if ((boxes->box_format != XGPU_BOX_XYWH_I32 && boxes->box_format != XGPU_BOX_XYXY_F32) || boxes->capacity < 1 || boxes->capacity > XGPU_MAX_OVERLAY_BOXES ||
            boxes->n_palette < 1 || boxes->n_palette > 16 || boxes->thickness < 1 || boxes->fill_alpha < 0 || boxes->fill_alpha > 255)
            return XGPU_ERR_INVALID_ARGUMENT;
        *why = "boxes: d_boxes is NULL, or an array is not aligned to 4";
        if (!boxes->d_boxes || ((uintptr_t)boxes->d_boxes | (uintptr_t)boxes->d_count | (uintptr_t)boxes->d_labels) % 4) return XGPU_ERR_INVALID_ARGUMENT;
    }
    return XGPU_OK;
}

// the bytes of layer l's bitmap the kernels may read: (height - 1) * pitch + width * bpp; 0 for a box
size_t overlay_layer_bytes(const xgpu_overlay_layer &l)
{
    if (l.kind == XGPU_OVL_BOX) return 0;
    const size_t row = (size_t)l.width * layer_bpp(l.kind);
    return (size_t)(l.height - 1) * (l.pitch ? l.pitch : row) + row;
}

static uint32_t rgba_word(const uint8_t c[4]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24); }

// checked layers and boxes -> the kernels' records (blk: the context's block k_overlay_prepare fills, or NULL without boxes)
void overlay_fill_args(const xgpu_overlay_layer *layers, int n, const xgpu_overlay_boxes *boxes, const OvlBlock *blk, int maxv, OvlArgs &o)
{
    o.boxes = boxes ? blk : NULL;
    o.n = n;
    o.maxv = maxv;
    o.box_thickness = boxes ? boxes->thickness : 1;
    o.box_fill_alpha = boxes ? boxes->fill_alpha : 0;
    for (int i = 0; i < n; i++) {
        const xgpu_overlay_layer &l = layers[i];
        OvlLayer &d = o.layer[i];
        d.x0 = l.x; d.y0 = l.y; d.x1 = l.x + l.width; d.y1 = l.y + l.height;
        d.kind = l.kind; d.opacity = l.opacity; d.thickness = l.kind == XGPU_OVL_BOX ? l.thickness : 0;
        d.colour = rgba_word(l.colour); d.fill = rgba_word(l.fill);
        d.pix = l.kind == XGPU_OVL_BOX ? NULL : (const uint8_t *)l.d_pixels;
        d.pitch = l.kind == XGPU_OVL_BOX ? 0 : (uint32_t)(l.pitch ? l.pitch : (size_t)l.width * layer_bpp(l.kind));
    }
}

void overlay_fill_prepare(const xgpu_overlay_boxes *boxes, OvlBlock *blk, int pw, int ph, OvlPrepArgs &p)
{
    memset(&p, 0, sizeof(p));
    p.blk = blk; p.boxes = boxes->d_boxes; p.count = boxes->d_count; p.labels = boxes->d_labels;
    p.capacity = boxes->capacity; p.box_format = boxes->box_format; p.n_palette = boxes->n_palette;
    p.pw = pw; p.ph = ph;
    for (int i = 0; i < 16; i++) p.palette[i] = rgba_word(boxes->palette[i]);
}
