// k_output_rois_dev.hip - the descriptor block of the batched regions of interest (k_output_rois.hip) made on the device, from boxes that are already there
// (xgpu_pic_output_device_rois_dev): a detector's boxes never visit the host, and the exact-integer tap construction that dominated
// the host-box call runs here, one lane per table row.  The two passes are k_output_rois.hip's, unchanged: they read the RoiDesc records and the tables this
// kernel writes exactly as they read the host's.
//   k_rois_prepare   grid (capacity), 256 lanes: one workgroup per box.  Every lane derives the box's status from the same uniform loads (the box, the count):
//                    snap (scale_taps.h: the rule xgpu_roi_snap restates on the host), the bounds, the letterbox rule, the ratio limits.  A live, accepted box gets
//                    its four tables - the rows of a table spread over the lanes, each row built by scale_taps.h's two functions exactly as xgpu_scale_taps builds
//                    it (the same int64 numerators, one 64-bit division for the row's first candidate and one per tap) - into its own fixed-size slot; then, behind
//                    a barrier, the lanes check what scale_build_tables checks on the host: rows inside the plane that move right monotonically, and the span 64
//                    image columns reach against the LDS the call was sized for.  Lane 0 writes the record and the result.
// What the host derived from the rectangles - grids, LDS, offsets - comes from the bounds here (rois_dev_layout, xgpu_api.hip), so nothing is read back.
// A box that is not XGPU_ROI_OK gets a record with no width and no inner part: the vertical pass leaves at once, pass 2 stages nothing and writes the pad value
// into every element - or, for an index at or above the count (skip), nothing at all.
#include "xgpu_internal.h"
#include "scale_taps.h"

// one table of one box: row o is lane o % 256's.  Vertical tables row by row (stride kw), horizontal ones transposed (stride N); zeros behind count up to kw.
__device__ __forceinline__ int prep_table(uint8_t *slot, uint32_t off_first, uint32_t off_count, uint32_t off_w, int n, int sub, int site, int N, int filter,
                                          bool transposed)
{
    ScaleAxis ax;
    scale_axis_init(ax, n, sub, site, N, filter);
    int32_t *first = (int32_t *)(slot + off_first), *count = (int32_t *)(slot + off_count);
    int16_t *w = (int16_t *)(slot + off_w);
    for (int o = threadIdx.x; o < N; o += blockDim.x) {
        int32_t i0;
        int64_t U;
        const int cnt = scale_tap_span(ax, o, &i0, &U);
        first[o] = i0;
        count[o] = cnt;
        if (transposed) scale_tap_weights(ax, o, i0, cnt, U, w + o, (size_t)N, ax.kw);
        else            scale_tap_weights(ax, o, i0, cnt, U, w + (size_t)o * ax.kw, 1, ax.kw);
    }
    return transposed ? N : ax.kw;
}

// scale_build_tables' checks on a finished table: bit 0 - a row outside the plane or left of its predecessor; bit 1 (cap >= 0: a horizontal table) - 64 columns
// of the image, in which column 0 of the table is column x_off, reach further than cap samples from an 8-sample-aligned start
__device__ __forceinline__ int check_table(const uint8_t *slot, uint32_t off_first, uint32_t off_count, int n, int N, int x_off, int cap)
{
    const int32_t *first = (const int32_t *)(slot + off_first), *count = (const int32_t *)(slot + off_count);
    int bad = 0;
    for (int o = threadIdx.x; o < N; o += blockDim.x) {
        const int f = first[o], c = count[o];
        if (f < 0 || c < 1 || f + c > n) bad |= 1;
        if (o && (f < first[o - 1] || f + c < first[o - 1] + count[o - 1])) bad |= 1;
    }
    if (cap >= 0)
        for (int g = -x_off + 64 * (int)threadIdx.x; g < N; g += 64 * (int)blockDim.x) {
            const int ob = max(g, 0), ol = min(g + 63, N - 1);
            if (ol >= ob && ((first[ol] + count[ol] + 7) & ~7) - (first[ob] & ~7) > cap) bad |= 2;
        }
    return bad;
}

__global__ __launch_bounds__(256) void k_rois_prepare(const RoisPrepArgs a)
{
    __shared__ int flags;
    const int r = blockIdx.x;
    int live = a.capacity;
    if (a.count) live = min(max(*a.count, 0), a.capacity);
    xgpu_roi used = { 0, 0, 0, 0 };
    int in[4] = { 0, 0, 0, 0 };
    int status = XGPU_ROI_UNUSED;
    if (r < live) {
        status = roi_snap_box(a.box_format, (const uint8_t *)a.boxes + (size_t)r * 16, a.pw, a.ph, &used);
        if (status == XGPU_ROI_OK) {
            if (used.width > a.mw || used.height > a.mh) status = XGPU_ROI_TOO_LARGE;
            else {
                roi_inner(used.width, used.height, a.wd, a.hd, a.fit, in);
                if (!scale_ratio_ok(used.width, in[2]) || !scale_ratio_ok(used.height, in[3])) status = XGPU_ROI_RATIO;
            }
        }
    }
    uint8_t *slot = a.blk + a.tab + (size_t)r * a.slot;
    int st0 = 0, st1 = 0, st2 = 0, st3 = 0;
    if (status == XGPU_ROI_OK) {      // uniform: the box and the count are the same loads in every lane
        if (threadIdx.x == 0) flags = 0;
        const int v = a.chroma_loc >> 1, vsite = v == 0 ? 1 : (v == 1 ? 0 : 2);      // ChromaSampleLocType >> 1: centred, top, bottom - in half luma samples
        st0 = prep_table(slot, a.off_first[0], a.off_count[0], a.off_w[0], used.height, 1, 0, in[3], a.filter, false);
        st1 = prep_table(slot, a.off_first[1], a.off_count[1], a.off_w[1], used.height >> 1, 2, vsite, in[3], a.filter, false);
        st2 = prep_table(slot, a.off_first[2], a.off_count[2], a.off_w[2], used.width, 1, 0, in[2], a.filter, true);
        st3 = prep_table(slot, a.off_first[3], a.off_count[3], a.off_w[3], used.width >> 1, 2, a.chroma_loc & 1, in[2], a.filter, true);
        __syncthreads();
        const int bad = check_table(slot, a.off_first[0], a.off_count[0], used.height, in[3], 0, -1) |
                        check_table(slot, a.off_first[1], a.off_count[1], used.height >> 1, in[3], 0, -1) |
                        check_table(slot, a.off_first[2], a.off_count[2], used.width, in[2], in[0], a.capy) |
                        check_table(slot, a.off_first[3], a.off_count[3], used.width >> 1, in[2], in[0], a.capc);
        if (bad) atomicOr(&flags, bad);
        __syncthreads();
        const int fl = flags;
        if (fl & 1) status = XGPU_ROI_INVALID;
        else if (fl & 2) status = XGPU_ROI_TOO_LARGE;
    }
    if (threadIdx.x) return;
    const bool ok = status == XGPU_ROI_OK;
    RoiDesc d;
    d.dst = (uint64_t)r * a.image_pitch;
    d.x = ok ? used.x : 0; d.y = ok ? used.y : 0; d.w = ok ? used.width : 0; d.h = ok ? used.height : 0;
    d.ix = ok ? in[0] : 0; d.iy = ok ? in[1] : 0; d.iw = ok ? in[2] : 0; d.ih = ok ? in[3] : 0;
    d.mid = (uint32_t)r * a.mid_slot;
    d.mpy = (d.w + 7) & ~7; d.mpc = ((d.w >> 1) + 7) & ~7;
    const uint32_t base = a.tab + (uint32_t)r * a.slot;
    #pragma unroll
    for (int t = 0; t < 4; t++) { d.first[t] = base + a.off_first[t]; d.count[t] = base + a.off_count[t]; d.wt[t] = base + a.off_w[t]; }
    d.stride[0] = st0; d.stride[1] = st1; d.stride[2] = st2; d.stride[3] = st3;
    d.skip = status == XGPU_ROI_UNUSED;
    d.pad_[0] = d.pad_[1] = 0;
    ((RoiDesc *)a.blk)[r] = d;
    if (a.results) {
        xgpu_roi_result res;
        res.status = status;
        res.used.x = d.x; res.used.y = d.y; res.used.width = d.w; res.used.height = d.h;
        res.inner[0] = d.ix; res.inner[1] = d.iy; res.inner[2] = d.iw; res.inner[3] = d.ih;
        a.results[r] = res;
    }
}

void launch_rois_prepare(const RoisPrepArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_rois_prepare, dim3((unsigned)a.capacity), dim3(256), 0, s, a);
}

// the row builder alone, for one table in xgpu_scale_taps' own layout (xgpu_test_scale_taps_device)
__global__ __launch_bounds__(256) void k_test_scale_taps(int n_plane, int subsampling, int siting, int n_dst, int filter, int32_t *first, int32_t *count, int16_t *w,
                                                         int w_stride)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n_dst) return;
    ScaleAxis ax;
    scale_axis_init(ax, n_plane, subsampling, siting, n_dst, filter);
    int32_t i0;
    int64_t U;
    const int cnt = scale_tap_span(ax, o, &i0, &U);
    first[o] = i0;
    count[o] = cnt;
    if (w && cnt <= w_stride) scale_tap_weights(ax, o, i0, cnt, U, w + (size_t)o * w_stride, 1, w_stride);
}

void launch_test_scale_taps(int n_plane, int subsampling, int siting, int n_dst, int filter, int32_t *first, int32_t *count, int16_t *w, int w_stride, hipStream_t s)
{
    hipLaunchKernelGGL(k_test_scale_taps, dim3((unsigned)((n_dst + 255) / 256)), dim3(256), 0, s, n_plane, subsampling, siting, n_dst, filter, first, count, w, w_stride);
}
