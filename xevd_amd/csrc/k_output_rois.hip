// k_output_rois.hip - several rectangles of one decoded picture, each resized to the same dw x dh, converted and normalised, as a batch of images in the caller's
// device memory (xgpu_pic_output_device_rois): the tiles a detector runs on, the boxes a classifier or tracker runs on - [N, 3, H, W] from one call.  Image i is,
// bit for bit, what xgpu_pic_output_device_scaled writes with the crop set to rectangle i (INTEGRATION.md sections 8d, 8e); with XGPU_FIT_LETTERBOX the rectangle
// keeps its shape inside the image and the rest of the image is the pad value.  tests/roi_ref.py restates the batch on top of tests/scale_ref.py.
//
// The two passes are k_output_scaled.hip's - the same lane functions (output_common.h), so the arithmetic exists once - with the rectangle taken from blockIdx.z;
// their bodies are output_resize.h's rois_vertical (the bicubic batch's too) and rois_horizontal, which the colour-managed and linear-light batches run with
// their own policies:
// a call is two launches and one upload however many rectangles it has.  What differs per rectangle lives in one device block the host lays out
// (xgpu_api.hip): a RoiDesc per rectangle - where it lies in the picture, the filtered part of its image, its image in the destination, its own intermediate -
// and behind them the tap tables, one set per distinct (source size, inner size): the tiles of a grid share one.
//   k_rois_vertical     grid (columns of the widest rectangle / 512, rows of the tallest inner part / 4, 3 n): plane blockIdx.z % 3 of rectangle blockIdx.z / 3.
//                       The row index is uniform per wave and the descriptor per workgroup, so descriptor, first / count and the weights are scalar loads.
//                       Workgroups past a smaller rectangle's columns or rows leave at once.
//   k_rois_horizontal   grid (dw / 64, dh / rows, n): 64 columns x `rows` rows of the IMAGE, so that the same lanes that filter also write the pad elements around
//                       the inner part and every destination element is written exactly once.  A workgroup that the inner part does not reach stages nothing.
//                       The LDS a row needs is the widest span of all rectangles (the host measures it for workgroups laid over the image, not the inner part).
// Nothing outside a rectangle reaches a result: taps end at its edge (the tables are made for its size), and what the 16-byte loads of the vertical pass read past
// its width lands in columns of the intermediate no tap reads - as with the crop of the single-image call.
// The same two kernels serve xgpu_pic_output_device_rois_dev (k_output_rois_dev.hip), whose block k_rois_prepare writes on the device: there a record may have no
// width and no inner part (a refused box: the whole image is the pad value) or be marked skip (no element is written), and grids and LDS are sized for the
// call's bounds, not for the boxes.
#pragma clang fp contract(off)
#include "output_resize.h"

__global__ __launch_bounds__(256) void k_rois_vertical(const RoisOutArgs a)
{
    rois_vertical<false>(a);
}

template <bool PLANAR, int DT, template <int> class CONV>
__global__ __launch_bounds__(256) void k_rois_horizontal(const RoisOutArgs a)
{
    rois_horizontal<TriangleRow, PlainPixel<CONV>, true, PLANAR, DT>(a);
}
struct RoisHorizontal {
    template <bool PLANAR, bool RGB, int DT> static auto kernel()
    {
        if constexpr (RGB) return k_rois_horizontal<PLANAR, DT, RgbConv>; else return k_rois_horizontal<PLANAR, DT, YuvConv>;
    }
};

// max_w: the widest rectangle; max_ih: the tallest inner part
void launch_rois_vertical(const RoisOutArgs &a, int max_w, int max_ih, hipStream_t s)
{
    hipLaunchKernelGGL(k_rois_vertical, vertical_grid(max_w, max_ih, (unsigned)(3 * a.n)), dim3(64, 4), 0, s, a);
}

void launch_output_rois(const RoisOutArgs &a, int layout, int dtype, int max_w, int max_ih, hipStream_t s)
{
    launch_rois_vertical(a, max_w, max_ih, s);
    launch_horizontal<RoisHorizontal, TriangleRow>(a, layout, dtype, (unsigned)a.n, s);      // on the widest span of the batch
}
