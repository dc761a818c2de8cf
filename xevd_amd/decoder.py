"""Host-side mirror of the reference's coarse decode sequence for the reconstruction path, over the C ABI.

Mirrors, per picture, what xevd_dec_nalu does after entropy decoding (src_base/xevd.c:1890-1983):
    slice/refp set-up -> recon of every CU -> deblock (vertical edges, then horizontal) -> picbuf_expand -> DPB
Plumbing only (ctypes + numpy); all arithmetic happens in xevd_amd/libxevd_hip.so.  There is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import abi


_DTYPE_CODES = {}      # accepted names -> {torch dtype: XGPU_OUT_* code}; each subset is made at its first use, because torch is imported inside the methods


def _codes(*names):
    """the torch dtypes an output accepts -> their XGPU_OUT_* codes: those called `names` in torch, or - no names - all of them (uint16 where torch has it)"""
    codes = _DTYPE_CODES.get(names)
    if codes is None:
        import torch
        every = {"uint8": abi.OUT_U8, "int16": abi.OUT_U16, "uint16": abi.OUT_U16, "float16": abi.OUT_F16, "bfloat16": abi.OUT_BF16, "float32": abi.OUT_F32}
        codes = _DTYPE_CODES[names] = {getattr(torch, n): every[n] for n in (names or every) if getattr(torch, n, None) is not None}
    return codes


def _out_tensor(out, shape, dtype, dev):
    """the tensor an output fills: `out` if it has that shape, dtype and device, a new one for None"""
    if out is None:
        import torch
        out = torch.empty(shape, dtype=dtype, device=dev)
    if out.device != dev or out.dtype != dtype or out.shape != tuple(shape):
        raise ValueError(f"out: expected {tuple(shape)} {dtype} on {dev}, got {tuple(out.shape)} {out.dtype} on {out.device}")
    return out


_IMAGE_ROWS = ("W x 3 elements ", "W elements in planes of H rows ")      # how _row_pitch names the rows of an [h, W, 3] / [3, h, W] image


def _row_pitch(st, planar, h, row, last, what=None):
    """The elements between two rows of a tensor with strides st whose last three dimensions are planes [C, h, W] (planar: dense rows of `row` elements, planes of h
    rows) or pixels [h, W, last] (rows of `row` = W * last elements); a leading image stride (a batch) is free.  `what`: how the ValueError names such rows
    (None: as the rows of an image of the picture outputs)."""
    s = st[-3:]
    pitch = s[1] if planar else s[0]
    if (planar and (s[2] != 1 or s[0] != pitch * h)) or (not planar and s[1:] != (last, 1)) or pitch < row:
        raise ValueError(f"out: strides {st} are not rows of {what or _IMAGE_ROWS[planar]}")
    return pitch


class XgpuError(RuntimeError):
    pass


class XgpuDecoder:
    def __init__(self, width, height, bit_depth=8, device=0, log2_ctu=6, iqt=0, admvp=0, addb=0, alf=0, max_pics=6,
                 bit_depth_chroma=None, chroma_qp_tables=None, eipd=0):
        self.lib = abi.load()
        self.sp = abi.make_seq_params(width, height, bit_depth, log2_ctu, device, iqt, admvp, addb, alf, max_pics,
                                      bit_depth_chroma, eipd)
        self._tables = None
        if chroma_qp_tables is not None:
            self._tables = [np.ascontiguousarray(t, np.int8) for t in chroma_qp_tables]
            for i in range(2):
                self.sp.chroma_qp_table[i] = self._tables[i].ctypes.data_as(C.POINTER(C.c_int8))
        self.ctx = C.c_void_p()
        rc = self.lib.xgpu_open(C.byref(self.sp), C.byref(self.ctx))
        if rc != 0:
            raise XgpuError(f"xgpu_open failed: {rc}")
        self.width, self.height, self.bit_depth = width, height, bit_depth
        self._batches = []

    # -- helpers -------------------------------------------------------------------------------------
    def _chk(self, rc, what):
        if rc < 0:
            raise XgpuError(f"{what} failed: {rc}: {self.lib.xgpu_last_error(self.ctx).decode()}")
        return rc

    def close(self):
        if self.ctx:
            for b in self._batches:
                self.lib.xgpu_batch_destroy(self.ctx, b)
            self._batches = []
            self.lib.xgpu_close(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        self._chk(self.lib.xgpu_sync(self.ctx), "xgpu_sync")

    # -- pictures ------------------------------------------------------------------------------------
    def pic_alloc(self):
        return self._chk(self.lib.xgpu_pic_alloc(self.ctx), "xgpu_pic_alloc")

    def pic_free(self, pic):
        self._chk(self.lib.xgpu_pic_free(self.ctx, pic), "xgpu_pic_free")

    def pic_upload(self, pic, planes):
        y, u, v = (np.ascontiguousarray(p, np.int16) for p in planes)
        self._chk(self.lib.xgpu_pic_upload(self.ctx, pic, y.ctypes.data, y.shape[1], u.ctypes.data, v.ctypes.data, u.shape[1]),
                  "xgpu_pic_upload")

    def pic_download(self, pic):
        y = np.zeros((self.height, self.width), np.int16)
        u = np.zeros((self.height // 2, self.width // 2), np.int16)
        v = np.zeros_like(u)
        self._chk(self.lib.xgpu_pic_download(self.ctx, pic, y.ctypes.data, self.width, u.ctypes.data, v.ctypes.data, self.width // 2),
                  "xgpu_pic_download")
        return [y, u, v]

    def pic_output(self, pic, out_bit_depth=0, crop=(0, 0, 0, 0), dra=None):
        """The picture as the bytes of a .yuv file frame (Y, U, V planes, tight rows): converted to `out_bit_depth` (0 = the coding
        depth; 8 -> one byte per sample) and cropped by (left, right, top, bottom) luma samples on the device (xgpu_pic_output).
        dra: (luma_inv_scale_lut, cb_inv_scale_lut, cr_inv_scale_lut), 1024 int32 each - the DRA post-filter's tables."""
        bd = out_bit_depth or self.bit_depth
        n = self.lib.xgpu_pic_output_size(self.ctx, bd, *crop)
        if n == 0:
            raise ValueError(f"invalid output format: bit depth {bd}, crop {crop}")
        out = np.empty(n, np.uint8)
        dl, keep = self._dra_luts(dra)
        self._chk(self.lib.xgpu_pic_output(self.ctx, pic, dl, bd, *crop, out.ctypes.data, n), "xgpu_pic_output")
        return out

    @staticmethod
    def _dra_luts(dra):
        """(luma, cb, cr) inverse tables -> (byref(xgpu_dra_luts) or None, keepalive)"""
        if dra is None:
            return None, None
        keep = [np.ascontiguousarray(t, np.int32) for t in dra]
        assert all(t.size == 1024 for t in keep)
        d = abi.DraLuts()
        d.luma_inv_scale_lut = keep[0].ctypes.data
        d.chroma_inv_scale_lut[0], d.chroma_inv_scale_lut[1] = keep[1].ctypes.data, keep[2].ctypes.data
        return C.byref(d), (keep, d)

    def pic_output_tensor(self, pic, layout="rgb", channels_last=False, dtype=None, matrix=1, full_range=False, chroma_loc=0, upsample="linear",
                          crop=(0, 0, 0, 0), dra=None, out=None, bgr=False, out_bit_depth=0, colour=None, size=None, filter="bilinear", mean=None, std=None,
                          rois=None, fit="stretch", pad=0.0, snap=False, count=None, max_roi=None, results=False):
        """The picture in device memory as a torch tensor on cuda:{device}, converted on the device (xgpu_pic_output_device) on torch's current
        stream - no host round trip.  layout "rgb": [3, H, W] (channels_last: [H, W, 3]) R'G'B' (bgr: B, G, R) with dtype torch.uint8, torch.int16 /
        torch.uint16 (values at the coding depth), torch.float16, torch.bfloat16 or torch.float32 (0..1), through `matrix` (H.273 MatrixCoefficients
        1, 4, 5, 6, 7, 9), full_range, chroma_loc (ChromaSampleLocType 0..5) and upsample "linear" / "nearest"; layout "yuv420p": the bytes of
        pic_output (1-D, uint8 for 8-bit output - dtype torch.uint8 - else 16-bit samples at the coding depth).
        Video surfaces: layout "nv12": [H * 3 // 2, W] - H luma rows, then H / 2 rows Cb0 Cr0 Cb1 Cr1 ... - torch.uint8 (8-bit samples), or a 16-bit
        integer type with the samples at out_bit_depth (0 = the coding depth) in the low bits; "p016": the same shape, 16-bit, sample << (16 - D) with
        D = out_bit_depth (0 = the coding depth; 10 is P010, 12 is P012); "yuv444": [3, H, W] (channels_last: [H, W, 3]) Y, Cb, Cr at luma resolution
        (chroma upsampled by upsample / chroma_loc as for "rgb"): torch.uint8 (8-bit samples), 16-bit integers (the coding depth) or floats - H.273's
        E'Y in 0..1, E'Cb and E'Cr in -0.5..0.5 by full_range.  out_bit_depth: "nv12" / "p016" only; for "rgb" / "yuv444" it must be 0 or the coding depth.
        colour: layout "rgb" only - dict(src_primaries, src_transfer, dst_primaries, dst_transfer, tone_map, src_peak, dst_peak, linear_scale) (the keyword
        arguments of abi.make_colour_transform: H.273 code points, peaks in cd/m2): the R'G'B' of the stream's colour space linearised, taken to the
        destination primaries, tone-mapped or scaled, and re-encoded with the destination transfer (8 = linear light) in the same kernel
        (xgpu_pic_output_device_cm).
        crop: (left, right, top, bottom), even.  out: a tensor to fill instead (its strides may pad the rows: row_pitch); it is also what is returned.
        size=(H, W): layouts "rgb" / "yuv444" resized to H x W on the device (xgpu_pic_output_device_scaled) - the crop is the region
        of interest, filter "bilinear" (the antialiased triangle of torch's interpolate(antialias=True)) or "area"; the chroma planes are filtered straight onto
        the destination grid (upsample is not read).  mean / std (float dtypes; three values or one): out = (v - mean[k]) * (float32(1) / float32(std[k])), k the
        channel's position in the output.  size=None: the unscaled call, and filter / mean / std must be left alone.  size= together with colour= raises
        ValueError here, with and without rois=: that combination is pic_output_scaled_cm(pic, size, colour, ...).
        rois=[(x, y, w, h), ...] (with size=): every rectangle - luma samples inside the picture minus the crop, even - resized to H x W in one call
        (xgpu_pic_output_device_rois): [N, 3, H, W] (channels_last: [N, H, W, 3]); image i is what size= with the crop set to
        rectangle i gives.  fit "stretch", or "letterbox": the rectangle keeps its shape inside the image (abi.roi_inner says where) and the rest is `pad` - one
        value or three, in the output's channel order, before the normalise; integers for the integer dtypes.  snap=True rounds odd rectangles outward to even
        and clamps them to the picture; otherwise such a rectangle raises ValueError.  out: any tensor of that shape whose images are laid out as size= lays
        out its one image, a batch stride apart.
        rois=<torch tensor on the decoder's device> (with size=): the boxes a detector left on the GPU, read there (xgpu_pic_output_device_rois_dev, INTEGRATION.md
        section 8f) - int32 [N, 4] (x, y, w, h) or float32 [N, 4] (x1, y1, x2, y2), contiguous; no host read, no synchronisation.  Every box is snapped outward to
        even and into the picture (abi.roi_snap restates the rule); image i is what rois=[used_i] gives.  count=<int32 tensor of one element>: the first
        min(max(count, 0), N) boxes are live, the images of the others are not touched.  max_roi=(H, W): the largest snapped box the call is sized for (default: the
        picture minus the crop).  A box that cannot be served - a non-finite coordinate, empty after snapping, larger than max_roi, a ratio outside the scaled
        output's limits - gives an image that is all `pad` (so pad is checked for either fit).  results=True returns (images, results): results int32 [N, 9] =
        status (abi.ROI_OK, ROI_UNUSED, ROI_INVALID, ROI_EMPTY, ROI_TOO_LARGE, ROI_RATIO), the box used (x, y, w, h), its inner part (abi.roi_inner)."""
        import torch
        if size is not None:      # every argument the scaled, ROI and device-box paths read, by its name
            a = {"pic": pic, "layout": layout, "channels_last": channels_last, "dtype": dtype, "matrix": matrix, "full_range": full_range, "chroma_loc": chroma_loc,
                 "crop": crop, "dra": dra, "out": out, "bgr": bgr, "out_bit_depth": out_bit_depth, "colour": colour, "size": size, "filter": filter, "mean": mean,
                 "std": std, "rois": rois, "fit": fit, "pad": pad, "snap": snap, "count": count, "max_roi": max_roi, "results": results}
        if rois is not None:
            if size is None:
                raise ValueError("rois: the batch of rectangles needs size=(H, W)")
            if isinstance(rois, torch.Tensor):
                if snap:
                    raise ValueError("snap: boxes in device memory are always snapped")
                return self._pic_output_tensor_rois_dev(a)
            if count is not None or max_roi is not None or results:
                raise ValueError("count, max_roi and results belong to rois=<tensor on the device>")
            return self._pic_output_tensor_rois(a)
        pad_set = pad != 0 if isinstance(pad, (int, float)) else np.any(np.asarray(pad) != 0)
        if fit != "stretch" or snap or pad_set or count is not None or max_roi is not None or results:
            raise ValueError("fit, pad, snap, count, max_roi and results belong to rois=")
        if size is not None:
            return self._pic_output_tensor_scaled(a)
        if filter != "bilinear" or mean is not None or std is not None:
            raise ValueError("filter, mean and std belong to the scaled output: they need size=(H, W)")
        if dtype is None:
            dtype = torch.int16 if layout == "p016" else torch.uint8      # P016 has 16-bit words only
        codes = _codes()
        if dtype not in codes:
            raise ValueError(f"unsupported output dtype {dtype}")
        if upsample not in ("linear", "nearest"):
            raise ValueError(f"upsample must be 'linear' or 'nearest', not {upsample!r}")
        if colour is not None and layout != "rgb":
            raise ValueError(f"colour: a colour transform needs layout 'rgb', not {layout!r}")
        cl, cr, ct, cb = (int(v) for v in crop)
        w, h = self.width - cl - cr, self.height - ct - cb
        dev = torch.device("cuda", self.sp.device)
        obd = int(out_bit_depth)
        up = abi.UPSAMPLE_LINEAR if upsample == "linear" else abi.UPSAMPLE_NEAREST
        if layout in ("rgb", "yuv444") and obd not in (0, self.bit_depth):
            raise ValueError(f"{layout}: out_bit_depth must be 0 or the coding depth {self.bit_depth}, not {obd}")
        if layout == "yuv420p":
            if codes[dtype] not in (abi.OUT_U8, abi.OUT_U16):
                raise ValueError("yuv420p: dtype torch.uint8 (8-bit output) or a 16-bit integer type (the coding depth)")
            fmt = abi.make_output_format(abi.OUT_YUV420P, codes[dtype], out_bit_depth=8 if codes[dtype] == abi.OUT_U8 else self.bit_depth, crop=crop)
            n = self.lib.xgpu_pic_output_device_size(self.ctx, C.byref(fmt))
            if n == 0:
                raise ValueError(f"invalid output format: crop {crop}")
            shape = (n // dtype.itemsize,)
        elif layout in ("nv12", "p016"):
            if codes[dtype] != abi.OUT_U16 and (layout == "p016" or codes[dtype] != abi.OUT_U8):
                raise ValueError(f"{layout}: dtype must be a 16-bit integer type{' or torch.uint8 (8-bit samples)' if layout == 'nv12' else ''}")
            if codes[dtype] == abi.OUT_U8:
                if obd not in (0, 8):
                    raise ValueError("nv12: torch.uint8 holds 8-bit samples; out_bit_depth above 8 needs a 16-bit integer dtype")
                obd = 8
            shape = (h * 3 // 2, w)
            fmt = abi.make_output_format(abi.OUT_NV12 if layout == "nv12" else abi.OUT_P016, codes[dtype], out_bit_depth=obd, crop=crop)
        elif layout in ("rgb", "yuv444"):
            lay = (abi.OUT_RGB_INTERLEAVED, abi.OUT_RGB_PLANAR) if layout == "rgb" else (abi.OUT_YUV444_INTERLEAVED, abi.OUT_YUV444_PLANAR)
            fmt = abi.make_output_format(lay[0] if channels_last else lay[1], codes[dtype], bgr=bgr, matrix=matrix, full_range=full_range,
                                         chroma_loc=chroma_loc, upsample=up, crop=crop)
        else:
            raise ValueError(f"layout must be 'rgb', 'yuv420p', 'nv12', 'p016' or 'yuv444', not {layout!r}")
        if layout in ("rgb", "yuv444"):
            out = _out_tensor(out, (h, w, 3) if channels_last else (3, h, w), dtype, dev)
            fmt.row_pitch = _row_pitch(out.stride(), not channels_last, h, 3 * w if channels_last else w, 3) * dtype.itemsize
        else:
            out = _out_tensor(out, shape, dtype, dev)
            st = out.stride()
            if layout == "yuv420p":
                if st != (1,):
                    raise ValueError("out: must be contiguous")
            elif st[1] != 1 or st[0] < w:
                raise ValueError(f"out: strides {st} are not rows of W elements")
            else:
                fmt.row_pitch = st[0] * dtype.itemsize
        dl, self._dra_keep = self._dra_luts(dra)      # (kept until the next call: the tables are copied asynchronously)
        if self.lib.xgpu_pic_output_device_size(self.ctx, C.byref(fmt)) == 0:
            raise ValueError(f"invalid output format (layout {layout}, out_bit_depth {out_bit_depth}, matrix {matrix}, chroma_loc {chroma_loc}, crop {crop})")
        if colour is None:
            self._device_call("xgpu_pic_output_device", out, pic, dl, C.byref(fmt))
        else:
            cm = abi.make_colour_transform(**colour)
            self._device_call("xgpu_pic_output_device_cm", out, pic, dl, C.byref(fmt), C.byref(cm))
        return out

    _PACKED_LAYOUTS = {"rgba": (abi.PACKED_RGBA, False), "bgra": (abi.PACKED_RGBA, True), "rgb10a2": (abi.PACKED_RGB10A2, False),
                       "bgr10a2": (abi.PACKED_RGB10A2, True), "yuyv": (abi.PACKED_YUYV, False), "uyvy": (abi.PACKED_UYVY, False)}

    def pic_output_packed(self, pic, layout="rgba", dtype=None, alpha=1.0, matrix=1, full_range=False, chroma_loc=0, upsample="linear", crop=(0, 0, 0, 0),
                          dra=None, colour=None, out_bit_depth=0, out=None):
        """The picture as a packed display surface in device memory, a torch tensor on cuda:{device}, made on the device on torch's current stream
        (xgpu_pic_output_device_packed).  layout "rgba" / "bgra": [H, W, 4] R G B A (B G R A) in any dtype of pic_output_tensor's "rgb" -
        the three colour elements are that call's, bit for bit, with `colour` those of its colour-managed form; A = alpha (0..1) as an integer code
        (floor(alpha * (2^D - 1) + 0.5), D = 8 for torch.uint8, else the coding depth) or as the dtype's float.  "rgb10a2" / "bgr10a2": [H, W] torch.int32, one word
        R | G << 10 | B << 20 | A << 30 per pixel (bgr10a2: B low, R at 20) with 10-bit codes whatever the coding depth and A = floor(alpha * 3 + 0.5); dtype and
        out_bit_depth stay unset.  "yuyv" / "uyvy": packed 4:2:2, [H, W, 2] - pixel x holds Y and, by its parity, Cb or Cr ("uyvy": the chroma sample first) -
        torch.uint8 (8-bit samples: YUY2 / UYVY) or a 16-bit integer type with the sample at out_bit_depth (0 = the coding depth) in the high bits of the word
        (10: Y210); luma is NV12's, chroma keeps half width and goes to full height by upsample ("nearest": the row above; "linear": the vertical quarter
        weights of chroma_loc); matrix, full_range, alpha are not read and colour must be None.
        out: a tensor to fill instead, rows of that shape whose stride may pad them (row_pitch); it is also what is returned."""
        import torch
        if layout not in self._PACKED_LAYOUTS:
            raise ValueError(f"layout must be one of {', '.join(map(repr, self._PACKED_LAYOUTS))}, not {layout!r}")
        lay, bgr = self._PACKED_LAYOUTS[layout]
        if upsample not in ("linear", "nearest"):
            raise ValueError(f"upsample must be 'linear' or 'nearest', not {upsample!r}")
        cl, cr, ct, cb = (int(v) for v in crop)
        w, h = self.width - cl - cr, self.height - ct - cb
        obd = int(out_bit_depth)
        if lay == abi.PACKED_RGB10A2:
            if dtype not in (None, torch.int32) or obd != 0:
                raise ValueError(f"{layout}: the words are torch.int32; dtype and out_bit_depth stay unset")
            dtype, code, shape, last = torch.int32, 0, (h, w), 1
        else:
            yuv = lay in (abi.PACKED_YUYV, abi.PACKED_UYVY)
            if dtype is None:
                dtype = torch.uint8
            codes = _codes("uint8", "int16", "uint16") if yuv else _codes()
            if dtype not in codes:
                raise ValueError(f"{layout}: unsupported output dtype {dtype}")
            code = codes[dtype]
            if yuv:
                if colour is not None:
                    raise ValueError(f"colour: a colour transform needs one of the RGB layouts, not {layout!r}")
                if code == abi.OUT_U8:
                    if obd not in (0, 8):
                        raise ValueError(f"{layout}: torch.uint8 holds 8-bit samples; out_bit_depth above 8 needs a 16-bit integer dtype")
                    obd = 8
            elif obd not in (0, self.bit_depth):
                raise ValueError(f"{layout}: out_bit_depth must be 0 or the coding depth {self.bit_depth}, not {obd}")
            last = 2 if yuv else 4
            shape = (h, w, last)
        fmt = abi.make_packed_format(lay, code, bgr=bgr, out_bit_depth=obd, matrix=matrix, full_range=full_range, chroma_loc=chroma_loc,
                                     upsample=abi.UPSAMPLE_LINEAR if upsample == "linear" else abi.UPSAMPLE_NEAREST, crop=crop, alpha=alpha)
        cm = None if colour is None else abi.make_colour_transform(**colour)
        if w <= 0 or h <= 0:
            raise ValueError(f"invalid packed output format: crop {crop} leaves no picture")
        out = _out_tensor(out, shape, dtype, torch.device("cuda", self.sp.device))
        st = out.stride()
        if st[1:] != ((last, 1) if len(shape) == 3 else (1,)) or st[0] < w * last:
            raise ValueError(f"out: strides {st} are not rows of W x {last} elements")
        fmt.row_pitch = st[0] * dtype.itemsize
        rc = self.lib.xgpu_output_packed_check(C.byref(fmt), None, self.width, self.height, self.bit_depth)
        if rc == 0 and cm is not None:
            rc = self._cm_check(abi.make_output_format(abi.OUT_RGB_INTERLEAVED), cm)
        if rc < 0:
            raise ValueError(f"invalid packed output format ({rc}): layout {layout}, dtype {dtype}, out_bit_depth {out_bit_depth}, matrix {matrix}, "
                             f"chroma_loc {chroma_loc}, alpha {alpha}, crop {crop}, colour {colour}")
        dl, self._dra_keep = self._dra_luts(dra)      # (kept until the next call: the tables are copied asynchronously)
        self._device_call("xgpu_pic_output_device_packed", out, pic, dl, C.byref(fmt), None if cm is None else C.byref(cm))
        return out

    def lut3d_create(self, nodes, shaper=None):
        """A 3D LUT of this context -> its handle (xgpu_lut3d_create).  nodes: the path of a .cube file (lut3d.load_cube: its 1D block and
        DOMAIN_MIN / MAX become the shaper unless shaper= is given), a float array [n, n, n, 3] / [n^3, 3] in .cube order (red fastest; quantised by
        xgpu_lut3d_from_float) or uint16 nodes of that shape.  shaper: None (the identity), uint16 [3, 2^B] positions, or dict(curve=, in_min=, in_max=) - the
        arguments of xgpu_lut3d_shaper.  The tables are made by the library's helpers, never here."""
        from . import lut3d
        if isinstance(nodes, (str, os.PathLike)):
            cube = lut3d.load_cube(nodes)
            nodes = cube["nodes"]
            if shaper is None:
                shaper = cube["shaper"]
        nodes = np.asarray(nodes)
        if nodes.dtype != np.uint16:
            nodes = abi.lut3d_from_float(self.lib, nodes)
            if isinstance(nodes, int):
                raise ValueError(f"lut3d_create: invalid cube ({nodes}): 2 .. 65 nodes per axis")
        nodes = np.ascontiguousarray(nodes).reshape(-1, 3)
        n = int(round(nodes.shape[0] ** (1.0 / 3.0)))
        if n * n * n != nodes.shape[0]:
            raise ValueError(f"lut3d_create: {nodes.shape[0]} nodes are no cube")
        if isinstance(shaper, dict):
            shaper = abi.lut3d_shaper(self.lib, self.bit_depth, **shaper)
            if isinstance(shaper, int):
                raise ValueError(f"lut3d_create: invalid shaper arguments ({shaper})")
        sp = None
        if shaper is not None:
            shaper = np.ascontiguousarray(shaper)
            if shaper.dtype != np.uint16 or shaper.shape != (3, 1 << self.bit_depth):
                raise ValueError(f"lut3d_create: the shaper is uint16 [3, {1 << self.bit_depth}]")
            sp = shaper.ctypes.data_as(C.POINTER(C.c_uint16))
        h = C.c_int(-1)
        self._chk(self.lib.xgpu_lut3d_create(self.ctx, n, nodes.ctypes.data_as(C.POINTER(C.c_uint16)), sp, C.byref(h)), "xgpu_lut3d_create")
        return h.value

    def lut3d_destroy(self, lut):
        self._chk(self.lib.xgpu_lut3d_destroy(self.ctx, int(lut)), "xgpu_lut3d_destroy")

    _LUT3D_LAYOUTS = {"rgb": None, "rgba": (abi.PACKED_RGBA, False), "bgra": (abi.PACKED_RGBA, True), "rgb10a2": (abi.PACKED_RGB10A2, False),
                      "bgr10a2": (abi.PACKED_RGB10A2, True)}

    def pic_output_lut3d(self, pic, lut, layout="rgb", channels_last=False, dtype=None, out_bit_depth=0, alpha=1.0, matrix=1, full_range=False, chroma_loc=0,
                         upsample="linear", crop=(0, 0, 0, 0), dra=None, bgr=False, out=None):
        """The picture through the 3D LUT `lut` (a handle of lut3d_create) as a torch tensor on cuda:{device}, made on the device on torch's current stream
        (xgpu_pic_output_device_lut3d / _packed_lut3d).  layout "rgb": pic_output_tensor's "rgb" shapes and dtypes - out_bit_depth 16 with
        a 16-bit integer dtype stores the LUT's 16-bit value -; "rgba" / "bgra" / "rgb10a2" / "bgr10a2": pic_output_packed's shapes, dtypes and alpha.  matrix,
        full_range, chroma_loc, upsample, crop and dra make the R'G'B' code the LUT reads, as in those calls."""
        import torch
        if layout not in self._LUT3D_LAYOUTS:
            raise ValueError(f"layout must be one of {', '.join(map(repr, self._LUT3D_LAYOUTS))}, not {layout!r}")
        if upsample not in ("linear", "nearest"):
            raise ValueError(f"upsample must be 'linear' or 'nearest', not {upsample!r}")
        up = abi.UPSAMPLE_LINEAR if upsample == "linear" else abi.UPSAMPLE_NEAREST
        cl, cr, ct, cb = (int(v) for v in crop)
        w, h = self.width - cl - cr, self.height - ct - cb
        if w <= 0 or h <= 0:
            raise ValueError(f"invalid output format: crop {crop} leaves no picture")
        dev = torch.device("cuda", self.sp.device)
        obd = int(out_bit_depth)
        if layout == "rgb":
            dtype = torch.uint8 if dtype is None else dtype
            codes = _codes()
            if dtype not in codes:
                raise ValueError(f"unsupported output dtype {dtype}")
            fmt = abi.make_output_format(abi.OUT_RGB_INTERLEAVED if channels_last else abi.OUT_RGB_PLANAR, codes[dtype], bgr=bgr, out_bit_depth=obd, matrix=matrix,
                                         full_range=full_range, chroma_loc=chroma_loc, upsample=up, crop=crop)
            out = _out_tensor(out, (h, w, 3) if channels_last else (3, h, w), dtype, dev)
            fmt.row_pitch = _row_pitch(out.stride(), not channels_last, h, 3 * w if channels_last else w, 3) * dtype.itemsize
            rc = self.lib.xgpu_output_lut3d_check(C.byref(fmt), None, 2, self.width, self.height, self.bit_depth)
            name = "xgpu_pic_output_device_lut3d"
        else:
            if channels_last or bgr:
                raise ValueError(f"{layout}: channels_last and bgr belong to layout 'rgb'")
            lay, pbgr = self._LUT3D_LAYOUTS[layout]
            if lay == abi.PACKED_RGB10A2:
                if dtype not in (None, torch.int32) or obd != 0:
                    raise ValueError(f"{layout}: the words are torch.int32; dtype and out_bit_depth stay unset")
                dtype, code, shape, last = torch.int32, 0, (h, w), 1
            else:
                dtype = torch.uint8 if dtype is None else dtype
                codes = _codes()
                if dtype not in codes:
                    raise ValueError(f"{layout}: unsupported output dtype {dtype}")
                code, shape, last = codes[dtype], (h, w, 4), 4
            fmt = abi.make_packed_format(lay, code, bgr=pbgr, out_bit_depth=obd, matrix=matrix, full_range=full_range, chroma_loc=chroma_loc, upsample=up, crop=crop,
                                         alpha=alpha)
            out = _out_tensor(out, shape, dtype, dev)
            st = out.stride()
            if st[1:] != ((last, 1) if len(shape) == 3 else (1,)) or st[0] < w * last:
                raise ValueError(f"out: strides {st} are not rows of W x {last} elements")
            fmt.row_pitch = st[0] * dtype.itemsize
            rc = self.lib.xgpu_output_lut3d_check(None, C.byref(fmt), 2, self.width, self.height, self.bit_depth)
            name = "xgpu_pic_output_device_packed_lut3d"
        if rc < 0:
            raise ValueError(f"invalid LUT output format ({rc}): layout {layout}, dtype {dtype}, out_bit_depth {out_bit_depth}, matrix {matrix}, "
                             f"chroma_loc {chroma_loc}, alpha {alpha}, crop {crop}")
        dl, self._dra_keep = self._dra_luts(dra)      # (kept until the next call: the tables are copied asynchronously)
        self._device_call(name, out, pic, dl, C.byref(fmt), int(lut))
        return out

    def dither_create(self, kind="blue", size=64, seed=1, levels=None):
        """A dither matrix of this context -> its handle (xgpu_dither_create).  kind "bayer": the recursive Bayer matrix of side `size`
        (a power of two, 2 .. 128); "blue": the blue-noise permutation of that side (4 .. 128) from `seed`; both have size^2 levels and are made by the library's
        constructors, never here.  An integer array [mh, mw] is uploaded as it is: sides powers of two in 1 .. 128, `levels` = L, a power of two in 2 .. 2^14 above
        every rank (None: the least such power)."""
        if isinstance(kind, str):
            if kind not in ("bayer", "blue"):
                raise ValueError(f"dither_create: kind must be 'bayer', 'blue' or an array of ranks, not {kind!r}")
            n = int(size)
            log2n = n.bit_length() - 1
            if n < 1 or n != 1 << log2n or levels is not None:
                raise ValueError(f"dither_create: size must be a power of two and levels unset for {kind!r}")
            rank = abi.dither_bayer(self.lib, log2n) if kind == "bayer" else abi.dither_blue(self.lib, log2n, seed)
            if isinstance(rank, int):
                raise ValueError(f"dither_create: {kind!r} has no matrix of side {size} ({rank})")
            k = 2 * log2n
        else:
            rank = np.asarray(kind)
            if rank.ndim != 2 or rank.dtype.kind not in "iu" or rank.size == 0 or rank.min() < 0 or rank.max() >= 1 << 14:
                raise ValueError("dither_create: the ranks are a non-empty integer array [mh, mw] with values in 0 .. 2^14 - 1")
            k = max(int(rank.max()).bit_length(), 1) if levels is None else int(levels).bit_length() - 1
            if levels is not None and (int(levels) < 2 or int(levels) != 1 << k):
                raise ValueError(f"dither_create: levels must be a power of two in 2 .. 16384, not {levels}")
            rank = np.ascontiguousarray(rank, np.uint16)
        h = C.c_int(-1)
        self._chk(self.lib.xgpu_dither_create(self.ctx, rank.shape[1], rank.shape[0], k, rank.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(h)), "xgpu_dither_create")
        self.__dict__.setdefault("_dither_shapes", {})[h.value] = (rank.shape[1], rank.shape[0], k)
        return h.value

    def dither_destroy(self, dither):
        self._chk(self.lib.xgpu_dither_destroy(self.ctx, int(dither)), "xgpu_dither_destroy")
        self.__dict__.setdefault("_dither_shapes", {}).pop(int(dither), None)

    def dither_shape(self, dither):
        """(mw, mh, k) of a handle of dither_create, or None"""
        return self.__dict__.get("_dither_shapes", {}).get(int(dither))

    _DITHER_LAYOUTS = {"rgb": None, "nv12": None, "p016": None, "rgba": (abi.PACKED_RGBA, False), "bgra": (abi.PACKED_RGBA, True),
                       "rgb10a2": (abi.PACKED_RGB10A2, False), "bgr10a2": (abi.PACKED_RGB10A2, True)}

    def _int_output_setup(self, word, layout, colour, out, channels_last, dtype, out_bit_depth, alpha, matrix, full_range, chroma_loc, upsample, crop, bgr):
        """what the dithered and the overlaid output share: the layouts of _DITHER_LAYOUTS in integer dtypes -> (the tensor to fill, its xgpu_output_format or
        None, its xgpu_packed_format or None, the transform or None, the entry point's name, the torch dtype); word: the entry points' last word, "dithered" or "overlaid", which the messages use too"""
        what = f"a {word}" if word[0] not in "aeiou" else f"an {word}"
        import torch
        if layout not in self._DITHER_LAYOUTS:
            raise ValueError(f"layout must be one of {', '.join(map(repr, self._DITHER_LAYOUTS))}, not {layout!r}")
        if upsample not in ("linear", "nearest"):
            raise ValueError(f"upsample must be 'linear' or 'nearest', not {upsample!r}")
        up = abi.UPSAMPLE_LINEAR if upsample == "linear" else abi.UPSAMPLE_NEAREST
        cl, cr, ct, cb = (int(v) for v in crop)
        w, h = self.width - cl - cr, self.height - ct - cb
        if w <= 0 or h <= 0:
            raise ValueError(f"invalid output format: crop {crop} leaves no picture")
        dev = torch.device("cuda", self.sp.device)
        obd = int(out_bit_depth)
        cm = None if colour is None else abi.make_colour_transform(**colour)
        ints = _codes("uint8", "int16", "uint16")
        packed = self._DITHER_LAYOUTS[layout]
        if packed is None:
            if dtype is None:
                dtype = torch.int16 if layout == "p016" else torch.uint8
            if dtype not in ints:
                raise ValueError(f"{layout}: {what} output has integer dtypes, not {dtype}")
            code = ints[dtype]
            if layout == "rgb":
                fmt = abi.make_output_format(abi.OUT_RGB_INTERLEAVED if channels_last else abi.OUT_RGB_PLANAR, code, bgr=bgr, out_bit_depth=obd, matrix=matrix,
                                             full_range=full_range, chroma_loc=chroma_loc, upsample=up, crop=crop)
                out = _out_tensor(out, (h, w, 3) if channels_last else (3, h, w), dtype, dev)
                fmt.row_pitch = _row_pitch(out.stride(), not channels_last, h, 3 * w if channels_last else w, 3) * dtype.itemsize
            else:
                if channels_last or bgr:
                    raise ValueError(f"{layout}: channels_last and bgr belong to layout 'rgb'")
                if code == abi.OUT_U8 and layout == "nv12":
                    if obd not in (0, 8):
                        raise ValueError("nv12: torch.uint8 holds 8-bit samples; out_bit_depth above 8 needs a 16-bit integer dtype")
                    obd = 8
                fmt = abi.make_output_format(abi.OUT_NV12 if layout == "nv12" else abi.OUT_P016, code, out_bit_depth=obd, crop=crop)
                if word == "overlaid":      # the layers' colours go through the forward matrix of these two; the samples themselves never read them
                    fmt.matrix, fmt.full_range = int(matrix), int(bool(full_range))
                out = _out_tensor(out, (h * 3 // 2, w), dtype, dev)
                st = out.stride()
                if st[1] != 1 or st[0] < w:
                    raise ValueError(f"out: strides {st} are not rows of W elements")
                fmt.row_pitch = st[0] * dtype.itemsize
            f_arg, pf_arg, name = C.byref(fmt), None, f"xgpu_pic_output_device_{word}"
        else:
            if channels_last or bgr:
                raise ValueError(f"{layout}: channels_last and bgr belong to layout 'rgb'")
            lay, pbgr = packed
            if lay == abi.PACKED_RGB10A2:
                if dtype not in (None, torch.int32) or obd != 0:
                    raise ValueError(f"{layout}: the words are torch.int32; dtype and out_bit_depth stay unset")
                dtype, code, shape, last = torch.int32, 0, (h, w), 1
            else:
                dtype = torch.uint8 if dtype is None else dtype
                if dtype not in ints:
                    raise ValueError(f"{layout}: {what} output has integer dtypes, not {dtype}")
                code, shape, last = ints[dtype], (h, w, 4), 4
            fmt = abi.make_packed_format(lay, code, bgr=pbgr, out_bit_depth=obd, matrix=matrix, full_range=full_range, chroma_loc=chroma_loc, upsample=up, crop=crop,
                                         alpha=alpha)
            out = _out_tensor(out, shape, dtype, dev)
            st = out.stride()
            if st[1:] != ((last, 1) if len(shape) == 3 else (1,)) or st[0] < w * last:
                raise ValueError(f"out: strides {st} are not rows of W x {last} elements")
            fmt.row_pitch = st[0] * dtype.itemsize
            f_arg, pf_arg, name = None, C.byref(fmt), f"xgpu_pic_output_device_packed_{word}"
        return out, (fmt if pf_arg is None else None), (fmt if pf_arg is not None else None), cm, name, dtype

    def pic_output_dithered(self, pic, dither, layout="rgb", phase=(0, 0), colour=None, out=None, channels_last=False, dtype=None, out_bit_depth=0, alpha=1.0,
                            matrix=1, full_range=False, chroma_loc=0, upsample="linear", crop=(0, 0, 0, 0), dra=None, bgr=False):
        """The picture with the dither matrix `dither` (a handle of dither_create) at `phase` (x, y) in place of the final rounding, as a torch tensor on
        cuda:{device}, made on the device on torch's current stream (xgpu_pic_output_device_dithered / _packed_dithered).  layout "rgb",
        "nv12", "p016": pic_output_tensor's shapes and arguments, integer dtypes only; "rgba" / "bgra" / "rgb10a2" / "bgr10a2": pic_output_packed's.  colour: a
        colour transform as those calls take it (the RGB layouts and the packed ones)."""
        out, f, pf, cm, name, dtype = self._int_output_setup("dithered", layout, colour, out, channels_last, dtype, out_bit_depth, alpha, matrix, full_range, chroma_loc,
                                                             upsample, crop, bgr)
        f_arg, pf_arg = (C.byref(f), None) if pf is None else (None, C.byref(pf))
        rc = self.lib.xgpu_output_dither_check(f_arg, pf_arg, None, 1, 1, 1, self.width, self.height, self.bit_depth)
        if rc == 0 and cm is not None:
            rc = self._cm_check(abi.make_output_format(abi.OUT_RGB_INTERLEAVED), cm) if layout not in ("nv12", "p016") else -1
        if rc < 0:
            raise ValueError(f"invalid dithered output format ({rc}): layout {layout}, dtype {dtype}, out_bit_depth {out_bit_depth}, matrix {matrix}, "
                             f"chroma_loc {chroma_loc}, alpha {alpha}, crop {crop}, colour {colour}")
        dl, self._dra_keep = self._dra_luts(dra)      # (kept until the next call: the tables are copied asynchronously)
        dp = abi.make_dither_params(dither, phase)
        self._device_call(name, out, pic, dl, f_arg if pf_arg is None else pf_arg, None if cm is None else C.byref(cm), C.byref(dp))
        return out

    def _overlay_layers(self, layers, dev):
        """layer dicts -> (the xgpu_overlay_layer array or None, their count, the tensors it points into)"""
        import torch
        layers = list(layers or ())
        if len(layers) > abi.MAX_OVERLAY_LAYERS:
            raise ValueError(f"layers: at most {abi.MAX_OVERLAY_LAYERS}, not {len(layers)}")
        arr, keep = (abi.OverlayLayer * max(len(layers), 1))(), []
        for i, l in enumerate(layers):
            l = dict(l)
            if ("image" in l) == ("box" in l):
                raise ValueError(f"layers[{i}]: one of image= and box=")
            opacity = l.pop("opacity", 255)
            if "box" in l:
                x, y, w, h = (int(v) for v in l.pop("box"))
                colour, fill, thickness = l.pop("colour", (255, 255, 255, 255)), l.pop("fill", (0, 0, 0, 0)), l.pop("thickness", 1)
                arr[i] = abi.make_overlay_layer(abi.OVL_BOX, x, y, w, h, opacity, colour=colour, fill=fill, thickness=thickness)
            else:
                img = l.pop("image")
                order = l.pop("order", "rgba")
                if order not in ("rgba", "bgra"):
                    raise ValueError(f"layers[{i}]: order must be 'rgba' or 'bgra', not {order!r}")
                if not isinstance(img, torch.Tensor) or img.device != dev or img.dtype != torch.uint8 or img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] != 4) or img.numel() == 0:
                    raise ValueError(f"layers[{i}]: image is a torch.uint8 tensor [h, w, 4] or [h, w] on {dev}")
                bpp = 4 if img.dim() == 3 else 1
                st = img.stride()
                if (bpp == 4 and st[1:] != (4, 1)) or (bpp == 1 and st[1] != 1) or st[0] < img.shape[1] * bpp:
                    raise ValueError(f"layers[{i}]: strides {st} are not rows of pixels")
                kind = abi.OVL_A8 if bpp == 1 else abi.OVL_BGRA8 if order == "bgra" else abi.OVL_RGBA8
                arr[i] = abi.make_overlay_layer(kind, l.pop("x", 0), l.pop("y", 0), img.shape[1], img.shape[0], opacity, d_pixels=img.data_ptr(), pitch=st[0],
                                                colour=l.pop("colour", (255, 255, 255, 255)))
                keep.append(img)
            if l:
                raise ValueError(f"layers[{i}]: unknown keys {sorted(l)}")
        return (arr if layers else None), len(layers), keep

    def _overlay_boxes(self, boxes, dev):
        """boxes dict -> (xgpu_overlay_boxes or None, the tensors it points into)"""
        import torch
        if boxes is None:
            return None, []
        b = dict(boxes)
        t = b.pop("tensor")
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dim() != 2 or t.shape[1] != 4 or t.dtype not in (torch.int32, torch.float32) or not t.is_contiguous():
            raise ValueError(f"boxes: tensor is a contiguous [n, 4] torch.int32 (x, y, w, h) or torch.float32 (x1, y1, x2, y2) tensor on {dev}")
        keep, ptr = [t], {}
        for key in ("count", "labels"):
            v = b.pop(key, None)
            if v is not None:
                if not isinstance(v, torch.Tensor) or v.device != dev or v.dtype != torch.int32 or not v.is_contiguous() or v.numel() < (1 if key == "count" else t.shape[0]):
                    raise ValueError(f"boxes: {key} is a contiguous torch.int32 tensor on {dev}" + (" with one label per box" if key == "labels" else ""))
                keep.append(v)
            ptr[key] = 0 if v is None else v.data_ptr()
        ob = abi.make_overlay_boxes(abi.BOX_XYXY_F32 if t.dtype == torch.float32 else abi.BOX_XYWH_I32, t.data_ptr(), t.shape[0], ptr["count"], ptr["labels"],
                                    palette=b.pop("palette", ((255, 0, 0, 255),)), thickness=b.pop("thickness", 2), fill_alpha=b.pop("fill_alpha", 0))
        if b:
            raise ValueError(f"boxes: unknown keys {sorted(b)}")
        return ob, keep

    def pic_output_overlaid(self, pic, layers=None, boxes=None, layout="rgb", colour=None, out=None, channels_last=False, dtype=None, out_bit_depth=0, alpha=1.0,
                            matrix=1, full_range=False, chroma_loc=0, upsample="linear", crop=(0, 0, 0, 0), dra=None, bgr=False):
        """The picture with `layers` alpha-blended over it, as a torch tensor on cuda:{device}, made on the device on torch's current stream
        (xgpu_pic_output_device_overlaid / _packed_overlaid).  layout "rgb", "nv12", "p016": pic_output_tensor's shapes and arguments,
        integer dtypes only; "rgba" / "bgra" / "rgb10a2" / "bgr10a2": pic_output_packed's.  colour: a colour transform as those calls take it (the RGB layouts and
        the packed ones); the layers' colours are codes of the destination and are not transformed.
        layers: at most 16 dicts, blended in list order, positions in the cropped W x H image (they may lie partly or wholly outside) -
          dict(image=<torch.uint8 cuda tensor [h, w, 4] or [h, w]>, x=0, y=0, opacity=255, order="rgba" | "bgra", colour=(r, g, b, a)): a bitmap with straight
          alpha, or - [h, w] - the coverage of `colour`;
          dict(box=(x, y, w, h), thickness=1, colour=(r, g, b, a), fill=(r, g, b, a), opacity=255): a frame in `colour`, its interior in `fill`.
        boxes: dict(tensor=<[n, 4] torch.int32 x, y, w, h | torch.float32 x1, y1, x2, y2>, count=<int32 tensor or None>, labels=<int32 [n] or None>,
          palette=[(r, g, b, a), ...], thickness=2, fill_alpha=0): at most 256 boxes a detector left on the device, painted before the layers; the host reads none
          of the tensors and nothing synchronises.
        The tensors of layers and boxes are read on torch's current stream; the decoder keeps references to them until its next overlaid call."""
        out, f, pf, cm, name, dtype = self._int_output_setup("overlaid", layout, colour, out, channels_last, dtype, out_bit_depth, alpha, matrix, full_range, chroma_loc,
                                                             upsample, crop, bgr)
        f_arg, pf_arg = (C.byref(f), None) if pf is None else (None, C.byref(pf))
        arr, n, keep = self._overlay_layers(layers, out.device)
        ob, keep_b = self._overlay_boxes(boxes, out.device)
        b_arg = None if ob is None else C.byref(ob)
        rc = self.lib.xgpu_output_overlay_check(f_arg, pf_arg, None, arr, n, b_arg, self.width, self.height, self.bit_depth)
        if rc == 0 and cm is not None:
            rc = self._cm_check(abi.make_output_format(abi.OUT_RGB_INTERLEAVED), cm) if layout not in ("nv12", "p016") else -1
        if rc < 0:
            raise ValueError(f"invalid overlaid output ({rc}): layout {layout}, dtype {dtype}, out_bit_depth {out_bit_depth}, matrix {matrix}, "
                             f"chroma_loc {chroma_loc}, alpha {alpha}, crop {crop}, colour {colour}, {n} layers, boxes {None if boxes is None else tuple(boxes['tensor'].shape)}")
        dl, self._dra_keep = self._dra_luts(dra)      # (kept until the next call: the tables are copied asynchronously)
        self._overlay_keep = keep + keep_b
        self._device_call(name, out, pic, dl, f_arg if pf_arg is None else pf_arg, None if cm is None else C.byref(cm), arr, n, b_arg)
        return out

    def _scaled_setup(self, a):
        """what the scaled outputs check and build alike -> (torch dtype, xgpu_output_format, xgpu_scale_params, H, W, device)"""
        import torch
        layout, colour, filter, mean, std = a["layout"], a["colour"], a["filter"], a["mean"], a["std"]
        if layout not in ("rgb", "yuv444"):
            raise ValueError(f"size: the scaled output has layouts 'rgb' and 'yuv444', not {layout!r}")
        if colour is not None:
            raise ValueError("size: the scaled output takes no colour transform here - pic_output_scaled_cm(pic, size, colour, ...) is the call that does")
        if filter not in ("bilinear", "area"):
            raise ValueError(f"filter must be 'bilinear' or 'area', not {filter!r}")
        if int(a["out_bit_depth"]) not in (0, self.bit_depth):
            raise ValueError(f"{layout}: out_bit_depth must be 0 or the coding depth {self.bit_depth}, not {a['out_bit_depth']}")
        dtype = torch.uint8 if a["dtype"] is None else a["dtype"]
        codes = _codes()
        if dtype not in codes:
            raise ValueError(f"unsupported output dtype {dtype}")
        if (mean is not None or std is not None) and codes[dtype] in (abi.OUT_U8, abi.OUT_U16):
            raise ValueError("mean / std: the normalise needs a float dtype")
        h, w = int(a["size"][0]), int(a["size"][1])
        lay = (abi.OUT_RGB_INTERLEAVED, abi.OUT_RGB_PLANAR) if layout == "rgb" else (abi.OUT_YUV444_INTERLEAVED, abi.OUT_YUV444_PLANAR)
        fmt = abi.make_output_format(lay[0] if a["channels_last"] else lay[1], codes[dtype], bgr=a["bgr"], matrix=a["matrix"], full_range=a["full_range"],
                                     chroma_loc=a["chroma_loc"], crop=a["crop"], upsample=a.get("upsample", abi.UPSAMPLE_LINEAR))      # (read by the linear-light form only)
        sc = abi.make_scale_params(w, h, abi.SCALE_BILINEAR if filter == "bilinear" else abi.SCALE_AREA, mean=mean, std=std)
        return dtype, fmt, sc, h, w, torch.device("cuda", self.sp.device)

    @staticmethod
    def _rois_fit(a):
        """what a batch checks before _scaled_setup -> the XGPU_FIT_* code"""
        if a["colour"] is not None:
            raise ValueError("rois: the batch of rectangles takes no colour transform here - pic_output_scaled_cm(pic, size, colour, rois=...) is the call that does")
        if a["fit"] not in ("stretch", "letterbox"):
            raise ValueError(f"fit must be 'stretch' or 'letterbox', not {a['fit']!r}")
        return abi.FIT_LETTERBOX if a["fit"] == "letterbox" else abi.FIT_STRETCH

    def _cm_check(self, fmt, cm):
        """0, or the code xgpu_colour_tables refuses transform `cm` with on layout fmt.layout - remembered per transform: making the tables in double precision
        costs more host time than the whole call whose arguments it checks, and a stream asks for the same transform picture after picture"""
        memo = self.__dict__.setdefault("_cm_checked", {})
        key = (fmt.layout, self.bit_depth, cm.src_primaries, cm.src_transfer, cm.dst_primaries, cm.dst_transfer, cm.tone_map, cm.src_peak, cm.dst_peak, cm.linear_scale)
        if key not in memo:
            if len(memo) >= 64:
                memo.clear()
            memo[key] = self.lib.xgpu_colour_tables(C.byref(fmt), C.byref(cm), self.bit_depth, C.byref(abi.ColourTables()))
        return memo[key]

    def _pic_output_tensor_scaled(self, a, cm=None, lin=False):
        """pic_output_tensor with size=(H, W); cm: pic_output_scaled_cm's xgpu_colour_transform; lin: its linear_light"""
        dtype, fmt, sc, h, w, dev = self._scaled_setup(a)

        def refuse():
            if lin:      # xgpu_output_scaled_lin_check's order: the plain call's refusals, the intermediate's, then the layout's and the transform's
                rc = self.lib.xgpu_output_scaled_check(C.byref(fmt), C.byref(sc), self.width, self.height, self.bit_depth)
                if rc == 0:      # without a transform the check stops at the intermediate (-104) or at the missing transform; the transform's own answer is remembered
                    big = self.lib.xgpu_output_scaled_lin_check(C.byref(fmt), C.byref(sc), None, self.width, self.height, self.bit_depth) == -104
                    rc = -104 if big else self._cm_check(fmt, cm)
                if rc < 0:
                    raise ValueError(f"invalid linear-light scaled output ({rc}): size {tuple(a['size'])}, matrix {a['matrix']}, chroma_loc {a['chroma_loc']}, "
                                     f"crop {a['crop']}, mean {a['mean']}, std {a['std']}, transform {cm.src_primaries}/{cm.src_transfer} -> "
                                     f"{cm.dst_primaries}/{cm.dst_transfer}")
            elif cm is not None:      # xgpu_output_scaled_cm_check's order: the plain call's refusals, then the layout's and the transform's
                rc = self.lib.xgpu_output_scaled_check(C.byref(fmt), C.byref(sc), self.width, self.height, self.bit_depth) or self._cm_check(fmt, cm)
                if rc < 0:
                    raise ValueError(f"invalid colour-managed scaled output ({rc}): size {tuple(a['size'])}, matrix {a['matrix']}, chroma_loc {a['chroma_loc']}, "
                                     f"crop {a['crop']}, mean {a['mean']}, std {a['std']}, transform {cm.src_primaries}/{cm.src_transfer} -> "
                                     f"{cm.dst_primaries}/{cm.dst_transfer}")
            elif self.lib.xgpu_output_scaled_size(C.byref(fmt), C.byref(sc), self.width, self.height, self.bit_depth) == 0:
                raise ValueError(f"invalid scaled output (layout {a['layout']}, size {tuple(a['size'])}, matrix {a['matrix']}, chroma_loc {a['chroma_loc']}, "
                                 f"crop {a['crop']}, mean {a['mean']}, std {a['std']})")
        out, planar = a["out"], not a["channels_last"]
        if out is None:
            refuse()      # before a tensor is made, and again with its pitch
        out = _out_tensor(out, (3, h, w) if planar else (h, w, 3), dtype, dev)
        fmt.row_pitch = _row_pitch(out.stride(), planar, h, w if planar else 3 * w, 3) * dtype.itemsize
        refuse()
        dl, self._dra_keep = self._dra_luts(a["dra"]) if a["dra"] is not None else (None, None)      # (kept until the next call: the tables are copied asynchronously)
        if cm is not None:
            self._device_call("xgpu_pic_output_device_scaled_lin" if lin else "xgpu_pic_output_device_scaled_cm", out, a["pic"], dl, C.byref(fmt), C.byref(sc), C.byref(cm))
        else:
            self._device_call("xgpu_pic_output_device_scaled", out, a["pic"], dl, C.byref(fmt), C.byref(sc))
        return out

    def _pic_output_tensor_rois(self, a, cm=None, lin=False):
        """pic_output_tensor with size=(H, W) and rois=[...]; cm: pic_output_scaled_cm's xgpu_colour_transform; lin: its linear_light"""
        fit = self._rois_fit(a)
        dtype, fmt, sc, h, w, dev = self._scaled_setup(a)
        rois = [tuple(int(v) for v in r) for r in a["rois"]]
        if a["snap"]:       # outward to even, then into the picture minus the crop
            cl, cr, ct, cb = (int(v) for v in a["crop"])
            pw, ph = self.width - cl - cr, self.height - ct - cb
            snapped = []
            for x, y, rw, rh in rois:
                x0, y0, x1, y1 = max(x & ~1, 0), max(y & ~1, 0), min((x + rw + 1) & ~1, pw), min((y + rh + 1) & ~1, ph)
                snapped.append((x0, y0, x1 - x0, y1 - y0))
            rois = snapped
        n = len(rois)
        ra = abi.make_rois(rois)
        rp = abi.make_roi_params(fit, a["pad"])

        def refuse():
            bad = C.c_int(-1)
            rc = self.lib.xgpu_output_rois_check(C.byref(fmt), C.byref(sc), C.byref(rp), ra, n, self.width, self.height, self.bit_depth, C.byref(bad))
            if rc == 0 and lin:      # the 512 MiB rule on the float32 intermediate; the transform itself is checked (and remembered) below
                rc = self.lib.xgpu_output_rois_lin_check(C.byref(fmt), C.byref(sc), C.byref(rp), ra, n, None, self.width, self.height, self.bit_depth, C.byref(bad))
                rc = rc if bad.value >= 0 else 0
            if rc < 0:
                at = f"roi {bad.value} {rois[bad.value]}: " if 0 <= bad.value < n else ""
                raise ValueError(f"invalid batch of rectangles ({rc}): {at}layout {a['layout']}, size {tuple(a['size'])}, fit {a['fit']}, pad {a['pad']}, "
                                 f"crop {a['crop']}, mean {a['mean']}, std {a['std']}, {n} rectangles")
            if cm is not None:      # the batch's own refusals first, then the transform's
                rc = self._cm_check(fmt, cm)
                if rc < 0:
                    raise ValueError(f"invalid colour transform ({rc}): {cm.src_primaries}/{cm.src_transfer} -> {cm.dst_primaries}/{cm.dst_transfer}")
        out, planar = a["out"], not a["channels_last"]
        if out is None:
            refuse()      # before a tensor is made, and again with its pitches
        out = _out_tensor(out, (n, 3, h, w) if planar else (n, h, w, 3), dtype, dev)
        st = out.stride()
        fmt.row_pitch = _row_pitch(st, planar, h, w if planar else 3 * w, 3) * dtype.itemsize
        rp.image_pitch = st[0] * dtype.itemsize if n > 1 else 0
        refuse()
        dl, self._dra_keep = self._dra_luts(a["dra"]) if a["dra"] is not None else (None, None)      # (kept until the next call: the tables are copied asynchronously)
        if cm is not None:
            self._device_call("xgpu_pic_output_device_rois_lin" if lin else "xgpu_pic_output_device_rois_cm", out, a["pic"], dl, C.byref(fmt), C.byref(sc), C.byref(rp), ra, n, C.byref(cm))
        else:
            self._device_call("xgpu_pic_output_device_rois", out, a["pic"], dl, C.byref(fmt), C.byref(sc), C.byref(rp), ra, n)
        return out

    def _pic_output_tensor_rois_dev(self, a):
        """pic_output_tensor with size=(H, W) and rois=<tensor on the device>"""
        import torch
        fit = self._rois_fit(a)
        dtype, fmt, sc, h, w, dev = self._scaled_setup(a)
        rois, count, results = a["rois"], a["count"], a["results"]
        if rois.device != dev or rois.dtype not in (torch.int32, torch.float32) or rois.dim() != 2 or rois.shape[1] != 4 or not rois.is_contiguous():
            raise ValueError(f"rois: a contiguous int32 (x, y, w, h) or float32 (x1, y1, x2, y2) tensor [N, 4] on {dev}, not {tuple(rois.shape)} {rois.dtype} on "
                             f"{rois.device}{'' if rois.is_contiguous() else ', not contiguous'}")
        if count is not None and (not isinstance(count, torch.Tensor) or count.device != dev or count.dtype != torch.int32 or count.numel() != 1):
            raise ValueError(f"count: an int32 tensor of one element on {dev}")
        n = int(rois.shape[0])
        box_format = abi.BOX_XYWH_I32 if rois.dtype == torch.int32 else abi.BOX_XYXY_F32
        rp = abi.make_roi_params(fit, a["pad"])
        bounds = abi.make_roi_bounds(a["max_roi"])

        def refuse():
            rc = self.lib.xgpu_output_rois_dev_check(C.byref(fmt), C.byref(sc), C.byref(rp), C.byref(bounds), box_format, n, self.width, self.height, self.bit_depth)
            if rc < 0:
                raise ValueError(f"invalid batch of boxes ({rc}): layout {a['layout']}, size {tuple(a['size'])}, fit {a['fit']}, pad {a['pad']}, crop {a['crop']}, "
                                 f"mean {a['mean']}, std {a['std']}, max_roi {a['max_roi']}, {n} boxes")
        out, planar = a["out"], not a["channels_last"]
        if out is None:
            refuse()      # before a tensor is made, and again with its pitches
        out = _out_tensor(out, (n, 3, h, w) if planar else (n, h, w, 3), dtype, dev)
        st = out.stride()
        fmt.row_pitch = _row_pitch(st, planar, h, w if planar else 3 * w, 3) * dtype.itemsize
        rp.image_pitch = st[0] * dtype.itemsize if n > 1 else 0
        refuse()
        dl, self._dra_keep = self._dra_luts(a["dra"]) if a["dra"] is not None else (None, None)      # (kept until the next call: the tables are copied asynchronously)
        res = torch.empty((n, 9), dtype=torch.int32, device=dev) if results else None
        self._device_call("xgpu_pic_output_device_rois_dev", out, a["pic"], dl, C.byref(fmt), C.byref(sc), C.byref(rp), C.byref(bounds), box_format,
                          C.c_void_p(rois.data_ptr()), n, C.c_void_p(count.data_ptr()) if count is not None else None,
                          C.c_void_p(res.data_ptr()) if results else None)
        return (out, res) if results else out

    def pic_output_scaled_cm(self, pic, size, colour, rois=None, fit=None, pad=None, channels_last=False, dtype=None, matrix=1, full_range=False, chroma_loc=0,
                             crop=(0, 0, 0, 0), dra=None, out=None, bgr=False, filter="bilinear", mean=None, std=None, layout="rgb", linear_light=False,
                             upsample="linear"):
        """The scaled output with a colour transform (xgpu_pic_output_device_scaled_cm / _rois_cm): the picture - or, with host
        rois=[(x, y, w, h), ...], every rectangle - resized to size=(H, W), taken from the stream's colour space to the caller's by `colour` (pic_output_tensor's
        dict: the keyword arguments of abi.make_colour_transform), normalised by mean / std (float dtypes), on torch's current stream: [3, H, W] (channels_last:
        [H, W, 3]), with rois [N, 3, H, W] / [N, H, W, 3].  This is where size= and colour= meet: pic_output_tensor(size=..., colour=...) keeps raising ValueError.
        The encoded Y'CbCr samples are filtered (as in every scaled output), then each destination pixel goes through the transform of pic_output_tensor(colour=).
        Every other argument is pic_output_tensor's with size=; fit "stretch" (None) or "letterbox" and pad belong to rois= - pad is a value of the destination
        space, normalised like a pixel and never transformed.  layout: "rgb" only.  Boxes in device memory, warped and remapped outputs take no transform.
        linear_light=True (xgpu_pic_output_device_scaled_lin / _rois_lin): the filter runs on the linear light of the source
        primaries instead - every source pixel is converted as pic_output_tensor converts it (upsample "linear" / "nearest" and chroma_loc select the chroma
        upsampling; upsample is read in this form only) and linearised, the float32 values are filtered, and the rest of the transform follows.  It is what a
        reduced PQ / HLG picture with fine, high-contrast detail needs, and costs a float32 intermediate of 3 x H x (source width) x 4 bytes."""
        import torch
        if upsample not in ("linear", "nearest"):
            raise ValueError(f"upsample must be 'linear' or 'nearest', not {upsample!r}")
        if upsample != "linear" and not linear_light:
            raise ValueError("upsample belongs to linear_light=True: the other scaled outputs filter chroma on its own grid")
        if colour is None:
            raise ValueError("colour: the colour-managed scaled output needs a transform; pic_output_tensor(size=...) is the plain one")
        if layout != "rgb":
            raise ValueError(f"colour: a colour transform needs layout 'rgb', not {layout!r}")
        if isinstance(rois, torch.Tensor):
            raise ValueError("rois: boxes in device memory take no colour transform")
        if rois is None and (fit is not None or pad is not None):
            raise ValueError("fit and pad belong to rois=")
        a = {"pic": pic, "layout": layout, "channels_last": channels_last, "dtype": dtype, "matrix": matrix, "full_range": full_range, "chroma_loc": chroma_loc,
             "crop": crop, "dra": dra, "out": out, "bgr": bgr, "out_bit_depth": 0, "colour": None, "size": size, "filter": filter, "mean": mean, "std": std,
             "rois": rois, "fit": fit or "stretch", "pad": 0.0 if pad is None else pad, "snap": False,
             "upsample": abi.UPSAMPLE_LINEAR if upsample == "linear" else abi.UPSAMPLE_NEAREST}
        cm = abi.make_colour_transform(**colour)
        if rois is not None:
            return self._pic_output_tensor_rois(a, cm, bool(linear_light))
        return self._pic_output_tensor_scaled(a, cm, bool(linear_light))

    def pic_output_resampled(self, pic, size, kernel="catmull-rom", antialias=True, rois=None, fit=None, pad=None, layout="rgb", channels_last=False, dtype=None,
                             matrix=1, full_range=False, chroma_loc=0, crop=(0, 0, 0, 0), dra=None, bgr=False, mean=None, std=None, out=None):
        """The scaled output with a bicubic filter (xgpu_pic_output_device_resampled / _rois_resampled): the picture - or, with host
        rois=[(x, y, w, h), ...], every rectangle - resized to size=(H, W) on torch's current stream: [3, H, W] (channels_last: [H, W, 3]), with rois
        [N, 3, H, W] / [N, H, W, 3].  kernel "catmull-rom" (alias "bicubic": Keys a = -1/2, PIL's BICUBIC and torch's bicubic with antialias=True), "cubic-0.75"
        (Keys a = -3/4: torch's bicubic with antialias=False, OpenCV's INTER_CUBIC) or "mitchell"; antialias=True widens the kernel by the reduction ratio.
        Every other argument is pic_output_tensor's with size=; fit "stretch" (None) or "letterbox" and pad belong to rois=.  Boxes in device memory, colour
        transforms, the ladder, warped and remapped outputs have no bicubic form; pic_output_tensor(filter=...) keeps its two names."""
        import torch
        if kernel not in abi.RESAMPLE_KERNELS:
            raise ValueError(f"kernel must be one of {sorted(abi.RESAMPLE_KERNELS)}, not {kernel!r}")
        if antialias not in (True, False, 0, 1):
            raise ValueError(f"antialias must be True or False, not {antialias!r}")
        if isinstance(rois, torch.Tensor):
            raise ValueError("rois: boxes in device memory have no bicubic form")
        if rois is None and (fit is not None or pad is not None):
            raise ValueError("fit and pad belong to rois=")
        a = {"pic": pic, "layout": layout, "channels_last": channels_last, "dtype": dtype, "matrix": matrix, "full_range": full_range, "chroma_loc": chroma_loc,
             "crop": crop, "dra": dra, "out": out, "bgr": bgr, "out_bit_depth": 0, "colour": None, "size": size, "filter": "bilinear", "mean": mean, "std": std,
             "fit": fit or "stretch"}
        code = abi.FIT_STRETCH if rois is None else self._rois_fit(a)
        dtype, fmt, sc, h, w, dev = self._scaled_setup(a)
        rs = abi.make_resample_params(w, h, kernel, bool(antialias), mean=mean, std=std)
        planar, batch = not channels_last, rois is not None
        if batch:
            rois = [tuple(int(v) for v in r) for r in rois]
            n, ra, rp = len(rois), abi.make_rois(rois), abi.make_roi_params(code, 0.0 if pad is None else pad)

        def refuse():
            bad = C.c_int(-1)
            if batch:
                rc = self.lib.xgpu_output_rois_resampled_check(C.byref(fmt), C.byref(rs), C.byref(rp), ra, n, self.width, self.height, self.bit_depth, C.byref(bad))
            else:
                rc = self.lib.xgpu_output_resampled_check(C.byref(fmt), C.byref(rs), self.width, self.height, self.bit_depth)
            if rc < 0:
                at = f"roi {bad.value} {rois[bad.value]}: " if batch and 0 <= bad.value < n else ""
                raise ValueError(f"invalid resampled output ({rc}): {at}layout {layout}, size {tuple(size)}, kernel {kernel}, fit {fit}, pad {pad}, matrix {matrix}, "
                                 f"chroma_loc {chroma_loc}, crop {crop}, mean {mean}, std {std}")
        if out is None:
            refuse()      # before a tensor is made, and again with its pitches
        image = (3, h, w) if planar else (h, w, 3)
        out = _out_tensor(out, (n,) + image if batch else image, dtype, dev)
        st = out.stride()
        fmt.row_pitch = _row_pitch(st, planar, h, w if planar else 3 * w, 3) * dtype.itemsize
        if batch:
            rp.image_pitch = st[0] * dtype.itemsize if n > 1 else 0
        refuse()
        dl, self._dra_keep = self._dra_luts(dra) if dra is not None else (None, None)      # (kept until the next call: the tables are copied asynchronously)
        if batch:
            self._device_call("xgpu_pic_output_device_rois_resampled", out, pic, dl, C.byref(fmt), C.byref(rs), C.byref(rp), ra, n)
        else:
            self._device_call("xgpu_pic_output_device_resampled", out, pic, dl, C.byref(fmt), C.byref(rs))
        return out

    def pic_output_surfaces(self, pic, sizes, layout="nv12", dtype=None, out_bit_depth=0, filter="bilinear", chroma_loc=0, dst_chroma_loc=None, crop=(0, 0, 0, 0),
                            dra=None, out=None):
        """The picture as a ladder of scaled video surfaces - one tensor per (H, W) of `sizes` (1 .. abi.MAX_RUNGS, even), all in one layout "nv12", "p016" or
        "yuv420p" - from one call on torch's current stream (xgpu_pic_output_device_ladder): what an encoder takes for the 2160p /
        1080p / 720p renditions of a transcode.  Shapes and dtypes are those pic_output_tensor gives the layout at that size: "nv12" / "p016" [H * 3 // 2, W]
        (torch.uint8 for 8-bit NV12, else a 16-bit integer type; out_bit_depth 0 = the coding depth), "yuv420p" 1-D (torch.uint8: 8-bit samples, else
        out_bit_depth or the coding depth).  Luma is the scaled output's luma; the chroma planes are filtered from the half-resolution planes straight onto the
        rung's half-resolution grid, whose siting is dst_chroma_loc (None: chroma_loc, the source's).  filter "bilinear" (antialiased) or "area"; crop (left,
        right, top, bottom, even) is the source.  out: a list of tensors to fill, one per size (the row stride of an "nv12" / "p016" tensor becomes the rung's
        row_pitch; they must not overlap); it is also what is returned."""
        import torch
        if layout not in ("nv12", "p016", "yuv420p"):
            raise ValueError(f"layout must be 'nv12', 'p016' or 'yuv420p', not {layout!r}")
        if filter not in ("bilinear", "area"):
            raise ValueError(f"filter must be 'bilinear' or 'area', not {filter!r}")
        sizes = [(int(h), int(w)) for h, w in sizes]
        if not 1 <= len(sizes) <= abi.MAX_RUNGS:
            raise ValueError(f"sizes: 1..{abi.MAX_RUNGS} renditions, not {len(sizes)}")
        if any(h < 2 or w < 2 or (h | w) & 1 for h, w in sizes):
            raise ValueError(f"sizes: every (H, W) must be even and at least 2, got {sizes}")
        if out is not None and len(out) != len(sizes):
            raise ValueError(f"out: {len(sizes)} tensors, one per size, not {len(out)}")
        if dst_chroma_loc is not None and int(dst_chroma_loc) not in range(6):
            raise ValueError(f"dst_chroma_loc must be None or 0..5, not {dst_chroma_loc!r}")
        if dtype is None:
            dtype = torch.int16 if layout == "p016" else torch.uint8      # P016 has 16-bit words only
        codes = _codes("uint8", "int16", "uint16")
        if dtype not in codes:
            raise ValueError(f"{layout}: dtype must be torch.uint8 or a 16-bit integer type, not {dtype}")
        obd = int(out_bit_depth)
        if codes[dtype] == abi.OUT_U8:
            if layout == "p016":
                raise ValueError("p016: dtype must be a 16-bit integer type")
            if obd not in (0, 8):
                raise ValueError(f"{layout}: torch.uint8 holds 8-bit samples; out_bit_depth above 8 needs a 16-bit integer dtype")
            obd = 8
        lay = {"nv12": abi.OUT_NV12, "p016": abi.OUT_P016, "yuv420p": abi.OUT_YUV420P}[layout]
        fmt = abi.make_output_format(lay, codes[dtype], out_bit_depth=obd, chroma_loc=chroma_loc, crop=crop)
        lp = abi.make_ladder_params(abi.SCALE_BILINEAR if filter == "bilinear" else abi.SCALE_AREA, dst_chroma_loc)
        es = dtype.itemsize

        def refuse(rungs):
            rc = self.lib.xgpu_output_ladder_check(C.byref(fmt), C.byref(lp), rungs, len(sizes), self.width, self.height, self.bit_depth)
            if rc != 0:
                raise ValueError(f"invalid surface ladder ({rc}: layout {layout}, sizes {sizes}, out_bit_depth {out_bit_depth}, chroma_loc {chroma_loc}, "
                                 f"dst_chroma_loc {dst_chroma_loc}, crop {crop})")
        tight = [self.lib.xgpu_output_ladder_rung_size(C.byref(fmt), w, h, 0, self.bit_depth) for h, w in sizes]
        refuse(abi.make_rungs([(w, h, 0, None, n) for (h, w), n in zip(sizes, tight)]))      # before a tensor is made, and again with the pitches
        dev = torch.device("cuda", self.sp.device)
        outs, spec = [], []
        for i, (h, w) in enumerate(sizes):
            t = _out_tensor(None if out is None else out[i], (w * h * 3 // 2,) if layout == "yuv420p" else (h * 3 // 2, w), dtype, dev)
            st, pitch = t.stride(), 0
            if layout == "yuv420p":
                if st != (1,):
                    raise ValueError("out: must be contiguous")
            elif st[1] != 1 or st[0] < w:
                raise ValueError(f"out: strides {st} are not rows of W elements")
            else:
                pitch = st[0] * es
            nbytes = (sum((n - 1) * s for n, s in zip(t.shape, st)) + 1) * es      # the bytes the tensor spans from data_ptr()
            outs.append(t)
            spec.append((w, h, pitch, t.data_ptr(), nbytes))
        rungs = abi.make_rungs(spec)
        refuse(rungs)
        dl, self._dra_keep = self._dra_luts(dra)      # (kept until the next call: the tables are copied asynchronously)
        cur, run = self._run_stream(dev)
        self._chk(self.lib.xgpu_pic_output_device_ladder(self.ctx, pic, dl, C.byref(fmt), C.byref(lp), rungs, len(sizes), C.c_void_p(run.cuda_stream)),
                  "xgpu_pic_output_device_ladder")
        if run is not cur:
            cur.wait_stream(run)
        return outs

    def pic_output_warped(self, pic, maps, size, layout="rgb", channels_last=False, dtype=None, matrix=1, full_range=False, chroma_loc=0, crop=(0, 0, 0, 0),
                          dra=None, bgr=False, samples=1, border="clamp", pad=0.0, mean=None, std=None, out=None, status=False):
        """N affine maps of the picture, each giving one H x W image (size=(H, W)), converted and normalised like pic_output_tensor(size=...), as one batch
        [N, 3, H, W] (channels_last: [N, H, W, 3]) from one kernel launch (xgpu_pic_output_device_warp): rotated boxes, crops aligned
        by a similarity transform, flips, shears.  Integer arithmetic from the map to (Y, Cb, Cr): tests/warp_ref.py restates the result bit for bit.
        maps: a sequence of 6-float thetas (theta takes destination pixel centres (ox + 0.5, oy + 0.5) to continuous source coordinates of the picture minus the
        crop; abi.warp_from_matrix converts them, abi.warp_from_rotated_box makes the map of a rotated box), or a numpy int64 [N, 6] array of Q16 maps, or a
        contiguous torch int64 [N, 6] tensor on the decoder's device - maps some kernel left there, read on the device with no host read and no
        synchronisation; a map outside the limits then gives an image that is all `pad`, and status=True also returns the int32 [N] tensor (0 = written,
        1 = refused).  samples 1, 2 or 4: sub-positions per axis (antialiases reductions up to about that factor).  border "clamp" replicates the picture's edge,
        "pad" writes `pad` (one value or three, in the output's channel order, before the normalise; integers for the integer dtypes) where the pixel's centre
        lies outside the picture.  out: a tensor of that shape whose rows may be padded and whose images may lie a batch stride apart."""
        import torch
        if border not in ("clamp", "pad"):
            raise ValueError(f"border must be 'clamp' or 'pad', not {border!r}")
        a = {"layout": layout, "colour": None, "filter": "bilinear", "mean": mean, "std": std, "out_bit_depth": 0, "dtype": dtype, "size": size,
             "channels_last": channels_last, "bgr": bgr, "matrix": matrix, "full_range": full_range, "chroma_loc": chroma_loc, "crop": crop}
        dtype, fmt, sc, h, w, dev = self._scaled_setup(a)
        on_device = isinstance(maps, torch.Tensor)
        if on_device:
            if maps.device != dev or maps.dtype != torch.int64 or maps.dim() != 2 or maps.shape[1] != 6 or not maps.is_contiguous():
                raise ValueError(f"maps: a contiguous int64 tensor [N, 6] on {dev}, not {tuple(maps.shape)} {maps.dtype} on {maps.device}"
                                 f"{'' if maps.is_contiguous() else ', not contiguous'}")
            n, ma = int(maps.shape[0]), None
        else:
            if status:
                raise ValueError("status belongs to maps=<tensor on the device>")
            if isinstance(maps, np.ndarray) and maps.dtype == np.int64:
                if maps.ndim != 2 or maps.shape[1] != 6:
                    raise ValueError(f"maps: an int64 array [N, 6], not {maps.shape}")
                rows = maps
            else:
                rows = []
                for i, theta in enumerate(maps):
                    if len(theta) != 6:
                        raise ValueError(f"maps: theta {i} has {len(theta)} entries, not 6")
                    m = abi.warp_from_matrix(self.lib, theta)
                    if not isinstance(m, tuple):
                        raise ValueError(f"maps: theta {i} {tuple(float(v) for v in theta)} is not finite or leaves the limits of a map ({m})")
                    rows.append(m)
            n, ma = len(rows), abi.make_warp_maps(rows)
        wp = abi.make_warp_params(samples, abi.WARP_PAD if border == "pad" else abi.WARP_CLAMP, pad)

        def refuse():
            rc, bad = abi.output_warp_check(self.lib, fmt, sc, wp, ma, n, self.width, self.height, self.bit_depth)
            if rc < 0:
                at = f"map {bad} {tuple(int(v) for v in rows[bad])}: " if 0 <= bad < n else ""
                raise ValueError(f"invalid batch of maps ({rc}): {at}layout {layout}, size {tuple(size)}, samples {samples}, border {border}, pad {pad}, crop {crop}, "
                                 f"mean {mean}, std {std}, {n} maps")
        planar = not channels_last
        if out is None:
            refuse()      # before a tensor is made, and again with its pitches
        out = _out_tensor(out, (n, 3, h, w) if planar else (n, h, w, 3), dtype, dev)
        st = out.stride()
        fmt.row_pitch = _row_pitch(st, planar, h, w if planar else 3 * w, 3) * dtype.itemsize
        wp.image_pitch = st[0] * dtype.itemsize if n > 1 else 0
        refuse()
        dl, self._dra_keep = self._dra_luts(dra) if dra is not None else (None, None)      # (kept until the next call: the tables are copied asynchronously)
        res = torch.empty((n,), dtype=torch.int32, device=dev) if on_device and status else None
        self._device_call("xgpu_pic_output_device_warp", out, pic, dl, C.byref(fmt), C.byref(sc), C.byref(wp),
                          C.c_void_p(maps.data_ptr()) if on_device else ma, int(on_device), n, C.c_void_p(res.data_ptr()) if res is not None else None)
        return (out, res) if on_device and status else out

    def pic_output_remapped(self, pic, grid, size, step=0, samples=1, border="clamp", pad=None, layout="rgb", channels_last=False, dtype=None, matrix=1,
                            full_range=False, chroma_loc=0, crop=(0, 0, 0, 0), dra=None, bgr=False, mean=None, std=None, out=None):
        """N coordinate grids of the picture, each giving one H x W image (size=(H, W)) whose every pixel reads the picture at a position of its own, converted
        and normalised like pic_output_tensor(size=...), as one batch [N, 3, H, W] (channels_last: [N, H, W, 3]) from one kernel launch
        (xgpu_pic_output_device_remap): lens undistortion, fisheye views, perspective maps, a flow field.  Integer arithmetic from the
        node to (Y, Cb, Cr): tests/remap_ref.py restates the result bit for bit.
        grid: a torch tensor on the decoder's device, [N, gh, gw, 2] or [gh, gw, 2] (one image), (gh, gw) = abi.remap_grid_dims(lib, size, step): a node (x, y)
        every 2^step destination pixels (step 0 .. 6; 0: one per pixel), interpolated exactly in between.  int32: Q16, 1 / 65536 luma sample, 0 = the centre of
        sample 0 of the picture minus the crop, INT32_MIN in either coordinate = invalid (abi.remap_from_warp / _from_homography / _from_lens make such grids);
        float32: luma samples, a non-finite coordinate = invalid.  Each grid must be contiguous; grids may lie a batch stride apart (a multiple of 8 bytes).  It is
        read on the device with no host read and no synchronisation.  A numpy array of one of the two dtypes is uploaded first.
        samples 1, 2 or 4: sub-positions per axis along the grid's local derivatives.  border "clamp" replicates the picture's edge, "pad" writes `pad` where
        the pixel's position lies outside the picture; a pixel that reads an invalid node is `pad` under either (pad: one value or three, in the output's
        channel order, before the normalise; integers for the integer dtypes; default 0).  out: as for pic_output_warped."""
        import torch
        if border not in ("clamp", "pad"):
            raise ValueError(f"border must be 'clamp' or 'pad', not {border!r}")
        a = {"layout": layout, "colour": None, "filter": "bilinear", "mean": mean, "std": std, "out_bit_depth": 0, "dtype": dtype, "size": size,
             "channels_last": channels_last, "bgr": bgr, "matrix": matrix, "full_range": full_range, "chroma_loc": chroma_loc, "crop": crop}
        dtype, fmt, sc, h, w, dev = self._scaled_setup(a)
        if isinstance(grid, np.ndarray):
            if grid.dtype not in (np.int32, np.float32):
                raise ValueError(f"grid: an int32 (Q16) or float32 array, not {grid.dtype}")
            grid = torch.from_numpy(np.ascontiguousarray(grid)).to(dev)
        dims = abi.remap_grid_dims(self.lib, (h, w), step)
        if not isinstance(dims, tuple):
            raise ValueError(f"step must be 0..6 and size at least (1, 1), not step {step}, size {tuple(size)}")
        if not isinstance(grid, torch.Tensor) or grid.device != dev or grid.dtype not in (torch.int32, torch.float32):
            raise ValueError(f"grid: an int32 or float32 tensor on {dev} (or such a numpy array)")
        if grid.dim() == 3:
            grid = grid.unsqueeze(0)
        one = dims[0] * dims[1] * 2
        if grid.dim() != 4 or tuple(grid.shape[1:]) != (*dims, 2) or grid.shape[0] < 1 or grid.stride()[1:] != (dims[1] * 2, 2, 1) \
                or (grid.shape[0] > 1 and (grid.stride(0) < one or grid.stride(0) % 2)):
            raise ValueError(f"grid: [N, {dims[0]}, {dims[1]}, 2] for size {(h, w)} at step {step}, every grid contiguous and an even number of elements apart, not "
                             f"{tuple(grid.shape)} with strides {grid.stride()}")
        n = int(grid.shape[0])
        rp = abi.make_remap_params(abi.GRID_F32 if grid.dtype == torch.float32 else abi.GRID_Q16_I32, step, samples, abi.WARP_PAD if border == "pad" else abi.WARP_CLAMP,
                                   0.0 if pad is None else pad, grid_pitch=grid.stride(0) * 4 if n > 1 else 0)

        def refuse():
            rc = abi.output_remap_check(self.lib, fmt, sc, rp, n, self.width, self.height, self.bit_depth)
            if rc < 0:
                raise ValueError(f"invalid remapped output ({rc}): layout {layout}, size {tuple(size)}, step {step}, samples {samples}, border {border}, pad {pad}, "
                                 f"crop {crop}, mean {mean}, std {std}, {n} grids")
        planar = not channels_last
        if out is None:
            refuse()      # before a tensor is made, and again with its pitches
        out = _out_tensor(out, (n, 3, h, w) if planar else (n, h, w, 3), dtype, dev)
        st = out.stride()
        fmt.row_pitch = _row_pitch(st, planar, h, w if planar else 3 * w, 3) * dtype.itemsize
        rp.image_pitch = st[0] * dtype.itemsize if n > 1 else 0
        refuse()
        dl, self._dra_keep = self._dra_luts(dra) if dra is not None else (None, None)      # (kept until the next call: the tables are copied asynchronously)
        self._device_call("xgpu_pic_output_device_remap", out, pic, dl, C.byref(fmt), C.byref(sc), C.byref(rp), C.c_void_p(grid.data_ptr()),
                          abi.remap_grid_size(self.lib, sc, rp, n), n)
        return out

    def _run_stream(self, dev):
        """(torch's current stream, the stream a kernel of the C ABI is queued on): torch's default stream is the null stream, whose handle (0) means "the
        context's stream" to the C ABI - such a call runs on a side stream of torch's between two stream waits instead (the caller makes the second one)"""
        import torch
        cur = torch.cuda.current_stream(dev)
        run = cur
        if cur.cuda_stream == 0:
            if getattr(self, "_side", None) is None:
                self._side = torch.cuda.Stream(device=dev)
            run = self._side
            run.wait_stream(cur)
        return cur, run

    def _device_call(self, name, out, *args):
        """lib.<name>(ctx, *args, out's memory, the bytes it spans, stream): an output into device memory, queued on _run_stream's stream and joined to torch's
        current stream; a negative code raises XgpuError"""
        nbytes = out.numel() * out.element_size()      # the bytes the tensor spans from data_ptr(): all of them, or - rows or images apart - up to its last element
        if not out.is_contiguous():
            nbytes = (sum((n - 1) * s for n, s in zip(out.shape, out.stride())) + 1) * out.element_size()
        cur, run = self._run_stream(out.device)
        self._chk(getattr(self.lib, name)(self.ctx, *args, C.c_void_p(out.data_ptr()), nbytes, C.c_void_p(run.cuda_stream)), name)
        if run is not cur:
            cur.wait_stream(run)

    def frame_side_info(self, pic, kind="blocks", lists="both", dtype=None, per_poc=False, channels_last=False, crop=(0, 0, 0, 0), out=None):
        """The coding side information of the picture decoded LAST as a torch tensor on cuda:{device}, on torch's current stream (xgpu_frame_side_info,
        INTEGRATION.md section 8c).  `pic` must be the slot of the last decode_picture / frame_end: the SCU map it is read from is per decoder, the next
        picture overwrites it - anything else raises XgpuError.
        kind "blocks": [9, height / 4, width / 4] torch.int16, one entry per 4x4 luma unit of the uncropped picture - planes 0-3 the list 0 / list 1 vectors (x, y,
        quarter samples), 4 / 5 the POC distance of each list's reference (0: list unused), 6 the mode (0 intra, 1 inter, 2 skip, 6 IBC), 7 the QP, 8 flags (bit 0
        luma cbf, 1 / 2 left / top block edge, 3 ats_inter); crop must be 0.
        kind "flow": a dense motion field in luma samples, [C, H, W] (channels_last: [H, W, C]), C = 2 (x, y) per list of lists = "both" | 0 | 1, dtype
        torch.float16 (the default) or torch.float32, per_poc: divided by the POC distance; crop (left, right, top, bottom), even.
        out: a tensor to fill instead (its strides may pad the rows); it is also what is returned."""
        import torch
        cl, cr, ct, cb = (int(v) for v in crop)
        dev = torch.device("cuda", self.sp.device)
        if kind == "blocks":
            if dtype not in (None, torch.int16):
                raise ValueError("blocks: dtype is torch.int16")
            dtype = torch.int16
            h, w = self.height // 4, self.width // 4
            shape, planar, rows_w = (9, h, w), True, w
            fmt = abi.make_side_format(abi.SIDE_BLOCKS, abi.OUT_U16, crop=crop)
        elif kind == "flow":
            dtype = torch.float16 if dtype is None else dtype
            codes = _codes("float16", "float32")
            if dtype not in codes:
                raise ValueError(f"flow: dtype torch.float16 or torch.float32, not {dtype}")
            if lists not in ("both", 0, 1):
                raise ValueError(f"lists must be 'both', 0 or 1, not {lists!r}")
            ch = 4 if lists == "both" else 2
            h, w = self.height - ct - cb, self.width - cl - cr
            planar = not channels_last
            shape, rows_w = ((ch, h, w), w) if planar else ((h, w, ch), ch * w)
            fmt = abi.make_side_format(abi.SIDE_FLOW_PLANAR if planar else abi.SIDE_FLOW_INTERLEAVED, codes[dtype],
                                       lists=3 if lists == "both" else 1 + int(lists), per_poc=bool(per_poc), crop=crop)
        else:
            raise ValueError(f"kind must be 'blocks' or 'flow', not {kind!r}")
        if self.lib.xgpu_side_info_size(C.byref(fmt), self.width, self.height) == 0:
            raise ValueError(f"invalid side-information format (kind {kind}, lists {lists}, crop {crop})")
        out = _out_tensor(out, shape, dtype, dev)
        fmt.row_pitch = _row_pitch(out.stride(), planar, h, rows_w, shape[2], f"{rows_w} elements{' in planes of H rows' if planar else ''}") * dtype.itemsize
        self._device_call("xgpu_frame_side_info", out, pic, C.byref(fmt))
        return out

    def batch_residual(self, h, kind="yuv420", dtype=None, channels_last=False, crop=(0, 0, 0, 0), out=None):
        """The prediction residual of batch `h` - what the reconstruction adds to the prediction before the clip, 0 where nothing is coded - as a torch
        tensor on cuda:{device}, on torch's current stream (xgpu_batch_residual).  Valid once the batch's residual pass is queued
        (batch_recon / decode_picture of it, batch_prepare, or the batch passed as next_batch) and until batch_destroy, which may follow at once.
        kind "yuv420": (flat, (Y, Cb, Cr)) - a flat torch.int16 tensor in the plane order and tight layout of pic_output, and its three views [H, W],
        [H / 2, W / 2], [H / 2, W / 2]; kind "444": [3, H, W] (channels_last: [H, W, 3]) with chroma replicated, dtype torch.int16 (the default),
        torch.float32 (r * 2^-bit_depth, exact) or torch.float16; kind "energy": [3, height / 4, width / 4] torch.float32, sum |r| per 4x4 luma unit and
        component, crop must be 0.  crop (left, right, top, bottom), even.
        out: a tensor to fill instead ("yuv420": the flat one, contiguous; else its strides may pad the rows); it is what is returned (for "yuv420": first)."""
        import torch
        cl, cr, ct, cb = (int(v) for v in crop)
        dev = torch.device("cuda", self.sp.device)
        h_, w_ = self.height - ct - cb, self.width - cl - cr
        if kind == "yuv420":
            if dtype not in (None, torch.int16):
                raise ValueError("yuv420: dtype is torch.int16")
            dtype = torch.int16
            fmt = abi.make_resid_format(abi.RESID_YUV420, abi.OUT_U16, crop=crop)
            shape, planar, rows_w = (h_ * w_ * 3 // 2,), None, 0
        elif kind == "444":
            dtype = torch.int16 if dtype is None else dtype
            codes = _codes("int16", "float16", "float32")
            if dtype not in codes:
                raise ValueError(f"444: dtype torch.int16, torch.float16 or torch.float32, not {dtype}")
            planar = not channels_last
            shape, rows_w = ((3, h_, w_), w_) if planar else ((h_, w_, 3), 3 * w_)
            fmt = abi.make_resid_format(abi.RESID_444_PLANAR if planar else abi.RESID_444_INTERLEAVED, codes[dtype], crop=crop)
        elif kind == "energy":
            if dtype not in (None, torch.float32):
                raise ValueError("energy: dtype is torch.float32")
            dtype = torch.float32
            h_, w_ = self.height // 4, self.width // 4
            shape, planar, rows_w = (3, h_, w_), True, w_
            fmt = abi.make_resid_format(abi.RESID_ENERGY, abi.OUT_F32, crop=crop)
        else:
            raise ValueError(f"kind must be 'yuv420', '444' or 'energy', not {kind!r}")
        if self.lib.xgpu_resid_size(C.byref(fmt), self.width, self.height) == 0:
            raise ValueError(f"invalid residual format (kind {kind}, dtype {dtype}, crop {crop})")
        out = _out_tensor(out, shape, dtype, dev)
        if planar is None:
            if out.stride() != (1,):
                raise ValueError("out: must be contiguous")
        else:
            fmt.row_pitch = _row_pitch(out.stride(), planar, h_, rows_w, 3, f"{rows_w} elements{' in planes of H rows' if planar else ''}") * dtype.itemsize
        self._device_call("xgpu_batch_residual", out, h, C.byref(fmt))
        if kind == "yuv420":
            ny, nc = h_ * w_, (h_ // 2) * (w_ // 2)
            return out, (out[:ny].view(h_, w_), out[ny:ny + nc].view(h_ // 2, w_ // 2), out[ny + nc:].view(h_ // 2, w_ // 2))
        return out

    def pic_compare(self, pic, ref, crop=(0, 0, 0, 0), ssim=True, block_map=False, out=None, sync=True):
        """Slot `pic` against a reference, compared on the device in one pass over both on torch's current stream (xgpu_pic_compare, INTEGRATION.md section
        8h): per component Y, Cb, Cr the samples compared, the sum of squared differences, how many samples differ, the largest difference and the first
        differing position, and - ssim=True - the exact 8x8-window integer SSIM.
        ref: a slot number (it may be `pic`), or the picture as a tensor on the decoder's device in pic_output's plane order - the flat tensor
        pic_output_tensor(layout="yuv420p") returns for the uncropped picture, or any 1-D or [height * 3 // 2, pitch] tensor (rows of `pitch` elements for luma,
        of pitch / 2 for the chroma planes behind it) of torch.uint8 (8-bit streams) or a 16-bit integer type.  crop (left, right, top, bottom), even, is
        applied to both pictures.  block_map=True: also the SSE of every 16x16 luma block and of the co-located 8x8 chroma blocks, an int64 tensor
        [3, ceil(H / 16), ceil(W / 16)].
        sync=True: a dict - n, sse, n_diff, first_diff ((y, x) or None), max_abs, ssim_windows, ssim_q30 as lists of three Python ints, psnr and ssim as lists
        of three floats (abi.psnr / abi.ssim), map: the tensor or None.  sync=False: nothing is read back - the raw result, an int64 tensor of 20 words laid
        out as xgpu_compare_result (abi.compare_result_dict reads it), or with block_map the pair (result, map).  out: a tensor to take the raw result."""
        import torch
        dev = torch.device("cuda", self.sp.device)
        if isinstance(ref, torch.Tensor):
            codes = _codes("uint8", "int16", "uint16")
            if ref.dtype not in codes or ref.device != dev:
                raise ValueError(f"ref: a torch.uint8 or 16-bit integer tensor on {dev}, not {ref.dtype} on {ref.device}")
            es = ref.element_size()
            if ref.dim() == 1 and ref.stride() == (1,):
                pitch, span = 0, ref.numel() * es
            elif ref.dim() == 2 and ref.shape[0] == self.height * 3 // 2 and ref.stride(1) == 1:
                pitch, span = ref.stride(0) * es, ((ref.shape[0] - 1) * ref.stride(0) + ref.shape[1]) * es
            else:
                raise ValueError(f"ref: a contiguous 1-D tensor or [{self.height * 3 // 2}, pitch] rows, not {tuple(ref.shape)} with strides {ref.stride()}")
            r = abi.make_compare_ref(d_yuv=ref.data_ptr(), size=span, dtype=codes[ref.dtype], row_pitch=pitch)
        else:
            r = abi.make_compare_ref(pic=int(ref))
        p = abi.make_compare_params(crop, ssim, block_map)
        res = _out_tensor(out, (C.sizeof(abi.CompareResult) // 8,), torch.int64, dev)
        if res.stride() != (1,):
            raise ValueError("out: must be contiguous")
        cl, cr, ct, cb = (int(v) for v in crop)
        mshape = (3, max(-(-(self.height - ct - cb) // 16), 0), max(-(-(self.width - cl - cr) // 16), 0)) if block_map else (0,)
        bmap = torch.empty(mshape, dtype=torch.int64, device=dev)      # (no map: no memory, the call gets NULL and 0 bytes)
        self._device_call("xgpu_pic_compare", bmap, pic, C.byref(r), C.byref(p), C.c_void_p(res.data_ptr()))
        if not sync:
            return (res, bmap) if block_map else res
        d = abi.compare_result_dict(res.cpu().numpy())
        d["psnr"], d["ssim"] = abi.psnr(d, self.bit_depth), abi.ssim(d)
        d["first_diff"] = [None if f == (1 << 64) - 1 else (f >> 32, f & 0xFFFFFFFF) for f in d["first_diff"]]
        d["map"] = bmap if block_map else None
        return d

    def pic_stats(self, pic, crop=(0, 0, 0, 0), hist_bits=8, percentiles=(100, 9999), light=None, out=None, sync=True):
        """What is in slot `pic`, taken on the device in one pass on torch's current stream (xgpu_pic_stats): per component Y, Cb, Cr
        the number of samples, their sum, sum of squares, minimum and maximum, a histogram of 2^hist_bits bins (0: none; else 4 .. the coding depth) and the
        two `percentiles` of it (in 1 / 10000: the lower edge of the bin that holds them).  crop (left, right, top, bottom), even.
        light=dict(transfer=, matrix=1, full_range=False, chroma_loc=0, upsample="linear"): also the histogram of max(R', G', B') of every pixel - the codes
        pic_output_tensor(layout="rgb", dtype=torch.uint16) makes with those options - and the light level under the stream's transfer characteristic (H.273).
        sync=True: a dict - n, sum, sum_sq, min, max as lists of three Python ints, pctl as three pairs, mean and var (population variance) as lists of three
        floats (abi.stats_moments has the exact fractions), hist: an int32 tensor [3, 2^hist_bits] on the device or None; and light_hist: an int32 tensor [2^B]
        or None, light_n, light_max_code, light_pctl_code, light_max, light_pctl (linear light of those codes, 0 .. 1), light_sum, light_mean - all 0 without
        light= -, and for transfer 16 (PQ) max_cll and max_fall, this picture's contributions in cd/m2.
        sync=False: nothing is read back - (result, hist, light_hist): the raw result, an int64 tensor of 22 words laid out as xgpu_stats_result
        (abi.stats_result_dict reads it), and the two histograms or None.  out: a tensor to take the raw result."""
        import torch
        dev = torch.device("cuda", self.sp.device)
        kw = {}
        if light is not None:
            kw = dict(light)
            if "transfer" not in kw:
                raise ValueError("light: needs transfer= (H.273 TransferCharacteristics of the stream)")
            up = kw.pop("upsample", "linear")
            if up not in ("nearest", "linear"):
                raise ValueError(f"light: upsample must be 'nearest' or 'linear', not {up!r}")
            kw["upsample"] = abi.UPSAMPLE_NEAREST if up == "nearest" else abi.UPSAMPLE_LINEAR
            if set(kw) - {"transfer", "matrix", "full_range", "chroma_loc", "upsample"}:
                raise ValueError(f"light: unknown option in {sorted(kw)}")
        p = abi.make_stats_params(crop, hist_bits, percentiles, light is not None, **kw)
        res = _out_tensor(out, (C.sizeof(abi.StatsResult) // 8,), torch.int64, dev)
        if res.stride() != (1,):
            raise ValueError("out: must be contiguous")
        nb, nl = (1 << int(hist_bits) if hist_bits else 0), (1 << self.bit_depth if light is not None else 0)
        words = self.lib.xgpu_stats_hist_size(C.byref(p), self.bit_depth) // 4      # (invalid parameters: 0 - no memory, and the call says what is wrong)
        flat = torch.empty((words,), dtype=torch.int32, device=dev)
        self._device_call("xgpu_pic_stats", flat, pic, C.byref(p), C.c_void_p(res.data_ptr()))
        hist = flat[:3 * nb].view(3, nb) if nb else None
        lhist = flat[3 * nb:] if nl else None
        if not sync:
            return res, hist, lhist
        d = abi.stats_result_dict(res.cpu().numpy())
        mean, var = abi.stats_moments(d)
        d["mean"], d["var"] = [float(m) for m in mean], [float(v) for v in var]
        d["hist"], d["light_hist"] = hist, lhist
        if light is not None and int(kw["transfer"]) == 16:
            d["max_cll"], d["max_fall"] = 10000.0 * d["light_max"], 10000.0 * d["light_mean"]
        return d

    def pic_md5(self, pic, dra=None):
        """the picture signature made on the device (xgpu_pic_md5): [Y, U, V] digests of 16 bytes - the MD5 of every plane's 16-bit samples as the reference's
        xevd_md5_imgb makes it; with `dra` tables (as pic_output takes them) of the DRA-mapped picture"""
        dl, keep = self._dra_luts(dra)
        out = np.zeros((3, 16), np.uint8)
        self._chk(self.lib.xgpu_pic_md5(self.ctx, pic, dl, out.ctypes.data), "xgpu_pic_md5")
        return [bytes(out[c]) for c in range(3)]

    def host_alloc(self, nbytes, dtype=np.uint8):
        """pinned host memory from the backend as a numpy array (freed with the decoder): for coefficient arenas and output buffers"""
        p = C.c_void_p()
        self._chk(self.lib.xgpu_host_alloc(self.ctx, nbytes, C.byref(p)), "xgpu_host_alloc")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (nbytes,)).view(dtype)

    def pic_output_async(self, pic, out, out_bit_depth=0, crop=(0, 0, 0, 0)):
        """queue conversion + packing + the copy into `out` (uint8 array, pinned for a truly asynchronous copy) -> ticket for pic_output_wait"""
        t = C.c_int()
        self._chk(self.lib.xgpu_pic_output_async(self.ctx, pic, None, out_bit_depth or self.bit_depth, *crop, out.ctypes.data, out.nbytes, C.byref(t)),
                  "xgpu_pic_output_async")
        return t.value

    def pic_output_wait(self, ticket):
        self._chk(self.lib.xgpu_pic_output_wait(self.ctx, ticket), "xgpu_pic_output_wait")

    def batch_dmvr_mvs(self, h):
        """the vectors kept for temporal prediction of the batch's DMVR candidates after batch_recon: [n_sub_blocks][list][x/y], quarter samples"""
        n = self._chk(self.lib.xgpu_batch_dmvr_mvs(self.ctx, h, None, 0), "xgpu_batch_dmvr_mvs")
        out = np.zeros((max(n, 1), 2, 2), np.int16)
        self._chk(self.lib.xgpu_batch_dmvr_mvs(self.ctx, h, out.ctypes.data, n), "xgpu_batch_dmvr_mvs")
        return out[:n]

    def batch_info(self, h):
        """what the batch builder made of the batch: CU / TB / work-item counts, nodes and depth of the dependency graph (xgpu_batch_info)"""
        v = (C.c_int * 8)()
        self._chk(self.lib.xgpu_batch_info(self.ctx, h, v), "xgpu_batch_info")
        return dict(zip(("n_cu", "n_tb", "itdq_items", "dep_nodes", "dep_nodes_level1", "dep_levels", "dmvr_sub_blocks", "affine_tiles"), list(v)))

    def batch_wait_upload(self, h):
        self._chk(self.lib.xgpu_batch_wait_upload(self.ctx, h), "xgpu_batch_wait_upload")

    def pic_upload_padded(self, pic, bufs):
        y, u, v = (np.ascontiguousarray(p, np.int16) for p in bufs)
        self._chk(self.lib.xgpu_pic_upload_padded(self.ctx, pic, y.ctypes.data, u.ctypes.data, v.ctypes.data), "xgpu_pic_upload_padded")

    def pic_download_padded(self, pic):
        y = np.zeros((self.height + 2 * abi.PAD_L, self.width + 2 * abi.PAD_L), np.int16)
        u = np.zeros((self.height // 2 + 2 * abi.PAD_C, self.width // 2 + 2 * abi.PAD_C), np.int16)
        v = np.zeros_like(u)
        self._chk(self.lib.xgpu_pic_download_padded(self.ctx, pic, y.ctypes.data, u.ctypes.data, v.ctypes.data), "xgpu_pic_download_padded")
        return [y, u, v]

    def pic_download_padded_luma(self, pic):
        """the padded luma plane alone (what a front end that refines vectors itself registers with xhost_parser_set_ref_luma)"""
        y = np.zeros((self.height + 2 * abi.PAD_L, self.width + 2 * abi.PAD_L), np.int16)
        self._chk(self.lib.xgpu_pic_download_padded(self.ctx, pic, y.ctypes.data, None, None), "xgpu_pic_download_padded")
        return y

    # -- per picture ---------------------------------------------------------------------------------
    def frame_begin(self, pic, poc, refs, qp_u_offset=0, qp_v_offset=0, deblock_on=0, alf_on=0, alpha_off=0, beta_off=0):
        """refs: {(idx, list): (pic_slot, poc)}"""
        fp = abi.FrameParams()
        fp.pic, fp.poc = pic, poc
        for l in range(2):
            idxs = [i for (i, ll) in refs if ll == l]
            fp.num_refp[l] = (max(idxs) + 1) if idxs else 0
        for (i, l), (slot, rpoc) in refs.items():
            fp.refp_pic[i][l] = slot
            fp.refp_poc[i][l] = rpoc
        fp.qp_u_offset, fp.qp_v_offset = qp_u_offset, qp_v_offset
        fp.deblock_alpha_offset, fp.deblock_beta_offset = alpha_off, beta_off
        fp.deblock_on, fp.alf_on = int(deblock_on), int(alf_on)
        self._chk(self.lib.xgpu_frame_begin(self.ctx, C.byref(fp)), "xgpu_frame_begin")

    def batch_create(self, batch):
        cb, keep = abi.make_cu_batch(batch)
        h = C.c_void_p()
        self._chk(self.lib.xgpu_batch_create(self.ctx, C.byref(cb), C.byref(h)), "xgpu_batch_create")
        self._batches.append(h)
        return h

    def batch_create_from_struct(self, cu_batch):
        """xgpu_batch_create on a filled abi.CuBatch (e.g. the one inside the host parser's xhost_picture): no numpy round trip"""
        h = C.c_void_p()
        self._chk(self.lib.xgpu_batch_create(self.ctx, C.byref(cu_batch), C.byref(h)), "xgpu_batch_create")
        self._batches.append(h)
        return h

    def batch_resid(self, h, n_coef):
        out = np.zeros(max(n_coef, 1), np.int16)
        self._chk(self.lib.xgpu_test_batch_resid(self.ctx, h, out.ctypes.data), "xgpu_test_batch_resid")
        return out

    def batch_destroy(self, h):
        self._batches = [b for b in self._batches if b.value != h.value]
        self.lib.xgpu_batch_destroy(self.ctx, h)

    def batch_prepare(self, h):
        """queue the batch's residual pass ahead of its picture (xgpu_batch_prepare)"""
        self._chk(self.lib.xgpu_batch_prepare(self.ctx, h), "xgpu_batch_prepare")

    def batch_recon(self, h, next_batch=None):
        """next_batch: the NEXT picture's batch - its residual pass is queued with this picture's kernels (xgpu_batch_recon_ahead)"""
        if next_batch is None:
            self._chk(self.lib.xgpu_batch_recon(self.ctx, h), "xgpu_batch_recon")
        else:
            self._chk(self.lib.xgpu_batch_recon_ahead(self.ctx, h, next_batch), "xgpu_batch_recon_ahead")

    def deblock(self):
        self._chk(self.lib.xgpu_deblock(self.ctx), "xgpu_deblock")

    def alf(self, params):
        ap, keep = abi.make_alf_params(params)
        self._chk(self.lib.xgpu_alf(self.ctx, C.byref(ap)), "xgpu_alf")

    def pad(self):
        self._chk(self.lib.xgpu_pad(self.ctx), "xgpu_pad")

    def frame_end(self):
        self._chk(self.lib.xgpu_frame_end(self.ctx), "xgpu_frame_end")

    def decode_picture(self, pic, poc, refs, batch_handle, deblock=True, pad=True, qp_u_offset=0, qp_v_offset=0,
                       alpha_off=0, beta_off=0, alf=None, next_batch=None):
        """The coarse sequence of xevd_dec_nalu for one picture (src_base/xevd.c:1905-1983, src_main/xevdm.c:3136-3219)."""
        self.frame_begin(pic, poc, refs, qp_u_offset, qp_v_offset, deblock_on=deblock, alf_on=alf is not None,
                         alpha_off=alpha_off, beta_off=beta_off)
        self.batch_recon(batch_handle, next_batch)      # with the next picture's residual pass under this picture's dependency kernel
        if deblock:
            self.deblock()
        if alf is not None:
            self.alf(alf)
        if pad:
            self.pad()
        self.frame_end()

    # -- measurement ---------------------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._chk(self.lib.xgpu_timing_enable(self.ctx, 1 if on else 0), "xgpu_timing_enable")

    def timing_reset(self):
        self._chk(self.lib.xgpu_timing_reset(self.ctx), "xgpu_timing_reset")

    def timing_get(self):
        ms = (C.c_double * abi.K_COUNT)()
        n = (C.c_longlong * abi.K_COUNT)()
        self._chk(self.lib.xgpu_timing_get(self.ctx, ms, n), "xgpu_timing_get")
        return {abi.K_NAMES[i]: (ms[i], n[i]) for i in range(abi.K_COUNT)}

    def measure_copy_bw(self, nbytes=1 << 30, iters=10):
        g = C.c_double()
        self._chk(self.lib.xgpu_measure_copy_bw(self.ctx, nbytes, iters, C.byref(g)), "xgpu_measure_copy_bw")
        return g.value

    # -- fine-grained shims --------------------------------------------------------------------------
    def test_mc(self, plane, ref_x, ref_y, has_dx, has_dy, gmv_x, gmv_y, w, h, bit_depth, luma=True):
        plane = np.ascontiguousarray(plane, np.int16)
        pred = np.zeros((h, w), np.int16)
        fn = self.lib.xgpu_test_mc_l if luma else self.lib.xgpu_test_mc_c
        self._chk(fn(self.ctx, plane.ctypes.data, plane.shape[1], plane.shape[0], ref_x, ref_y, has_dx, has_dy, gmv_x, gmv_y,
                     pred.ctypes.data, w, h, bit_depth), "xgpu_test_mc")
        return pred

    def test_recon(self, coef, pred, is_coef, rec, bit_depth):
        """fn_recon's shape: coef / pred [cuh][cuw], rec [cuh][s_rec] (only its first cuw columns are written) -> rec"""
        coef, pred = np.ascontiguousarray(coef, np.int16), np.ascontiguousarray(pred, np.int16)
        rec = np.ascontiguousarray(rec, np.int16).copy()
        self._chk(self.lib.xgpu_test_recon(self.ctx, coef.ctypes.data, pred.ctypes.data, int(is_coef), pred.shape[1], pred.shape[0], rec.shape[1],
                                           rec.ctypes.data, bit_depth), "xgpu_test_recon")
        return rec

    def test_dbk(self, plane, x, y, st, hor, bit_depth, plane_v=None, st_v=0):
        """fn_dbk / fn_dbk_chroma's shape on one edge segment of a small plane (both chroma planes when plane_v is given) -> filtered plane(s)"""
        plane = np.ascontiguousarray(plane, np.int16).copy()
        if plane_v is None:
            self._chk(self.lib.xgpu_test_dbk(self.ctx, plane.ctypes.data, plane.shape[1], plane.shape[0], x, y, st, int(hor), bit_depth), "xgpu_test_dbk")
            return plane
        plane_v = np.ascontiguousarray(plane_v, np.int16).copy()
        self._chk(self.lib.xgpu_test_dbk_chroma(self.ctx, plane.ctypes.data, plane_v.ctypes.data, plane.shape[1], plane.shape[0], x, y, st, st_v, int(hor),
                                                bit_depth), "xgpu_test_dbk_chroma")
        return plane, plane_v

    def test_itdq(self, coef, log2w, log2h, qp, bit_depth, tr_v=0, tr_h=0, log2s=None):
        """len(qp) blocks of one size class through the residual kernel.  tr_v / tr_h: 0 DCT-II, 1 DST-VII, 2 DCT-VIII (the kernel's TR_* codes); log2s: log2 of the
        row stride (default: the width), block i then starts at i * (h << log2s) and the samples outside its columns come back untouched"""
        coef = np.ascontiguousarray(coef, np.int16).copy()
        qp = np.ascontiguousarray(qp, np.uint8)
        log2s = log2w if log2s is None else log2s
        assert coef.size == len(qp) << (log2s + log2h), "n blocks of h << log2s samples"
        self._chk(self.lib.xgpu_test_itdq_ex(self.ctx, coef.ctypes.data, len(qp), log2w, log2h, qp.ctypes.data, bit_depth, tr_v, tr_h, log2s), "xgpu_test_itdq_ex")
        return coef

    def test_itdq_pairs(self, coef, log2w, log2h, qp, bit_depth, tr_v=0, tr_h=0, log2s=None):
        """test_itdq through the pair form (two work items per workgroup, IQT contexts only); the samples outside a block's columns come back as 0x5A5A"""
        coef = np.ascontiguousarray(coef, np.int16).copy()
        qp = np.ascontiguousarray(qp, np.uint8)
        log2s = log2w if log2s is None else log2s
        assert coef.size == len(qp) << (log2s + log2h), "n blocks of h << log2s samples"
        self._chk(self.lib.xgpu_test_itdq_pairs(self.ctx, coef.ctypes.data, len(qp), log2w, log2h, qp.ctypes.data, bit_depth, tr_v, tr_h, log2s), "xgpu_test_itdq_pairs")
        return coef

    def test_itdq_pairs_mixed(self, coef, groups, qp, bit_depth):
        """groups: rows of (n_blocks, log2w, log2h, tr_v, tr_h, log2s), each group's blocks back to back from the next multiple of 64 samples; qp: one per block in
        group order.  One launch of the pair form over all of them; what no block covers comes back as 0x5A5A"""
        coef = np.ascontiguousarray(coef, np.int16).copy()
        qp = np.ascontiguousarray(qp, np.uint8)
        groups = np.ascontiguousarray(groups, np.int32).reshape(-1, 6)
        total = 0
        for n, lw, lh, _, _, ls in groups.tolist():
            total = ((total + 63) & ~63) + (n << (ls + lh))
        assert coef.size == total and len(qp) == int(groups[:, 0].sum())
        self._chk(self.lib.xgpu_test_itdq_pairs_mixed(self.ctx, coef.ctypes.data, len(groups), groups.ctypes.data, qp.ctypes.data, bit_depth), "xgpu_test_itdq_pairs_mixed")
        return coef
