"""Bitstream -> pictures on the GPU: the decoder loop a user of the reference's xevd_decode / xevd_pull pair would write on top of
the two C ABIs (include/xevd_host.h parser, include/xevd_hip.h backend).  The host parser runs in its own thread, one picture
ahead (entropy decoding of picture k+1 overlaps the upload + kernels of picture k); DPB slots are managed by POC exactly as the
parser reports them (references by POC, released POCs).  Plumbing only - no sample arithmetic here."""
import queue
import threading

from . import abi, stream
from .decoder import XgpuDecoder


class StreamDecoder:
    def __init__(self, data, device=0, prefetch=2, verify_md5=False, apply_crop=False, parser_threads=1):
        """verify_md5: check downloaded pictures against the stream's picture-signature SEIs (the reference's
        XEVD_CFG_SET_USE_PIC_SIGNATURE), raising on a mismatch"""
        self.data, self.device, self.prefetch, self.verify_md5 = data, device, prefetch, verify_md5
        self._lock, self._dec, self._abort = threading.Lock(), None, False
        self.parser_threads = parser_threads      # host threads for the tiles of one picture (xhost_parser_set_threads)
        self.apply_crop = apply_crop      # packed output: cut the SPS conformance window (the reference application writes uncropped pictures)

    N_SLOTS = 33      # the parser keeps at most 32 reference pictures (+ the current one): a slot is always free

    def _producer(self, q):
        """parser thread: entropy decoding, and - zero-copy, while the parser's arrays are valid - the hand-over of every picture's CU batch to
        the backend (builder + upload into pooled buffers).  The backend context is not thread-safe: calls on it are serialised by self._lock."""
        def to_device(p, cu_batch):
            with self._lock:
                if self._dec is None:
                    self._dec = XgpuDecoder(p["width"], p["height"], p["bit_depth"], device=self.device, iqt=p["iqt"], admvp=p["admvp"], addb=p["addb"], alf=p["tool_alf"],
                                            eipd=p["eipd"], max_pics=34, chroma_qp_tables=p["chroma_qp_tables"], bit_depth_chroma=p["bit_depth_chroma"])
                return self._dec.batch_create_from_struct(cu_batch)
        try:
            for p in stream.iter_stream(self.data, consume_batch=to_device, threads=self.parser_threads):
                if p["n_dmvr_sub"]:
                    p["_dmvr"] = [threading.Event(), None]
                if p["needs_ref_luma"]:
                    p["_luma"] = [threading.Event(), None]
                q.put(p)
                if p["needs_ref_luma"]:
                    # tool_dmvr with tool_hmvp / tool_mmvd: the parser refines merge vectors itself while it parses the NEXT pictures and reads this
                    # picture's decoded luma for it - the consumer downloads it (padded) right behind the picture's kernels
                    while not p["_luma"][0].wait(0.05):
                        if self._abort:
                            return
                    p["set_ref_luma"](p["poc"], p["_luma"][1], abi.PAD_L)
                if p["n_dmvr_sub"]:
                    # sps->tool_dmvr: the temporal candidates of later pictures read this picture's REFINED vectors - the parser waits for the
                    # backend's (xgpu_batch_dmvr_mvs, fetched by the consumer right after the picture's kernels were queued)
                    while not p["_dmvr"][0].wait(0.05):
                        if self._abort:
                            return
                    p["dmvr_feedback"](p["_dmvr"][1])
            q.put(None)
        except Exception as e:      # surfaced in the consumer thread
            q.put(e)

    @staticmethod
    def signature_ok(p, planes):
        """the stream's picture-signature SEI (MD5 per plane over 16-bit samples, xevd_picbuf_check_signature) against decoded planes"""
        import hashlib
        import numpy as np
        return all(hashlib.md5(np.ascontiguousarray(pl, "<i2").tobytes()).digest() == p["md5"][c] for c, pl in enumerate(planes))

    @classmethod
    def tensor_options(cls, p, options):
        """the keyword arguments of XgpuDecoder.pic_output_tensor for picture p: matrix, range and chroma siting from the stream's VUI (a VUI that leaves
        them unspecified, or none: BT.709, limited range, type 0), the conformance-window crop and DRA tables of the picture - `options` override all"""
        col = p["colour"]
        kw = {"matrix": 1, "full_range": False, "chroma_loc": 0, "dra": p["dra"]}
        if col["vui_present"]:
            kw["full_range"] = bool(col["full_range"])
            kw["chroma_loc"] = col["chroma_sample_loc_type"]
            if col["matrix_coefficients"] != 2:      # 2 = unspecified
                kw["matrix"] = col["matrix_coefficients"]
        kw.update(options)
        return kw

    @classmethod
    def light_options(cls, colour, options=None):
        """the `light=` argument of XgpuDecoder.pic_stats for a stream whose VUI says `colour` (params["colour"]): matrix, range and chroma siting as
        tensor_options takes them, the transfer characteristic as colour_transform does (a VUI that leaves it unspecified, or none: BT.709) - `options`
        (a dict, or True / None for none) override all"""
        kw = cls.tensor_options({"colour": colour, "dra": None}, {})
        del kw["dra"]
        kw["transfer"] = 1
        if colour["vui_present"] and colour["transfer_characteristics"] != 2:
            kw["transfer"] = colour["transfer_characteristics"]
        if isinstance(options, dict):
            kw.update(options)
        return kw

    # `to=` presets: (ColourPrimaries, TransferCharacteristics) of the output (H.273; transfer 8 = linear light)
    COLOUR_PRESETS = {"srgb": (1, 13), "bt709": (1, 1), "linear-bt709": (1, 8), "bt2020": (9, 14), "linear-bt2020": (9, 8), "pq-bt2020": (9, 16),
                      "hlg-bt2020": (9, 18), "p3-d65": (12, 13), "linear-p3-d65": (12, 8)}

    @classmethod
    def colour_transform(cls, colour, to):
        """the `colour=` argument of XgpuDecoder.pic_output_tensor for a stream whose VUI says `colour` (params["colour"]) and the destination `to`: a preset
        name of COLOUR_PRESETS, or dict(to=name, ...) with any of tone_map, src_peak, dst_peak, linear_scale.  The source side is the VUI's colour_primaries /
        transfer_characteristics; where the VUI is absent or says 2 (unspecified): BT.709 / BT.709, as for the matrix.  tone_map defaults to on from an HDR
        source (PQ, HLG) to an SDR-encoded destination (neither linear nor PQ / HLG), else off."""
        opts = {"to": to} if isinstance(to, str) else dict(to)
        name = opts.pop("to")
        if name not in cls.COLOUR_PRESETS:
            raise ValueError(f"to: unknown colour preset {name!r} (one of {', '.join(sorted(cls.COLOUR_PRESETS))})")
        sp = st = 1
        if colour["vui_present"]:
            sp = colour["colour_primaries"] if colour["colour_primaries"] != 2 else 1
            st = colour["transfer_characteristics"] if colour["transfer_characteristics"] != 2 else 1
        dp, dt = cls.COLOUR_PRESETS[name]
        cm = {"src_primaries": sp, "src_transfer": st, "dst_primaries": dp, "dst_transfer": dt, "tone_map": st in (16, 18) and dt not in (8, 16, 18)}
        for k, v in opts.items():
            if k not in ("tone_map", "src_peak", "dst_peak", "linear_scale"):
                raise ValueError(f"to: unknown option {k!r}")
            cm[k] = v
        return cm

    def pictures(self, download=True, output_bit_depth=None, tensor=None, to=None, side=None, size=None, mean=None, std=None, rois=None, fit=None, pad=None,
                 residual=None, compare=None, stats=None, warp=None, remap=None, remap_step=0, surfaces=None, surface_layout="nv12", surface_options=None,
                 linear_light=False, resample=None, packed=None, lut=None, dither=None, overlay=None):
        """generator of (params, planes or None) in DECODING order; planes = [Y, U, V] int16 arrays of the active area, or - with
        output_bit_depth (0 = the coding depth) - the bytes of one .yuv frame, converted and packed on the device, or - with
        tensor=dict(...) (keyword arguments of XgpuDecoder.pic_output_tensor, {} for the defaults) - a torch tensor on the GPU converted on torch's
        current stream, by default with the colour description of the stream's VUI (tensor_options) and the SPS crop when apply_crop is set.
        to="srgb" | "bt709" | "linear-bt709" | "linear-bt2020" | "pq-bt2020" | ... (colour_transform; with tensor=, layout "rgb"): the picture in that colour
        space, from the primaries and transfer characteristics of the stream's VUI.  With size= (and host rois=, a list or a callable) the picture is resized and
        transformed in one call (XgpuDecoder.pic_output_scaled_cm); boxes in device memory, warp= and remap= take no colour transform.
        linear_light=True (with tensor=, size= and to=): that call filters the linear light of the source instead of its encoded samples
        (pic_output_scaled_cm's linear_light; tensor=dict(upsample="nearest") goes with it) - gamma-correct resize, what a reduced HDR picture needs.
        side=dict(...) (keyword arguments of XgpuDecoder.frame_side_info, {} for the block planes): the coding side information of every picture - motion
        vectors, modes, QP - as a torch tensor under params["side_info"] (the yielded tuple keeps its shape), taken right behind the picture's kernels, before
        the next picture overwrites the map it is read from; kind "flow" defaults to the SPS crop when apply_crop is set
        residual=dict(...) (keyword arguments of XgpuDecoder.batch_residual, {} for the int16 4:2:0 planes): the prediction residual of every picture under
        params["residual"] - for kind "yuv420" the pair (flat tensor, (Y, Cb, Cr) views) -, taken before the picture's batch goes back to the pool; the crop
        defaults to the SPS crop when apply_crop is set (kind "energy": no crop)
        size=(H, W), mean=, std= (with tensor=, layouts "rgb" / "yuv444"): every picture resized to H x W and normalised in the same call (pic_output_tensor's
        size / mean / std; tensor=dict(filter="area") for the box filter) - what a model takes, without a full-size tensor in between
        resample="bicubic" | "catmull-rom" | "cubic-0.75" | "mitchell" or dict(kernel=, antialias=) (with tensor= and size=; host rois=, fit=, pad= go with it):
        that resize with a bicubic filter instead (XgpuDecoder.pic_output_resampled) - the resize CLIP / SigLIP, DINOv2 and most timm models were trained
        with.  Not together with to=, linear_light, warp=, remap= or boxes in device memory
        rois=[(x, y, w, h), ...] or a callable(params) -> such a list (with tensor= and size=; called behind the picture's kernels, so params["side_info"] is
        there when side= is given), fit=, pad=: every picture as the batch [N, 3, H, W] of its rectangles (pic_output_tensor's rois / fit / pad;
        tensor=dict(snap=True) for boxes a detector made).  The list, or what the callable returns, may also be a torch tensor on the decoder's device - int32
        [N, 4] xywh or float32 [N, 4] xyxy, a detector's boxes where it left them: they are read on the device, with no host read in between
        (pic_output_tensor's rois=<tensor>; tensor=dict(count=, max_roi=) go with it)
        warp=[theta, ...], an int64 [N, 6] array or tensor of Q16 maps, or a callable(params) -> one of these (with tensor= and size=, called as rois= is):
        every picture as the batch [N, 3, H, W] of its affine maps (XgpuDecoder.pic_output_warped; tensor=dict(samples=, border=, pad=, status=) go with it,
        and pic_output_tensor's arguments that the warped output does not have must be left out).  Not together with rois=
        remap=grid, or a callable(params) -> grid (with tensor= and size=, called as warp= is): every picture as the batch [N, 3, H, W] of its coordinate grids
        (XgpuDecoder.pic_output_remapped: an int32 Q16 or float32 tensor on the decoder's device - made once, used for every picture - or such a numpy array;
        remap_step = its step; tensor=dict(samples=, border=, pad=) go with it).  Not together with rois= or warp=
        compare=callable(params) -> a reference or None, or a sequence of such indexed in decoding order (shorter: the pictures past its end are not
        compared): every picture against its reference on the device (XgpuDecoder.pic_compare: a tensor in pic_output's plane order on the decoder's device; a
        dict(ref=..., ssim=..., block_map=...) passes pic_compare's other arguments), taken right behind the picture's kernels; the result - pic_compare's
        dict - under params["compare"], None where there was no reference.  The crop defaults to the SPS crop when apply_crop is set
        stats=dict(...) (keyword arguments of XgpuDecoder.pic_stats, {} for the defaults) or a callable(params) -> such a dict or None: the statistics of every
        picture - census, histograms, percentiles - under params["stats"] (pic_stats' dict; with sync=False its tuple of device tensors), taken right behind the
        picture's kernels.  light=True or light=dict(...) in it adds the light level with the matrix, range, chroma siting and transfer characteristic of the
        stream's VUI (light_options; the dict overrides them).  The crop defaults to the SPS crop when apply_crop is set
        surfaces=[(H, W), ...], surface_layout="nv12" | "p016" | "yuv420p": every picture as a ladder of scaled video surfaces, one tensor per size, under
        params["surfaces"] (XgpuDecoder.pic_output_surfaces, next to whatever else was asked: the yielded tuple keeps its shape) - the renditions of a
        transcode, where an encoder takes them.  surface_options=dict(...) passes its other arguments (dtype, out_bit_depth, filter, dst_chroma_loc);
        chroma_loc and the DRA tables are the stream's, the crop defaults to the SPS crop when apply_crop is set
        packed=dict(layout=..., ...) (keyword arguments of XgpuDecoder.pic_output_packed): every picture as a packed display surface - RGBA, 10:10:10:2, packed
        4:2:2 - under params["packed"], next to whatever else was asked as surfaces= is.  Matrix, range, chroma siting and the DRA tables are the stream's
        (tensor_options), the crop defaults to the SPS crop when apply_crop is set, and with to= the RGB layouts' colour= is made from the stream's VUI as it is
        for tensor=
        lut=<path of a .cube file> | <nodes, as XgpuDecoder.lut3d_create takes them> | <a handle of that call> (with tensor=, layout "rgb", and / or packed= with
        one of its RGB layouts): every picture through that 3D LUT (XgpuDecoder.pic_output_lut3d) - a look, a log to display or HDR to
        SDR conversion that exists only as a table.  A path or nodes are uploaded once, at the first picture.  Not together with to=, size=, rois=, warp=,
        remap= or surfaces=: the LUT has the full-size RGB and packed forms only
        dither="blue" | "bayer" | dict(kind=, size=, seed=, temporal=True) | <a handle of XgpuDecoder.dither_create> (with tensor=, layouts "rgb", "nv12", "p016",
        and / or packed= with one of its RGB layouts; integer dtypes): every picture with that dither matrix in place of the final rounding
        (XgpuDecoder.pic_output_dithered; kind / size / seed as dither_create takes them, 64 and 1 by default).  The matrix is made
        and uploaded once, at the first picture.  temporal=True moves it from picture to picture by xgpu_dither_phase(poc & 0xFFFFFFFF); without it the phase is
        (0, 0).  to= goes with it; an option that has no dithered form (size=, rois=, warp=, remap=, resample=, surfaces=, lut=, mean=, std=, float dtypes, the
        other layouts) raises XgpuError before decoding starts
        overlay=dict(layers=[...], boxes=dict(...)) or a callable(params) -> such a dict or None (with tensor=, layouts "rgb", "nv12", "p016", and / or packed=
        with one of its RGB layouts; integer dtypes; called behind the picture's kernels as rois= is): every picture with those layers alpha-blended over it
        (XgpuDecoder.pic_output_overlaid) - a logo, a subtitle plane, the boxes a detector left on the device.  to= goes with it (the
        layers are codes of the destination); an option that has no overlaid form (dither=, lut=, size=, rois=, warp=, remap=, resample=, surfaces=, mean=,
        std=, float dtypes, the other layouts) raises XgpuError before decoding starts"""
        if overlay is not None:
            from .decoder import XgpuError
            if not callable(overlay) and (not isinstance(overlay, dict) or set(overlay) - {"layers", "boxes"}):
                raise XgpuError("overlay: dict(layers=, boxes=) or a callable(params) that returns one")
            if tensor is None and packed is None:
                raise XgpuError("overlay: needs tensor=dict(...) or packed=dict(layout=...)")
            clash = [k for k, v in (("dither", dither), ("lut", lut), ("size", size), ("mean", mean), ("std", std), ("rois", rois), ("warp", warp), ("remap", remap),
                                    ("resample", resample), ("surfaces", surfaces), ("linear_light", linear_light or None)) if v is not None]
            if clash:
                raise XgpuError(f"overlay: not together with {', '.join(k + '=' for k in clash)} - the overlaid output has the full-size RGB, NV12 / P016 and packed RGB forms only")
            for what, opts, layouts, first in (("tensor", tensor, ("rgb", "nv12", "p016"), "rgb"), ("packed", packed, ("rgba", "bgra", "rgb10a2", "bgr10a2"), "rgba")):
                if opts is None:
                    continue
                if opts.get("layout", first) not in layouts:
                    raise XgpuError(f"overlay: {what} layout {opts['layout']!r} has no overlaid form (one of {', '.join(layouts)})")
                dt = opts.get("dtype")
                if dt is not None and (getattr(dt, "is_floating_point", False) or "float" in str(dt)):
                    raise XgpuError(f"overlay: an overlaid output has integer dtypes, not {dt}")
                if to is not None and opts.get("layout", first) in ("nv12", "p016"):
                    raise XgpuError("overlay: to= needs an RGB layout")
        dither_opts = None
        if dither is not None:
            from .decoder import XgpuError
            if isinstance(dither, (str, int)):
                dither_opts = {"handle": dither} if isinstance(dither, int) else {"kind": dither}
            else:
                dither_opts = dict(dither)
            if set(dither_opts) - {"kind", "size", "seed", "temporal", "handle"}:
                raise XgpuError(f"dither: a kind, a handle or dict(kind=, size=, seed=, temporal=), not the keys {sorted(dither_opts)}")
            if "handle" not in dither_opts and dither_opts.setdefault("kind", "blue") not in ("blue", "bayer"):
                raise XgpuError(f"dither: kind must be 'blue' or 'bayer', not {dither_opts['kind']!r}")
            if tensor is None and packed is None:
                raise XgpuError("dither: needs tensor=dict(...) or packed=dict(layout=...)")
            clash = [k for k, v in (("size", size), ("mean", mean), ("std", std), ("rois", rois), ("warp", warp), ("remap", remap), ("resample", resample),
                                    ("surfaces", surfaces), ("lut", lut), ("linear_light", linear_light or None)) if v is not None]
            if clash:
                raise XgpuError(f"dither: not together with {', '.join(k + '=' for k in clash)} - the dithered output has the full-size RGB, NV12 / P016 and packed RGB forms only")
            for what, opts, layouts, first in (("tensor", tensor, ("rgb", "nv12", "p016"), "rgb"), ("packed", packed, ("rgba", "bgra", "rgb10a2", "bgr10a2"), "rgba")):
                if opts is None:
                    continue
                if opts.get("layout", first) not in layouts:
                    raise XgpuError(f"dither: {what} layout {opts['layout']!r} has no dithered form (one of {', '.join(layouts)})")
                dt = opts.get("dtype")
                if dt is not None and (getattr(dt, "is_floating_point", False) or "float" in str(dt)):
                    raise XgpuError(f"dither: a dithered output has integer dtypes, not {dt}")
                if to is not None and opts.get("layout", first) in ("nv12", "p016"):
                    raise XgpuError("dither: to= needs an RGB layout")
        if lut is not None:
            if tensor is None and packed is None:
                raise ValueError("lut: needs tensor=dict(...) or packed=dict(layout=...)")
            clash = [k for k, v in (("to", to), ("size", size), ("rois", rois), ("warp", warp), ("remap", remap), ("surfaces", surfaces)) if v is not None]
            if clash:
                raise ValueError(f"lut: not together with {', '.join(k + '=' for k in clash)} - the 3D LUT has the full-size RGB and packed outputs only")
            if tensor is not None and tensor.get("layout", "rgb") != "rgb":
                raise ValueError(f"lut: a 3D LUT needs tensor layout 'rgb', not {tensor['layout']!r}")
            if packed is not None and packed.get("layout", "rgba") in ("yuyv", "uyvy"):
                raise ValueError(f"lut: a 3D LUT needs one of the packed RGB layouts, not {packed['layout']!r}")
        lut_handle = []
        if surfaces is None and surface_options is not None:
            raise ValueError("surface_options: needs surfaces=[(H, W), ...]")
        if to is not None and tensor is None and packed is None:
            raise ValueError("to: needs tensor=dict(...) or packed=dict(...)")
        if linear_light and (tensor is None or size is None or to is None):
            raise ValueError("linear_light: needs tensor=dict(...), size=(H, W) and to=")
        if (size is not None or mean is not None or std is not None) and tensor is None:
            raise ValueError("size / mean / std: need tensor=dict(...)")
        if rois is not None and (tensor is None or size is None):
            raise ValueError("rois: need tensor=dict(...) and size=(H, W)")
        if (fit is not None or pad is not None) and rois is None:
            raise ValueError("fit / pad: need rois=")
        if warp is not None and rois is not None:
            raise ValueError("warp: not together with rois=")
        if warp is not None and (tensor is None or size is None or to is not None):
            raise ValueError("warp: needs tensor=dict(...) and size=(H, W), and takes no colour transform")
        if remap is not None and (rois is not None or warp is not None):
            raise ValueError("remap: not together with rois= or warp=")
        if remap is not None and (tensor is None or size is None or to is not None):
            raise ValueError("remap: needs tensor=dict(...) and size=(H, W), and takes no colour transform")
        if resample is not None:
            if tensor is None or size is None:
                raise ValueError("resample: needs tensor=dict(...) and size=(H, W)")
            if to is not None or linear_light or warp is not None or remap is not None:
                raise ValueError("resample: the bicubic resize takes no colour transform (to=, linear_light) and has no warped or remapped form")
            if rois is not None and not callable(rois) and not isinstance(rois, (list, tuple)):
                raise ValueError("resample: boxes in device memory have no bicubic form - rois= a list of rectangles, or a callable that returns one")
            resample = {"kernel": resample} if isinstance(resample, str) else dict(resample)
            if set(resample) - {"kernel", "antialias"}:
                raise ValueError(f"resample: a kernel name or dict(kernel=, antialias=), not the keys {sorted(set(resample) - {'kernel', 'antialias'})}")
        q = queue.Queue(maxsize=self.prefetch)
        th = threading.Thread(target=self._producer, args=(q,), daemon=True)
        th.start()
        slots, free = {}, []
        n_decoded = [0]

        def lut_of(dec):
            if not lut_handle:      # (under the lock) an int is a handle of dec.lut3d_create, anything else is what that call takes
                lut_handle.append(int(lut) if isinstance(lut, int) else dec.lut3d_create(lut))
            return lut_handle[0]

        dither_made = []

        def dither_of(dec, p):      # (under the lock) -> (handle, phase) of picture p; the matrix is made at the first picture
            if not dither_made:
                h = dither_opts["handle"] if "handle" in dither_opts else dec.dither_create(dither_opts["kind"], dither_opts.get("size", 64), dither_opts.get("seed", 1))
                if dec.dither_shape(h) is None:
                    from .decoder import XgpuError
                    raise XgpuError(f"dither: {h} names no dither matrix of this decoder")
                dither_made.append((int(h),) + tuple(dec.dither_shape(h)[:2]))
            h, mw, mh = dither_made[0]
            return h, abi.dither_phase(dec.lib, p["poc"] & 0xFFFFFFFF, mw, mh) if dither_opts.get("temporal") else (0, 0)

        overlay_last = [None, None]      # (picture, what the callable returned for it): one call per picture, and nothing of it in the picture's params

        def overlay_of(p):          # the layers and boxes of picture p as pic_output_overlaid's keyword arguments
            if overlay_last[0] is not p:
                overlay_last[:] = [p, (overlay(p) if callable(overlay) else overlay) or {}]
            return {k: overlay_last[1].get(k) for k in ("layers", "boxes")}

        def decode(p):
            dec, hb = self._dec, p["batch"]
            if p["is_idr"]:
                free.extend(slots.values()); slots.clear()
            cur = free.pop()
            refs = {(i, l): (slots[poc], poc) for l in range(2) for i, poc in enumerate(p["refs"][l])}
            with self._lock:
                dec.decode_picture(cur, p["poc"], refs, hb, deblock=p["deblock_on"], pad=True, qp_u_offset=p["qp_u_offset"], qp_v_offset=p["qp_v_offset"],
                                   alpha_off=p["alpha_off"], beta_off=p["beta_off"], alf=p["alf"])
                if side is not None:           # the SCU map is this picture's until the next frame_begin: before any other output
                    kw = dict(side)
                    if kw.get("kind") == "flow":
                        kw.setdefault("crop", p["crop"] if self.apply_crop else (0, 0, 0, 0))
                    p["side_info"] = dec.frame_side_info(cur, **kw)
                if residual is not None:       # the arena is the batch's: before batch_destroy
                    kw = dict(residual)
                    if kw.get("kind", "yuv420") != "energy":
                        kw.setdefault("crop", p["crop"] if self.apply_crop else (0, 0, 0, 0))
                    p["residual"] = dec.batch_residual(hb, **kw)
                if compare is not None:
                    i = n_decoded[0]
                    ref = compare(p) if callable(compare) else compare[i] if i < len(compare) else None
                    p["compare"] = None
                    if ref is not None:
                        kw = dict(ref) if isinstance(ref, dict) else {"ref": ref}
                        kw.setdefault("crop", p["crop"] if self.apply_crop else (0, 0, 0, 0))
                        p["compare"] = dec.pic_compare(cur, **kw)
                if stats is not None:
                    kw = stats(p) if callable(stats) else stats
                    p["stats"] = None
                    if kw is not None:
                        kw = dict(kw)
                        kw.setdefault("crop", p["crop"] if self.apply_crop else (0, 0, 0, 0))
                        if kw.get("light"):      # True or a dict: on top of the VUI's colour description
                            kw["light"] = self.light_options(p["colour"], kw["light"])
                        elif "light" in kw:
                            kw["light"] = None
                        p["stats"] = dec.pic_stats(cur, **kw)
                n_decoded[0] += 1
                if p["n_dmvr_sub"]:
                    p["_dmvr"][1] = dec.batch_dmvr_mvs(hb)
                    p["_dmvr"][0].set()
                if p["needs_ref_luma"]:
                    p["_luma"][1] = dec.pic_download_padded_luma(cur)
                    p["_luma"][0].set()
                dec.batch_destroy(hb)          # back to the pool; queued kernels keep reading it (same HIP stream)
            if surfaces is not None:
                opts = self.tensor_options(p, {})
                kw = {"chroma_loc": opts["chroma_loc"], "dra": opts["dra"], "crop": p["crop"] if self.apply_crop else (0, 0, 0, 0)}
                kw.update(surface_options or {})
                with self._lock:
                    p["surfaces"] = dec.pic_output_surfaces(cur, surfaces, layout=surface_layout, **kw)
            if packed is not None:
                kw = self.tensor_options(p, packed)
                kw.setdefault("crop", p["crop"] if self.apply_crop else (0, 0, 0, 0))
                if to is not None and kw.get("layout", "rgba") not in ("yuyv", "uyvy"):
                    kw.setdefault("colour", self.colour_transform(p["colour"], to))
                with self._lock:
                    if overlay is not None:
                        p["packed"] = dec.pic_output_overlaid(cur, **overlay_of(p), **kw)
                    elif dither_opts is not None:
                        h, ph = dither_of(dec, p)
                        p["packed"] = dec.pic_output_dithered(cur, h, phase=ph, **kw)
                    else:
                        p["packed"] = dec.pic_output_packed(cur, **kw) if lut is None else dec.pic_output_lut3d(cur, lut_of(dec), **kw)
            planes = None
            if tensor is not None:
                kw = self.tensor_options(p, tensor)
                kw.setdefault("crop", p["crop"] if self.apply_crop else (0, 0, 0, 0))
                if to is not None:
                    kw.setdefault("colour", self.colour_transform(p["colour"], to))
                for k, v in (("size", size), ("mean", mean), ("std", std), ("rois", rois(p) if callable(rois) else rois), ("fit", fit), ("pad", pad)):
                    if v is not None:
                        kw.setdefault(k, v)
                with self._lock:
                    if overlay is not None:
                        planes = dec.pic_output_overlaid(cur, **overlay_of(p), **kw)
                    elif dither_opts is not None:
                        h, ph = dither_of(dec, p)
                        planes = dec.pic_output_dithered(cur, h, phase=ph, **kw)
                    elif lut is not None:
                        planes = dec.pic_output_lut3d(cur, lut_of(dec), **kw)
                    elif resample is not None:
                        planes = dec.pic_output_resampled(cur, **resample, **kw)
                    elif warp is not None:
                        planes = dec.pic_output_warped(cur, warp(p) if callable(warp) else warp, **kw)
                    elif remap is not None:
                        planes = dec.pic_output_remapped(cur, remap(p) if callable(remap) else remap, step=remap_step, **kw)
                    elif kw.get("colour") is not None and kw.get("size") is not None:      # size= and to= meet in a call of their own (host rois included)
                        planes = dec.pic_output_scaled_cm(cur, linear_light=bool(linear_light), **kw)
                    else:
                        planes = dec.pic_output_tensor(cur, **kw)
            elif download and output_bit_depth is not None:
                planes = dec.pic_output(cur, output_bit_depth, p["crop"] if self.apply_crop else (0, 0, 0, 0), dra=p["dra"])
            elif download and p["dra"] is not None:      # the DRA post-filter belongs to the output: planes through the output kernel
                import numpy as np
                w, h = p["width"], p["height"]
                flat = dec.pic_output(cur, max(p["bit_depth"], 9), dra=p["dra"]).view("<u2").astype(np.int16) if p["bit_depth"] > 8 else None
                if flat is None:
                    raise RuntimeError("DRA on 8-bit pictures: use output_bit_depth")
                planes = [flat[:w * h].reshape(h, w), flat[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), flat[w * h * 5 // 4:].reshape(h // 2, w // 2)]
            elif download:
                planes = dec.pic_download(cur)
                if self.verify_md5 and p["md5"] is not None and not self.signature_ok(p, planes):
                    raise RuntimeError(f"picture signature mismatch at POC {p['poc']} (XEVD_ERR_BAD_CRC)")
            for poc in p["release"]:      # unmarked when THIS picture is stored (it may still have referenced them)
                if poc in slots:
                    free.append(slots.pop(poc))
            if p["is_ref"]:
                slots[p["poc"]] = cur
            else:
                free.append(cur)
            return planes

        try:
            while True:
                p = q.get()
                if p is None:
                    break
                if isinstance(p, Exception):
                    raise p
                if not free and not slots:
                    with self._lock:
                        free = [self._dec.pic_alloc() for _ in range(self.N_SLOTS)]
                yield p, decode(p)
            if self._dec is not None and not download:
                self._dec.sync()
        finally:
            # let the parser thread finish (it may be inside a backend call), then release the device
            self._abort = True
            while th.is_alive():
                try:
                    q.get(timeout=0.05)
                except queue.Empty:
                    pass
            if self._dec is not None:
                self._dec.close()
                self._dec = None

    def output_order(self, output_bit_depth=None, tensor=None, to=None, side=None, size=None, mean=None, std=None, rois=None, fit=None, pad=None, residual=None,
                     compare=None, stats=None, warp=None, remap=None, remap_step=0, surfaces=None, surface_layout="nv12", surface_options=None,
                     linear_light=False, resample=None, packed=None, lut=None, dither=None, overlay=None):
        """all pictures in output order (ascending POC inside every IDR period), as xevd_pull's bumping delivers them; with tensor=dict(...) (as
        pictures takes it, `to` too) every picture is converted on the device and copied to the host as it arrives: numpy arrays of the tensors' shape;
        side=dict(...) (as pictures takes it): params["side_info"] of every picture, as a numpy array too; residual=dict(...) (as pictures takes it):
        params["residual"] as numpy - for kind "yuv420" the pair (flat array, (Y, Cb, Cr) views of it); compare= (as pictures takes it, the callable and the
        sequence in DECODING order): params["compare"], its map as a numpy array; stats= (as pictures takes it): params["stats"], its histograms as numpy arrays;
        surfaces= / surface_layout= / surface_options= (as pictures takes them): params["surfaces"], a list of numpy arrays; resample= (as pictures takes it);
        packed=dict(...) (as pictures takes it): params["packed"], a numpy array; lut=, dither= and overlay= (as pictures takes them)"""
        out, epoch = [], -1
        for p, planes in self.pictures(output_bit_depth=output_bit_depth, tensor=tensor, to=to, side=side, size=size, mean=mean, std=std, rois=rois, fit=fit, pad=pad,
                                       residual=residual, compare=compare, stats=stats, warp=warp, remap=remap, remap_step=remap_step, surfaces=surfaces,
                                       surface_layout=surface_layout, surface_options=surface_options, linear_light=linear_light, resample=resample,
                                       packed=packed, lut=lut, dither=dither, overlay=overlay):
            if p["is_idr"]:
                epoch += 1
            if surfaces is not None:      # (synchronises torch's current stream: the tensors are complete)
                p["surfaces"] = [t.cpu().numpy() for t in p["surfaces"]]
            if packed is not None:
                p["packed"] = p["packed"].cpu().numpy()
            if tensor is not None:
                # (synchronises torch's current stream: the slot's tensor is complete); device boxes with results=True: the pair, both as arrays
                planes = tuple(t.cpu().numpy() for t in planes) if isinstance(planes, tuple) else planes.cpu().numpy()
            if side is not None:
                p["side_info"] = p["side_info"].cpu().numpy()
            if residual is not None:
                r = p["residual"]
                if isinstance(r, tuple):      # kind "yuv420": the views again, over the host copy
                    flat = r[0].cpu().numpy()
                    ny, (hc, wc) = r[1][0].numel(), r[1][1].shape
                    r = (flat, (flat[:ny].reshape(r[1][0].shape), flat[ny:ny + hc * wc].reshape(hc, wc), flat[ny + hc * wc:].reshape(hc, wc)))
                else:
                    r = r.cpu().numpy()
                p["residual"] = r
            if compare is not None and p["compare"] is not None and p["compare"]["map"] is not None:
                p["compare"]["map"] = p["compare"]["map"].cpu().numpy()
            if stats is not None and isinstance(p["stats"], dict):
                for k in ("hist", "light_hist"):
                    if p["stats"][k] is not None:
                        p["stats"][k] = p["stats"][k].cpu().numpy()
            p["decode_index"] = len(out)       # place in decoding order
            out.append(((epoch, p["poc"]), p, planes))
        return [(p, planes) for _, p, planes in sorted(out, key=lambda t: t[0])]
