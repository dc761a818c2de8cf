"""GPU suite for the overlaid output (xgpu_pic_output_device_overlaid / _packed_overlaid): every layer set in every layout and dtype
against the numpy restatement tests/overlay_ref.py applied to the plain call's output, bit for bit; the properties that need no reference; refusals that launch
nothing; the stream player and the command-line tool.  No tolerance anywhere: every comparison is equality."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_io
import overlay_ref as ov
from xevd_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -101, -104
# (width, height, crop): the dither suite's shapes, for its reasons - the three-channel family at 8 pixels per lane -> 2x2, 18x10, 522x14 (a tail lane, a second row
# of workgroups, a second workgroup in x); the semi-planar family at 16 columns per lane -> 2x2, 34x10, 1034x14
SHAPES_RGB = [(8, 8, (2, 4, 4, 2)), (24, 16, (2, 4, 2, 4)), (528, 16, (2, 4, 2, 0))]
SHAPES_SEMI = [(16, 8, (2, 12, 4, 2)), (40, 16, (2, 4, 2, 4)), (1040, 16, (2, 4, 2, 0))]
PQ_SRGB = dict(src_primaries=9, src_transfer=16, dst_primaries=1, dst_transfer=13, tone_map=True)


def small_planes(w, h, bd, kind, seed=5):
    """random samples over the whole range, or a checker of the rails 0 and 2^B - 1 (luma and the two chroma planes out of phase): every clip is reached"""
    top = (1 << bd) - 1
    if kind == "random":
        rng = np.random.default_rng(seed + w + bd)
        return [rng.integers(0, top + 1, s).astype(np.int16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    return [(((yy + xx) & 1) * top).astype(np.int16), ((((cy >> 1) + cx) & 1) * top).astype(np.int16), (((cy + (cx >> 1) + 1) & 1) * top).astype(np.int16)]


def pictures(shapes):
    """name -> (width, height, bit depth, kind, crop)"""
    return {f"{kind}_{w}x{h}_{bd}b": (w, h, bd, kind, crop) for (w, h, crop), bd, kind in itertools.product(shapes, (8, 10, 12), ("random", "rails"))}


PICS_RGB, PICS_SEMI = pictures(SHAPES_RGB), pictures(SHAPES_SEMI)


def host(t):
    """an integer tensor written by the device as a numpy array of unsigned elements"""
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


# ------------------------------------------------------------------------------------------------ the forms: every supported layout and dtype
def rgb_forms(bd):
    """(name, the overlaid call's keyword arguments, the plain call, the reference on its output): RGB planar / interleaved and RGBA in U8 / U16, 10:10:10:2; the
    conversion's own arguments rotate, the layers do not depend on them"""
    import torch
    top = (1 << bd) - 1
    forms = []
    for n, (cl, u16, bgr) in enumerate(itertools.product((False, True), (False, True), (False, True))):
        kw = dict(layout="rgb", channels_last=cl, bgr=bgr, dtype=torch.int16 if u16 else torch.uint8, matrix=(1, 9, 5)[n % 3], full_range=bool(n & 1), chroma_loc=n % 6,
                  upsample=("linear", "nearest")[(n >> 1) & 1])
        forms.append((f"rgb cl{int(cl)} u16{int(u16)} bgr{int(bgr)}", kw, "tensor",
                      lambda v, layers, boxes, cl=cl, bgr=bgr, m=top if u16 else 255: ov.rgb(v, m, layers, boxes, channels_last=cl, bgr=bgr)))
    for n, (u16, bgr) in enumerate(itertools.product((False, True), (False, True))):
        kw = dict(layout="bgra" if bgr else "rgba", dtype=torch.int16 if u16 else torch.uint8, alpha=0.4, matrix=(9, 1)[n & 1], chroma_loc=(n + 2) % 6,
                  upsample=("nearest", "linear")[n & 1])
        forms.append((f"{kw['layout']} u16{int(u16)}", kw, "packed", lambda v, layers, boxes, bgr=bgr, m=top if u16 else 255: ov.rgba(v, m, layers, boxes, bgr=bgr)))
    for bgr in (False, True):
        kw = dict(layout="bgr10a2" if bgr else "rgb10a2", alpha=1 / 3, full_range=bgr)
        forms.append((kw["layout"], kw, "packed", lambda v, layers, boxes, bgr=bgr: ov.rgb10a2(v, layers, boxes, bgr=bgr)))
    return forms


def cm_forms(bd):
    """one RGB and one RGBA case with a transform: the layers are codes of the destination, blended over the transformed picture"""
    return [("rgb cm", dict(layout="rgb", channels_last=True, matrix=9, chroma_loc=2, colour=PQ_SRGB), "tensor",
             lambda v, layers, boxes: ov.rgb(v, 255, layers, boxes, channels_last=True)),
            ("bgra cm", dict(layout="bgra", matrix=9, chroma_loc=2, colour=PQ_SRGB, alpha=0.5), "packed", lambda v, layers, boxes: ov.rgba(v, 255, layers, boxes, bgr=True))]


def semi_forms(bd):
    """NV12 U8, NV12 U16 at depths 9 / 10 / 12, P016 at depths 8 / 10 / 12 - with the matrices and ranges the layers' colours go through"""
    import torch
    forms = [("nv12", dict(dtype=torch.uint8), 8)]
    forms += [("nv12", dict(dtype=torch.int16, out_bit_depth=d), d) for d in (9, 10, 12) if bd > 8 or d == 10]
    forms += [("p016", dict(out_bit_depth=d), d) for d in (8, 10, 12)]
    out = []
    for n, (layout, kw, d) in enumerate(forms):
        mat, full = (1, 9, 5, 7)[n % 4], bool(n & 1)
        out.append((f"{layout} D{d} m{mat} f{int(full)}", dict(kw, layout=layout, matrix=mat, full_range=full), "tensor",
                    lambda v, layers, boxes, d=d, mat=mat, full=full, lsh=16 - d if layout == "p016" else 0: ov.semiplanar(v, d, layers, boxes, mat, full, lsh)))
    return out


class Picture:
    """a decoder with one uploaded picture, and the plain calls' outputs of it by form"""

    def __init__(self, w, h, bd, kind, crop):
        from xevd_amd.decoder import XgpuDecoder
        self.planes, self.bd, self.crop = small_planes(w, h, bd, kind), bd, crop
        self.w, self.h = w - crop[0] - crop[1], h - crop[2] - crop[3]
        self.dec = XgpuDecoder(w, h, bd, device=0, max_pics=4)
        self.pic = self.dec.pic_alloc()
        self.dec.pic_upload(self.pic, self.planes)
        self.plain = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dec.close()

    def plain_of(self, form):
        name, kw, call, _ = form
        if name not in self.plain:
            fn = self.dec.pic_output_tensor if call == "tensor" else self.dec.pic_output_packed
            self.plain[name] = host(fn(self.pic, crop=self.crop, **kw))
        return self.plain[name]

    def overlaid(self, form, layers, boxes=None, **more):
        return host(self.dec.pic_output_overlaid(self.pic, layers=[api_layer(l) for l in layers], boxes=api_boxes(boxes), crop=self.crop, **form[1], **more))

    def check(self, forms, layers, boxes=None, what=""):
        """the overlaid call of every form against the reference on the plain call's output; -> the outputs"""
        outs = []
        for form in forms:
            got = self.overlaid(form, layers, boxes)
            exp = form[3](self.plain_of(form), layers, ref_boxes(boxes))
            assert got.dtype == exp.dtype and np.array_equal(got, exp), (what, form[0], int((got != exp).sum()), exp.size)
            outs.append(got)
        return outs


def api_layer(l):
    """a layer of the reference as XgpuDecoder.pic_output_overlaid takes it; pad: extra bytes / pixels behind every row of the bitmap (a pitch wider than the row)"""
    import torch
    if l["kind"] == "box":
        return {k: v for k, v in l.items() if k != "kind"}
    px = np.asarray(l["pixels"])
    pad = l.get("pad", 0)
    wide = np.full((px.shape[0], px.shape[1] + pad) + px.shape[2:], 0xEE, np.uint8)
    wide[:, :px.shape[1]] = px
    t = torch.from_numpy(wide).to("cuda:0")[:, :px.shape[1]]
    d = dict(image=t, x=l.get("x", 0), y=l.get("y", 0), opacity=l.get("opacity", 255))
    if l["kind"] == "a8":
        d["colour"] = l.get("colour", (255, 255, 255, 255))
    else:
        d["order"] = l["kind"]
    return d


def api_boxes(b):
    import torch
    if b is None:
        return None
    d = {k: v for k, v in b.items() if k not in ("array", "count", "labels", "tensor")}
    d["tensor"] = b["tensor"] if "tensor" in b else torch.from_numpy(np.ascontiguousarray(b["array"])).to("cuda:0")
    if b.get("count") is not None:
        d["count"] = torch.tensor([b["count"]], dtype=torch.int32, device="cuda:0")
    if b.get("labels") is not None:
        d["labels"] = torch.from_numpy(np.ascontiguousarray(b["labels"], np.int32)).to("cuda:0")
    return d


def ref_boxes(b):
    return None if b is None else {k: v for k, v in b.items() if k != "tensor"}


# ------------------------------------------------------------------------------------------------ the layer sets
def bitmap(rng, w, h, x, y, kind="rgba", rails=False, **kw):
    shape = (h, w) if kind == "a8" else (h, w, 4)
    px = rng.integers(0, 2, shape).astype(np.uint8) * 255 if rails else rng.integers(0, 256, shape).astype(np.uint8)
    return dict(kind=kind, pixels=px, x=x, y=y, **kw)


def layer_sets(w, h):
    """name -> layers, for a w x h image (2 x 2 at the least: what lies outside is legal and does nothing)"""
    rng = np.random.default_rng(17 + w)
    alphas = np.zeros((1, 6, 4), np.uint8)
    alphas[0, :, 3] = (0, 1, 127, 128, 254, 255)
    alphas[0, :, :3] = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255), (0, 0, 0), (255, 0, 255))      # colours on the rails
    sets = {
        "one pixel at an odd position": [bitmap(rng, 1, 1, 1, 1), bitmap(rng, 1, 1, 7, 3, "bgra", opacity=200)],
        "3 x 3 at (odd, odd), 4 x 4 at (3, 3)": [bitmap(rng, 3, 3, 1, 1), bitmap(rng, 4, 4, 3, 3, "a8", colour=(250, 20, 90, 230))],
        "edges that cut a lane's run": [bitmap(rng, 7, 3, 5, 1), bitmap(rng, 6, 2, 13, 2, "a8", colour=(10, 200, 30, 255)), bitmap(rng, 11, 4, 13, 5, "bgra")],
        "across x = 512 / 1024 and row 8": [bitmap(rng, 9, 5, 508, 6), bitmap(rng, 9, 5, 1020, 5, "bgra"), bitmap(rng, 30, 3, 500, 7, "a8", colour=(0, 255, 255, 200)),
                                           bitmap(rng, 40, 2, 1000, 7, "a8", colour=(255, 255, 0, 255))],
        "over the four edges, and outside": [bitmap(rng, 5, 3, -2, 1), bitmap(rng, 5, 3, w - 2, 0, "bgra"), bitmap(rng, 4, 5, 1, -3, "a8"), bitmap(rng, 4, 5, 0, h - 2),
                                             bitmap(rng, 3, 3, w + 3, h + 3), bitmap(rng, 3, 3, -10, -10, "a8"), bitmap(rng, 2, 2, w, 0), bitmap(rng, 2, 2, 0, -2)],
        "larger than the image": [bitmap(rng, w + 6, h + 4, -3, -2, "bgra")],
        "pitches wider than the row": [bitmap(rng, 5, 4, 1, 0, pad=3), bitmap(rng, 7, 3, 3, 1, "a8", pad=5, colour=(1, 2, 3, 254)), bitmap(rng, w, h, 0, 0, "bgra", pad=1, opacity=90)],
        "alphas x opacities": [dict(kind=k, pixels=alphas[..., (2, 1, 0, 3)] if k == "bgra" else alphas, x=1, y=y, opacity=o)
                               for y, (o, k) in enumerate(((0, "rgba"), (1, "bgra"), (128, "rgba"), (255, "bgra")))] +
                              [dict(kind="a8", pixels=alphas[..., 3], x=0, y=1, opacity=o, colour=(255, 0, 255, a)) for o, a in ((128, 255), (255, 127))],
        "colours on the rails": [bitmap(rng, min(w, 40), h, 0, 0, rails=True), bitmap(rng, 9, 3, 2, 1, "a8", rails=True, colour=(255, 255, 255, 255))],
        "sixteen layers": [bitmap(rng, 3 + i % 4, 2 + i % 3, (5 * i) % max(w - 1, 1) - 1, i % max(h - 1, 1), ("rgba", "bgra", "a8")[i % 3], opacity=255 - 13 * i) for i in range(12)] +
                          [dict(kind="box", box=(i, i % 3, 9 + i, 5), thickness=1 + i % 2, colour=(200, 10 * i, 0, 255 - 20 * i), fill=(0, 0, 255, 30 * i)) for i in range(4)],
    }
    return sets


def box_sets(w, h):
    return {
        "thickness 1, no fill": [dict(kind="box", box=(1, 1, 9, 6), thickness=1, colour=(255, 0, 0, 255))],
        "thickness 2, fill": [dict(kind="box", box=(3, 0, 12, 8), thickness=2, colour=(0, 255, 0, 200), fill=(0, 0, 255, 77), opacity=200)],
        "thickness above half the box": [dict(kind="box", box=(2, 1, 7, 5), thickness=4, colour=(9, 99, 199, 255), fill=(255, 255, 255, 255))],
        "partly outside": [dict(kind="box", box=(-4, -3, 11, 9), thickness=1, colour=(255, 255, 255, 255)),
                           dict(kind="box", box=(w - 6, h - 4, 12, 9), thickness=2, colour=(255, 255, 0, 255), fill=(1, 2, 3, 40))],
    }


# ------------------------------------------------------------------------------------------------ 1. every layer set, every form
@pytest.mark.parametrize("name", list(PICS_RGB))
def test_three_channel_layouts_are_the_reference(name):
    with Picture(*PICS_RGB[name]) as p:
        forms = rgb_forms(p.bd)
        for what, layers in {**layer_sets(p.w, p.h), **box_sets(p.w, p.h)}.items():
            p.check(forms, layers, what=what)


@pytest.mark.parametrize("name", list(PICS_SEMI))
def test_surfaces_are_the_reference(name):
    with Picture(*PICS_SEMI[name]) as p:
        forms = semi_forms(p.bd)
        for what, layers in {**layer_sets(p.w, p.h), **box_sets(p.w, p.h)}.items():
            p.check(forms, layers, what=what)


@pytest.mark.parametrize("name", ["random_24x16_10b", "rails_528x16_12b"])
def test_layers_over_a_colour_transform_are_the_reference(name):
    with Picture(*PICS_RGB[name]) as p:
        for what, layers in {**layer_sets(p.w, p.h), **box_sets(p.w, p.h)}.items():
            p.check(cm_forms(p.bd), layers, what=what)
        p.check(cm_forms(p.bd), [], device_boxes(p.w, p.h, "xywh")["overlapping"], what="device boxes")


# ------------------------------------------------------------------------------------------------ 2. order, frames
@pytest.mark.parametrize("name", ["random_24x16_10b", "rails_528x16_8b", "random_40x16_12b", "rails_1040x16_10b"])
def test_order_changes_the_result(name):
    rgbp = name in PICS_RGB
    with Picture(*(PICS_RGB if rgbp else PICS_SEMI)[name]) as p:
        forms = rgb_forms(p.bd) if rgbp else semi_forms(p.bd)
        rng = np.random.default_rng(1)
        a = dict(kind="box", box=(0, 0, 9, 7), thickness=9, colour=(255, 0, 0, 128))
        b = bitmap(rng, 8, 6, 3, 2, "bgra")
        b["pixels"][..., 3] = 160
        c = dict(kind="a8", pixels=np.full((5, 12), 200, np.uint8), x=1, y=3, colour=(0, 255, 64, 255), opacity=180)
        for layers in ([a, b], [a, b, c]):
            fwd = p.check(forms, layers, what="in order")
            rev = p.check(forms, layers[::-1], what="reversed")
            for f, x, y in zip(forms, fwd, rev):
                assert not np.array_equal(x, y), (f[0], len(layers))


@pytest.mark.parametrize("name", ["random_24x16_8b", "random_40x16_10b"])
def test_a_box_over_the_edge_draws_no_line_along_it(name):
    rgbp = name in PICS_RGB
    with Picture(*(PICS_RGB if rgbp else PICS_SEMI)[name]) as p:
        form = (rgb_forms(p.bd) if rgbp else semi_forms(p.bd))[0]      # planar RGB u8 / NV12 u8: plane 0 is R / luma
        plain = p.plain_of(form)
        box = dict(kind="box", box=(-5, 2, 11, 6), thickness=1, colour=(255, 255, 255, 255))
        got = p.check([form], [box])[0]
        luma = (lambda t: t[0]) if rgbp else (lambda t: t[:p.h])
        g, v = luma(got), luma(plain)
        assert np.array_equal(g[3:7, 0], v[3:7, 0]) and np.array_equal(g[3:7, :5], v[3:7, :5])      # no line down column 0: the left side lies at x = -5
        assert np.all(g[2, :6] >= 235) and np.all(g[7, :6] >= 235) and np.all(g[2:8, 5] >= 235)      # top, bottom and right side are there
        assert np.array_equal(g[:2], v[:2]) and np.array_equal(g[8:], v[8:])


# ------------------------------------------------------------------------------------------------ 3. device boxes
def device_boxes(w, h, fmt, n=8):
    """name -> boxes dict: the live count in every regime, labels of either sign and beyond the palette, NaN and empty boxes among live ones, overlapping boxes"""
    rng = np.random.default_rng(23 + w)
    x = rng.integers(-4, max(w - 2, 1), n); y = rng.integers(-3, max(h - 2, 1), n)
    bw = rng.integers(1, 14, n); bh = rng.integers(1, 9, n)
    if fmt == "xywh":
        arr = np.stack([x, y, bw, bh], axis=1).astype(np.int32)
        arr[2] = (3, 3, 0, 5); arr[5] = (4, 1, 6, -2)      # empty among live ones
    else:
        fr = rng.random((n, 4)).astype(np.float32)
        arr = (np.stack([x, y, x + bw, y + bh], axis=1) + fr).astype(np.float32)
        arr[2] = (np.nan, 1, 5, 5); arr[5] = (6, 2, 6, 8); arr[6, 2] = np.inf      # NaN, empty, and +inf (clamped: a box to the right edge and beyond)
    pal = [(255, 0, 0, 255), (0, 255, 0, 200), (0, 0, 255, 128), (255, 255, 255, 255), (0, 0, 0, 255)]
    labels = np.array([-1, 0, 4, 5, 7, -6, 2, 1][:n], np.int32)
    base = dict(array=arr, palette=pal, thickness=1, fill_alpha=60)
    sets = {f"count {c}": dict(base, count=c, labels=labels) for c in (0, 1, n, n + 3, -2)}
    sets["no count, no labels"] = dict(base, thickness=2, fill_alpha=0)
    sets["one palette entry"] = dict(base, labels=labels, palette=pal[:1], thickness=3)
    ov_arr = np.array([[1, 1, 12, 8], [4, 3, 12, 8], [0, 0, w, h], [6, 0, 3, h + 5]], np.int32)
    sets["overlapping"] = dict(array=ov_arr if fmt == "xywh" else np.stack([ov_arr[:, 0], ov_arr[:, 1], ov_arr[:, 0] + ov_arr[:, 2], ov_arr[:, 1] + ov_arr[:, 3]], axis=1).astype(np.float32) - np.float32(0.25),
                               palette=pal, labels=np.arange(4, dtype=np.int32), thickness=2, fill_alpha=100, count=4)
    return sets


@pytest.mark.parametrize("fmt", ["xywh", "xyxy"])
@pytest.mark.parametrize("name", ["random_8x8_8b", "rails_24x16_10b", "random_528x16_12b", "random_16x8_10b", "rails_40x16_12b", "random_1040x16_8b"])
def test_device_boxes_are_the_reference(name, fmt):
    rgbp = name in PICS_RGB
    with Picture(*(PICS_RGB if rgbp else PICS_SEMI)[name]) as p:
        forms = rgb_forms(p.bd) if rgbp else semi_forms(p.bd)
        logo = [bitmap(np.random.default_rng(2), 6, 4, 2, 1)]      # the host layers come after the boxes
        for what, boxes in device_boxes(p.w, p.h, fmt).items():
            p.check(forms, logo if "count 1" in what else [], boxes, what=what)


@pytest.mark.parametrize("name", ["random_528x16_10b", "rails_1040x16_10b"])
def test_256_device_boxes(name):
    rgbp = name in PICS_RGB
    with Picture(*(PICS_RGB if rgbp else PICS_SEMI)[name]) as p:
        forms = rgb_forms(p.bd) if rgbp else semi_forms(p.bd)
        rng = np.random.default_rng(5)
        arr = np.stack([rng.integers(-8, p.w, 256), rng.integers(-4, p.h, 256), rng.integers(1, 40, 256), rng.integers(1, 12, 256)], axis=1).astype(np.int32)
        pal = [tuple(int(v) for v in rng.integers(0, 256, 4)) for _ in range(16)]
        for count in (300,):      # (above the capacity: all 256 are live)
            p.check(forms, [], dict(array=arr, count=count, labels=rng.integers(-40, 40, 256).astype(np.int32), palette=pal, thickness=1, fill_alpha=90), what=f"256 boxes, count {count}")


def test_boxes_written_on_the_stream_just_before_the_call():
    """a torch op makes the boxes, the count and the labels on the current stream and the call follows with no synchronise in between"""
    import torch
    with Picture(*PICS_RGB["random_528x16_10b"]) as p:
        form = rgb_forms(p.bd)[2]
        plain = p.plain_of(form)
        seed = torch.arange(64 * 4, dtype=torch.int32, device="cuda:0").reshape(64, 4)
        big = torch.ones((2048, 2048), device="cuda:0")
        for k in range(3):
            _ = big @ big                                                # the stream is busy when the boxes are queued
            t = torch.stack([(seed[:, 0] * (7 + k)) % p.w - 3, (seed[:, 1] * 3) % p.h - 2, seed[:, 2] % 17 + 1, seed[:, 3] % 6 + 1], dim=1).contiguous()
            cnt = (t[:, 0] > 100).sum().to(torch.int32).reshape(1)
            lab = (t[:, 2] - 9).contiguous()
            boxes = dict(tensor=t, count=cnt, labels=lab, palette=[(255, 0, 0, 255), (0, 255, 0, 128)], thickness=1, fill_alpha=50)
            got = host(p.dec.pic_output_overlaid(p.pic, boxes=boxes, crop=p.crop, **form[1]))
            ref = dict(array=t.cpu().numpy(), count=int(cnt.item()), labels=lab.cpu().numpy(), palette=boxes["palette"], thickness=1, fill_alpha=50)
            assert np.array_equal(got, form[3](plain, [], ref)), k
            assert not np.array_equal(got, plain)


# ------------------------------------------------------------------------------------------------ 4. properties
@pytest.mark.parametrize("name", ["random_24x16_10b", "rails_528x16_12b", "random_40x16_12b", "rails_1040x16_8b"])
def test_nothing_to_blend_is_the_plain_call_padding_included(name):
    """zero layers, and layers whose every alpha or opacity is 0, give the plain call's bytes - the whole destination, pitch padding included"""
    import torch
    rgbp = name in PICS_RGB
    with Picture(*(PICS_RGB if rgbp else PICS_SEMI)[name]) as p:
        rng = np.random.default_rng(4)
        clear = bitmap(rng, p.w + 2, p.h + 2, -1, -1)
        clear["pixels"][..., 3] = 0
        nothing = {"zero layers": [], "alpha 0": [clear, dict(kind="a8", pixels=np.zeros((4, 9), np.uint8), x=1, y=1)],
                   "opacity 0": [bitmap(rng, 9, 5, 1, 1, opacity=0), dict(kind="box", box=(0, 0, p.w, p.h), thickness=2, colour=(255, 255, 255, 255), fill=(9, 9, 9, 255), opacity=0)],
                   "colour alpha 0": [dict(kind="a8", pixels=np.full((4, 9), 255, np.uint8), x=1, y=1, colour=(255, 255, 255, 0)),
                                      dict(kind="box", box=(1, 1, 8, 8), thickness=1, colour=(255, 0, 0, 0))]}
        empty_boxes = dict(array=np.array([[1, 1, 5, 5]], np.int32), count=0)
        for form in (rgb_forms(p.bd) if rgbp else semi_forms(p.bd)):
            tight = p.plain_of(form)
            plain_fn = p.dec.pic_output_tensor if form[2] == "tensor" else p.dec.pic_output_packed
            for what, layers in nothing.items():
                assert np.array_equal(p.overlaid(form, layers), tight), (form[0], what)
            assert np.array_equal(p.overlaid(form, [], empty_boxes), tight), form[0]
            if form[1].get("layout") == "rgb" and not form[1].get("channels_last"):
                continue
            # views into wider tensors: pitches and offsets that allow vector stores and that do not; the padding stays
            hh, ww = tight.shape[:2]
            for pad, off in (((-ww) % 16 + 16, 16), (3, 1)):
                bigs = [torch.full((hh, ww + pad) + tight.shape[2:], 7, dtype=plain_fn(p.pic, crop=p.crop, **form[1]).dtype, device="cuda:0") for _ in range(2)]
                views = [b[:, off:off + ww] for b in bigs]
                plain_fn(p.pic, crop=p.crop, out=views[0], **form[1])
                p.dec.pic_output_overlaid(p.pic, layers=[api_layer(l) for l in nothing["opacity 0"]], crop=p.crop, out=views[1], **form[1])
                assert torch.equal(bigs[0], bigs[1]), (form[0], pad, off)
                # ... and real layers land in the same place, the padding untouched
                layers = layer_sets(p.w, p.h)["over the four edges, and outside"]
                p.dec.pic_output_overlaid(p.pic, layers=[api_layer(l) for l in layers], crop=p.crop, out=views[1], **form[1])
                assert np.array_equal(host(views[1]), form[3](tight, layers, None)), (form[0], pad, off)
                assert bool((torch.cat([bigs[1][:, :off].flatten(), bigs[1][:, off + ww:].flatten()]) == 7).all()), (form[0], pad, off)


@pytest.mark.parametrize("name", ["random_24x16_12b", "random_40x16_10b"])
def test_an_opaque_cover_is_the_colour_everywhere(name):
    rgbp = name in PICS_RGB
    with Picture(*(PICS_RGB if rgbp else PICS_SEMI)[name]) as p:
        for col in ((255, 255, 255), (0, 0, 0), (200, 30, 90), (1, 254, 127)):
            cover = [dict(kind="box", box=(-2, -2, p.w + 4, p.h + 4), thickness=1, colour=(0, 0, 0, 255), fill=col + (255,))]
            px = np.empty((p.h, p.w, 4), np.uint8)
            px[...] = col + (255,)
            for layers in (cover, [dict(kind="rgba", pixels=px, x=0, y=0)]):
                if rgbp:
                    for form in rgb_forms(p.bd):
                        got = p.overlaid(form, layers)
                        kw = form[1]
                        if kw["layout"] == "rgb":
                            m = 255 if got.dtype == np.uint8 else (1 << p.bd) - 1
                            chans = got if kw["channels_last"] else got.transpose(1, 2, 0)
                            want = [(c * m + 127) // 255 for c in (col[::-1] if kw["bgr"] else col)]
                            assert np.all(chans == np.array(want)), (form[0], col)
                        elif kw["layout"] in ("rgba", "bgra"):
                            m = 255 if got.dtype == np.uint8 else (1 << p.bd) - 1
                            want = [(c * m + 127) // 255 for c in (col[::-1] if kw["layout"] == "bgra" else col)] + [int(np.floor(0.4 * m + 0.5))]
                            assert np.all(got == np.array(want)), (form[0], col)
                        else:
                            c3 = [(c * 1023 + 127) // 255 for c in (col[::-1] if kw["layout"] == "bgr10a2" else col)]
                            assert np.all(got == (c3[0] | c3[1] << 10 | c3[2] << 20 | 1 << 30)), (form[0], col)
                else:
                    for form in semi_forms(p.bd):
                        got = p.overlaid(form, layers).astype(np.int64)
                        kw = form[1]
                        d = 8 if got.dtype == np.uint8 and kw["layout"] == "nv12" else kw.get("out_bit_depth", 8)
                        lsh = 16 - d if kw["layout"] == "p016" else 0
                        ycc = ov.to_ycc(np.array(col), kw["matrix"], kw["full_range"], d)
                        assert np.all(got[:p.h] == ycc[0] << lsh) and np.all(got[p.h:, 0::2] == ycc[1] << lsh) and np.all(got[p.h:, 1::2] == ycc[2] << lsh), (form[0], col)


@pytest.mark.parametrize("name", ["random_40x16_10b", "rails_1040x16_12b"])
def test_nv12_luma_is_p016_luma_shifted(name):
    import torch
    with Picture(*PICS_SEMI[name]) as p:
        layers = [api_layer(l) for l in layer_sets(p.w, p.h)["sixteen layers"]]
        for d in (10, 12):
            kw = dict(layers=layers, crop=p.crop, matrix=9, out_bit_depth=d)
            nv = host(p.dec.pic_output_overlaid(p.pic, layout="nv12", dtype=torch.int16, **kw))
            p16 = host(p.dec.pic_output_overlaid(p.pic, layout="p016", **kw))
            assert np.array_equal(nv, p16 >> (16 - d)) and not np.any(p16 & ((1 << (16 - d)) - 1)), d


# ------------------------------------------------------------------------------------------------ 5. refusals, streams
def test_refused_calls_launch_nothing():
    import torch
    from xevd_amd.decoder import XgpuDecoder
    w, h, bd = 24, 16, 10
    dec = XgpuDecoder(w, h, bd, device=0, max_pics=4)
    pic = dec.pic_alloc()
    dec.pic_upload(pic, small_planes(w, h, bd, "random"))
    lib = dec.lib
    try:
        stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rgb = abi.make_output_format(abi.OUT_RGB_INTERLEAVED, abi.OUT_U8)
        nv12 = abi.make_output_format(abi.OUT_NV12, abi.OUT_U8, out_bit_depth=8)
        rgba = abi.make_packed_format(abi.PACKED_RGBA, abi.OUT_U8)
        need = lib.xgpu_output_packed_size(C.byref(rgba), w, h, bd)
        t = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        img = torch.full((4, 4, 4), 255, dtype=torch.uint8, device="cuda:0")
        torch.cuda.empty_cache()
        own = torch.empty(20 << 20, dtype=torch.uint8, device="cuda:0")      # with nothing cached, an allocation of its own: its last byte ends the range
        bx = torch.zeros((4, 4), dtype=torch.int32, device="cuda:0")
        hostbuf = np.zeros(max(need, 64), np.uint8)
        cm = abi.make_colour_transform(**PQ_SRGB)
        L = abi.make_overlay_layer
        ok = L(abi.OVL_RGBA8, 1, 1, 4, 4, d_pixels=img.data_ptr())
        B = abi.make_overlay_boxes
        calls = [(rgb, None, [ok], None, t.data_ptr(), 3 * w * h - 1, INVALID),                              # one byte short
                 (rgb, None, [ok], None, hostbuf.ctypes.data, need, INVALID),                                # host memory
                 (abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_U16), None, [ok], None, t.data_ptr() + 1, need, INVALID),
                 (abi.make_output_format(abi.OUT_RGB_PLANAR, matrix=2), None, [ok], None, t.data_ptr(), need, UNSUPPORTED),      # the plain call's refusal and code
                 (abi.make_output_format(abi.OUT_RGB_PLANAR, abi.OUT_F16), None, [ok], None, t.data_ptr(), need, UNSUPPORTED),   # a float dtype
                 (abi.make_output_format(abi.OUT_YUV444_PLANAR, abi.OUT_U8), None, [ok], None, t.data_ptr(), need, INVALID),     # a layout outside the list
                 (abi.make_output_format(abi.OUT_YUV420P, abi.OUT_U8, out_bit_depth=8), None, [ok], None, t.data_ptr(), need, INVALID),
                 (nv12, cm, [ok], None, t.data_ptr(), need, INVALID),                                        # a transform on a video surface
                 (rgb, abi.make_colour_transform(**dict(PQ_SRGB, src_transfer=17)), [ok], None, t.data_ptr(), need, UNSUPPORTED),
                 (rgb, None, [ok] * 17, None, t.data_ptr(), need, INVALID),                                  # the layers
                 (rgb, None, [L(5, 1, 1, 4, 4, d_pixels=img.data_ptr())], None, t.data_ptr(), need, INVALID),
                 (nv12, None, [L(abi.OVL_RGBA8, 1, 1, 4, 4, opacity=256, d_pixels=img.data_ptr())], None, t.data_ptr(), need, INVALID),
                 (rgba, None, [L(abi.OVL_BOX, 1, 1, 4, 4, thickness=0)], None, t.data_ptr(), need, INVALID),
                 (rgb, None, [L(abi.OVL_RGBA8, 1, 1, 4, 4)], None, t.data_ptr(), need, INVALID),                                  # no pixels
                 (rgb, None, [L(abi.OVL_RGBA8, 1, 1, 2, 2, d_pixels=img.data_ptr() + 2)], None, t.data_ptr(), need, INVALID),     # misaligned
                 (rgb, None, [L(abi.OVL_RGBA8, 1, 1, 4, 4, d_pixels=img.data_ptr(), pitch=12)], None, t.data_ptr(), need, INVALID),      # a pitch below the row
                 (rgb, None, [L(abi.OVL_A8, 1, 1, 16, 4, d_pixels=hostbuf.ctypes.data)], None, t.data_ptr(), need, INVALID),      # a bitmap in host memory
                 (rgba, None, [L(abi.OVL_RGBA8, 1, 1, 4, 4, d_pixels=own.data_ptr() + own.numel() - 32)], None, t.data_ptr(), need, INVALID),   # 64 bytes from 32 before the end
                 (nv12, None, [L(abi.OVL_A8, 1, 1, 4, 3, d_pixels=own.data_ptr() + own.numel() - 99, pitch=48)], None, t.data_ptr(), need, INVALID),      # 2 * 48 + 4 = 100 from 99 before the end
                 (rgb, None, [ok], B(abi.BOX_XYWH_I32, bx.data_ptr(), 257), t.data_ptr(), need, INVALID),    # the boxes
                 (rgb, None, [ok], B(abi.BOX_XYWH_I32, bx.data_ptr(), 4, n_palette=0), t.data_ptr(), need, INVALID),
                 (rgb, None, [ok], B(2, bx.data_ptr(), 4), t.data_ptr(), need, INVALID),
                 (rgb, None, [ok], B(abi.BOX_XYXY_F32, hostbuf.ctypes.data, 4), t.data_ptr(), need, INVALID),
                 (rgba, None, [ok], B(abi.BOX_XYXY_F32, bx.data_ptr(), 4, d_count=hostbuf.ctypes.data), t.data_ptr(), need, INVALID)]
        for f, c, layers, boxes, p, n, code in calls:
            fn = lib.xgpu_pic_output_device_overlaid if isinstance(f, abi.OutputFormat) else lib.xgpu_pic_output_device_packed_overlaid
            arr = (abi.OverlayLayer * len(layers))(*layers)
            rc = fn(dec.ctx, pic, None, C.byref(f), None if c is None else C.byref(c), arr, len(layers), None if boxes is None else C.byref(boxes), C.c_void_p(p), n, stream_h)
            assert rc == code, (f.layout, f.dtype, len(layers), layers[0].kind, p, n, rc)
            assert b"overlaid" in lib.xgpu_last_error(dec.ctx)
        assert lib.xgpu_pic_output_device_overlaid(dec.ctx, pic, None, C.byref(rgb), None, None, 1, None, C.c_void_p(t.data_ptr()), need, stream_h) == INVALID
        torch.cuda.synchronize()
        dec.sync()
        assert (t.cpu().numpy() == 0x5A).all() and not hostbuf.any()
        # the bitmap whose last byte is the allocation's last byte is accepted, and the call writes exactly `need` bytes
        last = L(abi.OVL_A8, 1, 1, 4, 3, d_pixels=own.data_ptr() + own.numel() - 100, pitch=48)
        arr = (abi.OverlayLayer * 2)(ok, last)
        own[-100:] = 255
        assert lib.xgpu_pic_output_device_packed_overlaid(dec.ctx, pic, None, C.byref(rgba), None, arr, 2, None, C.c_void_p(t.data_ptr()), need, stream_h) == 0
        torch.cuda.synchronize()
        assert (t[need:].cpu().numpy() == 0x5A).all() and (t[3:need:4].cpu().numpy() == 255).all()
        assert (t[:need].reshape(h, w, 4)[1:5, 1:5, :3].cpu().numpy() == 255).all()
        # the Python layer's own argument checks
        good = dict(image=img, x=0, y=0)
        for kw in (dict(layout="yuv444"), dict(layout="yuyv"), dict(layout="rgb", dtype=torch.float16), dict(layout="rgba", dtype=torch.float32),
                   dict(layout="nv12", colour=PQ_SRGB), dict(layout="rgb", matrix=2), dict(layout="nv12", matrix=2), dict(layers=[good] * 17), dict(layers=[dict(image=img, box=(0, 0, 1, 1))]),
                   dict(layers=[dict(image=img.cpu())]), dict(layers=[dict(image=img.to(torch.int16))]), dict(layers=[dict(image=img[:, :, :3])]), dict(layers=[dict(good, order="argb")]),
                   dict(layers=[dict(good, opacity=300)]), dict(layers=[dict(box=(0, 0, 0, 4))]), dict(layers=[dict(box=(0, 0, 4, 4), thickness=0)]), dict(layers=[dict(good, blend="add")]),
                   dict(boxes=dict(tensor=bx.to(torch.int64))), dict(boxes=dict(tensor=bx, labels=bx[:2, 0].contiguous())), dict(boxes=dict(tensor=bx, palette=[])),
                   dict(boxes=dict(tensor=torch.zeros((257, 4), dtype=torch.int32, device="cuda:0")))):
            with pytest.raises(ValueError):
                dec.pic_output_overlaid(pic, **kw)
    finally:
        dec.close()


def test_twice_on_one_decoder_and_on_a_callers_stream():
    import torch
    with Picture(*PICS_RGB["random_528x16_10b"]) as p:
        forms = [rgb_forms(p.bd)[0], rgb_forms(p.bd)[9]]
        sets = layer_sets(p.w, p.h)
        boxes = device_boxes(p.w, p.h, "xyxy")["count 8"]
        first = p.check(forms, sets["sixteen layers"], boxes)
        other = p.check(forms, sets["larger than the image"])
        again = p.check(forms, sets["sixteen layers"], boxes)
        assert all(np.array_equal(a, b) for a, b in zip(first, again)) and not any(np.array_equal(a, b) for a, b in zip(first, other))
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            on_stream = p.check(forms, sets["sixteen layers"], boxes, what="on a stream of the caller's")
        assert all(np.array_equal(a, b) for a, b in zip(first, on_stream))


# ------------------------------------------------------------------------------------------------ 6. stream and tool
def test_stream_decoder_overlays_what_the_callable_returns():
    import torch
    from xevd_amd.decoder import XgpuDecoder, XgpuError
    from xevd_amd.player import StreamDecoder
    d = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))
    data = d["bytes"].tobytes()
    rng = np.random.default_rng(8)
    logo = bitmap(rng, 20, 10, 0, 0)

    def layers_of(poc):
        return [dict(logo, x=3 + 2 * poc, y=1 + poc, opacity=255 - 10 * poc), dict(kind="box", box=(poc, 2, 30, 20), thickness=2, colour=(255, 255, 0, 255), fill=(0, 0, 0, 64))]

    calls = []

    def overlay(p):
        calls.append(p["poc"])
        return dict(layers=[api_layer(l) for l in layers_of(p["poc"])])

    seen = [(p, t, p["packed"]) for p, t in StreamDecoder(data).pictures(tensor=dict(layout="nv12"), packed=dict(layout="rgb10a2"), overlay=overlay)]
    assert len(seen) == int(d["n"]) and len(calls) == len(seen)
    fixed = [t for _, t in StreamDecoder(data).pictures(tensor=dict(layout="rgb"), overlay=dict(layers=[api_layer(logo)]))]
    for k, (p, t, t10) in enumerate(seen):
        planes = [d[f"p{k}_{c}"] for c in range(3)]
        h, w = planes[0].shape
        dec = XgpuDecoder(w, h, 10, device=0, max_pics=4)
        try:
            pic = dec.pic_alloc()
            dec.pic_upload(pic, planes)
            kw = StreamDecoder.tensor_options(p, {})
            ls = layers_of(p["poc"])
            assert np.array_equal(host(t), ov.semiplanar(host(dec.pic_output_tensor(pic, layout="nv12", **kw)), 8, ls, None, kw["matrix"], kw["full_range"])), k
            assert np.array_equal(host(t10), ov.rgb10a2(host(dec.pic_output_packed(pic, "rgb10a2", **kw)), ls)), k
            assert np.array_equal(host(fixed[k]), ov.rgb(host(dec.pic_output_tensor(pic, layout="rgb", **kw)), 255, [logo])), k
        finally:
            dec.close()
    # an option without an overlaid form: before decoding starts
    for kw in (dict(tensor=dict(layout="rgb"), size=(32, 32)), dict(tensor=dict(layout="yuv444")), dict(tensor=dict(layout="rgb", dtype=torch.float16)),
               dict(packed=dict(layout="yuyv")), dict(tensor=dict(layout="rgb"), lut=0), dict(), dict(tensor=dict(layout="nv12"), to="srgb"),
               dict(tensor=dict(layout="rgb"), dither="bayer"), dict(tensor=dict(layout="rgb"), surfaces=[(32, 32)])):
        with pytest.raises(XgpuError):
            next(StreamDecoder(data).pictures(overlay=dict(layers=[]), **kw))
    with pytest.raises(XgpuError):
        next(StreamDecoder(data).pictures(tensor={}, overlay=dict(layer=[])))


def test_app_overlays_a_logo(tmp_path):
    """tools/xevd_gpu_app.py --overlay on NV12 and on the RGB tensor path against its own NV12 and RGBA runs without the option, overlaid in numpy frame by frame"""
    d = np.load(os.path.join(golden_io.GOLDEN, "stream_ippp_10b_offsets.npz"))
    h, w = d["p0_0"].shape
    n = int(d["n"])
    rng = np.random.default_rng(9)
    logo, badge = bitmap(rng, 24, 12, 5, 3, opacity=200), bitmap(rng, 9, 9, -4, h - 5)
    src = tmp_path / "s.evc"
    src.write_bytes(d["bytes"].tobytes())
    np.save(tmp_path / "logo.npy", logo["pixels"])
    np.save(tmp_path / "badge.npy", badge["pixels"])
    opt = ["--overlay", f"{tmp_path / 'logo.npy'}:5:3:200", "--overlay", f"{tmp_path / 'badge.npy'}:-4:{h - 5}"]
    app = os.path.join(ROOT, "tools", "xevd_gpu_app.py")
    outs = {}
    for name, args in (("nv12", ["--pix-fmt", "nv12"]), ("nv12_ovl", ["--pix-fmt", "nv12"] + opt), ("rgba", ["--pix-fmt", "rgba"]), ("rgb_ovl", opt)):
        out = tmp_path / f"{name}.bin"
        r = subprocess.run([sys.executable, app, "-i", str(src), "-o", str(out)] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-2000:])
        outs[name] = np.fromfile(out, np.uint8)
    nv, nvo = outs["nv12"].reshape(n, h * 3 // 2, w), outs["nv12_ovl"].reshape(n, h * 3 // 2, w)
    rgba, rgbo = outs["rgba"].reshape(n, h, w, 4), outs["rgb_ovl"].reshape(n, h, w, 3)      # (RGBA's three colour elements are the RGB tensor's, bit for bit)
    for k in range(n):
        assert np.array_equal(nvo[k], ov.semiplanar(nv[k], 8, [logo, badge])), k
        assert np.array_equal(rgbo[k], ov.rgb(rgba[k][..., :3], 255, [logo, badge], channels_last=True)), k
    assert not np.array_equal(nv, nvo)
