"""BEV rendering: what the library computes, as pictures (include/disconet_hip.h :: dn_render_bev).

    render_bev(config, background / classes, heat, layers, scale)   one launch: every image of a batch -> RGB canvas [N, S H, S W, 3]
    host_render_bev(...)                                            the same call on numpy: the contract, byte for byte
    BoxLayer                                                        a set of boxes with its style; .detections(det), .tracks(det, report),
                                                                    .ground_truth(boxes, count) take the library's own dicts
    attention_sheet(...)                                            one row of panels per ego: the DiscoGraph weights over its scene
    write_png / read_png                                            8-bit RGB with zlib and struct only

Canvas row r is BEV x index r / S and column q is y index q / S -- bev_seq's own layout, no flip.  render_bev runs on
torch's current stream, allocates through torch's caching allocator and never waits for the device, so it can be captured
behind the forward and the tail (graph.GraphedStep); the exceptions are named where they occur (a dense voxel grid as
background, a palette given on the host).
"""
import ctypes
import struct
import zlib

import numpy as np
import torch

from . import _lib
from .ops import SpTensor, _need_gpu, _ptr, _stream, ego_list

MAX_SETS = 4
SCALES = (1, 2, 4)
GROUND = (255, 255, 255)
POINT = (32, 32, 32)
HEAT_COLOUR = (220, 30, 30)
GT_COLOUR = (0, 170, 0)
SCORE_LO = (40, 90, 255)
SCORE_HI = (255, 40, 0)
_BY = {"fixed": 0, "score": 1, "id": 2}
# include/disconet_hip.h :: DN_RENDER_ID_PALETTE (tests/test_render_host_cpu.py compares the two)
ID_PALETTE = np.asarray([
    229, 34, 34, 91, 229, 131, 107, 24, 165, 165, 153, 66, 34, 196, 229, 229, 91, 166, 59, 165, 24, 70, 66, 165,
    229, 99, 34, 91, 229, 178, 154, 24, 165, 144, 165, 66, 34, 131, 229, 229, 91, 120, 24, 165, 36, 103, 66, 165,
    229, 164, 34, 91, 229, 224, 165, 24, 130, 111, 165, 66, 34, 66, 229, 229, 109, 91, 24, 165, 83, 137, 66, 165,
    228, 229, 34, 91, 188, 229, 165, 24, 83, 78, 165, 66, 67, 34, 229, 229, 155, 91, 24, 165, 131, 165, 66, 161],
    dtype=np.uint8).reshape(32, 3)


def _rgb(c, what):
    c = tuple(int(v) for v in c)
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError("%s = %r: three integers in 0..255" % (what, c))
    return c


class BoxLayer:
    """One set of boxes and how it is painted.  boxes [N, K, 6] = (x, y, w, h, sin, cos) in metres (postprocess._corners'
    convention); count [N] (None: all K rows), scores [N, K], ids [N, K] -- device tensors for render_bev, numpy for
    host_render_bev.  by: "fixed" (colour), "score" (colour at 0 -> colour_hi at 1) or "id" (the 32-entry palette, a
    negative id skips the row).  thickness: the outline in canvas pixels (None: the call's scale); fill_alpha 0..255;
    heading: a tick from the centre along local +x."""

    def __init__(self, boxes, count=None, scores=None, ids=None, colour=GT_COLOUR, colour_hi=SCORE_HI, by="fixed",
                 thickness=None, fill_alpha=0, heading=True):
        if by not in _BY:
            raise ValueError("by = %r: one of %s" % (by, sorted(_BY)))
        if by == "score" and scores is None:
            raise ValueError("BoxLayer(by=\"score\") needs scores")
        if by == "id" and ids is None:
            raise ValueError("BoxLayer(by=\"id\") needs ids")
        if len(boxes.shape) != 3 or boxes.shape[2] != 6 or boxes.shape[1] < 1:
            raise ValueError("boxes %s: expected [N, K >= 1, 6]" % (tuple(boxes.shape),))
        n, k = int(boxes.shape[0]), int(boxes.shape[1])
        for name, t, numel in (("count", count, n), ("scores", scores, n * k), ("ids", ids, n * k)):
            if t is not None and int(np.prod(tuple(t.shape))) != numel:
                raise ValueError("%s %s does not go with boxes %s" % (name, tuple(t.shape), tuple(boxes.shape)))
        if thickness is not None and int(thickness) < 1:
            raise ValueError("thickness = %r: at least 1 canvas pixel" % (thickness,))
        if not 0 <= int(fill_alpha) <= 255:
            raise ValueError("fill_alpha = %r: 0..255" % (fill_alpha,))
        self.boxes, self.count, self.scores, self.ids = boxes, count, scores, ids
        self.colour, self.colour_hi = _rgb(colour, "colour"), _rgb(colour_hi, "colour_hi")
        self.by, self.thickness, self.fill_alpha, self.heading = by, thickness, int(fill_alpha), bool(heading)
        self.n, self.k = n, k

    @classmethod
    def detections(cls, det, **style):
        """detect()'s or late_fuse()'s dict (or pad_detections' on the host): coloured by score"""
        style = dict({"by": "score", "colour": SCORE_LO, "colour_hi": SCORE_HI}, **style)
        return cls(det["boxes"], det["count"], det["scores"], **style)

    @classmethod
    def tracks(cls, det, report, **style):
        """the detections that Sort.update(det) matched to a track or started one from, coloured by the track's id
        (report["det_track"]: -1, no track, is not painted)"""
        style = dict({"by": "id"}, **style)
        return cls(det["boxes"], det["count"], det.get("scores"), report["det_track"], **style)

    @classmethod
    def ground_truth(cls, gt_boxes, gt_count=None, **style):
        """padded ground truth (make_box_scene_batch's gt_boxes / gt_count): a green outline"""
        style = dict({"colour": GT_COLOUR}, **style)
        return cls(gt_boxes, gt_count, **style)

    def host(self):
        """the same layer on numpy (one device-to-host copy per tensor)"""
        from .postprocess import _host
        f = lambda t: None if t is None else _host(t)
        return BoxLayer(f(self.boxes), f(self.count), f(self.scores), f(self.ids), self.colour, self.colour_hi, self.by,
                        self.thickness, self.fill_alpha, self.heading)


class _RenderSet(ctypes.Structure):
    """struct dn_render_set"""
    _fields_ = ([(n, ctypes.c_void_p) for n in ("boxes", "count", "scores", "ids")] +
                [(n, ctypes.c_int32) for n in ("k", "thickness", "fill_alpha", "heading", "colour_by")] +
                [("colour", ctypes.c_uint8 * 4), ("colour_hi", ctypes.c_uint8 * 4), ("reserved", ctypes.c_int32)])


class _RenderDesc(ctypes.Structure):
    """struct dn_render_desc"""
    _fields_ = ([(n, ctypes.c_int32) for n in ("n", "h", "w", "scale")] +
                [("x_lo", ctypes.c_double), ("y_lo", ctypes.c_double), ("voxel", ctypes.c_double * 2)] +
                [(n, ctypes.c_void_p) for n in ("background", "palette", "heat")] +
                [(n, ctypes.c_int32) for n in ("bg_kind", "n_classes", "heat_h", "heat_w", "heat_alpha", "n_sets")] +
                [("heat_lo", ctypes.c_double), ("heat_hi", ctypes.c_double)] +
                [(n, ctypes.c_uint8 * 4) for n in ("ground", "point", "heat_colour")] +
                [("reserved", ctypes.c_int32), ("sets", _RenderSet * MAX_SETS)])


def _common_checks(config, scale, heat_range, heat_alpha, layers):
    vs = config.voxel_size
    if float(vs[0]) != float(vs[1]):
        raise ValueError("voxel_size %s: the pixels must be square" % (tuple(vs),))
    if int(scale) not in SCALES:
        raise ValueError("scale = %r: one of %s" % (scale, SCALES))
    lo, hi = float(heat_range[0]), float(heat_range[1])
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise ValueError("heat_range = %r: finite, hi > lo" % (heat_range,))
    if not 0 <= int(heat_alpha) <= 255:
        raise ValueError("heat_alpha = %r: 0..255" % (heat_alpha,))
    layers = tuple(layers)
    if len(layers) > MAX_SETS:
        raise ValueError("%d layers: at most %d" % (len(layers), MAX_SETS))
    for l in layers:
        if not isinstance(l, BoxLayer):
            raise TypeError("layers holds BoxLayer objects, got %s" % type(l).__name__)
    return int(scale), lo, hi, int(heat_alpha), layers


def _shape_of(config, background, classes, heat, layers):
    """(N, H, W) of the call: from the background, else the class map, else the config's map and the first tensor's N"""
    for t in (background, classes):
        if t is not None:
            s = tuple(t.shape)
            if len(s) == 5:                       # dense voxel grid [N, 1, H, W, Z]
                return s[0] * s[1], s[2], s[3]
            if len(s) == 4 and isinstance(t, SpTensor):
                return s[0], s[1], s[2]
            if len(s) != 3:
                raise ValueError("background / classes %s: expected [N, H, W]" % (s,))
            return s
    h, w = int(config.map_dims[0]), int(config.map_dims[1])
    if heat is not None:
        return int(heat.shape[0]), h, w
    if layers:
        return layers[0].n, h, w
    raise ValueError("nothing to draw: no background, class map, heat map or layer gives the number of images")


def _check_against(n, h, w, heat, layers):
    if w % 4:
        raise ValueError("map width %d: must be a multiple of 4" % w)
    if heat is not None:
        s = tuple(heat.shape)
        if len(s) != 3 or s[0] != n or h % s[1] or w % s[2]:
            raise ValueError("heat %s does not divide %d images of %d x %d" % (s, n, h, w))
    for l in layers:
        if l.n != n:
            raise ValueError("a layer of %d images in a call of %d" % (l.n, n))


def occupancy_words(background):
    """The occupancy words [N, H, W] int32 of a background: an SpTensor(bits=True) (ops.scatter_dense_bits), a word
    tensor as it is, or a dense [N, 1, H, W, Z <= 32] voxel grid through ops.scatter_dense_bits -- that form lists the
    occupied voxels with torch.nonzero, which waits for the device: inside a captured step pass the words."""
    from . import ops
    if isinstance(background, SpTensor):
        if not background.bits:
            raise _lib.DnError("render_bev: an SpTensor background must be an occupancy bit grid (ops.scatter_dense_bits)")
        return background.data
    if background.dim() == 5:
        n, h, w, z = background.shape[0] * background.shape[1], background.shape[2], background.shape[3], background.shape[4]
        if z > 32:
            raise ValueError("a voxel grid of %d layers does not fit one occupancy word" % z)
        idx = (background.reshape(n, h, w, z) > 0).nonzero()
        offsets = torch.zeros(n + 1, dtype=torch.int32, device=background.device)
        offsets[1:] = torch.bincount(idx[:, 0], minlength=n).cumsum(0).to(torch.int32)
        return ops.scatter_dense_bits(idx[:, 1:].to(torch.int32).contiguous(), offsets, n, (h, w, z)).data
    if background.dtype != torch.int32:
        raise _lib.DnError("render_bev: occupancy words are int32 [N, H, W] (got %s)" % background.dtype)
    return background.contiguous()


def render_bev(config, background=None, classes=None, palette=None, heat=None, heat_range=(0, 1), heat_alpha=160, layers=(),
               scale=2, out=None, ground=GROUND, point=POINT, heat_colour=HEAT_COLOUR):
    """Every image of a batch -> uint8 device tensor [N, scale H, scale W, 3] (dn_render_bev; host_render_bev states the
    bytes).  background: the scene's occupancy (see occupancy_words); or classes [N, H, W] int32 with palette [C, 3] uint8
    (a device tensor; a host palette is copied, which a captured step cannot do); neither: every pixel is `ground`.  heat:
    float32 [N, h, w] with H % h == 0 and W % w == 0, laid over the background in `heat_colour` at heat_alpha * the value's
    place in heat_range.  layers: up to 4 BoxLayer, painted in order.  out: a canvas to overwrite."""
    S, lo, hi, alpha, layers = _common_checks(config, scale, heat_range, heat_alpha, layers)
    if background is not None and classes is not None:
        raise ValueError("render_bev takes a background or a class map, not both")
    n, h, w = _shape_of(config, background, classes, heat, layers)
    _check_against(n, h, w, heat, layers)
    d = _RenderDesc()
    d.n, d.h, d.w, d.scale = n, h, w, S
    d.x_lo, d.y_lo = float(config.area_extents[0][0]), float(config.area_extents[1][0])
    d.voxel[0], d.voxel[1] = float(config.voxel_size[0]), float(config.voxel_size[1])
    keep = []                                             # what the descriptor points at, alive until the launch is enqueued
    dev = None
    if background is not None:
        words = occupancy_words(background)
        _need_gpu(words)
        keep.append(words)
        d.bg_kind, d.background, dev = 1, words.data_ptr(), words.device
    elif classes is not None:
        if palette is None:
            raise ValueError("a class map needs a palette [C, 3]")
        _need_gpu(classes)
        dev = classes.device
        cmap = classes.to(torch.int32).contiguous()
        pal = palette if isinstance(palette, torch.Tensor) else torch.as_tensor(np.asarray(palette, dtype=np.uint8))
        pal = pal.to(device=dev, dtype=torch.uint8).contiguous()
        if pal.dim() != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
            raise ValueError("palette %s: expected [C >= 1, 3]" % (tuple(pal.shape),))
        keep += [cmap, pal]
        d.bg_kind, d.background, d.palette, d.n_classes = 2, cmap.data_ptr(), pal.data_ptr(), int(pal.shape[0])
    if heat is not None:
        _need_gpu(heat)
        dev = dev or heat.device
        hm = heat.to(torch.float32).contiguous()
        keep.append(hm)
        d.heat, d.heat_h, d.heat_w = hm.data_ptr(), int(hm.shape[1]), int(hm.shape[2])
    d.heat_alpha, d.heat_lo, d.heat_hi = alpha, lo, hi
    for name, c in (("ground", ground), ("point", point), ("heat_colour", heat_colour)):
        getattr(d, name)[:3] = _rgb(c, name)
    d.n_sets = len(layers)
    for i, l in enumerate(layers):
        s = d.sets[i]
        for t in (l.boxes, l.count, l.scores, l.ids):
            if t is not None and not isinstance(t, torch.Tensor):
                raise _lib.DnError("render_bev needs device tensors (got %s); host_render_bev is the numpy form"
                                   % type(t).__name__)
        _need_gpu(l.boxes, l.count, l.scores, l.ids)
        dev = dev or l.boxes.device
        boxes = l.boxes.to(torch.float32).contiguous()
        count = None if l.count is None else l.count.to(torch.int32).contiguous()
        scores = None if l.scores is None else l.scores.to(torch.float32).contiguous()
        ids = None if l.ids is None else l.ids.to(torch.int32).contiguous()
        keep += [boxes, count, scores, ids]
        s.boxes, s.k = boxes.data_ptr(), l.k
        s.count = None if count is None else count.data_ptr()
        s.scores = None if scores is None else scores.data_ptr()
        s.ids = None if ids is None else ids.data_ptr()
        s.thickness = S if l.thickness is None else int(l.thickness)
        s.fill_alpha, s.heading, s.colour_by = l.fill_alpha, int(l.heading), _BY[l.by]
        s.colour[:3], s.colour_hi[:3] = l.colour, l.colour_hi
    if dev is None:
        raise _lib.DnError("render_bev: no device tensor in the call")
    shape = (n, S * h, S * w, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("out must be a contiguous uint8 device tensor %s" % (shape,))
    _lib.check(_lib.load().dn_render_bev(ctypes.byref(d), _ptr(out), _stream()), "dn_render_bev")
    return out


# ---------------------------------------------------------------------------
# the contract on the host: numpy, float64 and integers
# ---------------------------------------------------------------------------
def _blend(below, over, a):
    """BLEND of the contract on int64 arrays [..., 3]"""
    return (below * (255 - a) + over * a + 127) // 255


def _host_words_count(background):
    """min(popcount, 8) per pixel [N, H, W] from occupancy words or a dense voxel grid"""
    b = np.asarray(background.data.cpu().numpy() if isinstance(background, SpTensor) else background)
    if b.ndim == 5:
        occ = b.reshape(b.shape[0] * b.shape[1], b.shape[2], b.shape[3], b.shape[4]) > 0
        if occ.shape[-1] > 32:
            raise ValueError("a voxel grid of %d layers does not fit one occupancy word" % occ.shape[-1])
        return np.minimum(occ.sum(-1), 8).astype(np.int64)
    if b.ndim != 3 or b.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)):
        raise ValueError("occupancy words are int32 / uint32 [N, H, W]")
    bits = np.unpackbits(np.ascontiguousarray(b).view(np.uint8).reshape(b.shape + (4,)), axis=-1)
    return np.minimum(bits.sum(-1), 8).astype(np.int64)


def host_row_constants(row, x_lo, y_lo, voxel, S):
    """(X, Y, c', s', A, B) of a box row in canvas units, float64 in the contract's order; None when the row is skipped"""
    x, y, w, h, s, c = (np.float64(v) for v in row)
    if not all(np.isfinite(v) for v in (x, y, w, h, s, c)):
        return None
    nrm = np.sqrt(s * s + c * c)
    if not nrm > 0 or not w > 0 or not h > 0:
        return None
    S = np.float64(S)
    return (((x - x_lo) / voxel) * S, ((y - y_lo) / voxel) * S, c / nrm, s / nrm, ((w / 2.0) / voxel) * S,
            ((h / 2.0) / voxel) * S)


def host_row_colour(layer, i, j):
    """the colour of row j of image i (three ints); None when the colour rule skips the row (a negative id)"""
    if layer.by == "score":
        z = np.float64(np.asarray(layer.scores).reshape(layer.n, layer.k)[i, j])
        z = (z if z < 1.0 else np.float64(1.0)) if z > 0.0 else np.float64(0.0)
        l = int(np.floor(z * 255.0))
        return tuple((a * (255 - l) + b * l + 127) // 255 for a, b in zip(layer.colour, layer.colour_hi))
    if layer.by == "id":
        ident = int(np.asarray(layer.ids).reshape(layer.n, layer.k)[i, j])
        return None if ident < 0 else tuple(int(v) for v in ID_PALETTE[ident % 32])
    return layer.colour


def host_render_bev(config, background=None, classes=None, palette=None, heat=None, heat_range=(0, 1), heat_alpha=160,
                    layers=(), scale=2, out=None, ground=GROUND, point=POINT, heat_colour=HEAT_COLOUR):
    """render_bev on numpy arrays: the normative statement of dn_render_bev (include/disconet_hip.h), written for its
    bytes.  A row is evaluated on a window of the canvas that holds every pixel it can touch (the bounding circle grown by
    the thickness and a slack), as the kernel's tiles are."""
    S, lo, hi, alpha, layers = _common_checks(config, scale, heat_range, heat_alpha, layers)
    if background is not None and classes is not None:
        raise ValueError("render_bev takes a background or a class map, not both")
    n, h, w = (int(v) for v in _shape_of(config, background, classes, heat, layers))
    _check_against(n, h, w, heat, layers)
    ch, cw = S * h, S * w
    ground_c, point_c = np.asarray(_rgb(ground, "ground"), np.int64), np.asarray(_rgb(point, "point"), np.int64)
    heat_c = np.asarray(_rgb(heat_colour, "heat_colour"), np.int64)
    up = lambda a: np.repeat(np.repeat(a, S, axis=0), S, axis=1)        # [H, W, ...] -> the canvas, nearest
    points = None if background is None else _host_words_count(background)
    pal = lab = None
    if background is None and classes is not None:
        if palette is None:
            raise ValueError("a class map needs a palette [C, 3]")
        pal = np.asarray(palette.cpu().numpy() if isinstance(palette, torch.Tensor) else palette, dtype=np.int64).reshape(-1, 3)
        lab = np.asarray(classes).astype(np.int64)
    hm = None if heat is None else np.asarray(heat, dtype=np.float32)
    x_lo, y_lo = np.float64(config.area_extents[0][0]), np.float64(config.area_extents[1][0])
    voxel = np.float64(config.voxel_size[0])
    sets = []
    for layer in layers:
        sets.append((layer, np.float64(S if layer.thickness is None else int(layer.thickness)),
                     np.asarray(layer.boxes, dtype=np.float32).reshape(layer.n, layer.k, 6),
                     (np.full(n, layer.k) if layer.count is None else
                      np.clip(np.asarray(layer.count).astype(np.int64).reshape(n), 0, layer.k))))
    res = np.empty((n, ch, cw, 3), dtype=np.uint8)
    for i in range(n):                                                   # image by image: int64 canvases are large
        img = np.empty((ch, cw, 3), dtype=np.int64)
        img[:] = ground_c
        if points is not None:
            m = up(points[i])[..., None]
            img = (ground_c * (8 - m) + point_c * m + 4) // 8
        elif lab is not None:
            li = up(lab[i])
            ok = (li >= 0) & (li < len(pal))
            img = np.where(ok[..., None], pal[np.where(ok, li, 0)], ground_c)
        if hm is not None:
            v = np.repeat(np.repeat(hm[i], h // hm.shape[1], axis=0), w // hm.shape[2], axis=1)
            t = (up(v).astype(np.float64) - lo) / (hi - lo)
            nan = np.isnan(t)
            l = np.floor(np.clip(np.where(nan, 0.0, t), 0.0, 1.0) * 255.0).astype(np.int64)
            a = ((alpha * l + 127) // 255)[..., None]
            img = np.where(nan[..., None], img, _blend(img, heat_c, a))
        for layer, t, boxes, count in sets:
            for j in range(int(count[i])):
                k = host_row_constants(boxes[i, j], x_lo, y_lo, voxel, S)
                if k is None:
                    continue
                colour = host_row_colour(layer, i, j)
                if colour is None:
                    continue
                X, Y, c, s, A, B = k
                R = (np.sqrt(A * A + B * B) + t + 2.0) * 1.000001
                r0, r1 = int(np.clip(np.floor(X - R), 0, ch)), int(np.clip(np.ceil(X + R) + 1, 0, ch))
                q0, q1 = int(np.clip(np.floor(Y - R), 0, cw)), int(np.clip(np.ceil(Y + R) + 1, 0, cw))
                if r0 >= r1 or q0 >= q1:
                    continue
                dx = ((np.arange(r0, r1, dtype=np.float64) + 0.5) - X)[:, None]
                dy = ((np.arange(q0, q1, dtype=np.float64) + 0.5) - Y)[None, :]
                u = dx * c + dy * s
                v = dy * c - dx * s
                e = np.maximum(np.abs(u) - A, np.abs(v) - B)
                solid = (-t < e) & (e <= 0)
                if layer.heading:
                    solid |= (0 <= u) & (u <= A) & (np.abs(v) <= t / 2.0)
                win = img[r0:r1, q0:q1]
                col = np.asarray(colour, np.int64)
                if layer.fill_alpha > 0:
                    fill = (e <= 0) & ~solid
                    win[fill] = _blend(win[fill], col, layer.fill_alpha)
                win[solid] = col
        res[i] = img
    if out is not None:
        out[...] = res
        return out
    return res


# ---------------------------------------------------------------------------
# the DiscoGraph contact sheet
# ---------------------------------------------------------------------------
def disco_weights(model, bevs, trans_matrices, num_agent_tensor, batch_size):
    """The per-pixel edge weights of a DiscoNet's fusion for one batch: encode + fuse(want_weights=True) --
    [B, A, A, h * w], entry k of ego i's list (ops.ego_list: own map first) at [b, i, k]; ops.disco_fuse_mlp documents it."""
    from . import ops
    P = model._get_plan()
    trans = trans_matrices.to(device=bevs.device, dtype=torch.float32).contiguous()
    live = ops.live_agent_counts(num_agent_tensor, bevs.device)
    with torch.no_grad():
        enc = model.encode(bevs, P)
        return model.fuse(enc[model.layer], trans, live, batch_size, P, want_weights=True)[1]


def _sheet_panels(weights, b, ego, num_agent, only_v2i):
    shape = tuple(weights.shape)
    if len(shape) != 4:
        raise ValueError("weights %s: expected [B, E, A, h * w] (DiscoNet.fuse(..., want_weights=True))" % (shape,))
    side = int(round(shape[3] ** 0.5))
    if side * side != shape[3]:
        raise ValueError("weights of %d pixels are not a square map" % shape[3])
    return len(ego_list(int(ego), int(num_agent), bool(only_v2i))), side


def attention_sheet(config, background, weights, b, ego, num_agent, batch_size=1, only_v2i=False, ego_first=0, layers=(),
                    scale=2, heat_range=(0, 1), heat_alpha=200, heat_colour=HEAT_COLOUR, render=None):
    """One row of panels for ego `ego` of scene `b`: panel k is the ego's scene with the weight of entry k of its list
    (ops.ego_list(ego, num_agent, only_v2i): own map first) as the heat overlay.  background: the occupancy of every
    image [A * B, H, W] (agent-major) or of the ego's image alone [1, H, W]; weights [B, E, A, h * w] as
    DiscoNet.fuse(..., want_weights=True) returns them for the egos [ego_first, ego_first + E); num_agent: the scene's live
    count, an int.  layers: BoxLayer of ONE image (the ego's).  -> uint8 [scale H, panels * scale W, 3]; the panels are
    joined with torch.cat.  render=host_render_bev gives the host composition from numpy inputs."""
    host = render is not None
    render = render or render_bev
    panels, side = _sheet_panels(weights, b, ego, num_agent, only_v2i)
    if isinstance(background, SpTensor):
        background = background.data
    if background.shape[0] != 1:
        image = int(ego) * int(batch_size) + int(b)
        background = background[image:image + 1]
    out = []
    for k in range(panels):
        heat = weights[b, ego - ego_first, k].reshape(1, side, side)
        out.append(render(config, background=background, heat=heat, heat_range=heat_range, heat_alpha=heat_alpha,
                          heat_colour=heat_colour, layers=layers, scale=scale)[0])
    return np.concatenate(out, axis=1) if host else torch.cat(out, dim=1)


# ---------------------------------------------------------------------------
# PNG, 8-bit RGB, standard library only
# ---------------------------------------------------------------------------
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, image):
    """image [H, W, 3] uint8 (numpy or a tensor; a device tensor is copied to the host) -> an 8-bit RGB PNG, every
    scanline with filter 0"""
    if isinstance(image, torch.Tensor):
        image = image.detach().cpu().numpy()
    image = np.ascontiguousarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
        raise ValueError("write_png takes uint8 [H, W, 3], got %s %s" % (image.dtype, image.shape))
    h, w = image.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
    raw[:, 1:] = image.reshape(h, 3 * w)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                _chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _chunk(b"IEND", b""))


def read_png(path):
    """write_png's inverse: an 8-bit RGB PNG whose scanlines all carry filter 0 -> uint8 [H, W, 3]"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError("%s is not a PNG" % path)
    at, header, body = 8, None, b""
    while at < len(data):
        size, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        chunk = data[at + 8:at + 8 + size]
        if struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] != (zlib.crc32(kind + chunk) & 0xffffffff):
            raise ValueError("%s: bad CRC in chunk %r" % (path, kind))
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", chunk)
        elif kind == b"IDAT":
            body += chunk
        at += 12 + size
    if header is None or header[2:] != (8, 2, 0, 0, 0):
        raise ValueError("%s: read_png reads 8-bit RGB without interlace only (header %r)" % (path, header))
    w, h = header[:2]
    raw = np.frombuffer(zlib.decompress(body), dtype=np.uint8).reshape(h, 1 + 3 * w)
    if raw[:, 0].any():
        raise ValueError("%s: read_png reads filter 0 scanlines only" % path)
    return raw[:, 1:].reshape(h, w, 3).copy()
