"""What the reference's CoDetModule.predict_all does after the forward
(upstream:coperception/utils/CoDetModule.py, postprocess.py; SURVEY.md §8(f)
next #3): softmax + box decode for every anchor (one HIP kernel), candidate
selection, then rotated NMS on the host -- the reference runs NMS on the CPU too,
so this is its placement, not a fallback (predict_all / host_detections).
detect() runs the same tail on the GPU (dn_detect: top-k, rotated NMS, padded rows)
for graph-captured inference; host_detections is the reference it is tested against.
late_fuse() (dn_late_fuse) merges every agent's detections in each ego's frame behind detect() (`--com late`);
host_late_fuse is its contract in numpy.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .ops import _need_gpu, _ptr, _stream, ego_list


def make_anchors(config, map_hw=None, device="cuda"):
    """[H, W, A, 6] = (x, y, w, h, sin, cos): one anchor set per BEV cell centre."""
    h = w = map_hw or config.map_dims[0]
    vs = config.voxel_size
    xs = config.area_extents[0][0] + (torch.arange(h, dtype=torch.float64) + 0.5) * vs[0]
    ys = config.area_extents[1][0] + (torch.arange(w, dtype=torch.float64) + 0.5) * vs[1]
    a = torch.as_tensor(np.asarray(config.anchor_size), dtype=torch.float64)
    out = torch.zeros((h, w, a.shape[0], 6), dtype=torch.float64)
    out[..., 0] = xs[:, None, None]
    out[..., 1] = ys[None, :, None]
    out[..., 2] = a[None, None, :, 0]
    out[..., 3] = a[None, None, :, 1]
    out[..., 4] = torch.sin(a[None, None, :, 2])
    out[..., 5] = torch.cos(a[None, None, :, 2])
    return out.to(torch.float32).to(device)


def decode(result, anchors):
    """result = {"cls": [N, H*W*A, 2], "loc": [N, H, W, A, 1, 6]} from DiscoNet.forward ->
    (scores [N, H*W*A], boxes [N, H*W*A, 6]) on the GPU."""
    cls, loc = result["cls"], result["loc"]
    _need_gpu(cls, loc, anchors)
    n, apl = cls.shape[0], cls.shape[1]
    cls = cls.contiguous()
    loc = loc.reshape(n, apl, 6).contiguous()
    anchors = anchors.reshape(apl, 6).contiguous()
    scores = torch.empty((n, apl), dtype=torch.float32, device=cls.device)
    boxes = torch.empty((n, apl, 6), dtype=torch.float32, device=cls.device)
    _lib.check(_lib.load().dn_decode_boxes(_ptr(cls), _ptr(loc), _ptr(anchors), n, apl, _ptr(scores),
                                           _ptr(boxes), _stream()), "dn_decode_boxes")
    return scores, boxes


# ---------------------------------------------------------------------------
# host-side rotated NMS (vectorised over the candidates still alive)
# ---------------------------------------------------------------------------
def _corners(b):
    """[K, 6] boxes -> [K, 4, 2] corners, counter-clockwise."""
    n = np.maximum(np.hypot(b[:, 4], b[:, 5]), 1e-12)
    s, c = b[:, 4] / n, b[:, 5] / n
    dx, dy = b[:, 2] / 2.0, b[:, 3] / 2.0
    loc = np.stack([np.stack([-dx, -dy], -1), np.stack([dx, -dy], -1),
                    np.stack([dx, dy], -1), np.stack([-dx, dy], -1)], 1)          # [K, 4, 2]
    x = loc[..., 0] * c[:, None] - loc[..., 1] * s[:, None] + b[:, None, 0]
    y = loc[..., 0] * s[:, None] + loc[..., 1] * c[:, None] + b[:, None, 1]
    return np.stack([x, y], -1)


def _intersection_area(ca, cb):
    """area of the intersection of two convex quads (Sutherland-Hodgman)."""
    poly = [ca[i] for i in range(4)]
    for i in range(4):
        a, b = cb[i], cb[(i + 1) % 4]
        nxt = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            sp = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
            sq = (b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0])
            if sp >= 0:
                nxt.append(p)
            if sp * sq < 0:
                nxt.append(p + (sp / (sp - sq)) * (q - p))
        poly = nxt
        if len(poly) < 3:
            return 0.0
    p = np.asarray(poly)
    return 0.5 * abs(np.dot(p[:, 0], np.roll(p[:, 1], -1)) - np.dot(p[:, 1], np.roll(p[:, 0], -1)))


def nms_rotated(boxes, scores, iou_thr=0.01):
    """boxes [K, 6], scores [K] (numpy) -> indices kept, best score first; ties broken by
    the lower index."""
    order = np.argsort(-scores, kind="stable")
    boxes = np.asarray(boxes, dtype=np.float64)[order]
    corners = _corners(boxes)
    radius = 0.5 * np.hypot(boxes[:, 2], boxes[:, 3])
    area = boxes[:, 2] * boxes[:, 3]
    alive = np.ones(len(order), dtype=bool)
    keep = []
    for i in range(len(order)):
        if not alive[i]:
            continue
        keep.append(int(order[i]))
        rest = np.nonzero(alive[i + 1:])[0] + i + 1
        if len(rest) == 0:
            continue
        near = rest[np.hypot(boxes[rest, 0] - boxes[i, 0], boxes[rest, 1] - boxes[i, 1])
                    < radius[rest] + radius[i]]
        for j in near:
            inter = _intersection_area(corners[i], corners[j])
            union = area[i] + area[j] - inter
            if union > 0 and inter / union > iou_thr:
                alive[j] = False
    return np.asarray(keep, dtype=np.int64)


def host_detections(result, anchors, pre_nms_top_k=300, iou_thr=0.01, score_thr=None):
    """Per-image detections [(boxes [K, 6], scores [K])] of the heads' outputs (`result` = {"cls", "loc"}, agent-major
    images): decode (HIP), top-k by score (torch on the GPU), rotated NMS (host).  The host reference of detect()."""
    scores, boxes = decode(result, anchors)
    dets = []
    for i in range(scores.shape[0]):
        s, b = scores[i], boxes[i]
        if score_thr is not None:
            s = torch.where(s > score_thr, s, torch.full_like(s, -1.0))
        k = min(pre_nms_top_k, s.numel())
        # stable: descending score, ascending index among equals
        top = torch.sort(s, descending=True, stable=True)[1][:k]
        sb, bb = s[top].cpu().numpy(), b[top].cpu().numpy()
        valid = sb >= 0
        sb, bb = sb[valid], bb[valid]
        keep = nms_rotated(bb, sb, iou_thr)
        dets.append((bb[keep], sb[keep]))
    return dets


def predict_all(model, anchors, bevs, trans_matrices, num_agent_tensor, batch_size=1,
                pre_nms_top_k=300, iou_thr=0.01, score_thr=None):
    """Per-image detections [(boxes [K, 6], scores [K])] for the agent-major batch: forward
    (HIP), decode (HIP), top-k by score (torch on the GPU), rotated NMS (host)."""
    from .detector import heads         # (detector imports this module)
    with torch.no_grad():
        out = model(bevs, trans_matrices, num_agent_tensor, batch_size)
    return host_detections(heads(out), anchors, pre_nms_top_k, iou_thr, score_thr)


# ---------------------------------------------------------------------------
# the same tail on the GPU: one batched call, no host synchronisation (dn_detect)
# ---------------------------------------------------------------------------
MAX_TOP_K = 1024


def detect(result, anchors, pre_nms_top_k=300, iou_thr=0.01, score_thr=None):
    """host_detections' tail on the GPU for every image at once: top-k by score (descending, lower anchor index first),
    rotated greedy NMS, padded rows.  `result` = {"cls": [N, A, 2], "loc": [N, ..., 6]} (N agent-major images; with
    kd_flag pass the dict of the forward's tuple).  Returns device tensors {"boxes" [N, K, 6], "scores" [N, K],
    "index" [N, K] (anchor index within the image, -1 past count), "count" [N]}; rows >= count are zero.  Runs on torch's
    current stream, allocates through torch's caching allocator and never waits for the device, so it can be captured
    into a graph behind the forward (graph.GraphedStep).  One difference from host_detections: a NaN score is never a
    candidate (the host lets it take a top-k slot, then drops it)."""
    k = int(pre_nms_top_k)
    if not 1 <= k <= MAX_TOP_K:
        raise ValueError("pre_nms_top_k = %d: detect() supports 1..%d" % (k, MAX_TOP_K))
    cls, loc = result["cls"], result["loc"]
    _need_gpu(cls, loc, anchors)
    n, apl = cls.shape[0], cls.shape[1]
    cls = cls.contiguous()
    loc = loc.reshape(n, apl, 6).contiguous()
    anchors = anchors.reshape(apl, 6).contiguous()
    lib = _lib.load()
    dev = cls.device
    nbytes = int(lib.dn_detect_workspace_bytes(n, apl, k))
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    out = {"boxes": torch.empty((n, k, 6), dtype=torch.float32, device=dev),
           "scores": torch.empty((n, k), dtype=torch.float32, device=dev),
           "index": torch.empty((n, k), dtype=torch.int32, device=dev),
           "count": torch.empty((n,), dtype=torch.int32, device=dev)}
    use_thr = score_thr is not None
    _lib.check(lib.dn_detect(_ptr(cls), _ptr(loc), _ptr(anchors), n, apl, k, int(use_thr),
                             float(score_thr) if use_thr else 0.0, float(iou_thr), _ptr(out["boxes"]),
                             _ptr(out["scores"]), _ptr(out["index"]), _ptr(out["count"]), _ptr(ws), nbytes, _stream()),
               "dn_detect")
    return out


def detections_to_host(det):
    """detect()'s device tensors -> host_detections' form [(boxes [c, 6], scores [c])] with one device-to-host copy."""
    n, k = det["scores"].shape
    packed = torch.cat([det["boxes"].reshape(n, 6 * k), det["scores"], det["count"].view(torch.float32)[:, None]],
                       dim=1).cpu().numpy()
    counts = packed[:, 7 * k].view(np.int32)
    return [(packed[i, :6 * k].reshape(k, 6)[:counts[i]].copy(), packed[i, 6 * k:7 * k][:counts[i]].copy())
            for i in range(n)]


# ---------------------------------------------------------------------------
# late fusion (`--com late`): every agent's detections merged in each ego's frame, duplicates suppressed (dn_late_fuse)
# ---------------------------------------------------------------------------
MAX_LATE_AGENTS = 16
MAX_LATE_ROWS = 8192         # agents * K: the rows one ego's list can hold


def _flat_extents(extents):
    """((x_lo, x_hi), (y_lo, y_hi)) or a flat (x_lo, x_hi, y_lo, y_hi) -> four floats; None stays None"""
    if extents is None:
        return None
    flat = [float(v) for v in np.asarray(extents, dtype=np.float64).reshape(-1)]
    if len(flat) != 4:
        raise ValueError("extents must be ((x_lo, x_hi), (y_lo, y_hi)), got %r" % (extents,))
    return flat


def _ego_range(agents, ego_first, ego_count):
    E = agents if ego_count is None else int(ego_count)
    if not (0 <= ego_first and E > 0 and ego_first + E <= agents):
        raise ValueError("ego range [%d, %d) outside 0..%d" % (ego_first, ego_first + E, agents))
    return E


def late_fuse(det, trans_matrices, num_agent, batch_size, agents, top_k=None, iou_thr=0.01, only_v2i=False, extents=None,
              ego_first=0, ego_count=None):
    """Late fusion on the GPU (include/disconet_hip.h :: dn_late_fuse; host_late_fuse is its reference).  `det` is
    detect()'s dict of every agent's own detections (`--com lowerbound`), or any dict of device tensors "boxes"
    [A*B, K, 6], "scores" [A*B, K], "count" [A*B] (agent-major images, the rows need not be sorted); trans_matrices
    [B, A, A, 4, 4]; num_agent the live counts ([B], or the reference's [B, A] tensor).  Each served ego takes its own
    rows and every listed neighbour's rows carried into its frame -- with `extents` = ((x_lo, x_hi), (y_lo, y_hi)), pass
    config.area_extents[:2], only those whose centre lands strictly inside -- orders them by score and runs detect()'s
    greedy rotated NMS.  Returns device tensors {"boxes" [E*B, top_k, 6], "scores" [E*B, top_k], "source" [E*B, top_k]
    int32 (agent * K + row of the input; -1 past count), "count" [E*B]}, image (i - ego_first) * B + b, rows >= count zero:
    the form MeanAP, Sort, ClearMot, Identity and Hota take.  top_k defaults to K.  Runs on torch's current stream,
    allocates through torch's caching allocator and never waits for the device (graph.GraphedStep)."""
    boxes, scores, count = det["boxes"], det["scores"], det["count"]
    for t in (boxes, scores, count, trans_matrices):
        if not isinstance(t, torch.Tensor):
            raise _lib.DnError("late_fuse needs device tensors (got %s); host_late_fuse is the numpy reference"
                               % type(t).__name__)
    _need_gpu(boxes, scores, count, trans_matrices)
    A, B = int(agents), int(batch_size)
    n, k = scores.shape
    top_k = k if top_k is None else int(top_k)
    if n != A * B or tuple(boxes.shape) != (n, k, 6) or count.numel() != n:
        raise ValueError("late_fuse: boxes %s scores %s count %s for agents * batch = %d images" % (
            tuple(boxes.shape), tuple(scores.shape), tuple(count.shape), A * B))
    if tuple(trans_matrices.shape) != (B, A, A, 4, 4):
        raise ValueError("late_fuse: trans_matrices %s, expected %s" % (tuple(trans_matrices.shape), (B, A, A, 4, 4)))
    ext = _flat_extents(extents)
    E = agents if ego_count is None else int(ego_count)
    dev = scores.device
    boxes = boxes.to(torch.float32).contiguous()
    scores = scores.to(torch.float32).contiguous()
    count = count.to(torch.int32).contiguous()
    trans = trans_matrices.to(torch.float32).contiguous()
    live = _live_counts(num_agent, dev)
    lib = _lib.load()
    nbytes = int(lib.dn_late_fuse_workspace_bytes(B, A, k, top_k, ego_first, E))
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    rows, kk = max(E, 0) * B, max(top_k, 1)
    out = {"boxes": torch.empty((rows, kk, 6), dtype=torch.float32, device=dev),
           "scores": torch.empty((rows, kk), dtype=torch.float32, device=dev),
           "source": torch.empty((rows, kk), dtype=torch.int32, device=dev),
           "count": torch.empty((rows,), dtype=torch.int32, device=dev)}
    _lib.check(lib.dn_late_fuse(_ptr(boxes), _ptr(scores), _ptr(count), _ptr(trans), _ptr(live), B, A, k, int(bool(only_v2i)),
                                int(ego_first), E, top_k, float(iou_thr), int(ext is not None),
                                (ctypes.c_double * 4)(*(ext or [0.0] * 4)), _ptr(out["boxes"]), _ptr(out["scores"]),
                                _ptr(out["source"]), _ptr(out["count"]), _ptr(ws), nbytes, _stream()), "dn_late_fuse")
    return out


def _live_counts(num_agent, device):
    from .ops import live_agent_counts
    if not isinstance(num_agent, torch.Tensor):
        num_agent = torch.as_tensor(np.asarray(num_agent))
    return live_agent_counts(num_agent, device)


def host_late_fuse(det, trans_matrices, num_agent, batch_size, agents, top_k=None, iou_thr=0.01, only_v2i=False,
                   extents=None, ego_first=0, ego_count=None):
    """dn_late_fuse's contract in numpy, float64, on nms_rotated: the reference late_fuse() must equal bit for bit.  `det`
    is detect()'s dict or pad_detections' (tensors or numpy); num_agent [B] (or [B, A], column 0).  Returns numpy arrays
    {"boxes" [E*B, top_k, 6] float32, "scores" [E*B, top_k] float32, "source" [E*B, top_k] int32, "count" [E*B] int32}."""
    boxes = np.asarray(_host(det["boxes"]), dtype=np.float32)
    scores = np.asarray(_host(det["scores"]), dtype=np.float32)
    count = np.asarray(_host(det["count"])).reshape(-1)
    trans = np.asarray(_host(trans_matrices), dtype=np.float32)
    live = np.asarray(_host(num_agent))
    live = live[:, 0] if live.ndim == 2 else live.reshape(-1)
    A, B = int(agents), int(batch_size)
    n, k = scores.shape
    top_k = k if top_k is None else int(top_k)
    if n != A * B or boxes.shape != (n, k, 6) or count.shape[0] != n:
        raise ValueError("host_late_fuse: boxes %s scores %s count %s for agents * batch = %d images" % (
            boxes.shape, scores.shape, count.shape, A * B))
    if not 1 <= top_k <= MAX_TOP_K or not 1 <= k <= MAX_TOP_K or A > MAX_LATE_AGENTS or A * k > MAX_LATE_ROWS:
        raise ValueError("host_late_fuse: top_k = %d, K = %d, agents = %d: 1..%d rows, at most %d agents and %d rows in a list"
                         % (top_k, k, A, MAX_TOP_K, MAX_LATE_AGENTS, MAX_LATE_ROWS))
    if not (math.isfinite(iou_thr) and iou_thr >= 0):
        raise ValueError("host_late_fuse: iou_thr = %r, must be finite and >= 0" % (iou_thr,))
    E = _ego_range(A, ego_first, ego_count)
    ext = _flat_extents(extents)
    out = {"boxes": np.zeros((E * B, top_k, 6), dtype=np.float32), "scores": np.zeros((E * B, top_k), dtype=np.float32),
           "source": np.full((E * B, top_k), -1, dtype=np.int32), "count": np.zeros(E * B, dtype=np.int32)}
    for b in range(B):
        nl = max(0, min(int(live[b]), A))
        for i in range(ego_first, ego_first + E):
            lst = ego_list(i, nl, only_v2i)
            cb, cs, src = [], [], []
            for pos, j in enumerate(lst):
                img = j * B + b
                c = max(0, min(int(count[img]), k))
                rows = boxes[img, :c]
                if pos:                                  # a neighbour's rows, carried into the ego's frame
                    M = trans[b, i, j].astype(np.float64)
                    r64 = rows.astype(np.float64)
                    x, y, sn, cn = r64[:, 0], r64[:, 1], r64[:, 4], r64[:, 5]
                    rows = rows.copy()
                    rows[:, 0] = ((M[0, 0] * x + M[0, 1] * y) + M[0, 3]).astype(np.float32)
                    rows[:, 1] = ((M[1, 0] * x + M[1, 1] * y) + M[1, 3]).astype(np.float32)
                    rows[:, 4] = (M[1, 0] * cn + M[1, 1] * sn).astype(np.float32)
                    rows[:, 5] = (M[0, 0] * cn + M[0, 1] * sn).astype(np.float32)
                s = scores[img, :c]
                with np.errstate(invalid="ignore"):
                    ok = np.isfinite(s) & (s >= 0)
                if pos and ext is not None:
                    x32, y32 = rows[:, 0].astype(np.float64), rows[:, 1].astype(np.float64)
                    ok &= (ext[0] < x32) & (x32 < ext[1]) & (ext[2] < y32) & (y32 < ext[3])
                cb.append(rows[ok])
                cs.append(s[ok])
                src.append((j * k + np.nonzero(ok)[0]).astype(np.int32))
            cb, cs, src = np.concatenate(cb), np.concatenate(cs), np.concatenate(src)
            order = np.argsort(-cs.astype(np.float64), kind="stable")[:top_k]      # (list position, row) among equals
            cb, cs, src = cb[order], cs[order], src[order]
            keep = nms_rotated(cb, cs.astype(np.float64), iou_thr) if len(cs) else np.zeros(0, dtype=np.int64)
            o = (i - ego_first) * B + b
            out["boxes"][o, :len(keep)] = cb[keep]
            out["scores"][o, :len(keep)] = cs[keep]
            out["source"][o, :len(keep)] = src[keep]
            out["count"][o] = len(keep)
    return out


# ---------------------------------------------------------------------------
# mAP at IoU 0.5 / 0.7: ground-truth matching per frame (dn_ap_match on the GPU, numpy reference below) and the
# precision / recall curve on the host from one copy of the records
# ---------------------------------------------------------------------------
MAX_GT = 1024            # ground-truth rows per image
MAX_IOU_THRS = 8         # one bit per threshold in a record
MAX_AGENTS = 64          # per-agent ground-truth counters a MeanAP owns


def pad_boxes(rows, width=None):
    """list of [n_i, 6] box arrays -> (padded [N, width, 6] float32, counts [N] int32); width >= 1."""
    rows = [np.asarray(r, dtype=np.float32).reshape(-1, 6) for r in rows]
    width = max([1] + [len(r) for r in rows]) if width is None else int(width)
    out = np.zeros((len(rows), width, 6), dtype=np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, np.asarray([len(r) for r in rows], dtype=np.int32)


def pad_detections(boxes, scores, width=None):
    """per-image lists (boxes [n_i, 6], scores [n_i]) -> {"boxes" [N, K, 6], "scores" [N, K], "count" [N]} (numpy): the
    form detect() returns, for detections that come from elsewhere."""
    b, count = pad_boxes(boxes, width)
    s = np.zeros(b.shape[:2], dtype=np.float32)
    for i, r in enumerate(scores):
        s[i, :len(r)] = np.asarray(r, dtype=np.float32)
    return {"boxes": b, "scores": s, "count": count}


def _check_thrs(iou_thrs):
    thrs = [float(t) for t in iou_thrs]
    if not 1 <= len(thrs) <= MAX_IOU_THRS:
        raise ValueError("%d IoU thresholds: 1..%d are supported" % (len(thrs), MAX_IOU_THRS))
    if not all(0.0 < t <= 1.0 for t in thrs):
        raise ValueError("IoU thresholds %s: each must be in (0, 1]" % (thrs,))
    return thrs


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def host_match_ground_truth(det, gt_boxes, gt_count, iou_thrs=(0.5, 0.7)):
    """numpy / float64 reference of match_ground_truth (the steps dn_ap_match runs, on _corners / _intersection_area).
    `det` = {"boxes" [N, K, 6], "scores" [N, K], "count" [N]}, gt_boxes [N, G, 6], gt_count [N] (numpy or tensors) ->
    {"best_iou" [N, K] float64, "best_gt" [N, K] int32, "rank" [N, K] int32, "tp" [T, N, K] uint8} (numpy).
    A row is valid when it is below its image's count and its score is finite; the other rows get rank -1, best_gt -1,
    best_iou 0 and tp 0.  rank = position in the stable descending score order; best_gt = the lowest ground-truth index
    with the largest IoU among those that pass the strict circumscribed-circle test (an IoU of 0 never matches); a row is
    a true positive at t when best_iou >= t and no row of lower rank with the same best_gt has best_iou >= t."""
    thrs = _check_thrs(iou_thrs)
    boxes, scores, count = _host(det["boxes"]), _host(det["scores"]), _host(det["count"])
    gt_boxes, gt_count = _host(gt_boxes), _host(gt_count)
    n, k = scores.shape
    g = gt_boxes.shape[1]
    best_iou = np.zeros((n, k), dtype=np.float64)
    best_gt = np.full((n, k), -1, dtype=np.int32)
    rank = np.full((n, k), -1, dtype=np.int32)
    tp = np.zeros((len(thrs), n, k), dtype=np.uint8)
    for img in range(n):
        c, gc = min(max(int(count[img]), 0), k), min(max(int(gt_count[img]), 0), g)
        valid = np.nonzero(np.isfinite(scores[img, :c]))[0]
        order = valid[np.argsort(-scores[img, valid], kind="stable")]
        rank[img, order] = np.arange(len(order), dtype=np.int32)
        if gc == 0 or len(order) == 0:
            continue
        d = np.asarray(boxes[img, :c], dtype=np.float64)
        t = np.asarray(gt_boxes[img, :gc], dtype=np.float64)
        dc, tc = _corners(d), _corners(t)
        d_rad, t_rad = 0.5 * np.hypot(d[:, 2], d[:, 3]), 0.5 * np.hypot(t[:, 2], t[:, 3])
        d_area, t_area = d[:, 2] * d[:, 3], t[:, 2] * t[:, 3]
        for i in order:
            near = np.nonzero(np.hypot(t[:, 0] - d[i, 0], t[:, 1] - d[i, 1]) < t_rad + d_rad[i])[0]
            best, best_j = 0.0, -1
            for j in near:
                inter = _intersection_area(dc[i], tc[j])
                union = d_area[i] + t_area[j] - inter
                iou = inter / union if union > 0 else 0.0
                if iou > best:
                    best, best_j = iou, j
            best_iou[img, i], best_gt[img, i] = best, best_j
        for ti, thr in enumerate(thrs):
            taken = np.zeros(gc, dtype=bool)
            for i in order:
                if best_gt[img, i] >= 0 and best_iou[img, i] >= thr and not taken[best_gt[img, i]]:
                    taken[best_gt[img, i]] = True
                    tp[ti, img, i] = 1
    return {"best_iou": best_iou, "best_gt": best_gt, "rank": rank, "tp": tp}


def records_from_match(det, match):
    """The records one call contributes, in accumulation order (image, then rank): (scores [R] float32, tp [T, R] uint8,
    image [R] int32)."""
    scores, rank, tp = _host(det["scores"]), _host(match["rank"]), _host(match["tp"])
    s, f, im = [], [], []
    for img in range(scores.shape[0]):
        rows = np.nonzero(rank[img] >= 0)[0]
        rows = rows[np.argsort(rank[img, rows], kind="stable")]
        s.append(scores[img, rows])
        f.append(tp[:, img, rows])
        im.append(np.full(len(rows), img, dtype=np.int32))
    return (np.concatenate(s).astype(np.float32), np.concatenate(f, axis=1).astype(np.uint8), np.concatenate(im))


def average_precision_from_records(scores, tp, n_gt):
    """Area under the interpolated precision / recall curve (mmdetection's "area" mode) of the records (scores [R], tp [R]
    0 / 1) in float64: records by descending score, equal scores in the order given (the accumulation order); n_gt == 0
    -> 0.0."""
    if int(n_gt) == 0:
        return 0.0
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    hit = np.asarray(tp).reshape(-1).astype(bool)[np.argsort(-scores, kind="stable")]
    tps = np.cumsum(hit.astype(np.int64))
    fps = np.cumsum((~hit).astype(np.int64))
    recall = tps / int(n_gt)
    precision = tps / np.maximum(tps + fps, 1)
    mrec = np.concatenate([[0.0], recall, [1.0]])
    mpre = np.concatenate([[0.0], precision, [0.0]])
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    idx = np.nonzero(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[idx + 1] - mrec[idx]) * mpre[idx + 1]))


def _ap_inputs(det, gt_boxes, gt_count):
    boxes, scores, count = det["boxes"], det["scores"], det["count"]
    for t in (boxes, scores, count, gt_boxes, gt_count):
        if not isinstance(t, torch.Tensor):
            raise _lib.DnError("match_ground_truth / MeanAP.update need device tensors (got %s); "
                               "host_match_ground_truth is the numpy reference" % type(t).__name__)
    _need_gpu(boxes, scores, count, gt_boxes, gt_count)
    n, k = scores.shape
    g = gt_boxes.shape[1]
    if not 1 <= k <= MAX_TOP_K or not 1 <= g <= MAX_GT:
        raise ValueError("K = %d detection rows, G = %d ground-truth rows: 1..%d and 1..%d are supported"
                         % (k, g, MAX_TOP_K, MAX_GT))
    if tuple(boxes.shape) != (n, k, 6) or tuple(gt_boxes.shape) != (n, g, 6) or count.numel() != n or gt_count.numel() != n:
        raise ValueError("shapes: boxes %s scores %s count %s gt_boxes %s gt_count %s" % (
            tuple(boxes.shape), tuple(scores.shape), tuple(count.shape), tuple(gt_boxes.shape), tuple(gt_count.shape)))
    return (boxes.to(torch.float32).contiguous(), scores.to(torch.float32).contiguous(),
            count.to(torch.int32).contiguous(), gt_boxes.to(torch.float32).contiguous(),
            gt_count.to(torch.int32).contiguous(), n, k, g)


def _ap_match(det, gt_boxes, gt_count, thrs, accum=None):
    boxes, scores, count, gt_boxes, gt_count, n, k, g = _ap_inputs(det, gt_boxes, gt_count)
    lib = _lib.load()
    dev = scores.device
    nt = len(thrs)
    nbytes = int(lib.dn_ap_match_workspace_bytes(n, k, g, nt))
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    out = {"best_iou": torch.empty((n, k), dtype=torch.float64, device=dev),
           "best_gt": torch.empty((n, k), dtype=torch.int32, device=dev),
           "rank": torch.empty((n, k), dtype=torch.int32, device=dev),
           "tp": torch.empty((nt, n, k), dtype=torch.uint8, device=dev)}
    records, capacity, state, n_agents, batch = accum if accum is not None else (None, 0, None, 0, 1)
    _lib.check(lib.dn_ap_match(_ptr(boxes), _ptr(scores), _ptr(count), _ptr(gt_boxes), _ptr(gt_count), n, k, g,
                               (ctypes.c_double * nt)(*thrs), nt, _ptr(out["best_iou"]), _ptr(out["best_gt"]),
                               _ptr(out["rank"]), _ptr(out["tp"]), _ptr(ws), nbytes, _ptr(records), capacity,
                               _ptr(state), n_agents, batch, _stream()), "dn_ap_match")
    return out


def match_ground_truth(det, gt_boxes, gt_count, iou_thrs=(0.5, 0.7)):
    """Per-image ground-truth matching on the GPU (dn_ap_match; host_match_ground_truth is its reference).  `det` is
    detect()'s dict or any dict of device tensors "boxes" [N, K, 6], "scores" [N, K], "count" [N] (the rows need not be
    sorted); gt_boxes [N, G, 6], gt_count [N]; K, G <= 1024, up to 8 thresholds in (0, 1].  Returns device tensors
    {"best_iou" [N, K] float64, "best_gt" [N, K] int32, "rank" [N, K] int32, "tp" [T, N, K] uint8}.  Runs on torch's
    current stream and never waits for the device."""
    return _ap_match(det, gt_boxes, gt_count, _check_thrs(iou_thrs))


class MeanAP:
    """mAP over an evaluation run: update() after every frame's detect() (enqueues dn_ap_match on the current stream:
    matching on the GPU, records appended to device arrays at a device-resident cursor, no host synchronisation), compute()
    once at the end (one copy of the state words and one of the filled part of the records, then the precision / recall
    curve on the host in float64).

    Images are agent-major, `batch_size` per agent: image i belongs to agent i // batch_size (up to 64 agents).
    `capacity` = records (detections) the run may accumulate; compute() raises DnError when more arrived, or when a row
    below its count carried a non-finite score -- never a silently truncated metric.

    update() is usable inside graph.GraphedStep (forward + detect() + update() in one captured graph; every replay
    appends that frame's records).  GraphedStep runs its step three times to warm up before it captures and those runs
    append records too: call reset() after constructing the GraphedStep, before the first replay that counts."""

    def __init__(self, batch_size, iou_thrs=(0.5, 0.7), capacity=1 << 20):
        self.batch_size = int(batch_size)
        self.iou_thrs = _check_thrs(iou_thrs)
        self.capacity = int(capacity)
        if self.batch_size < 1 or self.capacity < 1:
            raise ValueError("MeanAP: batch_size = %d, capacity = %d, both must be positive" % (self.batch_size, self.capacity))
        self.n_agents = 0            # agents seen by update() (host-side: from the shapes only)
        self.records = None          # [capacity, 2] int32 on the device: {score bits, agent << 8 | tp bits}
        self.state = None            # [2 + MAX_AGENTS] int64 on the device: cursor, status, ground truth per agent

    def _allocate(self, device):
        self.records = torch.empty((self.capacity, 2), dtype=torch.int32, device=device)
        self.state = torch.empty((2 + MAX_AGENTS,), dtype=torch.int64, device=device)
        self.reset()

    def reset(self):
        """Forget every record and counter (a one-thread kernel on the current stream)."""
        if self.state is not None:
            _lib.check(_lib.load().dn_ap_reset(_ptr(self.state), MAX_AGENTS, _stream()), "dn_ap_reset")

    def update(self, det, gt_boxes, gt_count):
        """Match one call's detections (detect()'s dict) against its ground truth and append the records.  Enqueues only.
        Returns match_ground_truth's tensors for that call."""
        _ap_inputs(det, gt_boxes, gt_count)
        n = det["scores"].shape[0]
        agents = -(-n // self.batch_size)
        if agents > MAX_AGENTS:
            raise ValueError("MeanAP: %d images at batch %d are %d agents, at most %d" % (n, self.batch_size, agents, MAX_AGENTS))
        if self.state is None:
            self._allocate(det["scores"].device)
        self.n_agents = max(self.n_agents, agents)
        return _ap_match(det, gt_boxes, gt_count, self.iou_thrs,
                         (self.records, self.capacity, self.state, MAX_AGENTS, self.batch_size))

    def host_records(self):
        """(scores [R] float32, tp [T, R] uint8, agent [R] int32, gt per agent [n_agents] int64, status) -- waits for the
        device; R = records kept (at most capacity)."""
        if self.state is None:
            return (np.zeros(0, np.float32), np.zeros((len(self.iou_thrs), 0), np.uint8), np.zeros(0, np.int32),
                    np.zeros(0, np.int64), 0)
        state = self.state.cpu().numpy()
        filled = int(min(state[0], self.capacity))
        rec = self.records[:filled].cpu().numpy()
        flags = rec[:, 1].view(np.uint32)
        tp = np.stack([((flags >> t) & 1).astype(np.uint8) for t in range(len(self.iou_thrs))])
        return (rec[:, 0].copy().view(np.float32), tp, (flags >> 8).astype(np.int32),
                state[2:2 + self.n_agents].copy(), int(state[1]))

    def compute(self):
        """{"mAP@<t>": AP over every record, ..., "per_agent": [{"mAP@<t>": ..., "n_det", "n_gt", "n_tp"}, ...], "n_det",
        "n_gt", "n_tp"}; n_tp = true positives per threshold."""
        scores, tp, agent, gt, status = self.host_records()
        if status & 1:
            raise _lib.DnError("MeanAP: more detections arrived than the capacity of %d records; the metric would be "
                               "truncated (raise `capacity`)" % self.capacity)
        if status & 2:
            raise _lib.DnError("MeanAP: a detection with a non-finite score was passed to update()")
        names = ["mAP@%g" % t for t in self.iou_thrs]
        out = {name: average_precision_from_records(scores, tp[t], gt.sum()) for t, name in enumerate(names)}
        out["per_agent"] = []
        for a in range(self.n_agents):
            m = agent == a
            row = {name: average_precision_from_records(scores[m], tp[t][m], gt[a]) for t, name in enumerate(names)}
            row.update(n_det=int(m.sum()), n_gt=int(gt[a]), n_tp=[int(tp[t][m].sum()) for t in range(len(names))])
            out["per_agent"].append(row)
        out.update(n_det=int(len(scores)), n_gt=int(gt.sum()), n_tp=[int(tp[t].sum()) for t in range(len(names))])
        return out


# ---------------------------------------------------------------------------
# Stratified AP: every ground-truth box carries a stratum (own visibility or range from the ego, gt_strata), matching,
# records and counters per stratum on the GPU (dn_ap_match_strata), the figures on the host from the integer records.
#
# The metric, for a threshold t and a stratum s: a record is LEFT OUT when its reach bit t is set (best_gt >= 0 and
# best_iou >= t, claim won or not) and its stratum -- that of its best_gt -- is not s: it found a real box of another
# stratum or a don't-care box (stratum -1).  Every other record stays: a true positive when its tp bit t is set (its
# stratum is then s), a false positive otherwise (duplicates on a box of s, detections that reach nothing).  n_gt is the
# stratum's counter; recall = TP / n_gt, NaN when n_gt == 0 (AP is then 0.0).  The row "all" leaves out only the records
# that reach a don't-care box; its n_gt is the sum over the strata.
# ---------------------------------------------------------------------------
MAX_STRATA = 8           # (stratum + 1) shares a record word with the reach byte
STRATA_MODES = {"range": 0, "visibility": 1}


def _check_edges(mode, edges):
    if mode not in STRATA_MODES:
        raise ValueError("strata mode %r: one of %s" % (mode, " | ".join(STRATA_MODES)))
    e = [float(v) for v in np.asarray(edges, dtype=np.float64).reshape(-1)]
    if not 1 <= len(e) <= MAX_STRATA - 1:
        raise ValueError("%d strata edges: 1..%d are supported" % (len(e), MAX_STRATA - 1))
    if not all(np.isfinite(v) and v > 0 for v in e) or any(b <= a for a, b in zip(e, e[1:])):
        raise ValueError("strata edges %s: finite, positive and strictly ascending" % (e,))
    if mode == "visibility" and not all(v >= 1 and v == int(v) and v < 2 ** 31 for v in e):
        raise ValueError("strata edges %s: the edges of own visibility are integers >= 1 (returns)" % (e,))
    return STRATA_MODES[mode], e


def strata_names(mode, edges):
    """The names of the len(edges) + 1 strata of gt_strata(mode, edges), lowest first."""
    _, e = _check_edges(mode, edges)
    if mode == "visibility":
        e = [int(v) for v in e]
        if len(e) == 1:
            return ["hidden from the ego (< %d own returns)" % e[0], "seen by the ego (>= %d own returns)" % e[0]]
        return ["< %d own returns" % e[0]] + ["%d..%d own returns" % (a, b - 1) for a, b in zip(e, e[1:])] + [
            ">= %d own returns" % e[-1]]
    return ["< %g m" % e[0]] + ["%g..%g m" % (a, b) for a, b in zip(e, e[1:])] + [">= %g m" % e[-1]]


def host_gt_strata(gt_boxes, gt_count, mode, edges, own_hits=None):
    """numpy statement of gt_strata (dn_gt_strata), equal to it in every word: stratum [N, G] int32 of gt_boxes [N, G, 6],
    gt_count [N]; rows at or beyond the (clamped) count get -1.  The stratum of a row is the number of `edges` it has
    reached.  mode "range": d2 = x * x + y * y in float64 from the float32 centre, each operation rounded on its own,
    against the edges squared in float64 (no square root); a non-finite x or y gives -1.  mode "visibility":
    own_hits [N, G] (a lidar scene's "gt_own_hits") against integer edges; with the single edge 5 stratum 0 is "hidden
    from the ego", stratum 1 "seen by the ego itself"."""
    m, e = _check_edges(mode, edges)
    gt_boxes, gt_count = np.asarray(_host(gt_boxes), dtype=np.float32), _host(gt_count)
    n, g = gt_boxes.shape[:2]
    if m == 0:
        x, y = gt_boxes[..., 0].astype(np.float64), gt_boxes[..., 1].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            v = x * x + y * y
        ok = np.isfinite(gt_boxes[..., 0]) & np.isfinite(gt_boxes[..., 1])
        e = [q * q for q in e]
    else:
        if own_hits is None:
            raise ValueError("strata by own visibility need own_hits (a lidar scene's gt_own_hits)")
        v = np.asarray(_host(own_hits)).reshape(n, g).astype(np.float64)
        ok = np.ones((n, g), dtype=bool)
    st = np.zeros((n, g), dtype=np.int32)
    for q in e:
        with np.errstate(invalid="ignore"):
            st += (v >= q).astype(np.int32)
    gc = np.clip(gt_count.astype(np.int64), 0, g)
    st[~ok | (np.arange(g)[None, :] >= gc[:, None])] = -1
    return st


def gt_strata(gt_boxes, gt_count, mode, edges, own_hits=None):
    """The stratum of every ground-truth box on the GPU (dn_gt_strata; host_gt_strata is its statement and its docstring
    the rule): device tensors gt_boxes [N, G, 6], gt_count [N], own_hits [N, G] int32 for mode "visibility" -> [N, G]
    int32 on the device, len(edges) + 1 strata.  One launch on torch's current stream; never waits for the device."""
    m, e = _check_edges(mode, edges)
    for t in (gt_boxes, gt_count) + ((own_hits,) if m == 1 else ()):
        if not isinstance(t, torch.Tensor):
            raise _lib.DnError("gt_strata needs device tensors (got %s); host_gt_strata is the numpy form" % type(t).__name__)
    _need_gpu(gt_boxes, gt_count)
    n, g = gt_boxes.shape[:2]
    if tuple(gt_boxes.shape) != (n, g, 6) or gt_count.numel() != n or (m == 1 and tuple(own_hits.shape) != (n, g)):
        raise ValueError("shapes: gt_boxes %s gt_count %s own_hits %s" % (
            tuple(gt_boxes.shape), tuple(gt_count.shape), None if own_hits is None else tuple(own_hits.shape)))
    gt_boxes, gt_count = gt_boxes.to(torch.float32).contiguous(), gt_count.to(torch.int32).contiguous()
    own = own_hits.to(torch.int32).contiguous() if m == 1 else None
    out = torch.empty((n, g), dtype=torch.int32, device=gt_boxes.device)
    _lib.check(_lib.load().dn_gt_strata(_ptr(gt_boxes), _ptr(gt_count), _ptr(own), n, g, m, (ctypes.c_double * len(e))(*e),
                                        len(e), _ptr(out), _stream()), "dn_gt_strata")
    return out


def _check_strata(n_strata):
    n_strata = int(n_strata)
    if not 1 <= n_strata <= MAX_STRATA:
        raise ValueError("%d strata: 1..%d are supported" % (n_strata, MAX_STRATA))
    return n_strata


def host_match_strata(det, gt_boxes, gt_count, gt_stratum, n_strata, iou_thrs=(0.5, 0.7)):
    """numpy reference of match_ground_truth_strata: host_match_ground_truth's dict (unchanged) plus
    "gt_claim" [T, N, G] int32 (the rank of the detection that claimed the box at that threshold, -1 when none did and
    beyond gt_count), "stratum" [N, K] int32 (that of the row's best_gt; -1 when it has none), "reach" [N, K] uint8 (bit t:
    best_gt >= 0 and best_iou >= t, claim won or not), "counts" [N, S + 1] int64 (the image's boxes per stratum, the
    don't-care boxes last) and "status" (the bits one update leaves in the accumulator's status word when every record
    fits: 2 = a row below count had a non-finite score, 4 = a row below gt_count carried a stratum outside [-1, S), which
    counts as -1)."""
    thrs, s_n = _check_thrs(iou_thrs), _check_strata(n_strata)
    out = host_match_ground_truth(det, gt_boxes, gt_count, thrs)
    gt_count, words = _host(gt_count), np.asarray(_host(gt_stratum)).astype(np.int64)
    n, k = out["rank"].shape
    g = words.shape[1]
    gc = np.clip(gt_count.astype(np.int64), 0, g)
    below = np.arange(g)[None, :] < gc[:, None]
    bad = (words < -1) | (words >= s_n)
    st = np.where(bad, -1, words)
    scores, count = _host(det["scores"]), _host(det["count"])
    rows_below = np.arange(k)[None, :] < np.clip(count.astype(np.int64), 0, k)[:, None]
    out["status"] = (4 if (bad & below).any() else 0) | (2 if (~np.isfinite(scores) & rows_below).any() else 0)
    out["counts"] = np.stack([np.bincount(np.where(st[i, :gc[i]] < 0, s_n, st[i, :gc[i]]), minlength=s_n + 1)
                              for i in range(n)]).astype(np.int64)
    has = out["best_gt"] >= 0
    col = np.where(has, out["best_gt"], 0)
    out["stratum"] = np.where(has, np.take_along_axis(st, col.astype(np.int64), axis=1), -1).astype(np.int32)
    reach = np.zeros((n, k), dtype=np.uint8)
    claim = np.full((len(thrs), n, g), -1, dtype=np.int32)
    for t, thr in enumerate(thrs):
        reach |= ((has & (out["best_iou"] >= thr)).astype(np.uint8) << t).astype(np.uint8)
        img, row = np.nonzero(out["tp"][t])
        claim[t, img, out["best_gt"][img, row]] = out["rank"][img, row]
    out["reach"], out["gt_claim"] = reach, claim
    return out


def strata_records_from_match(det, match, batch_size=1):
    """The records one call contributes, in accumulation order (image, then rank), as dn_ap_match_strata writes them:
    [R, 4] uint32 {score bits, agent << 8 | tp bits, (stratum + 1) << 8 | reach bits, best_gt}; `match` is
    host_match_strata's dict."""
    scores, rank, tp = np.asarray(_host(det["scores"]), dtype=np.float32), _host(match["rank"]), _host(match["tp"])
    out = []
    for img in range(scores.shape[0]):
        rows = np.nonzero(rank[img] >= 0)[0]
        rows = rows[np.argsort(rank[img, rows], kind="stable")]
        bits = np.zeros(len(rows), dtype=np.uint32)
        for t in range(tp.shape[0]):
            bits |= tp[t, img, rows].astype(np.uint32) << np.uint32(t)
        rec = np.empty((len(rows), 4), dtype=np.uint32)
        rec[:, 0] = scores[img, rows].view(np.uint32)
        rec[:, 1] = np.uint32((img // int(batch_size)) << 8) | bits
        rec[:, 2] = ((match["stratum"][img, rows].astype(np.int64) + 1) << 8).astype(np.uint32) | match["reach"][img, rows]
        rec[:, 3] = match["best_gt"][img, rows].astype(np.int32).view(np.uint32)
        out.append(rec)
    return np.concatenate(out) if out else np.zeros((0, 4), dtype=np.uint32)


def _strata_row(scores, tp_word, st_word, thrs, stratum, n_gt):
    """one row of the table: stratum = None is "all" """
    st = (st_word >> 8).astype(np.int64) - 1
    row = {"n_gt": int(n_gt), "n_counted": [], "n_left_out": [], "n_tp": []}
    for t, thr in enumerate(thrs):
        reach = ((st_word >> t) & 1).astype(bool)
        left = reach & ((st == -1) if stratum is None else (st != stratum))
        keep = ~left
        hit = ((tp_word >> t) & 1).astype(np.uint8)[keep]
        row["AP@%g" % thr] = average_precision_from_records(scores[keep], hit, n_gt)
        row["recall@%g" % thr] = float(hit.sum()) / int(n_gt) if int(n_gt) else float("nan")
        row["n_counted"].append(int(keep.sum()))
        row["n_left_out"].append(int(left.sum()))
        row["n_tp"].append(int(hit.sum()))
    row["n_det"] = int(len(scores))
    return row


def stratified_ap_from_records(records, counts, n_strata, iou_thrs=(0.5, 0.7), names=None):
    """The stratified figures in float64 from the integer records (the rule: the comment above host_gt_strata's section).
    records [R, 4] 32-bit words in accumulation order (strata_records_from_match / StratifiedAP.host_records), counts
    [n_agents, S + 1] ground-truth boxes per agent and stratum (don't-care last).  Returns {"all": row, "strata": [row +
    "name", ...], "per_agent": [the "all" row of each agent's records, ...]}; a row is {"AP@<t>", "recall@<t>" (NaN when
    n_gt == 0), "n_gt", "n_det" (records looked at), and per threshold "n_counted", "n_left_out", "n_tp"}."""
    thrs, s_n = _check_thrs(iou_thrs), _check_strata(n_strata)
    names = ["stratum %d" % s for s in range(s_n)] if names is None else [str(v) for v in names]
    if len(names) != s_n:
        raise ValueError("%d names for %d strata" % (len(names), s_n))
    rec = np.ascontiguousarray(np.asarray(records)).view(np.uint32).reshape(-1, 4)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, s_n + 1)
    scores, tp_word, st_word = rec[:, 0].copy().view(np.float32), rec[:, 1] & np.uint32(0xff), rec[:, 2]
    agent = (rec[:, 1] >> 8).astype(np.int64)
    per_stratum = counts[:, :s_n].sum(axis=0) if len(counts) else np.zeros(s_n, np.int64)
    out = {"all": _strata_row(scores, tp_word, st_word, thrs, None, per_stratum.sum()), "strata": [], "per_agent": []}
    for s in range(s_n):
        row = {"name": names[s]}
        row.update(_strata_row(scores, tp_word, st_word, thrs, s, per_stratum[s]))
        out["strata"].append(row)
    for a in range(len(counts)):
        m = agent == a
        out["per_agent"].append(_strata_row(scores[m], tp_word[m], st_word[m], thrs, None, counts[a, :s_n].sum()))
    return out


def _ap_match_strata(det, gt_boxes, gt_count, gt_stratum, n_strata, thrs, accum=None):
    boxes, scores, count, gt_boxes, gt_count, n, k, g = _ap_inputs(det, gt_boxes, gt_count)
    if not isinstance(gt_stratum, torch.Tensor) or tuple(gt_stratum.shape) != (n, g):
        raise ValueError("gt_stratum: a device tensor [%d, %d] is needed (gt_strata makes one)" % (n, g))
    _need_gpu(gt_stratum)
    gt_stratum = gt_stratum.to(torch.int32).contiguous()
    lib = _lib.load()
    dev = scores.device
    nt = len(thrs)
    nbytes = int(lib.dn_ap_match_strata_workspace_bytes(n, k, g, nt, n_strata))
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    out = {"best_iou": torch.empty((n, k), dtype=torch.float64, device=dev),
           "best_gt": torch.empty((n, k), dtype=torch.int32, device=dev),
           "rank": torch.empty((n, k), dtype=torch.int32, device=dev),
           "tp": torch.empty((nt, n, k), dtype=torch.uint8, device=dev),
           "gt_claim": torch.empty((nt, n, g), dtype=torch.int32, device=dev)}
    records, capacity, state, n_agents, batch = accum if accum is not None else (None, 0, None, 0, 1)
    _lib.check(lib.dn_ap_match_strata(_ptr(boxes), _ptr(scores), _ptr(count), _ptr(gt_boxes), _ptr(gt_count),
                                      _ptr(gt_stratum), n, k, g, (ctypes.c_double * nt)(*thrs), nt, n_strata,
                                      _ptr(out["best_iou"]), _ptr(out["best_gt"]), _ptr(out["rank"]), _ptr(out["tp"]),
                                      _ptr(out["gt_claim"]), _ptr(ws), nbytes, _ptr(records), capacity, _ptr(state),
                                      n_agents, batch, _stream()), "dn_ap_match_strata")
    return out


def match_ground_truth_strata(det, gt_boxes, gt_count, gt_stratum, n_strata, iou_thrs=(0.5, 0.7)):
    """match_ground_truth through dn_ap_match_strata: the same four tensors, bit for bit, and "gt_claim" [T, N, G] int32 --
    the rank of the detection that claimed each ground-truth box at each threshold, -1 when none did.  gt_stratum [N, G]
    int32 on the device (gt_strata), n_strata <= 8.  host_match_strata is the reference."""
    return _ap_match_strata(det, gt_boxes, gt_count, gt_stratum, _check_strata(n_strata), _check_thrs(iou_thrs))


class StratifiedAP:
    """AP and recall per stratum of the ground truth over an evaluation run: update() after every frame's detect() with
    the frame's gt_strata() (enqueues dn_ap_match_strata on the current stream: matching, 16-byte records and per-stratum
    counters on the GPU, no host synchronisation), compute() once at the end (one copy of the state words and one of the
    filled records, then stratified_ap_from_records on the host in float64).  A box with stratum -1 is a don't-care box:
    it is counted apart and the detections that reach it are left out of every row.

    Images are agent-major, `batch_size` per agent (up to 64 agents); `names` label the strata in compute()'s rows.
    compute() raises DnError when more records arrived than `capacity`, when a row below its count carried a non-finite
    score, or when a ground-truth row carried a stratum outside [-1, n_strata) -- never a silently wrong metric.

    update() is usable inside graph.GraphedStep (forward + detect() + gt_strata() + update() in one captured graph; every
    replay appends that frame's records).  GraphedStep runs its step three times to warm up before it captures and those
    runs append records too: call reset() after constructing the GraphedStep, before the first replay that counts."""

    def __init__(self, batch_size, n_strata, names=None, iou_thrs=(0.5, 0.7), capacity=1 << 20):
        self.batch_size = int(batch_size)
        self.n_strata = _check_strata(n_strata)
        self.names = ["stratum %d" % s for s in range(self.n_strata)] if names is None else [str(v) for v in names]
        self.iou_thrs = _check_thrs(iou_thrs)
        self.capacity = int(capacity)
        if self.batch_size < 1 or self.capacity < 1:
            raise ValueError("StratifiedAP: batch_size = %d, capacity = %d, both must be positive" % (
                self.batch_size, self.capacity))
        if len(self.names) != self.n_strata:
            raise ValueError("StratifiedAP: %d names for %d strata" % (len(self.names), self.n_strata))
        self.n_agents = 0            # agents seen by update() (host-side: from the shapes only)
        self.records = None          # [capacity, 4] int32 on the device
        self.state = None            # [2 + MAX_AGENTS * (n_strata + 1)] int64 on the device

    def _allocate(self, device):
        self.records = torch.empty((self.capacity, 4), dtype=torch.int32, device=device)
        self.state = torch.empty((2 + MAX_AGENTS * (self.n_strata + 1),), dtype=torch.int64, device=device)
        self.reset()

    def reset(self):
        """Forget every record and counter (one zero-fill launch on the current stream)."""
        if self.state is not None:
            _lib.check(_lib.load().dn_ap_strata_reset(_ptr(self.state), MAX_AGENTS, self.n_strata, _stream()),
                       "dn_ap_strata_reset")

    def update(self, det, gt_boxes, gt_count, gt_stratum):
        """Match one call's detections (detect()'s dict) against its ground truth and append the records.  Enqueues only.
        Returns match_ground_truth_strata's tensors for that call."""
        _ap_inputs(det, gt_boxes, gt_count)
        n = det["scores"].shape[0]
        agents = -(-n // self.batch_size)
        if agents > MAX_AGENTS:
            raise ValueError("StratifiedAP: %d images at batch %d are %d agents, at most %d" % (
                n, self.batch_size, agents, MAX_AGENTS))
        if self.state is None:
            self._allocate(det["scores"].device)
        self.n_agents = max(self.n_agents, agents)
        return _ap_match_strata(det, gt_boxes, gt_count, gt_stratum, self.n_strata, self.iou_thrs,
                                (self.records, self.capacity, self.state, MAX_AGENTS, self.batch_size))

    def host_records(self):
        """(records [R, 4] uint32, counts [n_agents, S + 1] int64, status) -- waits for the device; R = records kept (at
        most capacity)."""
        if self.state is None:
            return np.zeros((0, 4), np.uint32), np.zeros((0, self.n_strata + 1), np.int64), 0
        state = self.state.cpu().numpy()
        filled = int(min(state[0], self.capacity))
        rec = self.records[:filled].cpu().numpy().view(np.uint32)
        counts = state[2:].reshape(MAX_AGENTS, self.n_strata + 1)[:self.n_agents].copy()
        return rec, counts, int(state[1])

    def compute(self):
        """stratified_ap_from_records of everything accumulated: {"all": row, "strata": [row with "name", ...],
        "per_agent": [row, ...]}."""
        rec, counts, status = self.host_records()
        if status & 1:
            raise _lib.DnError("StratifiedAP: more detections arrived than the capacity of %d records; the metric would be "
                               "truncated (raise `capacity`)" % self.capacity)
        if status & 2:
            raise _lib.DnError("StratifiedAP: a detection with a non-finite score was passed to update()")
        if status & 4:
            raise _lib.DnError("StratifiedAP: a ground-truth row carried a stratum outside [-1, %d)" % self.n_strata)
        return stratified_ap_from_records(rec, counts, self.n_strata, self.iou_thrs, self.names)
