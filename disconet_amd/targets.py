"""Training targets from ground-truth boxes: what the reference computes on the CPU when it creates the dataset
(upstream:tools/det/create_data_det.py, coperception/utils/obj_util.py: label, reg_target, allocation_mask per sample),
here per step on the GPU (dn_assign_targets) in the shapes CoDetModule.step reads.

The rule (SECOND / FaF; include/disconet_hip.h states it in full): an anchor is positive when its best rotated IoU over the
image's boxes reaches pos_thr, negative below neg_thr, don't care between; with force_match every box also makes its best
anchor positive.  A positive anchor regresses to the box code that postprocess.decode inverts.  host_assign_targets is
the numpy / float64 reference of the same rule, encode_boxes the numpy inverse of the decode.
"""
import numpy as np
import torch

from . import _lib
from .ops import _need_gpu, _ptr, _stream
from .postprocess import MAX_GT, _corners, _host, _intersection_area


def _check_thrs(pos_thr, neg_thr):
    pos_thr, neg_thr = float(pos_thr), float(neg_thr)
    if not 0.0 < neg_thr <= pos_thr <= 1.0:
        raise ValueError("thresholds neg %g, pos %g: 0 < neg_thr <= pos_thr <= 1 is required" % (neg_thr, pos_thr))
    return pos_thr, neg_thr


def assign_targets(anchors, gt_boxes, gt_count, pos_thr=0.6, neg_thr=0.45, force_match=True, want_match=False):
    """anchors [H, W, A, 6] (postprocess.make_anchors), gt_boxes [N, G, 6], gt_count [N] (postprocess.pad_boxes' form, the
    arrays MeanAP.update takes; G <= 1024), all on the GPU -> {"labels" [N, H*W*A, 2], "reg_targets" [N, H, W, A, 1, 6],
    "reg_loss_mask" [N, H, W, A, 1]} float32 device tensors, what CoDetModule.step reads as data[...] without a copy; with
    want_match also "matched_gt" [N, H*W*A] int32 (-1: not positive) and "best_iou" [N, H*W*A] float64.  Runs on torch's
    current stream, allocates through torch's caching allocator and never waits for the device: it can be captured into
    a graph."""
    pos_thr, neg_thr = _check_thrs(pos_thr, neg_thr)
    for t in (anchors, gt_boxes, gt_count):
        if not isinstance(t, torch.Tensor):
            raise _lib.DnError("assign_targets needs device tensors (got %s); host_assign_targets is the numpy reference"
                               % type(t).__name__)
    _need_gpu(anchors, gt_boxes, gt_count)
    if anchors.dim() != 4 or anchors.shape[-1] != 6:
        raise ValueError("anchors %s: [H, W, A, 6] is expected" % (tuple(anchors.shape),))
    h, w, a = (int(v) for v in anchors.shape[:3])
    apl = h * w * a
    if gt_boxes.dim() != 3 or gt_boxes.shape[-1] != 6 or gt_count.numel() != gt_boxes.shape[0] or gt_boxes.shape[0] < 1 \
            or apl < 1:
        raise ValueError("shapes: anchors %s gt_boxes %s gt_count %s" % (
            tuple(anchors.shape), tuple(gt_boxes.shape), tuple(gt_count.shape)))
    n, g = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    if not 1 <= g <= MAX_GT:
        raise ValueError("G = %d ground-truth rows: 1..%d are supported" % (g, MAX_GT))
    anchors = anchors.to(torch.float32).reshape(apl, 6).contiguous()
    gt_boxes = gt_boxes.to(torch.float32).contiguous()
    gt_count = gt_count.to(torch.int32).contiguous()
    lib = _lib.load()
    dev = gt_boxes.device
    nbytes = int(lib.dn_assign_targets_workspace_bytes(n, apl, g))
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    out = {"labels": torch.empty((n, apl, 2), dtype=torch.float32, device=dev),
           "reg_targets": torch.empty((n, h, w, a, 1, 6), dtype=torch.float32, device=dev),
           "reg_loss_mask": torch.empty((n, h, w, a, 1), dtype=torch.float32, device=dev)}
    if want_match:
        out["matched_gt"] = torch.empty((n, apl), dtype=torch.int32, device=dev)
        out["best_iou"] = torch.empty((n, apl), dtype=torch.float64, device=dev)
    _lib.check(lib.dn_assign_targets(_ptr(anchors), _ptr(gt_boxes), _ptr(gt_count), n, apl, g, pos_thr, neg_thr,
                                     int(bool(force_match)), _ptr(out["labels"]), _ptr(out["reg_targets"]),
                                     _ptr(out["reg_loss_mask"]), _ptr(out.get("matched_gt")), _ptr(out.get("best_iou")),
                                     _ptr(ws), nbytes, _stream()), "dn_assign_targets")
    return out


def encode_boxes(boxes, anchors):
    """The numpy inverse of the box decode (oracle.postprocess_ref.decode_boxes, dn_decode_boxes): boxes [..., 6] =
    (x, y, w, h, sin, cos) against anchors [..., 6] (broadcast) -> the code [..., 6] in float64; (sin, cos) is normalised
    by max(hypot, 1e-12) first, the anchor's is used as it is (as the decode does)."""
    b = np.asarray(boxes, dtype=np.float64)
    a = np.asarray(anchors, dtype=np.float64)
    n = np.maximum(np.hypot(b[..., 4], b[..., 5]), 1e-12)
    s, c = b[..., 4] / n, b[..., 5] / n
    return np.stack([(b[..., 0] - a[..., 0]) / a[..., 2], (b[..., 1] - a[..., 1]) / a[..., 3],
                     np.log(b[..., 2] / a[..., 2]), np.log(b[..., 3] / a[..., 3]),
                     s * a[..., 5] - c * a[..., 4], c * a[..., 5] + s * a[..., 4]], -1)


def host_pair_ious(anchors, boxes):
    """IoU of the (anchor, box) pairs that pass the strict circumscribed-circle test, on postprocess._corners /
    _intersection_area in float64: anchors [P, 6], boxes [J, 6] -> (anchor index [M], box index [M], IoU [M]) ordered by
    anchor, then box.  The candidates are found per box with numpy, so only the pairs themselves cost a polygon clip."""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 6)
    t = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    if not len(a) or not len(t):
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    a_rad, t_rad = 0.5 * np.hypot(a[:, 2], a[:, 3]), 0.5 * np.hypot(t[:, 2], t[:, 3])
    a_area, t_area = a[:, 2] * a[:, 3], t[:, 2] * t[:, 3]
    tc = _corners(t)
    ii, jj, vv = [], [], []
    for j in range(len(t)):
        near = np.nonzero(np.hypot(t[j, 0] - a[:, 0], t[j, 1] - a[:, 1]) < t_rad[j] + a_rad)[0]
        if not len(near):
            continue
        ac = _corners(a[near])
        for q, i in enumerate(near):
            inter = _intersection_area(ac[q], tc[j])
            union = a_area[i] + t_area[j] - inter
            ii.append(i)
            jj.append(j)
            vv.append(inter / union if union > 0 else 0.0)
    ii, jj, vv = np.asarray(ii, np.int64), np.asarray(jj, np.int64), np.asarray(vv, np.float64)
    order = np.lexsort((jj, ii))
    return ii[order], jj[order], vv[order]


def host_assign_targets(anchors, gt_boxes, gt_count, pos_thr=0.6, neg_thr=0.45, force_match=True, pairs=None):
    """numpy / float64 reference of assign_targets (the rule dn_assign_targets runs): anchors [..., 6], gt_boxes [N, G, 6],
    gt_count [N] (numpy or tensors) -> {"labels" [N, P, 2] float32, "reg_targets" [N, P, 6] float32, "reg_loss_mask" [N, P]
    float32, "matched_gt" [N, P] int32, "best_iou" [N, P] float64} with P the number of anchors.  `pairs`: per image
    host_pair_ious(anchors, the image's boxes), for a caller that has computed them already (they are the whole cost)."""
    pos_thr, neg_thr = _check_thrs(pos_thr, neg_thr)
    anchors = np.asarray(_host(anchors), dtype=np.float32).reshape(-1, 6)
    gt_boxes, gt_count = np.asarray(_host(gt_boxes), dtype=np.float32), _host(gt_count)
    n, g = gt_boxes.shape[0], gt_boxes.shape[1]
    p = len(anchors)
    labels = np.zeros((n, p, 2), np.float32)
    reg = np.zeros((n, p, 6), np.float32)
    mask = np.zeros((n, p), np.float32)
    matched = np.full((n, p), -1, np.int32)
    best_iou = np.zeros((n, p), np.float64)
    for img in range(n):
        gc = min(max(int(gt_count[img]), 0), g)
        ii, jj, vv = pairs[img] if pairs is not None else host_pair_ious(anchors, gt_boxes[img, :gc])
        best_j = np.full(p, -1, np.int64)
        row_max = np.zeros(gc, np.float64)
        row_arg = np.full(gc, -1, np.int64)
        for i, j, v in zip(ii.tolist(), jj.tolist(), vv.tolist()):      # by anchor, then row: strict > keeps the lowest
            if v > best_iou[img, i]:
                best_iou[img, i], best_j[i] = v, j
            if v > row_max[j]:
                row_max[j], row_arg[j] = v, i
        target = np.where(best_iou[img] >= pos_thr, best_j, -1)
        negative = best_iou[img] < neg_thr
        if force_match:
            for j in range(gc - 1, -1, -1):                             # descending: the lowest row writes last and wins
                if row_arg[j] >= 0:
                    target[row_arg[j]] = j
        pos = np.nonzero(target >= 0)[0]
        labels[img, negative, 0] = 1.0
        labels[img, pos] = (0.0, 1.0)
        mask[img, pos] = 1.0
        matched[img] = target
        if len(pos):
            reg[img, pos] = encode_boxes(gt_boxes[img, target[pos]], anchors[pos]).astype(np.float32)
    return {"labels": labels, "reg_targets": reg, "reg_loss_mask": mask, "matched_gt": matched, "best_iou": best_iou}
