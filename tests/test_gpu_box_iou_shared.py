"""What the shared pair body of rot_iou_device.h guarantees, on the MI355X: dn_assign_targets, dn_ap_match and the NMS
of dn_late_fuse stage a box, test the circumscribed circles and compute an IoU with the same code, so for the same
(box, column) pair they give the same float64 bits -- not merely values within the 1e-11 that each keeps to its host
reference (tests/test_gpu_assign.py, tests/test_gpu_ap.py; ocml's hypot and numpy's may differ in the last bit).

The shapes are the smallest that reach every edge of the shared code: 130 rows are three 64-lane blocks, the last with
two live lanes; 65 ground-truth rows are two assign chunks (64 + 1) and five 16-column pieces, the last holding one
column; 17 rows are two pieces; 0 rows is the early exit.  The rows behind the counts hold NaN, infinities and 1e30."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IOU_BAR = 1e-11                 # the bar of tests/test_gpu_assign.py and tests/test_gpu_ap.py
COUNTS = (65, 17, 0)
ROWS = 130
NMS_PAIRS = 16
GARBAGE = np.array([[np.nan] * 6, [0, 0, np.inf, 4, 0, 1], [0, 0, 1e30, 1e30, 0.6, 0.8], [1, 1, 2, 4, 0, 0]], np.float32)


def _draw(r, n):
    """n car-sized boxes (the sizes of assign_cases.crowd) with centres ~ U(-12, 12) m and any yaw"""
    b = np.zeros((n, 6), np.float32)
    yaw = r.uniform(-np.pi, np.pi, n)
    b[:, 0:2] = r.uniform(-12.0, 12.0, (n, 2))
    b[:, 2] = r.uniform(1.6, 2.4, n)
    b[:, 3] = r.uniform(3.5, 5.5, n)
    b[:, 4], b[:, 5] = np.sin(yaw), np.cos(yaw)
    return b


@functools.lru_cache(maxsize=None)
def _case():
    """(rows [130, 6], det, gt_boxes [3, 65, 6], gt_count [3], host_match_ground_truth's result, host_assign_targets')"""
    from disconet_amd import postprocess as P, targets as T
    r = np.random.default_rng(0)
    g = max(COUNTS)
    gb = np.zeros((len(COUNTS), g, 6), np.float32)
    for i, c in enumerate(COUNTS):                       # the ground truth first, then the rows
        gb[i, :c] = _draw(r, c)
        gb[i, c:] = GARBAGE[np.arange(g - c) % len(GARBAGE)]
    gc = np.asarray(COUNTS, np.int32)
    rows = _draw(r, ROWS)
    n = len(COUNTS)
    det = {"boxes": np.repeat(rows[None], n, 0).copy(), "count": np.full(n, ROWS, np.int32),
           "scores": np.repeat(np.linspace(0.99, 0.01, ROWS, dtype=np.float32)[None], n, 0).copy()}
    host_m = P.host_match_ground_truth(det, gb, gc)
    host_a = T.host_assign_targets(rows, gb, gc)         # force match: assign_arg computes every row's best pairs again
    # conditions on the inputs, nothing about the device: the two host references agree to the bit, and most rows overlap
    assert np.array_equal(host_m["best_iou"].view(np.uint64), host_a["best_iou"].view(np.uint64))
    assert (host_m["best_iou"] > 0).sum(1).tolist() == [126, 94, 0]
    return rows, det, gb, gc, host_m, host_a


@functools.lru_cache(maxsize=None)
def _device():
    """(match_ground_truth's result, assign_targets' with want_match) as numpy"""
    from disconet_amd import postprocess as P, targets as T
    rows, det, gb, gc, _, _ = _case()
    b, c = torch.as_tensor(gb).cuda(), torch.as_tensor(gc).cuda()
    m = P.match_ground_truth({k: torch.as_tensor(v).cuda() for k, v in det.items()}, b, c)
    a = T.assign_targets(torch.as_tensor(rows.reshape(1, ROWS, 1, 6)).cuda(), b, c, want_match=True)
    return {k: v.cpu().numpy() for k, v in m.items()}, {k: v.cpu().numpy() for k, v in a.items()}


def test_assign_and_ap_match_give_the_same_best_iou_bits():
    _, _, _, _, host_m, host_a = _case()
    dev_m, dev_a = _device()
    assert dev_m["best_iou"].dtype == np.float64 and dev_a["best_iou"].dtype == np.float64
    differ = dev_m["best_iou"].view(np.uint64) != dev_a["best_iou"].view(np.uint64)
    err_m = float(np.abs(dev_m["best_iou"] - host_m["best_iou"]).max())
    err_a = float(np.abs(dev_a["best_iou"] - host_a["best_iou"]).max())
    print("best_iou: %d of %d words differ between assign_targets and match_ground_truth; largest |device - host| "
          "%.3g (match), %.3g (assign)" % (int(differ.sum()), differ.size, err_m, err_a))
    assert not differ.any()
    assert err_m <= IOU_BAR and err_a <= IOU_BAR


def test_best_gt_equals_the_host():
    _, _, _, _, host_m, host_a = _case()
    dev_m, dev_a = _device()
    assert np.array_equal(dev_m["best_gt"], host_m["best_gt"])
    assert np.array_equal(dev_a["matched_gt"], host_a["matched_gt"])


def _two_rows(rows, gb, i, j):
    return np.stack([rows[i], gb[0, j]])[None], np.asarray([[0.9, 0.5]], np.float32)


def test_nms_suppresses_at_any_threshold_below_the_matched_iou():
    """A detection matched at IoU v and its ground-truth box, as the two rows of one image: the comparison is strict, so
    iou_thr = v keeps both and the next float64 below v keeps one.  nms_rotated does the same with the host's v."""
    from disconet_amd import postprocess as P
    rows, _, gb, _, host_m, _ = _case()
    dev_m, _ = _device()
    picked = np.nonzero(dev_m["best_iou"][0] > 0)[0][:NMS_PAIRS]
    assert len(picked) == NMS_PAIRS
    trans = torch.eye(4).reshape(1, 1, 1, 4, 4).cuda()
    live = torch.ones(1, dtype=torch.int32).cuda()
    one = np.ones(1, np.int32)
    for i in picked.tolist():
        j = int(dev_m["best_gt"][0, i])
        boxes, scores = _two_rows(rows, gb, i, j)
        hv = float(host_m["best_iou"][0, i])
        assert len(P.nms_rotated(boxes[0], scores[0], hv)) == 2 and len(P.nms_rotated(boxes[0], scores[0], np.nextafter(hv, 0.0))) == 1
        det = {"boxes": torch.as_tensor(boxes).cuda(), "scores": torch.as_tensor(scores).cuda(),
               "count": torch.as_tensor(2 * one).cuda()}
        v = float(dev_m["best_iou"][0, i])
        kept = [int(P.late_fuse(det, trans, live, 1, 1, iou_thr=t)["count"].item()) for t in (v, float(np.nextafter(v, 0.0)))]
        assert kept == [2, 1], (i, j, v, kept)
