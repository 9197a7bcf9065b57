"""Seeded and crafted cases for the mAP tests (tests/test_ap_host_cpu.py, tests/test_gpu_ap.py).  TEST infrastructure."""
import math

import numpy as np

THRS = (0.5, 0.7)
MARGIN = 1e-9


def make(seed, n_img=20, n_gt=24, dup=0.3, fp=10, quant=64, pitch=10.0):
    """Per-image lists (detections [n, 6], scores [n], ground truth [g, 6]).  pitch 10: separated ground truth; pitch 3.5:
    a crowd in which detections overlap several boxes.  Scores are quantised to 1/64 so that ties occur inside and across
    images; every seventh image has no ground truth, every fifth no false positives; 15 % of the boxes are missed, 30 %
    detected twice; the detections' (sin, cos) codes have length 1.7."""
    r = np.random.default_rng(seed)
    dets, scs, gts = [], [], []
    for i in range(n_img):
        g = n_gt if i % 7 else 0
        cells = r.permutation(36)[:g]
        gt = np.zeros((g, 6), np.float32)
        gt[:, 0] = (cells // 6) * pitch - 2.5 * pitch + r.uniform(-0.2, 0.2, g) * pitch
        gt[:, 1] = (cells % 6) * pitch - 2.5 * pitch + r.uniform(-0.2, 0.2, g) * pitch
        gt[:, 2] = r.uniform(1.6, 2.4, g)
        gt[:, 3] = r.uniform(3.5, 5.5, g)
        yaw = r.uniform(-math.pi, math.pi, g)
        gt[:, 4], gt[:, 5] = np.sin(yaw), np.cos(yaw)
        rows = []
        for j in range(g):
            if r.random() < 0.15:
                continue
            for _ in range(1 + (r.random() < dup) + (r.random() < dup / 3)):
                b = gt[j].copy()
                b[:2] += r.normal(0, 0.35, 2)
                b[2:4] *= np.exp(r.normal(0, 0.08, 2))
                y = yaw[j] + r.normal(0, 0.06)
                b[4], b[5] = 1.7 * math.sin(y), 1.7 * math.cos(y)
                rows.append(b)
        for _ in range(fp if i % 5 else 0):
            y = r.uniform(-3, 3)
            e = 3 * pitch
            rows.append(np.array([r.uniform(-e, e), r.uniform(-e, e), 2, 4.5, math.sin(y), math.cos(y)], np.float32))
        d = np.asarray(rows, np.float32).reshape(-1, 6)
        s = (np.floor(r.random(len(d)) * quant) / quant).astype(np.float32)
        p = r.permutation(len(d))
        dets.append(d[p])
        scs.append(s[p])
        gts.append(gt)
    return dets, scs, gts


def padded(dets, scs, gts, k=None, g=None):
    """the lists as ({"boxes", "scores", "count"}, gt_boxes, gt_count) numpy arrays"""
    from disconet_amd import postprocess as P
    gb, gc = P.pad_boxes(gts, g)
    return P.pad_detections(dets, scs, k), gb, gc


def lists(det, gt_boxes, gt_count):
    """the padded arrays back as the oracle's per-image lists"""
    b, s, c = np.asarray(det["boxes"]), np.asarray(det["scores"]), np.asarray(det["count"])
    gb, gc = np.asarray(gt_boxes), np.asarray(gt_count)
    n = len(c)
    return ([b[i, :c[i]] for i in range(n)], [s[i, :c[i]] for i in range(n)], [gb[i, :gc[i]] for i in range(n)])


def margins(det, gt_boxes, gt_count, thrs=THRS):
    """(smallest |best IoU - threshold|, smallest gap between a detection's two largest IoUs) over every detection with a
    positive IoU, on the product's host arithmetic: the precondition under which a last-bit difference between two fp64
    formulations cannot decide a match."""
    from disconet_amd import postprocess as P
    to_thr, gap = math.inf, math.inf
    dets, _, gts = lists(det, gt_boxes, gt_count)
    for d, t in zip(dets, gts):
        if not len(d) or not len(t):
            continue
        d, t = d.astype(np.float64), t.astype(np.float64)
        dc, tc = P._corners(d), P._corners(t)
        t_rad = 0.5 * np.hypot(t[:, 2], t[:, 3])
        for i in range(len(d)):
            near = np.nonzero(np.hypot(t[:, 0] - d[i, 0], t[:, 1] - d[i, 1]) < t_rad + 0.5 * math.hypot(d[i, 2], d[i, 3]))[0]
            ious = [0.0, 0.0]
            for j in near:
                inter = P._intersection_area(dc[i], tc[j])
                union = d[i, 2] * d[i, 3] + t[j, 2] * t[j, 3] - inter
                ious.append(inter / union if union > 0 else 0.0)
            ious.sort()
            if ious[-1] > 0:
                gap = min(gap, ious[-1] - ious[-2])
                to_thr = min([to_thr] + [abs(ious[-1] - thr) for thr in thrs])
    return to_thr, gap


def assert_margins(det, gt_boxes, gt_count, what, thrs=THRS):
    to_thr, gap = margins(det, gt_boxes, gt_count, thrs)
    print("%s: smallest |best - t| %.3g, smallest top-two gap %.3g" % (what, to_thr, gap))
    assert to_thr > MARGIN and gap > MARGIN, (what, to_thr, gap)


def _box(x, y, w, h, s=0.0, c=1.0):
    return [x, y, w, h, s, c]


def crafted():
    """Exact cases in dyadic coordinates (axis-aligned: the fp64 geometry is exact).  Returns (dets, scores, gts,
    expected) with expected[img] = (best_gt per row, best_iou per row, tp@0.5 per row, tp@0.7 per row)."""
    dets, scs, gts, exp = [], [], [], []
    # 0: a 1x4 box inside a 2x4 ground truth: IoU exactly 0.5 -> true positive at 0.5 (>=), not at 0.7
    dets.append([_box(0.5, 0, 1, 4)]); scs.append([0.9]); gts.append([_box(0, 0, 2, 4)])
    exp.append(([0], [0.5], [1], [0]))
    # 1: two identical ground truths -> the lower index
    dets.append([_box(8, 8, 2, 4)]); scs.append([0.5]); gts.append([_box(20, 20, 2, 4), _box(8, 8, 2, 4), _box(8, 8, 2, 4)])
    exp.append(([1], [1.0], [1], [1]))
    # 2: three detections on one ground truth, scores 0.9, 0.9, 0.8 -> only row 0 is a true positive
    dets.append([_box(0, 0, 2, 4)] * 3); scs.append([0.9, 0.9, 0.8]); gts.append([_box(0, 0, 2, 4)])
    exp.append(([0, 0, 0], [1.0, 1.0, 1.0], [1, 0, 0], [1, 0, 0]))
    # 3: ground truth and no detections: counts in n_gt
    dets.append([]); scs.append([]); gts.append([_box(0, 0, 2, 4), _box(16, 0, 2, 4)])
    exp.append(([], [], [], []))
    # 4: zero-area detection on a ground truth, a detection on a zero-area ground truth: never match
    dets.append([_box(0, 0, 0, 4), _box(16, 0, 2, 4)]); scs.append([0.75, 0.25])
    gts.append([_box(0, 0, 2, 4), _box(16, 0, 2, 0)])
    exp.append(([-1, -1], [0.0, 0.0], [0, 0], [0, 0]))
    # 5: un-normalised (sin, cos) codes: (0, 1.7) is yaw 0, (1.7, 0) turns a 4x2 box into the 2x4 ground truth; the
    #    third is the second rank on its ground truth at 0.5 (IoU 0.5) behind a higher score with IoU 1
    dets.append([_box(0, 0, 2, 4, 0, 1.7), _box(16, 0, 4, 2, 1.7, 0), _box(0.5, 0, 1, 4, 0, 0.25)]); scs.append([0.5, 0.5, 0.25])
    gts.append([_box(0, 0, 2, 4), _box(16, 0, 2, 4)])
    exp.append(([0, 1, 0], [1.0, 1.0, 0.5], [1, 1, 0], [1, 1, 0]))
    # 6: the lower score has the better box: at 0.7 only it qualifies, at 0.5 the higher score takes the ground truth
    dets.append([_box(0.5, 0, 1, 4), _box(0, 0, 2, 4)]); scs.append([0.75, 0.5]); gts.append([_box(0, 0, 2, 4)])
    exp.append(([0, 0], [0.5, 1.0], [1, 0], [0, 1]))
    as_np = lambda rows: [np.asarray(r, np.float32).reshape(-1, 6) for r in rows]   # noqa: E731
    return as_np(dets), [np.asarray(s, np.float32) for s in scs], as_np(gts), exp


def check_crafted(match, exp):
    """the expected discrete results of crafted() against a match dict of numpy arrays"""
    for img, (bg, bi, tp5, tp7) in enumerate(exp):
        c = len(bg)
        assert match["best_gt"][img, :c].tolist() == bg, (img, match["best_gt"][img, :c])
        assert match["best_iou"][img, :c].tolist() == bi, (img, match["best_iou"][img, :c])
        assert match["tp"][0, img, :c].tolist() == tp5, (img, match["tp"][0, img, :c])
        assert match["tp"][1, img, :c].tolist() == tp7, (img, match["tp"][1, img, :c])
        assert (match["best_gt"][img, c:] == -1).all() and not match["best_iou"][img, c:].any()
        assert (match["rank"][img, c:] == -1).all() and not match["tp"][:, img, c:].any()


def oracle_ap(dets, scs, gts, thr):
    from oracle import postprocess_ref as R
    return R.average_precision(dets, scs, gts, thr)


def host_ap(det, gt_boxes, gt_count, thrs=THRS, match=None):
    """[AP per threshold] of one padded call through the product's host reference"""
    from disconet_amd import postprocess as P
    match = match or P.host_match_ground_truth(det, gt_boxes, gt_count, thrs)
    s, tp, _ = P.records_from_match(det, match)
    return [P.average_precision_from_records(s, tp[t], int(np.asarray(gt_count).sum())) for t in range(len(thrs))]


def bits(x):
    return np.float64(x).view(np.uint64)
