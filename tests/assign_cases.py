"""Seeded and crafted cases for the target-assignment tests (tests/test_assign_host_cpu.py, tests/test_gpu_assign.py).
TEST infrastructure."""
import math

import numpy as np

MARGIN = 1e-9
POS, NEG = 0.6, 0.45

# (map_hw, boxes per image, seed): the seeds were picked on the CPU so that the host reference itself keeps every decision
# MARGIN away from flipping (margins() below); nothing is filtered out of a case.  host_pair_ious runs about 13 000 polygon
# clips a second and a car box meets about 12 000 anchors of a 0.25 m grid: each case is sized to about a minute of it.
CROWD_64 = (64, (64, 0, 8), 2)
CROWD_128 = (128, (16, 0, 24, 8), 6)
GRID_256 = (256, (4, 4), 1)


def crowd(map_hw, counts, seed, garbage=False):
    """(anchors [H, W, 6, 6] float32 numpy, gt_boxes [N, G, 6], gt_count [N]): per image `counts[i]` car-sized boxes with
    centres ~ U over the map less a 1 m rim and any yaw -- boxes overlap each other freely.  garbage: the rows behind the
    counts are filled with NaN, infinities and huge boxes."""
    from disconet_amd import Config, postprocess as P
    cfg = Config(map_hw=map_hw)
    anchors = P.make_anchors(cfg, device="cpu").numpy()
    half = float(cfg.area_extents[0][1])
    r = np.random.default_rng(seed)
    g = max(1, max(counts))
    boxes = np.zeros((len(counts), g, 6), np.float32)
    for i, c in enumerate(counts):
        yaw = r.uniform(-math.pi, math.pi, c)
        boxes[i, :c, 0:2] = r.uniform(-half + 1.0, half - 1.0, (c, 2))
        boxes[i, :c, 2] = r.uniform(1.6, 2.4, c)
        boxes[i, :c, 3] = r.uniform(3.5, 5.5, c)
        boxes[i, :c, 4], boxes[i, :c, 5] = np.sin(yaw), np.cos(yaw)
        if garbage:
            fill = np.array([[np.nan] * 6, [0, 0, np.inf, 4, 0, 1], [0, 0, 1e30, 1e30, 0.6, 0.8], [1, 1, 2, 4, 0, 0]], np.float32)
            boxes[i, c:] = fill[np.arange(g - c) % len(fill)]
    return anchors, boxes, np.asarray(counts, np.int32)


def pairs_of(anchors, gt_boxes, gt_count):
    from disconet_amd import targets as T
    return [T.host_pair_ious(anchors.reshape(-1, 6), gt_boxes[i, :int(gt_count[i])]) for i in range(len(gt_count))]


def margins(pairs, n_anchors, thrs=(POS, NEG)):
    """(smallest |an anchor's best IoU - a threshold|, smallest gap between an anchor's two largest IoUs, smallest gap
    between a box's two largest anchor IoUs) over the anchors / boxes with a positive IoU, on the host arithmetic.  For a
    box a missing second IoU counts as 0: its best anchor's IoU must itself be MARGIN above nothing, since "above 0" decides
    whether the box forces an anchor.  For an anchor only its positive IoUs compete (an IoU of 0 never matches), and an anchor
    with a single positive IoU has no second: whether that IoU is a sliver or 0 moves no label, mask or target -- both are
    far below neg_thr, and whether it is a row's largest is the box's margin."""
    to_thr, a_gap, b_gap = math.inf, math.inf, math.inf
    for ii, jj, vv in pairs:
        if not len(vv):
            continue
        for idx, cur in ((ii, "a"), (jj, "b")):
            order = np.lexsort((vv, idx))                       # by owner, IoU ascending within it
            o_idx, o_v = idx[order], vv[order]
            last = np.nonzero(np.append(o_idx[1:] != o_idx[:-1], True))[0]
            top = o_v[last]
            has2 = (last > 0) & (o_idx[np.maximum(last - 1, 0)] == o_idx[last])
            second = np.where(has2, o_v[np.maximum(last - 1, 0)], 0.0)
            live = top > 0
            if cur == "a":
                to_thr = min([to_thr] + [float(np.abs(top[live] - t).min()) for t in thrs if live.any()])
                live = live & (second > 0)
            if not live.any():
                continue
            gap = float((top - second)[live].min())
            if cur == "a":
                a_gap = min(a_gap, gap)
            else:
                b_gap = min(b_gap, gap)
    return to_thr, a_gap, b_gap


def assert_margins(pairs, n_anchors, what):
    to_thr, a_gap, b_gap = margins(pairs, n_anchors)
    print("%s: smallest |best - t| %.3g, smallest top-two gap per anchor %.3g, per box %.3g" % (what, to_thr, a_gap, b_gap))
    assert to_thr > MARGIN and a_gap > MARGIN and b_gap > MARGIN, (what, to_thr, a_gap, b_gap)


def _box(x, y, w, h, s=0.0, c=1.0):
    return [x, y, w, h, s, c]


def crafted():
    """Exact cases in dyadic coordinates (axis-aligned: the fp64 geometry is exact).  Returns (anchors [1, 5, 1, 6], gt_boxes
    [6, 2, 6], gt_count [6], expected) with expected[force][img] = {anchor: (matched_gt, best_iou, best row's label)}: the
    anchors not listed are negative with best_iou 0."""
    anchors = np.asarray([_box(0, 0, 2, 4), _box(0.25, 0, 2, 4), _box(15.5, 0, 2, 4), _box(17.5, 0, 2, 4),
                          _box(32, 0, 2, 4)], np.float32).reshape(1, 5, 1, 6)
    gts = [
        # 0: a box identical to anchor 4: IoU 1, positive, the code is zero but for tc = 1
        [_box(32, 0, 2, 4)],
        # 1: a 1x4 box inside anchor 4: IoU 0.5, between the thresholds -> don't care; it forces anchor 4 when forcing is on
        [_box(32.5, 0, 1, 4)],
        # 2: row 0 is anchor 1 itself and overlaps anchor 0 at 7/9 (a threshold match of anchor 0); row 1 overlaps anchor 0
        #    at 1/7 and anchor 1 at 1/15: it forces anchor 0, below pos_thr, over anchor 0's threshold match with row 0
        [_box(0.25, 0, 2, 4), _box(-1.5, 0, 2, 4)],
        # 3: two rows whose best anchor is anchor 4, at 1/15 and 1/7: the lower row wins the forced anchor
        [_box(30.25, 0, 2, 4), _box(33.5, 0, 2, 4)],
        # 4: one row at 1/3 with anchors 2 and 3 alike: the lower anchor index is forced
        [_box(16.5, 0, 2, 4)],
        # 5: no ground truth: everything is negative
        [],
    ]
    DC, NEGL, POSL = (0.0, 0.0), (1.0, 0.0), (0.0, 1.0)
    exp = {
        False: [{4: (0, 1.0, POSL)}, {4: (-1, 0.5, DC)}, {0: (0, 7 / 9, POSL), 1: (0, 1.0, POSL)}, {4: (-1, 1 / 7, NEGL)},
                {2: (-1, 1 / 3, NEGL), 3: (-1, 1 / 3, NEGL)}, {}],
        True: [{4: (0, 1.0, POSL)}, {4: (0, 0.5, POSL)}, {0: (1, 7 / 9, POSL), 1: (0, 1.0, POSL)}, {4: (0, 1 / 7, POSL)},
               {2: (0, 1 / 3, POSL), 3: (-1, 1 / 3, NEGL)}, {}],
    }
    from disconet_amd import postprocess as P
    gb, gc = P.pad_boxes([np.asarray(g, np.float32).reshape(-1, 6) for g in gts], 2)
    return anchors, gb, gc, exp


def check_crafted(res, exp_force, gt_boxes):
    """the expected results of crafted() against an assignment dict of numpy arrays ([N, P, ...] shapes)"""
    labels = np.asarray(res["labels"]).reshape(6, 5, 2)
    reg = np.asarray(res["reg_targets"]).reshape(6, 5, 6)
    mask = np.asarray(res["reg_loss_mask"]).reshape(6, 5)
    for img, rows in enumerate(exp_force):
        for a in range(5):
            m, iou, lab = rows.get(a, (-1, 0.0, (1.0, 0.0)))
            assert int(res["matched_gt"][img, a]) == m, (img, a, res["matched_gt"][img])
            assert float(res["best_iou"][img, a]) == iou, (img, a, res["best_iou"][img, a], iou)
            assert tuple(labels[img, a].tolist()) == lab, (img, a, labels[img, a])
            assert mask[img, a] == (1.0 if m >= 0 else 0.0)
            if m < 0:
                assert not reg[img, a].any()
    # codes of the exact positives: identical box -> (0, 0, 0, 0, 0, 1); the 1x4 box inside anchor 4 -> tx = 1/4, tw = log(1/2)
    assert reg[0, 4].tolist() == [0, 0, 0, 0, 0, 1]
    if exp_force[1][4][0] == 0:
        assert reg[1, 4].tolist() == [0.25, 0, float(np.float32(math.log(0.5))), 0, 0, 1]
