#!/usr/bin/env python
"""test_codet.py's evaluation run with the metric: the same flags, model and synthetic scenes; per frame the forward, the
detection tail (postprocess.detect) and MeanAP.update() -- all on the GPU, nothing read back -- and after the last frame
mAP@0.5 and mAP@0.7 per agent and overall, as the reference's test_codet.py prints them.

    python tools/det/eval_codet.py --com disco|sum|mean|max|lowerbound|late|agent [--resume ckpt.pth] [--num_agent 5] [--batch 1] [--frames 4] \
        [--pre_nms_top_k 300] [--iou_thr 0.01] [--score_thr T] [--gt synthetic|self|scene] \
        [--strata none|range|visibility] [--strata_edges 10,20] [--exchange f32|f16|mxfp8|mxfp4] [--exchange_cells N]

--gt synthetic: frame f is scored against synthetic.make_gt_boxes(images, seed=f, max_boxes=64) -- seeded boxes that
    have nothing to do with the synthetic occupancy (there is no V2X-Sim data here): the figure checks the plumbing, not
    the detector.
--gt self: every frame's detections are their own ground truth.  At the default --iou_thr 0.01 every kept box has IoU 1
    with itself and at most 0.01 with every other, so both figures are 1.0000: a smoke check that needs no labels.
--gt scene: frame f is synthetic.make_box_scene_batch(seed=f) -- occupancy that shows the scene's own boxes -- scored
    against those boxes: after `train_codet.py --targets boxes --logpath L`, `--gt scene --resume L/epoch_N.pth` prints an
    mAP that belongs to the detector.

--exchange f16|mxfp8|mxfp4 (--com disco): the neighbours' feature maps go through the wire format (disconet_amd.exchange:
    encoded and decoded on the GPU inside the forward); one more line gives the message bytes per agent per frame.

--exchange_cells N (--com disco): an agent sends only the N strongest cells of its map, in the --exchange format (f32
    included); the others arrive as zeros.  Two more lines: the capacity message's bytes, and after the run the mean cells
    sent and the bytes a variable-length link would have carried, from one read of the model's exchange_sent.

--com lowerbound: no collaboration.  --com late: the lowerbound detector (train `--com lowerbound`, pass its checkpoint)
    with postprocess.late_fuse between detect() and the metric: the agents' boxes merged in each ego's frame
    (disconet_amd.Detector owns the model, the checkpoint and that tail).

--strata range|visibility: the metric per stratum of the ground truth (postprocess.StratifiedAP in MeanAP's place, still
    nothing read back per frame).  range: the box centre's distance from the ego, edges in metres (default 10,20: three
    strata).  visibility: the image's own returns on the box (--scene lidar --gt scene only), default edge 5 = the
    scenes' min_points: stratum 0 holds the boxes an ego can only learn of through collaboration.  The per-agent and
    overall lines come from the "all" row; one line per stratum follows.  A detection that reaches a box of another
    stratum is left out of a stratum's row, not counted as a false positive (postprocess.stratified_ap_from_records).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from disconet_amd import ALL_DET_COM_MODES, Config, postprocess  # noqa: E402
from disconet_amd.synthetic import make_box_scene_batch, make_gt_boxes, make_scene_batch  # noqa: E402
from codet_common import add_exchange_flag, add_tail_flags, agents_of, exchange_line, exchange_sent_line, exchanges, detector_from_args, lidar_scene, require_com  # noqa: E402
from test_codet import build_parser  # noqa: E402  (the evaluation tool's command line)

GT_MAX_BOXES = 64


def build_eval_parser():
    ap = build_parser()
    add_tail_flags(ap, 300)
    add_exchange_flag(ap)
    ap.add_argument("--gt", choices=("synthetic", "self", "scene"), default="synthetic")
    ap.add_argument("--scene", choices=("boxes", "lidar"), default="boxes",
                    help="--gt scene: lidar = synthetic.make_lidar_scene_batch, ray-cast scans with occluders, scored against "
                         "the boxes that somebody in the scene sees")
    ap.add_argument("--strata", choices=("none", "range", "visibility"), default="none",
                    help="also print AP and recall per stratum of the ground truth: range from the ego, or the ego's own "
                         "returns on the box (visibility: --scene lidar --gt scene only)")
    ap.add_argument("--strata_edges", default=None,
                    help="comma-separated ascending edges: metres for range (default 10,20), returns for visibility (default 5)")
    return ap


STRATA_DEFAULT_EDGES = {"range": (10.0, 20.0), "visibility": (5.0,)}


def strata_edges_of(args):
    """the edges of --strata / --strata_edges, checked before anything is built"""
    if args.strata_edges is None:
        return list(STRATA_DEFAULT_EDGES[args.strata])
    try:
        edges = [float(v) for v in args.strata_edges.split(",")]
        postprocess.strata_names(args.strata, edges)
    except ValueError as e:
        raise SystemExit("--strata_edges %s: %s" % (args.strata_edges, e))
    return edges


def main(argv=None):
    args = build_eval_parser().parse_args(argv)
    if args.strata == "visibility" and not (args.scene == "lidar" and args.gt == "scene"):
        raise SystemExit("--strata visibility needs --scene lidar --gt scene: only the lidar scenes know how many returns "
                         "an ego's own scan put on a box")
    if args.tracking or args.visualization:
        print("note: --tracking / --visualization are accepted for compatibility; this tool prints the metric")
    require_com(args, ALL_DET_COM_MODES)
    if args.scene == "lidar" and args.gt != "scene":
        raise SystemExit("--scene lidar needs --gt scene: the lidar scenes are scored against their own visible boxes")
    num_agent = agents_of(args)

    config = Config("test", binary=True, only_det=True)
    detector = detector_from_args(args, config)      # without --resume the weights are random: seeded, so that a run can be reproduced
    n_images = num_agent * args.batch
    capacity = max(1, args.frames * n_images * args.pre_nms_top_k)
    if args.strata == "none":
        metric = postprocess.MeanAP(args.batch, capacity=capacity)
    else:
        edges = strata_edges_of(args)
        names = postprocess.strata_names(args.strata, edges)
        metric = postprocess.StratifiedAP(args.batch, len(names), names=names, capacity=capacity)

    for frame in range(args.frames):
        if args.gt == "scene":
            if args.scene == "lidar":
                scene = lidar_scene(args.batch, num_agent, config.map_dims[0], frame, GT_MAX_BOXES)
            else:
                scene = make_box_scene_batch(args.batch, num_agent, config.map_dims[0], seed=frame, boxes_per_scene=GT_MAX_BOXES,
                                             device="cuda")
            bevs, trans, na = scene["bev_seq"], scene["trans_matrices"], scene["num_agent"]
        else:
            bevs, trans, na = make_scene_batch(args.batch, num_agent, config.map_dims[0], jitter_seed=frame)
        det = detector(bevs.cuda(), trans.cuda(), na.cuda())
        if args.gt == "self":
            gt_boxes, gt_count = det["boxes"], det["count"]
        elif args.gt == "scene":
            gt_boxes, gt_count = scene["gt_boxes"], scene["gt_count"]
        else:
            gt_boxes, gt_count = (t.cuda() for t in make_gt_boxes(n_images, seed=frame, max_boxes=GT_MAX_BOXES))
        if args.strata == "none":
            metric.update(det, gt_boxes, gt_count)
        else:
            own = scene["gt_own_hits"] if args.strata == "visibility" else None
            metric.update(det, gt_boxes, gt_count, postprocess.gt_strata(gt_boxes, gt_count, args.strata, edges, own))

    res = metric.compute()
    strata = []
    if args.strata != "none":       # the lines below from the "all" row, under MeanAP's names
        strata = res["strata"]
        rows = [dict(row, **{"mAP@0.5": row["AP@0.5"], "mAP@0.7": row["AP@0.7"]}) for row in [res["all"]] + res["per_agent"]]
        res = dict(rows[0], per_agent=rows[1:])
    what = ("ground truth = the detections themselves" if args.gt == "self" else
            "ground truth = the boxes of the scenes%s" % ("" if args.resume else ", random weights") if args.gt == "scene" else
            "synthetic ground truth%s: plumbing, not accuracy" % ("" if args.resume else " and random weights"))
    print("%d frames x %d images (%s)" % (args.frames, n_images, what))
    if exchanges(args):
        print(exchange_line(args, config))
    if args.exchange_cells:
        print(exchange_sent_line(args, detector))
    for a, row in enumerate(res["per_agent"]):
        print("agent %d: mAP@0.5 %.4f  mAP@0.7 %.4f  (%d detections, %d ground-truth boxes, true positives %d / %d)" % (
            a, row["mAP@0.5"], row["mAP@0.7"], row["n_det"], row["n_gt"], row["n_tp"][0], row["n_tp"][1]))
    print("overall: mAP@0.5 %.4f  mAP@0.7 %.4f  (%d detections, %d ground-truth boxes, true positives %d / %d)" % (
        res["mAP@0.5"], res["mAP@0.7"], res["n_det"], res["n_gt"], res["n_tp"][0], res["n_tp"][1]))
    for s, row in enumerate(strata):
        print("stratum %d, %s: AP@0.5 %.4f  AP@0.7 %.4f  recall %.4f / %.4f  (%d ground-truth boxes, detections counted "
              "%d / %d, left out %d / %d)" % (
                  s, row["name"], row["AP@0.5"], row["AP@0.7"], row["recall@0.5"], row["recall@0.7"], row["n_gt"],
                  row["n_counted"][0], row["n_counted"][1], row["n_left_out"][0], row["n_left_out"][1]))


if __name__ == "__main__":
    main()
