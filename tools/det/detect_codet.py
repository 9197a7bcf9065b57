#!/usr/bin/env python
"""test_codet.py's evaluation run with detections: the same flags, model and synthetic scenes, and after every frame's
forward the detection tail on the GPU (postprocess.detect: top-k by score, rotated greedy NMS, one batched call).
Prints per frame the forward time, the per-image detection counts and the tail's device time (events).

    python tools/det/detect_codet.py --com disco|sum|mean|max|lowerbound|late [--resume ckpt.pth] [--num_agent 5] [--batch 1] \
        [--pre_nms_top_k 300] [--iou_thr 0.01] [--score_thr T]

--com lowerbound: no collaboration, every agent detects from its own view.  --com late: that detector (pass a lowerbound
checkpoint), then postprocess.late_fuse merges the agents' boxes in each ego's frame.
"""
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from disconet_amd import DET_COM_MODES, Config, build_model, postprocess  # noqa: E402
from disconet_amd.synthetic import make_scene_batch, randomize_bn_stats  # noqa: E402
from test_codet import build_parser  # noqa: E402  (the evaluation tool's command line)


def main(argv=None):
    ap = build_parser()
    ap.add_argument("--pre_nms_top_k", type=int, default=300)
    ap.add_argument("--iou_thr", type=float, default=0.01)
    ap.add_argument("--score_thr", type=float, default=None)
    args = ap.parse_args(argv)
    if args.tracking or args.visualization:
        print("note: --tracking / --visualization are accepted for compatibility; this tool prints the detection counts")
    if args.com not in DET_COM_MODES:
        raise SystemExit("only --com disco | sum | mean | max | lowerbound | late are built on the MI355X path (SURVEY.md §2.1 #8)")
    num_agent = args.num_agent + (1 if args.rsu else 0)

    config = Config("test", binary=True, only_det=True)
    model = build_model(args.com, config, layer=args.layer, kd_flag=args.kd_flag, num_agent=num_agent,
                        compress_level=args.compress_level, only_v2i=bool(args.only_v2i))
    if args.resume:
        checkpoint = torch.load(args.resume, map_location="cpu", weights_only=False)
        model.load_state_dict(checkpoint["model_state_dict"])
        print("loaded", args.resume, "epoch", checkpoint.get("epoch"))
    else:
        torch.manual_seed(0)
        randomize_bn_stats(model)
    model.eval().cuda()
    anchors = postprocess.make_anchors(config)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for frame in range(args.frames):
        bevs, trans, na = make_scene_batch(args.batch, num_agent, config.map_dims[0], jitter_seed=frame)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = model(bevs.cuda(), trans.cuda(), na.cuda(), args.batch)
        torch.cuda.synchronize()
        forward_ms = 1e3 * (time.perf_counter() - t0)
        result = out[0] if isinstance(out, tuple) else out
        start.record()
        det = postprocess.detect(result, anchors, pre_nms_top_k=args.pre_nms_top_k, iou_thr=args.iou_thr,
                                 score_thr=args.score_thr)
        if args.com == "late":            # every agent's boxes merged in each ego's frame, duplicates suppressed
            det = postprocess.late_fuse(det, trans.cuda(), na.cuda(), args.batch, num_agent, iou_thr=args.iou_thr,
                                        only_v2i=bool(args.only_v2i), extents=config.area_extents[:2])
        end.record()
        end.synchronize()
        print("frame %d: forward %.2f ms  detections per image %s  (top-k + rotated NMS%s on the GPU: %.3f ms)" % (
            frame, forward_ms, det["count"].tolist(), " + late fusion" if args.com == "late" else "", start.elapsed_time(end)))


if __name__ == "__main__":
    main()
