#!/usr/bin/env python
"""test_codet.py's evaluation run with detections: the same flags, model and synthetic scenes, and after every frame's
forward the detection tail on the GPU (postprocess.detect: top-k by score, rotated greedy NMS, one batched call).
Prints per frame the forward time, the per-image detection counts and the tail's device time (events).

    python tools/det/detect_codet.py --com disco|sum|mean|max|lowerbound|late|agent [--resume ckpt.pth] [--num_agent 5] [--batch 1] \
        [--pre_nms_top_k 300] [--iou_thr 0.01] [--score_thr T]

--com lowerbound: no collaboration, every agent detects from its own view.  --com late: that detector (pass a lowerbound
checkpoint), then postprocess.late_fuse merges the agents' boxes in each ego's frame (disconet_amd.Detector owns both).
Without --resume the weights are random: seeded before the model is built, so that a run can be reproduced.
"""
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from disconet_amd import ALL_DET_COM_MODES, Config  # noqa: E402
from disconet_amd.synthetic import make_scene_batch  # noqa: E402
from codet_common import add_exchange_flag, add_tail_flags, agents_of, detector_from_args, lidar_scene, require_com  # noqa: E402
from test_codet import build_parser  # noqa: E402  (the evaluation tool's command line)


def build_detect_parser():
    ap = build_parser()
    add_tail_flags(ap, 300)
    add_exchange_flag(ap)
    ap.add_argument("--scene", choices=("boxes", "lidar"), default="boxes",
                    help="boxes: the tool's seeded occupancy, as ever; lidar: synthetic.make_lidar_scene_batch(seed = frame), "
                         "ray-cast scans with occluders")
    return ap


def main(argv=None):
    args = build_detect_parser().parse_args(argv)
    if args.tracking or args.visualization:
        print("note: --tracking / --visualization are accepted for compatibility; this tool prints the detection counts")
    require_com(args, ALL_DET_COM_MODES)
    num_agent = agents_of(args)

    config = Config("test", binary=True, only_det=True)
    detector = detector_from_args(args, config)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for frame in range(args.frames):
        if args.scene == "lidar":
            seen = lidar_scene(args.batch, num_agent, config.map_dims[0], frame, 64)
            scene = tuple(seen[k] for k in ("bev_seq", "trans_matrices", "num_agent"))
        else:
            scene = make_scene_batch(args.batch, num_agent, config.map_dims[0], jitter_seed=frame)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bevs, trans, na = (t.cuda() for t in scene)
        result = detector.forward(bevs, trans, na)
        torch.cuda.synchronize()
        forward_ms = 1e3 * (time.perf_counter() - t0)
        start.record()
        det = detector.tail(result, trans, na)
        end.record()
        end.synchronize()
        print("frame %d: forward %.2f ms  detections per image %s  (top-k + rotated NMS%s on the GPU: %.3f ms)" % (
            frame, forward_ms, det["count"].tolist(), " + late fusion" if args.com == "late" else "", start.elapsed_time(end)))


if __name__ == "__main__":
    main()
