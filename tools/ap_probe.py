#!/usr/bin/env python
"""Time the mAP step at the bench batch (5 agents x 4 scenes, 256x256, K = 300) for G = 64 and G = 256 ground-truth rows
from synthetic.make_gt_boxes: MeanAP.update() (dn_ap_match: match + accumulate) eager and as a captured graph (device
events), postprocess.host_match_ground_truth for the same call on the host, and forward + detect + update as one graph
against forward + detect alone.  --nms_iou 1.0 keeps every one of the K rows valid (the NMS suppresses nothing): the
step's cost with full rows.  Prints one JSON line.  Per-kernel times: run this under `rocprofv3 --kernel-trace
--stats` in a run of its own (--iters 20)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from disconet_amd import Config, Detector, graph, postprocess  # noqa: E402
from disconet_amd.synthetic import make_gt_boxes, make_scene_batch  # noqa: E402
from disconet_amd.profiling import events_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--top_k", type=int, default=300)
    ap.add_argument("--gt_rows", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--nms_iou", type=float, default=0.01, help="detect()'s iou_thr; 1.0 keeps all top_k rows of every image")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host_reps", type=int, default=1)
    args = ap.parse_args(argv)
    detector = Detector("disco", Config(map_hw=args.map_hw), args.agents, args.batch, pre_nms_top_k=args.top_k,
                        iou_thr=args.nms_iou)
    bevs, trans, na = (t.cuda() for t in make_scene_batch(args.batch, args.agents, args.map_hw))
    n = args.agents * args.batch
    forward_detect = lambda: detector(bevs, trans, na)                               # noqa: E731
    det = forward_detect()
    counts = det["count"].cpu().tolist()
    out = {"images": n, "top_k": args.top_k, "nms_iou": args.nms_iou, "counts": counts, "iters": args.iters,
           "host_cpus": len(os.sched_getaffinity(0)), "torch_threads": torch.get_num_threads(), "gt": {}}
    both = graph.GraphedStep(forward_detect, range_guard=False)
    for g in args.gt_rows:
        gt_boxes, gt_count = (t.cuda() for t in make_gt_boxes(n, seed=0, max_boxes=g))
        metric = postprocess.MeanAP(args.batch, capacity=(args.iters + 8) * n * args.top_k)
        update = lambda: metric.update(det, gt_boxes, gt_count)                      # noqa: E731
        for _ in range(5):
            update()
        metric.reset()
        torch.cuda.synchronize()
        eager_ms = events_ms(update, args.iters)
        up_graph = graph.GraphedStep(update, range_guard=False)
        full = graph.GraphedStep(lambda: metric.update(forward_detect(), gt_boxes, gt_count), range_guard=False)
        up_ms, both_ms, full_ms = [], [], []
        for _ in range(3):                  # alternate the graphs: the host shares its GPU with other work
            metric.reset()
            up_ms.append(events_ms(up_graph, args.iters))
            both_ms.append(events_ms(both, args.iters))
            metric.reset()
            full_ms.append(events_ms(full, args.iters))
        metric.reset()
        match = update()
        res = metric.compute()
        host_s = []
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            postprocess.host_match_ground_truth(det, gt_boxes, gt_count)
            host_s.append(time.perf_counter() - t0)
        out["gt"][str(g)] = {
            "gt_boxes": int(gt_count.sum()), "matched_rows": int((match["best_gt"] >= 0).sum()),
            "true_positives": [int(v) for v in match["tp"].sum(dim=(1, 2)).tolist()],
            "mAP@0.5": res["mAP@0.5"], "mAP@0.7": res["mAP@0.7"],
            "update_eager_ms": round(eager_ms, 4), "update_graph_ms": round(min(up_ms), 4),
            "forward_detect_graph_ms": round(min(both_ms), 4), "forward_detect_update_graph_ms": round(min(full_ms), 4),
            "graph_overhead_frac": round(min(full_ms) / min(both_ms) - 1.0, 4),
            "host_match_ms": round(1e3 * min(host_s), 2),
            "host_over_graph": round(1e3 * min(host_s) / min(up_ms), 1),
        }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
