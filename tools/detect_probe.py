#!/usr/bin/env python
"""Time the detection tail at the bench batch (5 agents x 4 scenes, 256x256, K = 300): detect() eager and inside a
captured step (device events), the forward alone and forward + detect as graphs, and the host tail
(postprocess.host_detections) on the same outputs.  Prints one JSON line.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own (--iters 20)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from disconet_amd import Config, Detector, graph, postprocess  # noqa: E402
from disconet_amd.synthetic import make_scene_batch  # noqa: E402
from disconet_amd.profiling import events_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--top_k", type=int, default=300)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host_reps", type=int, default=1)
    args = ap.parse_args(argv)
    det = Detector("disco", Config(map_hw=args.map_hw), args.agents, args.batch, pre_nms_top_k=args.top_k)
    bevs, trans, na = (t.cuda() for t in make_scene_batch(args.batch, args.agents, args.map_hw))
    forward = lambda: det.forward(bevs, trans, na)                                  # noqa: E731
    result = forward()
    tail = lambda: det.tail(result, trans, na)                                      # noqa: E731
    for _ in range(5):
        tail()
    torch.cuda.synchronize()
    eager_ms = events_ms(tail, args.iters)
    fwd = graph.GraphedStep(forward, range_guard=False)
    both = graph.GraphedStep(lambda: det(bevs, trans, na), range_guard=False)
    det_graph = graph.GraphedStep(tail, range_guard=False)
    fwd_ms, both_ms, det_graph_ms = [], [], []
    for _ in range(3):                  # alternate the three graphs: the host shares its GPU with other work
        fwd_ms.append(events_ms(fwd, args.iters))
        both_ms.append(events_ms(both, args.iters))
        det_graph_ms.append(events_ms(det_graph, args.iters))
    counts = tail()["count"].cpu().tolist()
    host_s = []
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        postprocess.host_detections(result, det.anchors, pre_nms_top_k=args.top_k)
        host_s.append(time.perf_counter() - t0)
    out = {
        "images": args.agents * args.batch, "top_k": args.top_k, "counts": counts,
        "detect_eager_ms": round(eager_ms, 4),
        "detect_graph_ms": round(min(det_graph_ms), 4),
        "forward_graph_ms": round(min(fwd_ms), 4),
        "forward_detect_graph_ms": round(min(both_ms), 4),
        "graph_overhead_frac": round(min(both_ms) / min(fwd_ms) - 1.0, 4),
        "host_tail_ms": round(1e3 * min(host_s), 2),
        "host_speedup_vs_eager": round(1e3 * min(host_s) / eager_ms, 1),
        "host_cpus": len(os.sched_getaffinity(0)), "torch_threads": torch.get_num_threads(),
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
