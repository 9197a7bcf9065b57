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

from disconet_amd import Config, DiscoNet, graph, postprocess  # noqa: E402
from disconet_amd.synthetic import make_scene_batch, randomize_bn_stats  # noqa: E402


def _events_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--top_k", type=int, default=300)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host_reps", type=int, default=1)
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    cfg = Config(map_hw=args.map_hw)
    model = DiscoNet(cfg, kd_flag=0, num_agent=args.agents)
    randomize_bn_stats(model)
    model.eval().cuda()
    anchors = postprocess.make_anchors(cfg)
    bevs, trans, na = (t.cuda() for t in make_scene_batch(args.batch, args.agents, args.map_hw))

    def forward():
        with torch.no_grad():
            out = model(bevs, trans, na, args.batch)
        return out[0] if isinstance(out, tuple) else out

    result = forward()
    tail = lambda: postprocess.detect(result, anchors, pre_nms_top_k=args.top_k)    # noqa: E731
    for _ in range(5):
        tail()
    torch.cuda.synchronize()
    eager_ms = _events_ms(tail, args.iters)
    fwd = graph.GraphedStep(forward, range_guard=False)
    both = graph.GraphedStep(lambda: postprocess.detect(forward(), anchors, pre_nms_top_k=args.top_k),
                             range_guard=False)
    det_graph = graph.GraphedStep(tail, range_guard=False)
    fwd_ms, both_ms, det_graph_ms = [], [], []
    for _ in range(3):                  # alternate the three graphs: the host shares its GPU with other work
        fwd_ms.append(_events_ms(fwd, args.iters))
        both_ms.append(_events_ms(both, args.iters))
        det_graph_ms.append(_events_ms(det_graph, args.iters))
    counts = tail()["count"].cpu().tolist()
    host_s = []
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        postprocess.host_detections(result, anchors, pre_nms_top_k=args.top_k)
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
