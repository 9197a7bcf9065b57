#!/usr/bin/env python
"""Time the stratified mAP step beside the plain one: 20 images x K = 300 rows (about 40 valid) x 64 ground-truth rows from
synthetic.make_gt_boxes, 2 strata by range.  StratifiedAP.update() (dn_ap_match_strata) and MeanAP.update() (dn_ap_match)
alternate window by window in the same run, eager and as graph replays; device events around each window of --iters calls,
the median of 7 windows after a warm-up window, and the windows themselves (their spread is the yardstick for the
difference).  A third pair of graphs adds gt_strata() in front of the stratified update.  Writes
profiles/strata_probe.json and prints it.  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run
of its own (--iters 20)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import _lib, graph, postprocess  # noqa: E402
from disconet_amd.profiling import events_ms  # noqa: E402
from disconet_amd.synthetic import make_gt_boxes  # noqa: E402

WINDOWS = 7


def detections(gt_boxes, gt_count, k, valid, seed):
    """per image `valid` rows: three quarters jittered copies of ground-truth boxes (duplicates included), the rest
    elsewhere; rows beyond the count are zero"""
    r = np.random.default_rng(seed)
    n = len(gt_count)
    boxes, scores = np.zeros((n, k, 6), np.float32), np.zeros((n, k), np.float32)
    for i in range(n):
        src = r.integers(0, max(1, int(gt_count[i])), valid)
        rows = gt_boxes[i, src].copy()
        rows[:, :2] += r.normal(0, 0.3, (valid, 2)).astype(np.float32)
        far = r.random(valid) < 0.25
        rows[far, :2] = r.uniform(-30, 30, (int(far.sum()), 2)).astype(np.float32)
        boxes[i, :valid] = rows
        scores[i, :valid] = r.random(valid).astype(np.float32)
    return {"boxes": torch.from_numpy(boxes).cuda(), "scores": torch.from_numpy(scores).cuda(),
            "count": torch.full((n,), valid, dtype=torch.int32).cuda()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--top_k", type=int, default=300)
    ap.add_argument("--valid", type=int, default=40)
    ap.add_argument("--gt_rows", type=int, default=64)
    ap.add_argument("--edge", type=float, default=20.0, help="the range edge between the two strata, metres")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strata_probe.json"))
    args = ap.parse_args(argv)
    n = args.agents * args.batch
    gt_boxes, gt_count = make_gt_boxes(n, seed=0, max_boxes=args.gt_rows)
    det = detections(gt_boxes.numpy(), gt_count.numpy(), args.top_k, args.valid, seed=1)
    gt_boxes, gt_count = gt_boxes.cuda(), gt_count.cuda()
    stratum = postprocess.gt_strata(gt_boxes, gt_count, "range", (args.edge,))
    capacity = (args.iters + 8) * n * args.valid
    strat = postprocess.StratifiedAP(args.batch, 2, capacity=capacity)
    plain = postprocess.MeanAP(args.batch, capacity=capacity)
    calls = {
        "stratified": lambda: strat.update(det, gt_boxes, gt_count, stratum),
        "plain": lambda: plain.update(det, gt_boxes, gt_count),
        "stratified_with_gt_strata": lambda: strat.update(
            det, gt_boxes, gt_count, postprocess.gt_strata(gt_boxes, gt_count, "range", (args.edge,))),
    }
    for fn in calls.values():
        fn()
    graphs = {name: graph.GraphedStep(fn, range_guard=False) for name, fn in calls.items()}
    timed = {"eager": calls, "graph": graphs}
    windows = {kind: {name: [] for name in calls} for kind in timed}
    for w in range(WINDOWS + 1):                # window 0 warms up; the three calls alternate inside every window round
        for kind, fns in timed.items():
            for name, fn in fns.items():
                strat.reset()
                plain.reset()
                torch.cuda.synchronize()
                ms = events_ms(fn, args.iters)
                if w:
                    windows[kind][name].append(round(ms, 4))
    # one counted update each: the figures the two metrics give on this input
    strat.reset()
    plain.reset()
    calls["stratified"]()
    calls["plain"]()
    res_s, res_p = strat.compute(), plain.compute()
    out = {"dn_version": int(_lib.load().dn_version()), "images": n, "top_k": args.top_k, "valid_rows_per_image": args.valid,
           "gt_rows": args.gt_rows, "gt_boxes": int(gt_count.sum()), "strata": 2, "range_edge_m": args.edge,
           "iters": args.iters, "windows": WINDOWS,
           "n_gt_per_stratum": [row["n_gt"] for row in res_s["strata"]],
           "AP@0.5": {"plain": res_p["mAP@0.5"], "all": res_s["all"]["AP@0.5"],
                      "strata": [row["AP@0.5"] for row in res_s["strata"]]},
           "all_equals_plain_bits": bool(np.float64(res_p["mAP@0.5"]).view(np.uint64) ==
                                         np.float64(res_s["all"]["AP@0.5"]).view(np.uint64))}
    for kind in timed:
        for name in calls:
            ws = windows[kind][name]
            out["%s_%s_call_ms" % (name, kind)] = round(statistics.median(ws), 4)
            out["%s_%s_windows_ms" % (name, kind)] = ws
            out["%s_%s_spread_ms" % (name, kind)] = round(max(ws) - min(ws), 4)
        out["stratified_minus_plain_%s_ms" % kind] = round(
            out["stratified_%s_call_ms" % kind] - out["plain_%s_call_ms" % kind], 4)
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
