#!/usr/bin/env python
"""Call times of late fusion (`--com late`) at the bench's sizes: 5 agents x 4 scenes and 8 agents x 4 scenes, about 40
detections per image in K = 300 rows (the copies every agent holds of the scene's objects, in its own frame, plus false
positives of its own).  postprocess.late_fuse (dn_late_fuse: three launches) eager and as a captured graph, beside the
host path it replaces -- postprocess.detections_to_host (one device-to-host copy) + postprocess.host_late_fuse (the numpy
reference, written for its bits and not for speed).  Eager and replay alternate, window by window; device events around
windows of calls, the median of the windows.  These are CALL times (launches and the gaps between them included), not
kernel times.  The outputs are compared with the host's as bytes.  Prints one JSON line and writes it to
profiles/late_fuse_probe.json (--out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import Config, _lib, graph, postprocess  # noqa: E402
from disconet_amd.synthetic import make_trans_matrices  # noqa: E402

KEYS = ("boxes", "scores", "source", "count")


def make_detections(agents, batch, rows, objects, false_positives, seed, trans):
    """every agent's rows: its copy of each of the scene's `objects` boxes (placed in agent 0's frame within +-28 m, carried
    into the agent's own frame and dropped outside its extents), then `false_positives` boxes of its own; distinct scores"""
    rng = np.random.RandomState(seed)
    n = agents * batch
    det = {"boxes": np.zeros((n, rows, 6), dtype=np.float32), "scores": np.zeros((n, rows), dtype=np.float32),
           "count": np.zeros(n, dtype=np.int32)}
    t64 = trans.numpy().astype(np.float64)
    for b in range(batch):
        xy = rng.uniform(-28.0, 28.0, (objects, 2))
        yaw = rng.uniform(-np.pi, np.pi, objects)
        for j in range(agents):
            M = t64[b, j, 0]
            x = M[0, 0] * xy[:, 0] + M[0, 1] * xy[:, 1] + M[0, 3] + rng.normal(0, 0.05, objects)
            y = M[1, 0] * xy[:, 0] + M[1, 1] * xy[:, 1] + M[1, 3] + rng.normal(0, 0.05, objects)
            sn = M[1, 0] * np.cos(yaw) + M[1, 1] * np.sin(yaw)
            cs = M[0, 0] * np.cos(yaw) + M[0, 1] * np.sin(yaw)
            seen = (np.abs(x) < 32.0) & (np.abs(y) < 32.0)
            own = np.stack([x[seen], y[seen], np.full(seen.sum(), 2.0), np.full(seen.sum(), 4.5), sn[seen], cs[seen]], 1)
            fp = np.zeros((false_positives, 6))
            fp[:, 0:2] = rng.uniform(-30.0, 30.0, (false_positives, 2))
            fp[:, 2], fp[:, 3] = 2.0, 4.5
            a = rng.uniform(-np.pi, np.pi, false_positives)
            fp[:, 4], fp[:, 5] = np.sin(a), np.cos(a)
            both = np.concatenate([own, fp], 0)[:rows]
            img = j * batch + b
            det["boxes"][img, :len(both)] = both
            det["scores"][img, :len(both)] = np.sort(rng.uniform(0.05, 1.0, len(both)))[::-1]
            det["count"][img] = len(both)
    return det


def _window_ms(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def probe(agents, batch, args, extents):
    trans = make_trans_matrices(batch, agents, jitter_seed=0)
    det = make_detections(agents, batch, args.rows, args.objects, args.false_positives, agents, trans)
    live = [agents] * batch
    dev = {k: torch.from_numpy(v).cuda() for k, v in det.items()}
    d_trans, d_live = trans.cuda(), torch.tensor(live, dtype=torch.int32, device="cuda")

    def eager():
        return postprocess.late_fuse(dev, d_trans, d_live, batch, agents, extents=extents)

    out = eager()
    torch.cuda.synchronize()
    host_ms = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        rows = postprocess.detections_to_host(dev)
        padded = postprocess.pad_detections([b for b, _ in rows], [s for _, s in rows], args.rows)
        want = postprocess.host_late_fuse(padded, trans, live, batch, agents, extents=extents)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    same = all(out[k].cpu().numpy().tobytes() == want[k].tobytes() for k in KEYS)
    step = graph.GraphedStep(eager, range_guard=False)
    for fn in (eager, step):                 # warm both forms at this shape
        _window_ms(fn, args.calls)
    eager_ms, graph_ms = [], []
    for _ in range(args.windows):            # alternating: a drift of the machine lands on both
        eager_ms.append(_window_ms(eager, args.calls))
        graph_ms.append(_window_ms(step, args.calls))
    med = lambda v: float(np.median(v))
    return {"agents": agents, "batch": batch, "images": agents * batch, "rows": args.rows,
            "detections_per_image_in": round(float(det["count"].mean()), 1),
            "detections_per_image_out": round(float(want["count"].mean()), 1),
            "equal_to_host_bytes": bool(same),
            "late_fuse_eager_ms": round(med(eager_ms), 4), "late_fuse_eager_ms_min_max": [round(min(eager_ms), 4), round(max(eager_ms), 4)],
            "late_fuse_graph_ms": round(med(graph_ms), 4), "late_fuse_graph_ms_min_max": [round(min(graph_ms), 4), round(max(graph_ms), 4)],
            "host_copy_plus_host_late_fuse_ms": round(med(host_ms), 2),
            "host_over_graph": round(med(host_ms) / med(graph_ms), 1)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rows", type=int, default=300, help="K: detection rows per image")
    ap.add_argument("--objects", type=int, default=44)
    ap.add_argument("--false_positives", type=int, default=6)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host_repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "late_fuse_probe.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("late_fuse_probe.py measures on the GPU; there is none here")
    extents = Config().area_extents[:2]
    out = {"what": "call times (device events around windows of calls, median of the windows), not kernel times",
           "calls_per_window": args.calls, "windows": args.windows, "host_cpus": len(os.sched_getaffinity(0)),
           "dn_version": _lib.load().dn_version(), "sizes": [probe(a, args.batch, args, extents) for a in (5, 8)]}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
