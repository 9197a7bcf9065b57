#!/usr/bin/env python
"""Call times of the lidar scan at the bench batch (5 agents x 4 scenes = 20 images, 32 beams x 1024 azimuths = 32768 rays
an image, up to 24 cars + 10 occluders a scene: synthetic.lidar_world_solids of seeds 0..3, which keeps 34, 34, 34 and 32
solids -- seed 3 has two cars inside a sensor's keep-out): lidar.scan (dn_lidar_scan: a zero fill and two kernels) alone and followed by holistic.holistic_views(own=True) (bev_seq and bev_seq_teacher, one more launch),
each eager and as a graph replay, beside lidar.host_scan on this node's host (numpy, one run, wall clock).  Device events,
the median of 7 windows of --iters calls after a warm-up; the device results are checked to equal host_scan in every byte
in the same run.  These are call times on an otherwise idle device, not a share of any step.  Writes one JSON document
(--out, default profiles/lidar_probe.json) and prints it.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import Config, _lib, holistic, lidar  # noqa: E402
from disconet_amd.profiling import events_ms  # noqa: E402
from disconet_amd.synthetic import lidar_world_solids, make_trans_matrices  # noqa: E402

KEYS = ("points", "hit", "solid_hits", "gt_boxes", "gt_count", "gt_own_hits")


def median_ms(fn, iters, windows=7):
    events_ms(fn, iters)                                  # warm-up
    return round(statistics.median(events_ms(fn, iters) for _ in range(windows)), 4)


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--beams", type=int, default=32)
    ap.add_argument("--azimuths", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_probe.json"))
    args = ap.parse_args(argv)
    A, B = args.agents, args.batch
    cfg = Config(map_hw=args.map_hw)
    cars, blocks = 24, 10
    K = cars + blocks
    solids = np.zeros((B, K, 8))
    count, objects = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        rows, n = lidar_world_solids(A, args.map_hw, b, 0, cars, blocks)
        solids[b, :len(rows)], count[b], objects[b] = rows, len(rows), n
    host_args = (solids, count, objects, lidar.sensor_from_world(B, A), np.full(B, A, dtype=np.int32),
                 lidar.beam_table(args.beams, args.azimuths))
    kw = dict(half_extent=float(cfg.area_extents[0][1]), gt_rows=K)
    dev_args = tuple(torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in host_args)
    trans = make_trans_matrices(B, A).cuda()
    live = [A] * B
    R = args.beams * args.azimuths
    ranges = holistic.source_ranges(np.arange(A * B + 1) * R, live, A, B, own=True)      # kept as long as the graphs

    scan = lambda: lidar.scan(*dev_args, **kw)                                                          # noqa: E731

    def scan_views():
        r = lidar.scan(*dev_args, **kw)
        return r, holistic.holistic_views(r["cloud"], trans, live, B, cfg, own=True, ranges=ranges)

    t0 = time.perf_counter()
    want = lidar.host_scan(*host_args, **kw)
    host_ms = 1e3 * (time.perf_counter() - t0)
    got, views = scan_views()
    g_scan, cap_scan = graph_of(scan)
    g_both, (cap_both, cap_views) = graph_of(scan_views)
    g_scan.replay()
    g_both.replay()
    torch.cuda.synchronize()
    same = all(r[k].cpu().numpy().tobytes() == want[k].tobytes() for r in (got, cap_scan, cap_both) for k in KEYS)
    same_views = all(torch.equal(views[k], cap_views[k]) for k in ("dense", "own_dense"))
    res = {"dn_version": int(_lib.load().dn_version()), "images": A * B, "rays_per_image": args.beams * args.azimuths,
           "solids_per_scene": [int(c) for c in count], "map_hw": args.map_hw, "iters": args.iters, "windows": 7,
           "returns": int((want["hit"] >= 0).sum()), "ground_truth_rows": int(want["gt_count"].sum()),
           "device_equals_host_scan_in_every_byte": bool(same), "graph_views_equal_eager_views": bool(same_views),
           "scan_eager_call_ms": median_ms(scan, args.iters), "scan_graph_call_ms": median_ms(g_scan.replay, args.iters),
           "scan_views_eager_call_ms": median_ms(scan_views, args.iters),
           "scan_views_graph_call_ms": median_ms(g_both.replay, args.iters),
           "host_scan_wall_ms": round(host_ms, 1), "host": "the GPU node's host, numpy, one run"}
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if not (same and same_views):
        raise SystemExit("the device and host_scan disagree")


if __name__ == "__main__":
    main()
