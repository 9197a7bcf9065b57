#!/usr/bin/env python
"""Time the teacher's holistic views at the bench batch (5 agents x 4 scenes: 20 views, 100 sources,
synthetic.make_point_cloud(60000) per image, dense float32 grid and occupancy words): ops.voxelize_views (dn_voxelize_views,
one launch) as a captured graph and eager, beside the only way the library could make the same tensor on the device before
it: one torch transform per source (float64 sums in the contract's order, rounded to float32), torch.cat per view and one
ops.voxelize_occupy per view -- 100 transforms, 20 concatenations, 20 launches, which yields the dense grid only.  Both
are timed with device events over warmed runs; the loop is checked to write the same bytes first.  Prints one JSON line.
Per-kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (--iters 20)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from disconet_amd import Config, holistic, ops  # noqa: E402
from disconet_amd.synthetic import make_point_cloud, make_trans_matrices  # noqa: E402
from disconet_amd.profiling import events_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loop_iters", type=int, default=10)
    args = ap.parse_args(argv)
    A, B = args.agents, args.batch
    cfg = Config(map_hw=args.map_hw)
    clouds = [make_point_cloud(args.points, seed=k) for k in range(A * B)]
    trans = make_trans_matrices(B, A, jitter_seed=3).cuda()
    pts, offsets = holistic.pack_clouds(clouds, "cuda")
    src = holistic.view_sources([A] * B, A, B)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
    begin = i32([int(offsets[k]) for k in src["src_image"]])
    count = i32([int(offsets[k + 1] - offsets[k]) for k in src["src_image"]])
    view, pose = i32(src["src_view"]), i32(src["src_pose"])
    max_count = int(np.diff(offsets).max())
    poses = trans.reshape(-1, 4, 4).contiguous()
    want = ("dense", "bits")
    run = lambda w=want: ops.voxelize_views(pts, begin, count, view, pose, poses, src["n_views"], max_count,   # noqa: E731
                                            cfg.voxel_size, cfg.area_extents, cfg.map_dims, want=w)

    dev_clouds = [pts[int(offsets[k]):int(offsets[k + 1])] for k in range(A * B)]
    poses64 = poses.double()

    def loop():
        views = [[] for _ in range(src["n_views"])]
        for k, v, p in zip(src["src_image"], src["src_view"], src["src_pose"]):
            c = dev_clouds[k][:, :3]
            if p >= 0:
                T, x, y, z = poses64[p], c[:, 0].double(), c[:, 1].double(), c[:, 2].double()
                c = torch.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).float()
            views[v].append(c)
        return torch.stack([ops.voxelize_occupy(torch.cat(parts, 0).contiguous(), cfg.voxel_size, cfg.area_extents,
                                                cfg.map_dims) for parts in views], 0)[:, None]

    for _ in range(3):
        out = run()
        ref = loop()
    torch.cuda.synchronize()
    same = bool(torch.equal(out["dense"], ref)) and bool(torch.equal(out["bits"].nhwc(), out["dense"][:, 0]))
    res = {"views": src["n_views"], "sources": len(src["src_image"]), "points": int(offsets[-1]), "map_hw": args.map_hw,
           "occupied_cells": int(out["dense"].sum()), "loop_writes_the_same_bytes": same, "iters": args.iters,
           "one_launch_eager_ms": round(min(events_ms(run, args.iters) for _ in range(3)), 4),
           "one_launch_dense_only_eager_ms": round(min(events_ms(lambda: run(("dense",)), args.iters) for _ in range(3)), 4)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    torch.cuda.synchronize()
    res["one_launch_graph_ms"] = round(min(events_ms(g.replay, args.iters) for _ in range(3)), 4)
    res["torch_loop_ms"] = round(min(events_ms(loop, args.loop_iters) for _ in range(3)), 4)
    res["loop_over_one_launch"] = round(res["torch_loop_ms"] / res["one_launch_graph_ms"], 2)
    res["loop_over_one_launch_eager"] = round(res["torch_loop_ms"] / res["one_launch_eager_ms"], 2)
    print(json.dumps(res), flush=True)
    if not same:
        raise SystemExit("the torch loop and the one-launch call disagree")


if __name__ == "__main__":
    main()
