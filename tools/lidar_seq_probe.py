#!/usr/bin/env python
"""Call times of a lidar sequence at the bench batch (5 agents x 4 scenes = 20 images, 32 beams x 1024 azimuths, 40 frames:
synthetic.make_lidar_world_batch of seed 0, solids padded to 128 rows as the tools pad them): lidar.world_step
(dn_lidar_world_step, one launch) alone, lidar.Sequence.step() (world_step -> scan(ids=True) -> holistic_views(own=True))
eager and as a graph replay, beside Sequence.host_step on this node's host (numpy, --host_frames frames, wall clock).
Device events, the median of 7 windows of --iters calls after a warm-up; every call advances the world by a frame, as a
sequence does, and every window starts at frame 0 again (--iters = --frames by default: a window is the sequence).
Frames 0 .. --host_frames - 1 of the replayed graph are checked to equal host_step in every byte in the same run.  These
are call times on an otherwise idle device, not a share of any step.  Writes one JSON document (--out, default
profiles/lidar_seq_probe.json) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import Config, _lib, graph, lidar  # noqa: E402
from disconet_amd.profiling import events_ms  # noqa: E402
from disconet_amd.synthetic import make_lidar_world_batch  # noqa: E402


def median_ms(fn, iters, rewind, windows=7):
    """a window is frames 0 .. iters - 1: rewind() (the cursor zeroed by a device fill, outside the events) before each"""
    def window():
        rewind()
        return events_ms(fn, iters)
    window()                                              # warm-up
    return round(statistics.median(window() for _ in range(windows)), 4)


def flat(step):
    return {"bev_seq": step["bev_seq"], "trans_matrices": step["trans_matrices"], "gt_boxes": step["gt"]["boxes"],
            "gt_ids": step["gt"]["ids"], "gt_count": step["gt"]["count"], "gt_own_hits": step["gt_own_hits"]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--host_frames", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_seq_probe.json"))
    args = ap.parse_args(argv)
    cfg = Config(map_hw=args.map_hw)
    world = make_lidar_world_batch(args.batch, args.agents, args.map_hw, seed=0, frames=args.frames, rows=args.rows)
    seq = lidar.Sequence(world, cfg, gt_rows=args.rows)

    t0 = time.perf_counter()
    want = [flat(seq.host_step(f)) for f in range(args.host_frames)]
    host_ms = 1e3 * (time.perf_counter() - t0) / max(1, args.host_frames)

    step = graph.GraphedStep(seq.step, range_guard=False)
    seq.reset()
    same = True
    for f in range(args.host_frames):
        got = flat(step())
        same = same and all(got[k].cpu().numpy().tobytes() == want[f][k].tobytes() for k in want[f])

    def world_only():
        lidar.world_step(seq.world, seq.cursor, out=seq.state)

    res = {"dn_version": int(_lib.load().dn_version()), "images": args.agents * args.batch,
           "rays_per_image": len(seq.dirs_host), "frames": args.frames, "map_hw": args.map_hw,
           "solids_per_scene": [int(c) for c in world["solid_count"]], "cars_per_scene": [int(c) for c in world["object_count"]],
           "solid_rows": args.rows, "iters": args.iters, "windows": 7,
           "graph_equals_host_step_in_every_byte": bool(same), "frames_checked": args.host_frames,
           "world_step_call_ms": median_ms(world_only, args.iters, seq.cursor.zero_),
           "sequence_step_eager_call_ms": median_ms(seq.step, args.iters, seq.cursor.zero_),
           "sequence_step_graph_call_ms": median_ms(step, args.iters, seq.cursor.zero_),
           "host_step_wall_ms_per_frame": round(host_ms, 1), "host": "the GPU node's host, numpy"}
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    if not same:
        raise SystemExit("the replayed graph and host_step disagree")


if __name__ == "__main__":
    main()
