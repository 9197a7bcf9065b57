#!/usr/bin/env python
"""Time the tracking step at the bench's size (5 agents x 4 scenes = 20 images, about 40 detections each, K = 128 rows
from synthetic.make_track_sequence): tracking.Sort.update() (dn_track_step, one launch) eager and as a captured graph
(device events), and in the same run the host path it replaces -- postprocess.detections_to_host (one device-to-host
copy) + tracking.HostSort (the float64 reference, written for its bits and not for speed).  Every frame's outputs are
compared with the host's as bits.  Prints one JSON line and writes it to profiles/track_probe.json (--out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import _lib, graph, postprocess, tracking  # noqa: E402
from disconet_amd.synthetic import make_track_sequence  # noqa: E402
from disconet_amd.profiling import events_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--objects", type=int, default=38)
    ap.add_argument("--false_positives", type=int, default=4)
    ap.add_argument("--rows", type=int, default=128, help="K: detection rows per image")
    ap.add_argument("--frames", type=int, default=16, help="frames of the sequence; the timed loops cycle through them")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_probe.json"))
    args = ap.parse_args(argv)
    seq = [det for det, _ in make_track_sequence(args.frames, args.images, seed=0, objects=args.objects,
                                                 false_positives=args.false_positives, width=args.rows, extent=32.0)]
    dev = [{key: torch.from_numpy(det[key]).cuda() for key in det} for det in seq]
    static = {key: dev[0][key].clone() for key in dev[0]}
    scale = 4.0
    sort, host = tracking.Sort(scale=scale), tracking.HostSort(scale=scale)

    # the same bits as the host, frame by frame, and the host path's time (copy + reference)
    host_ms, same = [], True
    for f in range(args.frames):
        out = sort.update(dev[f])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = postprocess.detections_to_host(dev[f])
        want = host.update(postprocess.pad_detections([b for b, _ in rows], [s for _, s in rows], args.rows))
        host_ms.append(1e3 * (time.perf_counter() - t0))
        for key in want:
            same = same and np.array_equal(out[key].cpu().numpy().view(np.uint8), want[key].view(np.uint8))
    tracks = [int(w) for w in sort.state.view(args.images, -1)[:, 8:12].contiguous().cpu().numpy().view(np.int32).reshape(-1)]
    paths = sorted(set(host.last_path))

    frame = [0]

    def eager():
        frame[0] = (frame[0] + 1) % args.frames
        return sort.update(dev[frame[0]])

    eager_ms = min(events_ms(eager, args.iters) for _ in range(3))
    step = graph.GraphedStep(lambda: sort.update(static), range_guard=False)
    graph_ms = min(events_ms(step, args.iters) for _ in range(3))
    out = {"images": args.images, "rows": args.rows, "frames": args.frames, "iters": args.iters,
           "detections_per_image": round(float(np.mean([det["count"].mean() for det in seq])), 1),
           "tracks_per_image_after_sequence": round(float(np.mean(tracks)), 1), "association_paths_last_frame": paths,
           "equal_to_host_bits": bool(same), "update_eager_ms": round(eager_ms, 4), "update_graph_ms": round(graph_ms, 4),
           "host_copy_plus_hostsort_ms": round(float(np.median(host_ms)), 2),
           "host_over_graph": round(float(np.median(host_ms)) / graph_ms, 1),
           "host_cpus": len(os.sched_getaffinity(0)), "dn_version": _lib.load().dn_version(),
           "status_words": sort.status_words().tolist()}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
