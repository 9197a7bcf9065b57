#!/usr/bin/env python
"""Time the tracking-evaluation step at the bench's size (5 agents x 4 scenes = 20 images, about 40 reported tracks and
40 ground-truth boxes each, from synthetic.make_track_sequence(truth=True) through tracking.Sort):
tracking.ClearMot.update() (dn_mot_step, one launch) eager and as a captured graph (device events), and in the same run
the host path it replaces -- the tracker's report copied to the host + tracking.HostClearMot (the float64 reference,
written for its bits and not for speed).  Every frame's outputs and the final state are compared with the host's as
bits.  Prints one JSON line and writes it to profiles/mot_probe.json (--out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import _lib, graph, tracking  # noqa: E402
from disconet_amd.synthetic import make_track_sequence  # noqa: E402
from disconet_amd.profiling import events_ms  # noqa: E402

TRACK_KEYS = ("rect", "id", "count")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--false_positives", type=int, default=4)
    ap.add_argument("--frames", type=int, default=16, help="frames of the sequence; the timed loops cycle through them")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mot_probe.json"))
    args = ap.parse_args(argv)
    seq = make_track_sequence(args.frames, args.images, seed=0, objects=args.objects, false_positives=args.false_positives,
                              width=128, extent=32.0, truth=True)
    scale = 4.0
    sort = tracking.Sort(scale=scale)
    mot, host = tracking.ClearMot(4, scale=scale), tracking.HostClearMot(4, scale=scale)

    # the same bits as the host, frame by frame, and the host path's time (copy + reference)
    tracks_dev, gt_dev, host_ms, same = [], [], [], True
    for det, _, gt in seq:
        report = sort.update({key: torch.from_numpy(det[key]).cuda() for key in det})
        tracks_dev.append({key: report[key].clone() for key in TRACK_KEYS})
        gt_dev.append({key: torch.from_numpy(gt[key]).cuda() for key in gt})
        out = mot.update(tracks_dev[-1], gt_dev[-1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = host.update({key: tracks_dev[-1][key].cpu().numpy() for key in TRACK_KEYS}, gt)
        host_ms.append(1e3 * (time.perf_counter() - t0))
        for key in want:
            same = same and np.array_equal(out[key].cpu().numpy().view(np.uint8), want[key].view(np.uint8))
    same = same and np.array_equal(mot.state_bytes(), host.state_bytes())
    figures = mot.compute()["overall"]
    status = mot.status_words().tolist()

    frame = [0]

    def eager():
        frame[0] = (frame[0] + 1) % args.frames
        return mot.update(tracks_dev[frame[0]], gt_dev[frame[0]])

    eager_ms = min(events_ms(eager, args.iters) for _ in range(3))
    static_t = {key: tracks_dev[-1][key].clone() for key in TRACK_KEYS}
    static_g = {key: gt_dev[-1][key].clone() for key in gt_dev[-1]}
    step = graph.GraphedStep(lambda: mot.update(static_t, static_g), range_guard=False)
    graph_ms = min(events_ms(step, args.iters) for _ in range(3))
    out = {"images": args.images, "frames": args.frames, "iters": args.iters,
           "tracks_per_image": round(float(np.mean([t["count"].float().mean().item() for t in tracks_dev])), 1),
           "gt_per_image": round(float(np.mean([gt["count"].mean() for _, _, gt in seq])), 1),
           "equal_to_host_bits": bool(same), "update_eager_ms": round(eager_ms, 4), "update_graph_ms": round(graph_ms, 4),
           "host_copy_plus_hostclearmot_ms": round(float(np.median(host_ms)), 2),
           "host_over_graph": round(float(np.median(host_ms)) / graph_ms, 1),
           "MOTA": round(figures["MOTA"], 4), "MOTP": round(figures["MOTP"], 4), "TP": figures["TP"], "FP": figures["FP"],
           "FN": figures["FN"], "IDSW": figures["IDSW"], "Frag": figures["Frag"],
           "host_cpus": len(os.sched_getaffinity(0)), "dn_version": _lib.load().dn_version(), "status_words": status}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
