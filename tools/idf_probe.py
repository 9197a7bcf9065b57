#!/usr/bin/env python
"""Time the identity-metric path at the bench's size (5 agents x 4 scenes = 20 images, about 40 reported tracks and 40
ground-truth boxes each, 100 frames from synthetic.make_track_sequence(truth=True) through tracking.Sort):
tracking.Identity.update() (dn_idf_step, one launch) eager and as a captured graph, and Identity.finish() (dn_idf_finish,
one launch: the global assignment on the device) after the 100 frames, eager and as a graph -- device events around
many calls.  In the same run the host path they replace: per frame the tracker's report copied to the host +
tracking.HostIdentity.update() (the reference, written for its bits and not for speed), and at the end the copy of the
whole state (20 MB at the default sizes) that a host-side finish would need + HostIdentity.finish().  Every frame's
output, the final state and finish()'s two tensors are compared with the host's as bits.  Prints one JSON line and writes
it to profiles/idf_probe.json (--out)."""
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
    ap.add_argument("--frames", type=int, default=100, help="frames of the sequence; the timed step loops cycle through them")
    ap.add_argument("--host_frames", type=int, default=16, help="frames whose host path is timed (all are compared)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--max_gt_ids", type=int, default=256)
    ap.add_argument("--max_track_ids", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "idf_probe.json"))
    args = ap.parse_args(argv)
    seq = make_track_sequence(args.frames, args.images, seed=0, objects=args.objects, false_positives=args.false_positives,
                              width=128, extent=32.0, truth=True)
    scale = 4.0
    sizes = dict(scale=scale, max_gt_ids=args.max_gt_ids, max_track_ids=args.max_track_ids)
    sort = tracking.Sort(scale=scale)
    idf, host = tracking.Identity(4, **sizes), tracking.HostIdentity(4, **sizes)

    # the same bits as the host, frame by frame, and the host path's time per frame (copy + reference)
    tracks_dev, gt_dev, host_ms, same = [], [], [], True
    for f, (det, _, gt) in enumerate(seq):
        report = sort.update({key: torch.from_numpy(det[key]).cuda() for key in det})
        tracks_dev.append({key: report[key].clone() for key in TRACK_KEYS})
        gt_dev.append({key: torch.from_numpy(gt[key]).cuda() for key in gt})
        out = idf.update(tracks_dev[-1], gt_dev[-1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = host.update({key: tracks_dev[-1][key].cpu().numpy() for key in TRACK_KEYS}, gt)
        if f < args.host_frames:
            host_ms.append(1e3 * (time.perf_counter() - t0))
        same = same and np.array_equal(out["overlaps"].cpu().numpy().view(np.uint8), want["overlaps"].view(np.uint8))
    same = same and np.array_equal(idf.state_bytes(), host.state_bytes())

    # the finish after the whole sequence: on the device, and what a host-side finish would cost (state copy + reference)
    fin = idf.finish()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    state_host = idf.state.cpu()
    copy_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = host.finish()
    host_finish_ms = 1e3 * (time.perf_counter() - t0)
    for key in ("counts", "match"):
        same = same and np.array_equal(fin[key].cpu().numpy().view(np.uint8), want[key].view(np.uint8))
    figures = idf.compute()["overall"]
    status = idf.status_words().tolist()
    finish_eager_ms = min(events_ms(idf.finish, args.iters) for _ in range(3))
    finish_step = graph.GraphedStep(idf.finish, range_guard=False)
    finish_graph_ms = min(events_ms(finish_step, args.iters) for _ in range(3))

    # the step; the counts keep growing, which the step's work does not depend on
    frame = [0]

    def eager():
        frame[0] = (frame[0] + 1) % args.frames
        return idf.update(tracks_dev[frame[0]], gt_dev[frame[0]])

    eager_ms = min(events_ms(eager, args.iters) for _ in range(3))
    static_t = {key: tracks_dev[-1][key].clone() for key in TRACK_KEYS}
    static_g = {key: gt_dev[-1][key].clone() for key in gt_dev[-1]}
    step = graph.GraphedStep(lambda: idf.update(static_t, static_g), range_guard=False)
    graph_ms = min(events_ms(step, args.iters) for _ in range(3))
    out = {"images": args.images, "frames": args.frames, "iters": args.iters, "max_gt_ids": args.max_gt_ids,
           "max_track_ids": args.max_track_ids, "state_mb": round(state_host.numel() / 1e6, 2),
           "tracks_per_image": round(float(np.mean([t["count"].float().mean().item() for t in tracks_dev])), 1),
           "gt_per_image": round(float(np.mean([gt["count"].mean() for _, _, gt in seq])), 1),
           "gt_ids_per_image": round(float(fin["counts"][:, 4].float().mean().item()), 1),
           "track_ids_per_image": round(float(fin["counts"][:, 5].float().mean().item()), 1),
           "equal_to_host_bits": bool(same), "update_eager_ms": round(eager_ms, 4), "update_graph_ms": round(graph_ms, 4),
           "finish_eager_ms": round(finish_eager_ms, 4), "finish_graph_ms": round(finish_graph_ms, 4),
           "host_copy_plus_hostidentity_update_ms": round(float(np.median(host_ms)), 2),
           "host_state_copy_ms": round(copy_ms, 2), "host_finish_ms": round(host_finish_ms, 2),
           "host_update_over_graph": round(float(np.median(host_ms)) / graph_ms, 1),
           "host_copy_plus_finish_over_graph": round((copy_ms + host_finish_ms) / finish_graph_ms, 1),
           "IDF1": round(figures["IDF1"], 4), "IDP": round(figures["IDP"], 4), "IDR": round(figures["IDR"], 4),
           "IDTP": figures["IDTP"], "IDFP": figures["IDFP"], "IDFN": figures["IDFN"], "IDs": figures["IDs"],
           "GT_IDs": figures["GT_IDs"], "host_cpus": len(os.sched_getaffinity(0)), "dn_version": _lib.load().dn_version(),
           "status_words": status}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
