#!/usr/bin/env python
"""Call times of BEV rendering at the bench's size: 20 images of 256 x 256 at scale 4 (a canvas of 63 MB) and at scale 1,
with about 40 detections (coloured by score, translucent fill) plus 40 ground-truth boxes per image, the occupancy as
background and a 32 x 32 heat overlay.  render.render_bev (dn_render_bev: one launch) eager and as a captured graph,
beside the host path it replaces -- postprocess.detections_to_host (one device-to-host copy) + render.host_render_bev
(the numpy statement, written for its bytes and not for speed).  Eager and replay alternate, window by window; device
events around windows of calls, the median of the windows after a warm-up.  These are CALL times (the launch and the gaps
between calls included), not kernel times.  The canvas is compared with the host's as bytes.  Prints one JSON line and
writes it to profiles/render_probe.json (--out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import BoxLayer, Config, _lib, graph, postprocess, render  # noqa: E402


def make_boxes(rng, n, rows, per_image, half):
    boxes = np.zeros((n, rows, 6), dtype=np.float32)
    count = np.full(n, per_image, dtype=np.int32)
    boxes[:, :per_image, 0:2] = rng.uniform(-half, half, (n, per_image, 2))
    boxes[:, :per_image, 2] = rng.uniform(1.6, 2.4, (n, per_image))
    boxes[:, :per_image, 3] = rng.uniform(3.5, 5.5, (n, per_image))
    yaw = rng.uniform(-np.pi, np.pi, (n, per_image))
    boxes[:, :per_image, 4], boxes[:, :per_image, 5] = np.sin(yaw), np.cos(yaw)
    return boxes, count


def _window_ms(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def probe(scale, args, config):
    rng = np.random.RandomState(scale)
    n, hw = args.images, config.map_dims[0]
    half = float(config.area_extents[0][1])
    det_boxes, det_count = make_boxes(rng, n, args.rows, args.boxes, half)
    scores = np.zeros((n, args.rows), dtype=np.float32)
    scores[:, :args.boxes] = np.sort(rng.uniform(0.05, 1.0, (n, args.boxes)), axis=1)[:, ::-1]
    gt_boxes, gt_count = make_boxes(rng, n, 64, args.boxes, half)
    words = np.where(rng.uniform(0, 1, (n, hw, hw)) < 0.05, rng.randint(1, 1 << 13, (n, hw, hw)), 0).astype(np.int32)
    heat = rng.uniform(0, 1, (n, 32, 32)).astype(np.float32)
    det = {"boxes": torch.from_numpy(det_boxes).cuda(), "scores": torch.from_numpy(scores).cuda(),
           "count": torch.from_numpy(det_count).cuda()}
    d_gt, d_gt_count = torch.from_numpy(gt_boxes).cuda(), torch.from_numpy(gt_count).cuda()
    d_words, d_heat = torch.from_numpy(words).cuda(), torch.from_numpy(heat).cuda()
    canvas = torch.empty((n, scale * hw, scale * hw, 3), dtype=torch.uint8, device="cuda")

    def eager():
        return render.render_bev(config, background=d_words, heat=d_heat, scale=scale, out=canvas,
                                 layers=[BoxLayer.ground_truth(d_gt, d_gt_count), BoxLayer.detections(det, fill_alpha=60)])

    out = eager()
    torch.cuda.synchronize()
    host_ms = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        rows = postprocess.detections_to_host(det)
        padded = postprocess.pad_detections([b for b, _ in rows], [s for _, s in rows], args.rows)
        want = render.host_render_bev(config, background=words, heat=heat, scale=scale,
                                      layers=[BoxLayer.ground_truth(gt_boxes, gt_count),
                                              BoxLayer.detections(padded, fill_alpha=60)])
        host_ms.append(1e3 * (time.perf_counter() - t0))
    same = out.cpu().numpy().tobytes() == want.tobytes()
    step = graph.GraphedStep(eager, range_guard=False)
    for fn in (eager, step):                 # warm both forms at this shape
        _window_ms(fn, args.calls)
    eager_ms, graph_ms = [], []
    for _ in range(args.windows):            # alternating: a drift of the machine lands on both
        eager_ms.append(_window_ms(eager, args.calls))
        graph_ms.append(_window_ms(step, args.calls))
    med = lambda v: float(np.median(v))
    return {"images": n, "map": [hw, hw], "scale": scale, "canvas_bytes": int(canvas.numel()),
            "boxes_per_image": [args.boxes, args.boxes], "heat": [32, 32], "equal_to_host_bytes": bool(same),
            "render_eager_ms": round(med(eager_ms), 4), "render_eager_ms_min_max": [round(min(eager_ms), 4), round(max(eager_ms), 4)],
            "render_graph_ms": round(med(graph_ms), 4), "render_graph_ms_min_max": [round(min(graph_ms), 4), round(max(graph_ms), 4)],
            "canvas_gb_per_s_graph": round(canvas.numel() / med(graph_ms) / 1e6, 1),
            "host_copy_plus_host_render_ms": round(med(host_ms), 1),
            "host_over_graph": round(med(host_ms) / med(graph_ms), 1)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--rows", type=int, default=300, help="K: detection rows per image")
    ap.add_argument("--boxes", type=int, default=40, help="detections, and ground-truth boxes, per image")
    ap.add_argument("--calls", type=int, default=400, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host_repeats", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_probe.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("render_probe.py measures on the GPU; there is none here")
    config = Config()
    out = {"what": "call times (device events around windows of calls, median of the windows), not kernel times",
           "calls_per_window": args.calls, "windows": args.windows, "host_cpus": len(os.sched_getaffinity(0)),
           "dn_version": _lib.load().dn_version(), "sizes": [probe(s, args, config) for s in (4, 1)]}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
