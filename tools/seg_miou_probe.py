#!/usr/bin/env python
"""Time the mean-IoU path at the bench's seg size (5 agents x 4 scenes = 20 images, 256 x 256 pixels, 8 classes):
seg.MeanIoU.update() (dn_seg_confusion, one launch) eager and as a captured graph, with the int64 label maps the tools
hand it (update() then clamps and narrows them to int32 first: two torch kernels) and with int32 labels (the launch alone; also over
--rotate input sets in turn, which together exceed the last-level cache), on two inputs -- "scene":
synthetic.make_seg_scene_batch's label maps with logits that mostly agree with them (large uniform regions: a wave meets
one or two cells), "noise": uniform random labels and logits (a wave meets up to 64 cells, the worst case of the per-wave
aggregation).  In the same run the torch way (argmax + masked bincount of image * classes^2 + label * classes +
prediction, which waits for the device: the masked select has a data-dependent size), and what this card streams (a
48 MB read-reduce and copy, the measurement of tools/bw_probe.py) beside the launch's bytes / time.  Device events around
windows of --iters calls, --runs windows each; the median, the fastest and every window are reported.  The state after one
update is compared with seg.HostMeanIoU as bits.  Prints one JSON line and writes it to profiles/seg_miou_probe.json (--out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import _lib, graph, seg  # noqa: E402
from disconet_amd.synthetic import make_seg_scene_batch  # noqa: E402


def _window_us(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return 1e3 * start.elapsed_time(end) / iters


def _timed(fn, iters, runs):
    _window_us(fn, max(1, iters // 10))                                       # warm-up at the timed shape
    windows = sorted(_window_us(fn, iters) for _ in range(runs))
    return {"median_us": round(windows[len(windows) // 2], 2), "min_us": round(windows[0], 2),
            "windows_us": [round(w, 2) for w in windows]}


def torch_way(logits, labels, classes):
    n = logits.shape[0]
    pred = logits.argmax(-1)
    valid = (labels >= 0) & (labels < classes)
    cell = torch.arange(n, device=logits.device).view(n, 1, 1) * (classes * classes) + labels * classes + pred
    return torch.bincount(cell[valid], minlength=n * classes * classes)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--iters", type=int, default=2000, help="calls per timed window")
    ap.add_argument("--torch_iters", type=int, default=100, help="calls per timed window of the torch way")
    ap.add_argument("--runs", type=int, default=5, help="timed windows per figure")
    ap.add_argument("--rotate", type=int, default=8, help="input sets of the rotating figure (8 x 47 MB > the last-level cache)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_miou_probe.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("seg_miou_probe: no GPU; a time is measured on the MI355X or not at all")
    n, hw, c = args.agents * args.batch, args.map_hw, args.classes
    g = torch.Generator().manual_seed(0)
    scene = make_seg_scene_batch(args.batch, args.agents, hw, seed=0, ignore_border=2)["labels"]
    inputs = {
        "scene": (torch.nn.functional.one_hot(scene.clamp(min=0), c).float() * 3.0 + torch.randn(n, hw, hw, c, generator=g), scene),
        "noise": (torch.randn(n, hw, hw, c, generator=g), torch.randint(0, c, (n, hw, hw), generator=g)),
    }
    launch_bytes = n * hw * hw * (4 * c + 4)
    out = {"images": n, "map_hw": hw, "classes": c, "iters": args.iters, "torch_iters": args.torch_iters, "runs": args.runs,
           "rotate": args.rotate, "launch_read_mb": round(launch_bytes / 1e6, 1), "dn_version": _lib.load().dn_version(),
           "equal_to_host_bits": True}
    for name, (logits, labels) in inputs.items():
        z, y64 = logits.cuda().contiguous(), labels.cuda()
        y32 = y64.to(torch.int32)
        metric, host = seg.MeanIoU(n, c), seg.HostMeanIoU(n, c)
        pred = metric.update(z, y64, want_pred=True)
        want = host.update(logits, labels, want_pred=True)
        same = np.array_equal(metric.state.cpu().numpy(), host.state) and np.array_equal(pred.cpu().numpy(), want)
        same = same and np.array_equal(torch_way(z, y64, c).cpu().numpy(), host.state[:, :c * c].ravel())
        out["equal_to_host_bits"] = bool(out["equal_to_host_bits"] and same)
        row = {"mIoU": round(metric.compute()["overall"]["mIoU"], 4)}
        row["update_eager_int64_labels"] = _timed(lambda: metric.update(z, y64), args.iters, args.runs)
        row["update_eager_int32_labels"] = _timed(lambda: metric.update(z, y32), args.iters, args.runs)
        step64 = graph.GraphedStep(lambda: metric.update(z, y64, want_pred=True), range_guard=False)
        row["update_graph_int64_labels_with_pred"] = _timed(step64, args.iters, args.runs)
        step32 = graph.GraphedStep(lambda: metric.update(z, y32), range_guard=False)
        row["launch_alone_graph"] = _timed(step32, args.iters, args.runs)
        # back-to-back eager launches: the device runs one behind the other, the figure is the kernel's own time
        row["launch_alone_gb_per_s"] = round(launch_bytes / 1e3 / row["update_eager_int32_labels"]["median_us"], 1)
        # the same input every call stays in the 256 MB last-level cache: `rotate` input sets (more than the cache) in turn
        sets = [(z.clone(), y32.clone()) for _ in range(args.rotate)]
        turn = [0]

        def rotating():
            turn[0] = (turn[0] + 1) % len(sets)
            return metric.update(*sets[turn[0]])

        row["launch_alone_rotating_inputs"] = _timed(rotating, args.iters, args.runs)
        row["launch_alone_rotating_gb_per_s"] = round(launch_bytes / 1e3 / row["launch_alone_rotating_inputs"]["median_us"], 1)
        del sets
        row["torch_argmax_masked_bincount"] = _timed(lambda: torch_way(z, y64, c), args.torch_iters, args.runs)
        row["torch_over_graph_update"] = round(row["torch_argmax_masked_bincount"]["median_us"] /
                                               row["update_graph_int64_labels_with_pred"]["median_us"], 1)
        out[name] = row
    # what the card streams in this run (tools/bw_probe.py's measurement at the launch's size)
    x = torch.empty(48 * 1024 * 1024 // 4, device="cuda", dtype=torch.float32).normal_()
    y = torch.empty_like(x)
    out["stream_48mb"] = {"read_reduce": _timed(lambda: x.sum(), 200, args.runs), "copy": _timed(lambda: y.copy_(x), 200, args.runs)}
    out["stream_48mb"]["read_reduce_gb_per_s"] = round(x.numel() * 4 / 1e3 / out["stream_48mb"]["read_reduce"]["median_us"], 1)
    out["stream_48mb"]["copy_gb_per_s_read_plus_write"] = round(2 * x.numel() * 4 / 1e3 / out["stream_48mb"]["copy"]["median_us"], 1)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
