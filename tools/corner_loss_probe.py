#!/usr/bin/env python
"""Call times of the corner localisation loss against the smooth-L1 loss it stands in for and against its composition in torch.

At 5 agents x batch 4 and 8 agents x batch 4 images of 256 x 256 x 6 anchors, with two masks each -- "assigned": box scenes
(synthetic.make_box_scene_batch) through targets.assign_targets, the positive density of a training step; "5pct": the same
tensors with 5 % of the anchors masked at random -- three forms on the same device tensors:
  det_loss_corner   train_ops.det_loss_corner (dn_det_loss_corner: focal + corner loss, values and both gradients, one launch)
  det_loss          train_ops.det_loss (dn_det_loss: focal + smooth-L1, one launch)
  torch_corner      train_ops.host_corner_loss on the device tensors under autograd, forward + backward: the LOCALISATION half
                    only (boolean gather of the masked rows, decode, corners, norm; no focal loss)
timed eager, alternating between the forms, with device events around windows of --calls calls; the median of --windows windows
after a warm-up window of each, and the windows' minimum and maximum.  These are CALL times (launch overhead and the memset of
the two loss words included), not kernel times.  The bytes are computed from the shapes: what each launch must read and write
in HBM if nothing stayed in a cache.

criterion (at the "assigned" density): median(det_loss_corner) - median(det_loss) <= max - min of det_loss' own windows.

Prints one JSON line and writes it to profiles/corner_loss_probe.json (--out).

    python tools/corner_loss_probe.py [--windows 7] [--calls 100] [--out profiles/corner_loss_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from disconet_amd import Config, _lib, postprocess, targets, train_ops  # noqa: E402
from disconet_amd.synthetic import make_box_scene_batch  # noqa: E402

HW, ANCHORS = 256, 6
SIZES = ((5, 4), (8, 4))


def window_ms(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def case(A, B, dev):
    """labels / targets / mask of box scenes by assign_targets, predictions = targets + noise"""
    cfg = Config(map_hw=HW)
    anchors = postprocess.make_anchors(cfg, device=dev)
    scene = make_box_scene_batch(B, A, HW, seed=0, boxes_per_scene=64, device=dev)
    t = targets.assign_targets(anchors, scene["gt_boxes"], scene["gt_count"])
    n = A * B * HW * HW * ANCHORS
    g = torch.Generator(device="cpu").manual_seed(0)
    tg = t["reg_targets"].reshape(n, 6).contiguous()
    loc = tg + 0.2 * torch.randn(n, 6, generator=g).to(dev)
    cls = (torch.randn(n, 2, generator=g) * 3).to(dev)
    rand5 = (torch.rand(n, generator=g) < 0.05).float().to(dev)
    return {"cls": cls, "labels": t["labels"].reshape(n, 2).contiguous(), "loc": loc, "targets": tg,
            "mask": t["reg_loss_mask"].reshape(n).contiguous(), "mask5": rand5, "anchors": anchors.reshape(-1, 6), "norm": float(A * B)}


def bytes_mb(n, positives):
    mb = lambda b: round(b / 1e6, 1)
    return {"det_loss_corner": {"read": mb(n * (8 + 8 + 4) + positives * 3 * 24), "written": mb(n * (8 + 24))},
            "det_loss": {"read": mb(n * (8 + 8 + 24 + 24 + 4)), "written": mb(n * (8 + 24))}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corner_loss_probe.json"))
    args = ap.parse_args(argv)
    if args.windows < 5:
        raise SystemExit("--windows must be at least 5 (the median of fewer windows is not reported)")
    dev = torch.device("cuda:0")
    rows = []
    for A, B in SIZES:
        c = case(A, B, dev)
        n = c["loc"].shape[0]
        for density, mask in (("assigned", c["mask"]), ("5pct", c["mask5"])):
            det = (c["cls"], c["labels"], c["loc"], c["targets"], mask)

            def torch_corner():
                loc = c["loc"].detach().requires_grad_(True)
                train_ops.host_corner_loss(loc, c["targets"], mask, c["anchors"], c["norm"]).backward()
                return loc.grad

            forms = {"det_loss_corner": lambda: train_ops.det_loss_corner(*det, c["anchors"], norm=c["norm"]),
                     "det_loss": lambda: train_ops.det_loss(*det, norm=c["norm"]),
                     "torch_corner": torch_corner}
            # the three agree before anything is timed: the kernel's dloc against torch's on the device, the class half bit for bit
            losses, dcls, dloc = forms["det_loss_corner"]()
            ref = torch_corner()
            # (relative L2: at these counts some corner pair lies within micrometres, where fp32 leaves no digits of d / |d| to either form)
            err = float((dloc - ref).double().norm()) / max(float(ref.double().norm()), 1e-30)
            if not err < 1e-2 or not torch.equal(dcls, forms["det_loss"]()[1]):
                raise SystemExit("det_loss_corner disagrees with the torch composition (%g) or with det_loss' dcls" % err)
            for fn in forms.values():          # warm-up: allocator, clocks
                window_ms(fn, args.calls)
            samples = {k: [] for k in forms}
            for _ in range(args.windows):      # alternating: one window of every form per round
                for k, fn in forms.items():
                    samples[k].append(window_ms(fn, args.calls))
            torch.cuda.synchronize()
            positives = int((mask != 0).sum())
            med = {k: statistics.median(v) for k, v in samples.items()}
            spread = max(samples["det_loss"]) - min(samples["det_loss"])
            row = {"agents": A, "batch": B, "anchors": n, "mask": density, "positives": positives,
                   "positive_share": round(positives / n, 5), "dloc_rel_l2_diff_vs_torch": err,
                   "bytes_mb": bytes_mb(n, positives),
                   "call_ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                               for k, v in samples.items()},
                   "det_loss_window_spread_ms": round(spread, 4),
                   "corner_minus_det_loss_ms": round(med["det_loss_corner"] - med["det_loss"], 4)}
            if density == "assigned":
                row["criterion_met"] = bool(med["det_loss_corner"] - med["det_loss"] <= spread)
            rows.append(row)
    out = {"tool": "tools/corner_loss_probe.py",
           "what": "call time per loss call (device events around windows of calls), ms; median / min / max of the windows",
           "windows": args.windows, "calls_per_window": args.calls, "dn_version": _lib.load().dn_version(),
           "device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "cases": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
