#!/usr/bin/env python
"""Time the target assignment at the bench batch (5 agents x 4 scenes, 256 x 256 x 6 anchors, 64 ground-truth rows from
synthetic.make_box_scene_batch): targets.assign_targets (dn_assign_targets) eager and as a captured graph (device events,
after warm-up), the training step it precedes (CoDetModule.step on the same scenes and targets), and
targets.host_assign_targets on --host_images of the images (the host reference runs ~13 000 polygon clips a second).
Prints one JSON line.  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own
(--iters 20 --host_images 0 --no_step)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from disconet_amd import CoDetModule, Config, DiscoNet, postprocess, targets  # noqa: E402
from disconet_amd.synthetic import make_box_scene_batch  # noqa: E402
from disconet_amd.profiling import events_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--gt_rows", type=int, default=64)
    ap.add_argument("--pos_thr", type=float, default=0.6)
    ap.add_argument("--neg_thr", type=float, default=0.45)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--step_iters", type=int, default=20)
    ap.add_argument("--host_images", type=int, default=1, help="images timed through host_assign_targets (0: none)")
    ap.add_argument("--no_step", action="store_true", help="skip the training step")
    args = ap.parse_args(argv)
    cfg = Config(map_hw=args.map_hw)
    anchors = postprocess.make_anchors(cfg)
    scene = make_box_scene_batch(args.batch, args.agents, args.map_hw, seed=0, boxes_per_scene=args.gt_rows, device="cuda")
    gt_boxes, gt_count = scene["gt_boxes"], scene["gt_count"]
    n = args.agents * args.batch
    run = lambda force=True: targets.assign_targets(anchors, gt_boxes, gt_count, args.pos_thr, args.neg_thr,   # noqa: E731
                                                    force_match=force)
    for _ in range(5):
        t = run()
    torch.cuda.synchronize()
    out = {"images": n, "anchors_per_image": int(anchors.numel() // 6), "gt_rows": args.gt_rows,
           "gt_boxes": int(gt_count.sum()), "positives": int(t["reg_loss_mask"].sum()),
           "dont_care": int((t["labels"].sum(-1) == 0).sum()), "iters": args.iters,
           "assign_eager_ms": round(events_ms(run, args.iters), 4),
           "assign_no_force_eager_ms": round(events_ms(lambda: run(False), args.iters), 4)}
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
    out["assign_graph_ms"] = round(min(events_ms(g.replay, args.iters) for _ in range(3)), 4)
    if not args.no_step:
        torch.manual_seed(0)
        model = DiscoNet(cfg, kd_flag=0, num_agent=args.agents).cuda()
        module = CoDetModule(model, None, cfg, None, kd_flag=0)
        data = {k: scene[k] for k in ("bev_seq", "trans_matrices", "num_agent")}
        data.update(t)
        for _ in range(5):
            module.step(data, args.batch)
        torch.cuda.synchronize()
        out["train_step_ms"] = round(min(events_ms(lambda: module.step(data, args.batch), args.step_iters) for _ in range(3)), 4)
        out["assign_over_step"] = round(out["assign_graph_ms"] / out["train_step_ms"], 4)
    if args.host_images > 0:
        k = min(args.host_images, n)
        t0 = time.perf_counter()
        targets.host_assign_targets(anchors, gt_boxes[:k], gt_count[:k], args.pos_thr, args.neg_thr)
        out["host_images"] = k
        out["host_assign_s"] = round(time.perf_counter() - t0, 2)
        out["host_assign_s_all_images_scaled"] = round(out["host_assign_s"] * n / k, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
