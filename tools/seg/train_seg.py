#!/usr/bin/env python
"""Thin re-hosting of the reference's segmentation training entry point for `--com disco` (upstream:tools/seg/train_seg.py;
flag spelling as tools/det/train_codet.py).  The reference's tool body -- V2X-Sim loading, logging -- is out of scope
(SURVEY.md §8(f)); this shim builds SegDiscoNet the way the tool does, resumes from `--resume` if given, and runs
SegModule.step (train-mode forward, cross entropy, explicit HIP reverse pass, Adam) on synthetic scenes through the MI355X
path, writing `epoch_N.pth` with the det tool's checkpoint keys.

    python tools/seg/train_seg.py --com disco [--batch 1] [--nepoch 2] [--steps_per_epoch 8] [--num_agent 5] [--lr 0.001] \
        [--logpath logs/seg] [--resume logs/seg/epoch_2.pth] [--map_hw 256] [--labels random|scene] [--scenes 4]

--labels random (default): random occupancy (synthetic.make_scene_batch) and uniform random labels: the plumbing only.
--labels scene: synthetic.make_seg_scene_batch -- scenes whose occupancy shows the boxes their label maps are drawn from
    (cars = class 1, long vehicles = class 2, everything else = class 0).  The steps cycle through the scene seeds
    0 .. --scenes - 1, the frames that `eval_seg.py --resume <logpath>/epoch_N.pth` then scores with mIoU.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "det"))

from disconet_amd import SegDiscoNet, SegModule, load_checkpoint  # noqa: E402
from disconet_amd.synthetic import make_scene_batch, make_seg_scene_batch  # noqa: E402
from codet_common import agents_of  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("-d", "--data", default=None, help="(unused here: synthetic scenes)")
    ap.add_argument("--com", default="disco")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--nepoch", type=int, default=2)
    ap.add_argument("--steps_per_epoch", type=int, default=8)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--nworker", type=int, default=0)
    ap.add_argument("--log", action="store_true")
    ap.add_argument("--logpath", default="")
    ap.add_argument("--resume", default="")
    ap.add_argument("--kd_flag", type=int, default=0)
    ap.add_argument("--num_agent", type=int, default=5)
    ap.add_argument("--rsu", type=int, default=0)
    ap.add_argument("--only_v2i", type=int, default=0)
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--labels", choices=("random", "scene"), default="random",
                    help="scene: label maps drawn from the boxes the occupancy shows")
    ap.add_argument("--scenes", type=int, default=4, help="--labels scene: the steps cycle through this many scene seeds")
    return ap


def step_data(args, num_agent, epoch, it, device="cuda"):
    """The `data` dict of one SegModule.step."""
    seed = epoch * 1000 + it
    if args.labels == "scene":
        scene = make_seg_scene_batch(args.batch, num_agent, args.map_hw, seed=seed % max(1, args.scenes), device=device)
        return {k: scene[k] for k in ("bev_seq", "trans_matrices", "num_agent", "labels")}
    bevs, trans, na = make_scene_batch(args.batch, num_agent, args.map_hw, jitter_seed=seed)
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, 8, (bevs.shape[0], args.map_hw, args.map_hw), generator=g)
    return {"bev_seq": bevs[:, 0].permute(0, 3, 1, 2).to(device), "trans_matrices": trans.to(device), "num_agent": na.to(device),
            "labels": labels.to(device)}


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.com != "disco":
        raise SystemExit("only --com disco is built on the MI355X path (SURVEY.md §2.1 #8)")
    if args.kd_flag:
        raise SystemExit("the seg KD teacher is not built: --kd_flag 0 only")
    if args.steps_per_epoch < 1:
        raise SystemExit("--steps_per_epoch must be at least 1")
    num_agent = agents_of(args)
    torch.manual_seed(0)
    model = SegDiscoNet(num_agent=num_agent, only_v2i=bool(args.only_v2i))
    start_epoch, optimizer_state = 1, None
    if args.resume:
        ck = load_checkpoint(model, args.resume)
        optimizer_state = ck.get("optimizer_state_dict")
        start_epoch = int(ck.get("epoch", 0)) + 1
        print("resumed", args.resume, "-> epoch", start_epoch)
    model.cuda()
    segmodule = SegModule(model, lr=args.lr).build_engine()
    if optimizer_state is not None:
        segmodule.engine.load_state_dict(optimizer_state)
    for epoch in range(start_epoch, start_epoch + args.nepoch):
        t0, running, counted, last = time.perf_counter(), 0.0, 0, float("nan")
        for it in range(args.steps_per_epoch):
            out = segmodule.step(step_data(args, num_agent, epoch, it), args.batch)
            if not out.get("skipped"):         # (a batch without a live image: no step was taken)
                last = out["loss"]
                running += last
                counted += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lr = segmodule.engine.lr
        mean = running / counted if counted else float("nan")
        print("epoch %d: mean loss %.4f  last %.4f  %.1f scenes/s  lr %.2e" % (
            epoch, mean, last, args.batch * args.steps_per_epoch / dt, lr), flush=True)
        if args.logpath:
            os.makedirs(args.logpath, exist_ok=True)
            torch.save({"epoch": epoch, "model_state_dict": model.state_dict(),
                        "optimizer_state_dict": segmodule.engine.state_dict(),
                        "scheduler_state_dict": {"lr": lr}, "loss": mean},
                       os.path.join(args.logpath, "epoch_%d.pth" % epoch))


if __name__ == "__main__":
    main()
