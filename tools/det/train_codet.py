#!/usr/bin/env python
"""Thin re-hosting of the reference's training entry point for `--com disco`
(flag names from /root/reference/README.md:54-63).  The reference's tool body -- V2X-Sim
loading, anchor / target assembly, logging -- is out of scope; this shim
builds the student (and, with --kd_flag 1, the teacher) the way the reference's tool does,
resumes from `--resume` / `--resume_teacher` if given, and runs CoDetModule.step on synthetic
scenes and targets (there is no V2X-Sim data in this environment) through the MI355X path,
writing `epoch_N.pth` with the reference's checkpoint keys.

    python tools/det/train_codet.py --com disco|sum|mean|max|lowerbound|agent [--batch 4] [--nepoch 2] [--steps_per_epoch 8] \
        [--kd_flag 1 --resume_teacher teacher.pth --kd_weight 100000] [--resume epoch_1.pth] \
        [--logpath logs/] [--num_agent 5] [--layer 3] [--compress_level 0] [--only_v2i 0] \
        [--targets synthetic|boxes] [--pos_thr 0.6] [--neg_thr 0.45] [--scenes 4] [--loss_type faf_loss|corner_loss] \
        [--scene boxes|lidar] [--sequence_frames 0]

--targets synthetic (default): random occupancy and synthetic.make_train_targets (Bernoulli noise per anchor).
--targets boxes: synthetic.make_box_scene_batch -- scenes whose occupancy shows their ground-truth boxes -- with
    targets.assign_targets (dn_assign_targets, on the GPU) called every step: the anchor assignment the reference runs
    when it creates the dataset.  The steps cycle through the scene seeds 0 .. --scenes - 1, the frames that
    `eval_codet.py --gt scene --resume <logpath>/epoch_N.pth` then scores against their own boxes.
    With --kd_flag 1 the scenes also carry the teacher's holistic view (every agent's cloud merged into each ego's frame and
    voxelised: holistic.holistic_views, dn_voxelize_views, one launch per step) as data["bev_seq_teacher"]:

        python tools/det/train_codet.py --com disco --targets boxes --kd_flag 1 --resume_teacher teacher.pth

    Without --resume_teacher the teacher keeps its initial weights: the distillation target is then meaningless and only
    the plumbing is exercised (the tool says so).  Training the teacher itself is not built yet (TeacherNet is eval() only).

--scene lidar --sequence_frames N (N > 0, with --targets boxes): moving worlds instead of standing scenes -- a step's scene
    is sequence seed it % --scenes ((it * world + rank) % --scenes with several ranks; synthetic.make_lidar_world through
    lidar.Sequence) sought to frame (steps so far // --scenes) % N, the targets assigned from that frame's ground truth.  `eval_sort.py --source lidar --resume <logpath>/epoch_N.pth` then
    tracks with a detector that has seen moving worlds; --seed at or above --scenes picks a world it was not trained on.

--loss_type faf_loss (default): focal + smooth-L1 on the box codes.  corner_loss: focal + the corner distances of the decoded
    boxes (Config.loss_type, train_ops.det_loss_corner); the anchors it decodes against ride in data["anchors"].

Data-parallel: one process per GPU under torch.distributed.run; every rank trains its own
scenes and the flat gradient buffer is averaged by one RCCL all-reduce per step.
"""
import argparse
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from disconet_amd import COM_MODES, PARAM_COM_MODES, CoDetModule, Config, TeacherNet, build_model, load_checkpoint  # noqa: E402
from disconet_amd.synthetic import make_bevs, make_box_scene_batch, make_scene_batch, make_train_targets  # noqa: E402
from codet_common import agents_of, lidar_scene, lidar_sequence, require_com  # noqa: E402


TRAIN_COM_MODES = COM_MODES + ("lowerbound",) + PARAM_COM_MODES
SCENE_BOXES = 64      # --targets boxes: boxes per scene (eval_codet.py --gt scene builds the same scenes)


def _rsu_from_leftovers(args, rest):
    """The README writes the last flag as `-- rsu [0/1]` (a space after the dashes,
    /root/reference/README.md:63): argparse then sees "--" and the words `rsu` and `<value>`.
    Accept that spelling; anything else left over is an error, as argparse would report."""
    rest = [r for r in rest if r != "--"]
    if len(rest) == 2 and rest[0] == "rsu":
        digits = "".join(ch for ch in rest[1] if ch.isdigit())
        args.rsu = int(digits[-1]) if digits else 0     # "[0/1]" -> the placeholder's second choice
        rest = []
    if rest:
        raise SystemExit("unrecognized arguments: " + " ".join(rest))
    return args


def newest_checkpoint(path):
    """--auto_resume_path: the epoch_N.pth with the largest N under `path` (None if there is none)"""
    best, best_n = None, -1
    if path and os.path.isdir(path):
        for name in os.listdir(path):
            if name.startswith("epoch_") and name.endswith(".pth"):
                try:
                    n = int(name[len("epoch_"):-len(".pth")])
                except ValueError:
                    continue
                if n > best_n:
                    best, best_n = os.path.join(path, name), n
    return best


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("-d", "--data", default=None, help="(unused here: synthetic scenes)")
    ap.add_argument("--com", default="disco")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--nepoch", type=int, default=2)
    ap.add_argument("--steps_per_epoch", type=int, default=8)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--nworker", type=int, default=0)
    ap.add_argument("--log", action="store_true")
    ap.add_argument("--logpath", default="")
    ap.add_argument("--resume", default="")
    ap.add_argument("--resume_teacher", default="")
    ap.add_argument("--layer", type=int, default=3)
    ap.add_argument("--kd_flag", type=int, default=0)
    ap.add_argument("--kd_weight", type=float, default=100000.0)
    ap.add_argument("--num_agent", type=int, default=5)
    ap.add_argument("--rsu", type=int, default=0)
    ap.add_argument("--compress_level", type=int, default=0)
    ap.add_argument("--only_v2i", type=int, default=0)
    ap.add_argument("--auto_resume_path", default="",
                    help="resume from the newest epoch_N.pth under this directory, if any")
    ap.add_argument("--targets", choices=("synthetic", "boxes"), default="synthetic",
                    help="boxes: scenes with ground-truth boxes, targets assigned on the GPU every step")
    ap.add_argument("--pos_thr", type=float, default=0.6, help="--targets boxes: an anchor is positive from this IoU")
    ap.add_argument("--neg_thr", type=float, default=0.45, help="--targets boxes: an anchor is negative below this IoU")
    ap.add_argument("--scenes", type=int, default=4, help="--targets boxes: the steps cycle through this many scene seeds")
    ap.add_argument("--loss_type", choices=("faf_loss", "corner_loss"), default="faf_loss",
                    help="localisation loss: smooth-L1 on the box codes, or the corner distances of the decoded boxes")
    ap.add_argument("--scene", choices=("boxes", "lidar"), default="boxes",
                    help="--targets boxes: lidar = the same cars seen by ray-cast scans with occluders "
                         "(synthetic.make_lidar_scene_batch), the ground truth what somebody in the scene sees")
    ap.add_argument("--sequence_frames", type=int, default=0,
                    help="--scene lidar: N > 0 trains on moving worlds (lidar.Sequence): a step's scene is sequence seed "
                         "it %% --scenes (with several ranks (it * world + rank) %% --scenes) sought to frame "
                         "(steps so far // --scenes) %% N; 0: the static lidar scenes")
    return ap


def parse_args(argv=None):
    args, rest = build_parser().parse_known_args(argv)
    return _rsu_from_leftovers(args, rest)


_SEQUENCES = {}      # --sequence_frames: sequence seed -> its lidar.Sequence (a few small device tensors each)


def sequence_frame(args, num_agent, config, epoch, it, world=1, rank=0, device="cuda"):
    """--scene lidar --sequence_frames N: the scene of step `it` -- sequence seed (it * world + rank) % --scenes: it % --scenes
    on one GPU, as the static scenes cycle --, sought to frame (steps so far // --scenes) % N, the steps so far counted over
    all epochs and ranks, so that every seed walks through its N frames as the epochs go by -- in make_lidar_scene_batch's
    keys (the ground truth of that frame, what somebody in the scene sees)."""
    step = ((epoch - 1) * args.steps_per_epoch + it) * world + rank
    scenes = max(1, args.scenes)
    seed, frame = (it * world + rank) % scenes, (step // scenes) % args.sequence_frames
    seq = _SEQUENCES.get(seed)
    if seq is None:
        seq = _SEQUENCES[seed] = lidar_sequence(args.batch, num_agent, config, seed, args.sequence_frames, device=device)
    seq.seek(frame)
    out = seq.step(teacher=bool(args.kd_flag))
    out["gt_boxes"], out["gt_count"] = out["gt"]["boxes"], out["gt"]["count"]
    return out


def step_data(args, num_agent, hw, epoch, it, world=1, rank=0, anchors=None, device="cuda", config=None):
    """The `data` dict of one CoDetModule.step."""
    n_img = num_agent * args.batch
    if args.targets == "boxes":
        from disconet_amd import targets
        seed = ((epoch * 1000 + it) * world + rank) % max(1, args.scenes)
        if args.scene == "lidar" and args.sequence_frames > 0:
            scene = sequence_frame(args, num_agent, config, epoch, it, world, rank, device)
        elif args.scene == "lidar":
            scene = lidar_scene(args.batch, num_agent, hw, seed, SCENE_BOXES, device=device, teacher=bool(args.kd_flag))
        else:
            scene = make_box_scene_batch(args.batch, num_agent, hw, seed=seed, boxes_per_scene=SCENE_BOXES, device=device,
                                         teacher=bool(args.kd_flag))
        data = {k: scene[k] for k in ("bev_seq", "trans_matrices", "num_agent")}
        data.update(targets.assign_targets(anchors, scene["gt_boxes"], scene["gt_count"], args.pos_thr, args.neg_thr))
        data["anchors"] = anchors
        if args.kd_flag:
            data["bev_seq_teacher"] = scene["bev_seq_teacher"]
            data["kd_weight"] = args.kd_weight
        return data
    seed = (epoch * 1000 + it) * world + rank
    bevs, trans, na = make_scene_batch(args.batch, num_agent, hw, jitter_seed=seed)
    labels, targets, mask = make_train_targets(n_img, hw, seed=seed)
    data = {"bev_seq": bevs.to(device), "trans_matrices": trans.to(device), "num_agent": na.to(device),
            "labels": labels.to(device), "reg_targets": targets.to(device), "reg_loss_mask": mask.to(device)}
    if anchors is not None:      # (read by --loss_type corner_loss only)
        data["anchors"] = anchors
    if args.kd_flag:
        data["bev_seq_teacher"] = make_bevs(args.batch, num_agent, hw, p=0.05).to(device)
        data["kd_weight"] = args.kd_weight
    return data


def main(argv=None):
    args = parse_args(argv)
    if args.auto_resume_path and not args.resume:
        found = newest_checkpoint(args.auto_resume_path)
        if found:
            args.resume = found
    if args.com == "late":
        raise SystemExit("--com late has nothing of its own to train: train --com lowerbound and pass its checkpoint to the "
                         "det / track tools with --com late")
    require_com(args, TRAIN_COM_MODES)
    if args.scene == "lidar" and args.targets != "boxes":
        raise SystemExit("--scene lidar needs --targets boxes: the lidar scenes come with ground-truth boxes, not with targets")
    if args.sequence_frames < 0 or (args.sequence_frames and (args.scene != "lidar" or args.targets != "boxes")):
        raise SystemExit("--sequence_frames N >= 0, and N > 0 needs --scene lidar --targets boxes: the moving worlds are lidar "
                         "scenes, and they come with ground-truth boxes, not with targets")
    num_agent = agents_of(args)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl")

    config = Config("train", binary=True, only_det=True, loss_type=args.loss_type)
    hw = config.map_dims[0]
    torch.manual_seed(0)
    model = build_model(args.com, config, layer=args.layer, kd_flag=args.kd_flag, num_agent=num_agent,
                        compress_level=args.compress_level, only_v2i=bool(args.only_v2i)).cuda()
    teacher = None
    if args.kd_flag:
        teacher = TeacherNet(config).cuda()
        if args.resume_teacher:
            teacher.load_state_dict(torch.load(args.resume_teacher, map_location="cpu")["model_state_dict"])
            if rank == 0:
                print("teacher: resumed from", args.resume_teacher)
        elif rank == 0:
            print("teacher: no --resume_teacher, the teacher has its INITIAL weights: the distillation target is meaningless, "
                  "this run exercises the plumbing only")
        teacher.eval()
    start_epoch = 1
    optimizer_state = None
    if args.resume:
        ck = load_checkpoint(model, args.resume)
        optimizer_state = ck.get("optimizer_state_dict")
        start_epoch = int(ck.get("epoch", 0)) + 1
        print("resumed", args.resume, "-> epoch", start_epoch)
    fafmodule = CoDetModule(model, teacher, config, None, kd_flag=args.kd_flag, lr=args.lr)
    if optimizer_state is not None:
        fafmodule.engine.load_state_dict(optimizer_state)

    from disconet_amd import postprocess
    anchors = postprocess.make_anchors(config)      # once: the target assignment (--targets boxes) and the corner loss read them
    for epoch in range(start_epoch, start_epoch + args.nepoch):
        t0, running = time.perf_counter(), 0.0
        for it in range(args.steps_per_epoch):
            data = step_data(args, num_agent, hw, epoch, it, world, rank, anchors, config=config)
            out = fafmodule.step(data, args.batch)
            running += out["loss"]
        torch.cuda.synchronize()
        lr = fafmodule.scheduler_step(epoch)
        dt = time.perf_counter() - t0
        if rank == 0:
            fb = fafmodule.engine.f32_fallback_steps      # backward passes repeated on the fp32 kernels (a gradient outgrew its lift)
            print("epoch %d: mean loss %.4f  (%s)  %.1f scenes/s  lr %.2e%s" % (
                epoch, running / args.steps_per_epoch,
                ", ".join("%s %.4f" % (k, v) for k, v in out.items() if k != "loss"),
                world * args.batch * args.steps_per_epoch / dt, lr,
                "  [%d fp32 fallback step(s) so far]" % fb if fb else ""))
            if args.logpath:
                os.makedirs(args.logpath, exist_ok=True)
                torch.save({"epoch": epoch, "model_state_dict": model.state_dict(),
                            "optimizer_state_dict": fafmodule.engine.state_dict(),
                            "scheduler_state_dict": {"lr": lr}, "loss": running / args.steps_per_epoch},
                           os.path.join(args.logpath, "epoch_%d.pth" % epoch))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
