#!/usr/bin/env python
"""test_seg.py's run on labelled scenes, scored with mean IoU on the GPU -- what eval_codet.py is to test_codet.py.  The
reference's tools/seg/test_seg.py keeps the mIoU bookkeeping in the tool itself; here it is a tool of its own beside the
re-hosted test_seg.py, whose flags it takes (test_seg.build_parser) and whose output it leaves as it is.

    python tools/seg/eval_seg.py --com disco [--resume logs/seg/epoch_N.pth] [--num_agent 5] [--batch 1] [--frames 4] \\
        [--map_hw 256] [--labels scene]

--labels scene (the default and the only choice; the spelling of `train_seg.py --labels scene`): the frames are
    synthetic.make_seg_scene_batch's scenes, seeds 0 .. --frames - 1 (the ones `train_seg.py --labels scene` cycles
    through): SegModule.evaluate(metric=MeanIoU) per frame (one dn_seg_confusion launch
    behind the forward; the counts stay on the device), MeanIoU.compute() once at the end -- one line per agent and one
    overall with mIoU, pixel accuracy and the per-class IoU (seg.miou_line).
That bookkeeping is this project's own contract (include/disconet_seg.h), recalled from upstream's tool, not pinned to it.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "det"))

import test_seg  # noqa: E402  (tools/seg/test_seg.py: the flags)
from codet_common import agents_of  # noqa: E402
from disconet_amd import MeanIoU, SegDiscoNet, SegModule, load_checkpoint  # noqa: E402
from disconet_amd.seg import miou_line  # noqa: E402
from disconet_amd.synthetic import make_seg_scene_batch, randomize_bn_stats  # noqa: E402


def build_parser():
    ap = test_seg.build_parser()
    ap.add_argument("--labels", choices=("scene",), default="scene",
                    help="scene: labelled scenes (the ones train_seg.py --labels scene trains on)")
    return ap


def frame_data(args, num_agent, frame, device="cuda"):
    """The `data` dict of one SegModule.evaluate."""
    scene = make_seg_scene_batch(args.batch, num_agent, args.map_hw, seed=frame, device=device)
    return {k: scene[k] for k in ("bev_seq", "trans_matrices", "num_agent", "labels")}


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.com != "disco":
        raise SystemExit("only --com disco is built on the MI355X path (SURVEY.md §2.1 #8)")
    num_agent = agents_of(args)
    torch.manual_seed(0)
    model = SegDiscoNet(num_agent=num_agent, kd_flag=bool(args.kd_flag), only_v2i=bool(args.only_v2i))
    if args.resume:
        print("loaded", args.resume, "epoch", load_checkpoint(model, args.resume).get("epoch"))
    else:
        randomize_bn_stats(model)
    model.eval().cuda()
    mod = SegModule(model)
    metric = MeanIoU(num_agent * args.batch, model.n_classes)
    for frame in range(args.frames):
        data = frame_data(args, num_agent, frame)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = mod.evaluate(data, args.batch, metric=metric)
        torch.cuda.synchronize()
        print("frame %d: %.2f ms  pred %s  cross entropy %.4f" % (
            frame, 1e3 * (time.perf_counter() - t0), tuple(out["pred"].shape), out["loss"]))
    figures = metric.compute(agents=num_agent)
    for agent, row in enumerate(figures["per_agent"]):
        print(miou_line("agent %d" % agent, row))
    print(miou_line("overall", figures["overall"]))


if __name__ == "__main__":
    main()
