#!/usr/bin/env python
"""The stage behind the tracker in the reference's det pipeline (train -> test -> track -> evaluate the tracks: `make
sort`, then `make eval`): the CLEAR MOT figures of SORT's tracks, on the GPU.  Per frame, tracking.Sort.update() and
tracking.ClearMot.update() (behind forward -> postprocess.detect() with --source net) replay as ONE captured graph
(graph.GraphedStep); nothing is copied to the host before the end, where ClearMot.compute() makes one copy of the
counters.  Prints one line per agent and one overall: MOTA, MOTP, TP, FP, FN, IDSW, Frag, MT / PT / ML.  Behind them, the
identity figures in the same form (IDF1, IDP, IDR, IDTP / IDFP / IDFN, Dets, GT_Dets, IDs, GT_IDs): tracking.Identity.update()
runs in the same captured step, and Identity.compute() solves the one global assignment on the device and copies 8 words
per image.  Behind those, HOTA with its detection, association and localisation parts (HOTA, DetA, AssA, DetRe, DetPr,
AssRe, AssPr, LocA, HOTA(0), LocA(0), HOTALocA(0)): tracking.Hota.update() runs in the same captured step and logs every
frame on the device (--max_frames slots), and Hota.compute() matches all logged frames of all images at once there.

    python tools/track/eval_sort.py --com disco|sum|mean|max|lowerbound|late|agent [--source boxes|net|lidar] [--resume ckpt.pth] [--num_agent 5] [--batch 1] \
        [--seed 0] [--detections net|truth] [--frames 8] [--max_age 1] [--min_hits 3] [--iou_threshold 0.3] [--eval_iou 0.5] \
        [--max_gt_ids 256] [--max_track_ids 1024] [--max_frames FRAMES] [--exchange f32|f16|mxfp8|mxfp4] [--exchange_cells N]

--source boxes (default) skips the network: synthetic.make_track_sequence(truth=True) -- moving boxes with detection
noise, misses and false positives, evaluated against their noise-free boxes.  The mode that shows meaningful figures.
--source net runs test_codet.py's model on synthetic.make_box_scene_batch(seed = --seed), the same standing scene every
frame, with the scene's boxes as ground truth and their rows as identities (disconet_amd.Detector: the model, the
checkpoint and the tail of the --com mode).  Without --resume the weights are random -- seeded before the model is built,
so that a run can be reproduced -- and the detections have little to do with the boxes: the run shows the plumbing
only; after `train_codet.py --targets boxes --logpath L`, `--resume L/epoch_N.pth` gives figures that belong to the
detector.
--source lidar runs it on a world that moves: the lidar.Sequence of sequence seed --seed (synthetic.make_lidar_world: cars
and vans in four lanes, parked cars and occluders beside them, every agent a sensor riding in a lane) is stepped, scanned
and voxelised INSIDE the captured step, in front of the detector, and its ground truth -- the cars somebody sees, one id
per car across frames -- goes to the three metrics; a sequence is --frames replays with nothing uploaded between them.
After `train_codet.py --scene lidar --sequence_frames N --targets boxes --logpath L`, `--resume L/epoch_N.pth` gives the
tracking figures of that detector; other seeds are worlds it was not trained on.  --detections truth feeds the frame's
ground-truth boxes to SORT in place of the network: this world's counterpart of --source boxes, meaningful with no
checkpoint (what SORT loses on perfect detections: births, and cars that come back from behind something).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "det"))
sys.path.insert(0, HERE)

from disconet_amd import ALL_DET_COM_MODES, Config, tracking  # noqa: E402
from disconet_amd.synthetic import make_box_scene_batch  # noqa: E402
from codet_common import add_exchange_flag, add_sort_flags, add_source_flags, add_tail_flags, agents_of, check_source_flags, exchange_line, exchange_sent_line, exchanges, require_com  # noqa: E402
from test_codet import build_parser  # noqa: E402  (the evaluation tool's command line)
from track_step import build_step, lidar_net_scene  # noqa: E402


def parse_args(argv=None):
    ap = build_parser()
    add_source_flags(ap, "boxes")     # net: the model on a standing box scene (with untrained weights it shows the plumbing only)
    ap.add_argument("--seed", type=int, default=0,
                    help="make_track_sequence's / make_box_scene_batch's seed; --source lidar: the sequence seed")
    add_tail_flags(ap, 128)
    add_exchange_flag(ap)
    add_sort_flags(ap)
    ap.add_argument("--eval_iou", type=float, default=0.5, help="the IoU a track needs to count for a ground truth")
    ap.add_argument("--max_gt_ids", type=int, default=256)
    ap.add_argument("--max_track_ids", type=int, default=1024, help="the identity figures count track ids 1 .. this")
    ap.add_argument("--max_frames", type=int, default=None, help="frames HOTA logs per image (default: max(--frames, 1))")
    ap.set_defaults(frames=8)
    args = ap.parse_args(argv)
    if args.max_frames is None:
        args.max_frames = max(args.frames, 1)
    require_com(args, ALL_DET_COM_MODES)
    check_source_flags(args)
    return args


def main(argv=None):
    args = parse_args(argv)
    num_agent = agents_of(args)
    n = num_agent * args.batch
    config = Config("test", binary=True, only_det=True)
    scale = 1.0 / config.voxel_size[0]
    sort = tracking.Sort(max_age=args.max_age, min_hits=args.min_hits, iou_threshold=args.iou_threshold, scale=scale,
                         max_tracks=args.max_tracks)
    mot = tracking.ClearMot(args.batch, iou_threshold=args.eval_iou, scale=scale, max_gt_ids=args.max_gt_ids)
    idf = tracking.Identity(args.batch, iou_threshold=args.eval_iou, scale=scale, max_gt_ids=args.max_gt_ids,
                            max_track_ids=args.max_track_ids)
    hota = tracking.Hota(args.batch, scale=scale, max_gt_ids=args.max_gt_ids, max_track_ids=args.max_track_ids,
                         max_frames=args.max_frames)

    def evaluate(tracks, gt):
        return mot.update(tracks, gt), idf.update(tracks, gt), hota.update(tracks, gt)

    def net_scene():                   # a standing scene: every frame sees the same boxes, their rows are the identities
        scene = make_box_scene_batch(args.batch, num_agent, config.map_dims[0], seed=args.seed, device="cuda")
        rows = scene["gt_boxes"].shape[1]
        gt = {"boxes": torch.as_tensor(scene["gt_boxes"]).cuda(), "count": torch.as_tensor(scene["gt_count"]).cuda(),
              "ids": torch.arange(rows, dtype=torch.int32).repeat(n, 1).cuda()}
        return tuple(scene[key].cuda() for key in ("bev_seq", "trans_matrices", "num_agent")), None, gt

    if args.source != "boxes" and args.detections == "net" and not args.resume:
        print("note: untrained weights -- the figures below show the plumbing, not a detector")
    scene = (lambda: lidar_net_scene(args, config)) if args.source == "lidar" else net_scene
    step, load, _ = build_step(args, config, sort, scene, behind=evaluate, truth=True)
    mot.reset()                        # the warm-up runs of the capture advanced the tracker (build_step resets it) and were counted
    idf.reset()
    hota.reset()                       # ... and logged
    if step.detector is not None and step.detector.model.exchange_sent is not None:
        step.detector.model.exchange_sent.zero_()      # ... and sent cells

    for frame in range(args.frames):
        load(frame)
        step()
    step.drain()
    sort.status()                      # raises when a frame was truncated (more than 128 valid rows, no free slot, ...)
    figures = mot.compute()            # the one copy; raises on a sticky status bit of the evaluation
    print("%d frames, %d images (%d agents x batch %d), tracks need IoU >= %g" % (args.frames, n, num_agent, args.batch,
                                                                                  args.eval_iou))
    if exchanges(args):
        print(exchange_line(args, config))
    if args.exchange_cells and step.detector is not None:
        print(exchange_sent_line(args, step.detector))
    for a, row in enumerate(figures["per_agent"]):
        print(tracking.mot_line("agent %d" % a, row))
    print(tracking.mot_line("overall", figures["overall"]))
    identity = idf.compute()           # the assignment on the device, then 8 words per image; raises on a status bit
    for a, row in enumerate(identity["per_agent"]):
        print(tracking.idf_line("agent %d" % a, row))
    print(tracking.idf_line("overall", identity["overall"]))
    higher = hota.compute()            # every logged frame matched on the device; raises on a status bit (a full log too)
    for a, row in enumerate(higher["per_agent"]):
        print(tracking.hota_line("agent %d" % a, row))
    print(tracking.hota_line("overall", higher["overall"]))


if __name__ == "__main__":
    main()
