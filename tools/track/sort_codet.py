#!/usr/bin/env python
"""The last stage of the reference's det pipeline (train -> test -> track): SORT on the GPU behind the detection tail.
Per frame, forward -> postprocess.detect() -> tracking.Sort.update() replay as ONE captured graph (graph.GraphedStep;
nothing is copied to the host but the reported tracks that are written out), and one MOT file per agent
(`frame,id,x1,y1,w,h,score,-1,-1,-1`, rectangles in BEV pixels: scale = 1 / voxel_size[0]) lands under --logpath:
tracks_agent<a>.txt, or tracks_agent<a>_scene<b>.txt for --batch > 1 (every image is its own sequence).

    python tools/track/sort_codet.py --com disco|sum|mean|max|lowerbound|late|agent [--resume ckpt.pth] [--num_agent 5] [--batch 1] [--frames 8] \
        [--logpath logs/track] [--max_age 1] [--min_hits 3] [--iou_threshold 0.3] [--source net|boxes|lidar] [--seed 0] [--detections net|truth]

--source net (default): test_codet.py's model and synthetic scenes (disconet_amd.Detector: the model, the checkpoint and
the tail of the --com mode).  Without --resume the weights are random -- seeded before the model is built, so that a run
can be reproduced -- and the detections of two frames have little to do with each other; the run shows the plumbing.
--source boxes skips the network and feeds synthetic.make_track_sequence (moving boxes with detection noise, misses and
false positives): the mode that shows meaningful tracks, and it prints how many true identities kept a single track id.
--source lidar: the model on a world that moves -- the lidar.Sequence of sequence seed --seed, stepped, scanned and
voxelised inside the captured step (eval_sort.py's docstring says more); --detections truth feeds the frame's ground-truth
boxes to SORT in place of the network.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "det"))
sys.path.insert(0, HERE)

from disconet_amd import ALL_DET_COM_MODES, Config, tracking  # noqa: E402
from disconet_amd.synthetic import make_scene_batch  # noqa: E402
from codet_common import add_exchange_flag, add_sort_flags, add_source_flags, add_tail_flags, agents_of, check_source_flags, require_com  # noqa: E402
from test_codet import build_parser  # noqa: E402  (the evaluation tool's command line)
from track_step import build_step, lidar_net_scene  # noqa: E402


def parse_args(argv=None):
    ap = build_parser()
    add_source_flags(ap, "net")
    ap.add_argument("--seed", type=int, default=0, help="--source boxes: make_track_sequence's seed; --source lidar: the sequence seed")
    add_tail_flags(ap, 128)
    add_exchange_flag(ap)
    add_sort_flags(ap)
    ap.set_defaults(frames=8)
    args = ap.parse_args(argv)
    require_com(args, ALL_DET_COM_MODES)
    check_source_flags(args)
    return args


def main(argv=None):
    args = parse_args(argv)
    num_agent = agents_of(args)
    n = num_agent * args.batch
    config = Config("test", binary=True, only_det=True)
    sort = tracking.Sort(max_age=args.max_age, min_hits=args.min_hits, iou_threshold=args.iou_threshold,
                         scale=1.0 / config.voxel_size[0], max_tracks=args.max_tracks)

    def scene(frame):
        return make_scene_batch(args.batch, num_agent, config.map_dims[0], jitter_seed=frame)

    def net_scene():                   # a fresh scene every frame, no ground truth
        return tuple(t.cuda() for t in scene(0)), scene, None

    if args.source == "lidar" and args.detections == "net" and not args.resume:
        print("note: untrained weights -- the tracks below show the plumbing, not a detector")
    step, load, seq = build_step(args, config, sort, (lambda: lidar_net_scene(args, config)) if args.source == "lidar" else net_scene)

    logpath = args.logpath or os.path.join("logs", "track")
    os.makedirs(logpath, exist_ok=True)
    names = ["tracks_agent%d.txt" % (i // args.batch) if args.batch == 1 else
             "tracks_agent%d_scene%d.txt" % (i // args.batch, i % args.batch) for i in range(n)]
    files = [open(os.path.join(logpath, name), "w") for name in names]
    ids_of = {}                        # (image, true identity) -> the track ids its rows were given
    for frame in range(args.frames):
        load(frame)
        out = step()
        host = {key: out[key].cpu().numpy() for key in ("rect", "id", "score", "count", "det_track")}
        for img, rows in enumerate(tracking.mot_rows(host, frame + 1)):
            files[img].write("".join(row + "\n" for row in rows))
        print("frame %d: tracks reported per image %s" % (frame + 1, host["count"].tolist()))
        if args.source == "boxes":
            ident = seq[frame][1]
            for img, row in zip(*np.nonzero(ident >= 0)):
                ids_of.setdefault((int(img), int(ident[img, row])), set()).add(int(host["det_track"][img, row]))
    step.drain()
    for f in files:
        f.close()
    if args.source == "boxes":
        single = sum(1 for ids in ids_of.values() if len(ids) == 1 and min(ids) > 0)
        print("%d of %d true identities kept a single track id over %d frames" % (single, len(ids_of), args.frames))
    sort.status()                      # raises when a frame was truncated (more than 128 valid rows, no free slot, ...)
    print("wrote %s under %s" % (", ".join(names), logpath))


if __name__ == "__main__":
    main()
