#!/usr/bin/env python
"""The last stage of the reference's det pipeline (train -> test -> track): SORT on the GPU behind the detection tail.
Per frame, forward -> postprocess.detect() -> tracking.Sort.update() replay as ONE captured graph (graph.GraphedStep;
nothing is copied to the host but the reported tracks that are written out), and one MOT file per agent
(`frame,id,x1,y1,w,h,score,-1,-1,-1`, rectangles in BEV pixels: scale = 1 / voxel_size[0]) lands under --logpath:
tracks_agent<a>.txt, or tracks_agent<a>_scene<b>.txt for --batch > 1 (every image is its own sequence).

    python tools/track/sort_codet.py --com disco|sum|mean|max|lowerbound|late [--resume ckpt.pth] [--num_agent 5] [--batch 1] [--frames 8] \
        [--logpath logs/track] [--max_age 1] [--min_hits 3] [--iou_threshold 0.3] [--source net|boxes]

--source net (default): test_codet.py's model and synthetic scenes.  With random weights the detections of two frames
have little to do with each other; the run shows the plumbing.  --source boxes skips the network and feeds
synthetic.make_track_sequence (moving boxes with detection noise, misses and false positives): the mode that shows
meaningful tracks, and it prints how many true identities kept a single track id.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "det"))

from disconet_amd import DET_COM_MODES, Config, build_model, graph, postprocess, tracking  # noqa: E402
from disconet_amd.synthetic import make_scene_batch, make_track_sequence, randomize_bn_stats  # noqa: E402
from test_codet import build_parser  # noqa: E402  (the evaluation tool's command line)


def main(argv=None):
    ap = build_parser()
    ap.add_argument("--source", choices=("net", "boxes"), default="net")
    ap.add_argument("--seed", type=int, default=0, help="--source boxes: make_track_sequence's seed")
    ap.add_argument("--pre_nms_top_k", type=int, default=128)
    ap.add_argument("--iou_thr", type=float, default=0.01, help="the NMS threshold of detect()")
    ap.add_argument("--score_thr", type=float, default=None)
    ap.add_argument("--max_age", type=int, default=1)
    ap.add_argument("--min_hits", type=int, default=3)
    ap.add_argument("--iou_threshold", type=float, default=0.3, help="SORT's association threshold")
    ap.add_argument("--max_tracks", type=int, default=128)
    ap.set_defaults(frames=8)
    args = ap.parse_args(argv)
    if args.com not in DET_COM_MODES:
        raise SystemExit("only --com disco | sum | mean | max | lowerbound | late are built on the MI355X path (SURVEY.md §2.1 #8)")
    num_agent = args.num_agent + (1 if args.rsu else 0)
    n = num_agent * args.batch
    config = Config("test", binary=True, only_det=True)
    sort = tracking.Sort(max_age=args.max_age, min_hits=args.min_hits, iou_threshold=args.iou_threshold,
                         scale=1.0 / config.voxel_size[0], max_tracks=args.max_tracks)

    if args.source == "boxes":
        seq = make_track_sequence(args.frames, n, seed=args.seed)
        static = {key: torch.from_numpy(seq[0][0][key]).cuda() for key in ("boxes", "scores", "count")}

        def load(frame):
            for key in static:
                static[key].copy_(torch.from_numpy(seq[frame][0][key]))

        step = graph.GraphedStep(lambda: sort.update(static))
    else:
        model = build_model(args.com, config, layer=args.layer, kd_flag=args.kd_flag, num_agent=num_agent,
                            compress_level=args.compress_level, only_v2i=bool(args.only_v2i))
        if args.resume:
            checkpoint = torch.load(args.resume, map_location="cpu", weights_only=False)
            model.load_state_dict(checkpoint["model_state_dict"])
            print("loaded", args.resume, "epoch", checkpoint.get("epoch"))
        else:
            torch.manual_seed(0)
            randomize_bn_stats(model)
        model.eval().cuda()
        anchors = postprocess.make_anchors(config)
        bevs, trans, na = (t.cuda() for t in make_scene_batch(args.batch, num_agent, config.map_dims[0], jitter_seed=0))

        def load(frame):
            fresh = make_scene_batch(args.batch, num_agent, config.map_dims[0], jitter_seed=frame)
            for dst, src in zip((bevs, trans, na), fresh):
                dst.copy_(src)

        def forward_detect_track():
            with torch.no_grad():
                out = model(bevs, trans, na, args.batch)
            det = postprocess.detect(out[0] if isinstance(out, tuple) else out, anchors,
                                     pre_nms_top_k=args.pre_nms_top_k, iou_thr=args.iou_thr, score_thr=args.score_thr)
            if args.com == "late":        # inside the captured step: every agent's boxes merged in each ego's frame
                det = postprocess.late_fuse(det, trans, na, args.batch, num_agent, iou_thr=args.iou_thr,
                                            only_v2i=bool(args.only_v2i), extents=config.area_extents[:2])
            return sort.update(det)

        step = graph.GraphedStep(forward_detect_track)
    sort.reset()                       # the warm-up runs of the capture advanced the tracker

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
