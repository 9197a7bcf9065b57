#!/usr/bin/env python
"""eval_codet.py's loop with pictures: per frame the forward, the detection tail and disconet_amd.render_bev -- one launch
for every image of the batch -- and one PNG per frame and live agent under --logpath.

    python tools/det/visualize_codet.py --com disco|sum|mean|max|lowerbound|late|agent [--resume ckpt.pth] [--num_agent 5] \
        [--batch 1] [--frames 4] [--scale 2] [--gt scene|none] [--tracks 1] [--attention 1] [--map_hw 256] [--logpath logs/vis]

Frame f is synthetic.make_box_scene_batch(seed=f).  A picture shows the scene's occupancy, the ground truth (--gt scene) as a
green outline and the detections coloured by score (blue at 0 to red at 1).  Canvas rows are BEV x, columns BEV y, as
in bev_seq -- no flip.
--tracks 1: the boxes are those that tracking.Sort matched to a track or started one from, coloured by the track's id.
--attention 1 (--com disco only): also attention_f<frame>_agent<i>[_scene<b>].png, the ego's DiscoGraph sheet -- one panel
    per entry of its neighbour list (own map first), the entry's per-pixel weight laid over the scene.
Padded agent slots (agent >= the scene's live count) are not written.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from disconet_amd import ALL_DET_COM_MODES, BoxLayer, Config, render, tracking  # noqa: E402
from disconet_amd.synthetic import make_box_scene_batch  # noqa: E402
from codet_common import add_exchange_flag, add_sort_flags, add_tail_flags, agents_of, detector_from_args, lidar_scene, require_com  # noqa: E402
from test_codet import build_parser  # noqa: E402  (the evaluation tool's command line)

GT_MAX_BOXES = 64


def build_vis_parser():
    ap = build_parser()
    add_tail_flags(ap, 300)
    add_exchange_flag(ap)
    add_sort_flags(ap)
    ap.add_argument("--gt", choices=("scene", "none"), default="scene")
    ap.add_argument("--scale", type=int, default=2, choices=render.SCALES, help="canvas pixels per BEV cell")
    ap.add_argument("--tracks", type=int, default=0, help="1: boxes from SORT, coloured by id")
    ap.add_argument("--attention", type=int, default=0, help="1: the DiscoGraph weight sheet of every ego (--com disco)")
    ap.add_argument("--map_hw", type=int, default=256)
    ap.add_argument("--scene", choices=("boxes", "lidar"), default="boxes",
                    help="lidar: synthetic.make_lidar_scene_batch, ray-cast scans with occluders and the visible ground truth")
    return ap


def image_name(kind, frame, image, batch):
    agent, b = image // batch, image % batch
    return "%s_f%03d_agent%d%s.png" % (kind, frame, agent, "" if batch == 1 else "_scene%d" % b)


def main(argv=None):
    args = build_vis_parser().parse_args(argv)
    require_com(args, ALL_DET_COM_MODES)
    if args.attention and args.com != "disco":
        raise SystemExit("--attention 1 draws the DiscoGraph weights: --com disco only (got --com %s)" % args.com)
    num_agent = agents_of(args)
    config = Config("test", binary=True, only_det=True, map_hw=args.map_hw)
    detector = detector_from_args(args, config)
    sort = tracking.Sort(max_age=args.max_age, min_hits=args.min_hits, iou_threshold=args.iou_threshold,
                         scale=1.0 / config.voxel_size[0], max_tracks=args.max_tracks) if args.tracks else None
    logpath = args.logpath or os.path.join("logs", "vis")
    os.makedirs(logpath, exist_ok=True)
    written = 0
    for frame in range(args.frames):
        if args.scene == "lidar":
            scene = lidar_scene(args.batch, num_agent, config.map_dims[0], frame, GT_MAX_BOXES)
        else:
            scene = make_box_scene_batch(args.batch, num_agent, config.map_dims[0], seed=frame, boxes_per_scene=GT_MAX_BOXES,
                                         device="cuda")
        bevs, trans, na = scene["bev_seq"].cuda(), scene["trans_matrices"].cuda(), scene["num_agent"].cuda()
        det = detector(bevs, trans, na)
        layers = []
        if args.gt == "scene":
            layers.append(BoxLayer.ground_truth(scene["gt_boxes"].cuda(), scene["gt_count"].cuda()))
        layers.append(BoxLayer.tracks(det, sort.update(det)) if sort else BoxLayer.detections(det))
        words = render.occupancy_words(bevs)
        canvas = render.render_bev(config, background=words, layers=layers, scale=args.scale).cpu().numpy()
        weights = render.disco_weights(detector.model, bevs, trans, na, args.batch) if args.attention else None
        live = na[:, 0].cpu().tolist()
        for image in range(canvas.shape[0]):
            agent, b = image // args.batch, image % args.batch
            if agent >= live[b]:
                continue
            render.write_png(os.path.join(logpath, image_name("frame", frame, image, args.batch)), canvas[image])
            written += 1
            if weights is not None:
                sheet = render.attention_sheet(config, words, weights, b, agent, live[b], batch_size=args.batch,
                                               only_v2i=bool(args.only_v2i), scale=args.scale)
                render.write_png(os.path.join(logpath, image_name("attention", frame, image, args.batch)), sheet)
                written += 1
    if sort:
        sort.status()
    print("wrote %d PNG files under %s (%d frames, scale %d)" % (written, logpath, args.frames, args.scale))


if __name__ == "__main__":
    main()
