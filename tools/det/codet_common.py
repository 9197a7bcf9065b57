"""What the det, track and seg command lines share: the tail's and SORT's flags, the --com refusal, the --rsu rule and
the Detector of the parsed flags (the reference's flag names; test_codet.build_parser declares them)."""
from disconet_amd import Detector, exchange


def add_tail_flags(ap, pre_nms_top_k):
    ap.add_argument("--pre_nms_top_k", type=int, default=pre_nms_top_k)
    ap.add_argument("--iou_thr", type=float, default=0.01, help="the NMS threshold of detect()")
    ap.add_argument("--score_thr", type=float, default=None)


def add_sort_flags(ap):
    ap.add_argument("--max_age", type=int, default=1)
    ap.add_argument("--min_hits", type=int, default=3)
    ap.add_argument("--iou_threshold", type=float, default=0.3, help="SORT's association threshold")
    ap.add_argument("--max_tracks", type=int, default=128)


def add_exchange_flag(ap):
    ap.add_argument("--exchange", choices=tuple(exchange.FORMATS), default="f32",
                    help="the wire format of the exchanged feature map (--com disco): f16, mxfp8 or mxfp4 put what the "
                         "neighbours receive through exchange.roundtrip; f32 sends it as it is")
    ap.add_argument("--exchange_cells", type=int, default=0,
                    help="how many cells of the exchanged feature map an agent sends (--com disco): the N strongest by "
                         "max |v|, the others arrive as zeros; with any --exchange format; 0 sends every cell")


def exchanges(args):
    """does the command line put the exchanged map through exchange.roundtrip at all (a format or a cell budget)"""
    return getattr(args, "exchange", "f32") != "f32" or getattr(args, "exchange_cells", 0) != 0


def exchange_line(args, config):
    """--exchange other than f32, or --exchange_cells: the line eval_codet.py and eval_sort.py print, the message bytes per
    agent per frame (with a cell budget, of the fixed-capacity message)"""
    from disconet_amd.model import LAYER_CHANNEL
    side = config.map_dims[0] >> args.layer              # the exchanged level's side: level k is the map halved k times
    c = LAYER_CHANNEL[args.layer]
    cells = getattr(args, "exchange_cells", 0)
    if cells:
        return "exchange %s, %d cells: capacity %d bytes per agent per frame (%d of the %d cells of a %d x %d x %d map; f32 %d)" % (
            args.exchange, cells, exchange.cells_message_bytes(args.exchange, side, side, c, cells), cells, side * side,
            side, side, c, exchange.message_bytes("f32", side, side, c))
    return "exchange %s: %d bytes per agent per frame (a %d x %d x %d map; f32 %d)" % (
        args.exchange, exchange.message_bytes(args.exchange, side, side, c), side, side, c,
        exchange.message_bytes("f32", side, side, c))


def exchange_sent_line(args, detector):
    """--exchange_cells: the line the eval tools print after the run, from one read of the model's exchange_sent -- the
    mean cells an agent sent per frame and what a variable-length link would have carried for them"""
    from disconet_amd.model import LAYER_CHANNEL
    seen = detector.model.exchange_sent_summary()
    if seen is None:
        return "exchange sent: nothing (no frame ran)"
    c = LAYER_CHANNEL[args.layer]
    return "exchange sent: %.1f cells per agent per frame on average over %d frames (capacity %d), %.0f bytes sent per agent per frame" % (
        seen["mean_cells"], seen["frames"], args.exchange_cells, exchange.sent_bytes(args.exchange, c, seen["mean_cells"]))


def require_com(args, modes):
    if args.com not in modes:
        raise SystemExit("only --com %s are built on the MI355X path (SURVEY.md §2.1 #8)" % " | ".join(modes))


def agents_of(args):
    """--rsu 1: the road-side unit is one more agent"""
    return args.num_agent + (1 if args.rsu else 0)


LIDAR_SCENE_CARS = 24      # cars of a --scene lidar scene: 24 of the grid's 64 cells at map_hw = 256, so the occluders find free cells


def lidar_scene(batch, num_agent, map_hw, seed, gt_rows, device="cuda", teacher=False):
    """The scene of `--scene lidar` in every det tool: synthetic.make_lidar_scene_batch with LIDAR_SCENE_CARS cars and its
    default ten occluders, the ground truth padded to the tool's `gt_rows` rows.  (The tools' box scenes ask for gt_rows
    cars; that many would take every grid cell and leave no room for an occluder.)"""
    from disconet_amd.synthetic import make_lidar_scene_batch
    return make_lidar_scene_batch(batch, num_agent, map_hw, seed=seed, boxes_per_scene=min(LIDAR_SCENE_CARS, int(gt_rows)),
                                  gt_rows=gt_rows, device=device, teacher=teacher)


LIDAR_SEQUENCE_ROWS = 128    # solids (K) and ground-truth rows (G) of a --source lidar / --sequence_frames world: every slot of
                             # synthetic.make_lidar_world filled is 80 solids, so worlds of every seed share these shapes


def lidar_sequence(batch, num_agent, config, seed, frames, device="cuda"):
    """The moving world of `--source lidar` (track tools) and `--scene lidar --sequence_frames N` (train_codet.py): the
    lidar.Sequence of synthetic.make_lidar_world_batch(seed = the sequence seed), solids and ground truth padded to
    LIDAR_SEQUENCE_ROWS rows, so that every seed's ground truth has one width."""
    from disconet_amd import lidar
    from disconet_amd.synthetic import make_lidar_world_batch
    world = make_lidar_world_batch(batch, num_agent, config.map_dims[0], seed=seed, frames=max(1, int(frames)),
                                   rows=LIDAR_SEQUENCE_ROWS)
    return lidar.Sequence(world, config, gt_rows=LIDAR_SEQUENCE_ROWS, device=device)


def add_source_flags(ap, default):
    """--source / --detections of the track tools"""
    ap.add_argument("--source", choices=("net", "boxes", "lidar"), default=default,
                    help="lidar: a moving world scanned frame after frame inside the captured step (lidar.Sequence), "
                         "--seed picks the sequence")
    ap.add_argument("--detections", choices=("net", "truth"), default="net",
                    help="--source lidar: truth feeds the frame's ground-truth boxes to SORT in place of the network")


def check_source_flags(args):
    if args.detections == "truth" and args.source != "lidar":
        raise SystemExit("--detections truth needs --source lidar: the other sources have no per-frame ground truth to feed")
    if getattr(args, "exchange", "f32") != "f32" and (args.source == "boxes" or args.detections == "truth"):
        raise SystemExit("--exchange %s needs the network's detections (--source net | lidar, --detections net): nothing "
                         "is exchanged otherwise" % args.exchange)
    if getattr(args, "exchange_cells", 0) and (args.source == "boxes" or args.detections == "truth"):
        raise SystemExit("--exchange_cells %d needs the network's detections (--source net | lidar, --detections net): nothing "
                         "is exchanged otherwise" % args.exchange_cells)


def detector_from_args(args, config):
    """the Detector of the command line (the tail's flags and --exchange / --exchange_cells where the tool declares them), and the `loaded`
    line"""
    tail = {k: getattr(args, k) for k in ("pre_nms_top_k", "iou_thr", "score_thr", "exchange", "exchange_cells")
            if hasattr(args, k)}
    det = Detector(args.com, config, agents_of(args), args.batch, layer=args.layer, kd_flag=args.kd_flag,
                   compress_level=args.compress_level, only_v2i=bool(args.only_v2i), resume=args.resume, **tail)
    if args.resume:
        print("loaded", args.resume, "epoch", det.epoch)
    return det
