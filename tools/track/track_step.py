"""The captured per-frame step of the track tools (sort_codet.py, eval_sort.py): detections -> tracking.Sort.update() ->
whatever the tool runs behind it, as ONE graph (graph.GraphedStep), for every --source mode."""
import torch

from disconet_amd import graph
from disconet_amd.synthetic import make_track_sequence
from codet_common import agents_of, detector_from_args, lidar_sequence

PARTS = {0: ("boxes", "scores", "count"), 2: ("boxes", "ids", "count")}      # a frame of make_track_sequence: detections, ..., truth


def lidar_net_scene(args, config):
    """net_scene() of --source lidar in both track tools: the lidar.Sequence of sequence seed --seed.  The frame's inputs
    and ground truth come from Sequence.step() inside the captured step; load(0) rewinds the cursor that the capture's
    warm-up runs advanced, every later frame is the next replay with nothing written."""
    seq = lidar_sequence(args.batch, agents_of(args), config, args.seed, args.frames)

    def frame_inputs():
        out = seq.step()
        return (out["bev_seq"], out["trans_matrices"], out["num_agent"]), out["gt"]

    def refresh(frame):
        if frame == 0:
            seq.reset()

    return frame_inputs, refresh, None


def build_step(args, config, sort, net_scene, behind=None, truth=False):
    """-> (step, load, seq): per frame the tool calls load(frame), then step().

    --source boxes: seq = make_track_sequence(truth=truth); static device tensors of the detections (with truth, of the
        ground truth too) that load(frame) copies the frame's rows into.
    --source net: the Detector of the flags on net_scene()'s (inputs, refresh, gt): `inputs` the static device tensors
        (bevs, trans, num_agent), `refresh(frame)` their fresh values for load(frame) to copy in (None: a standing scene),
        `gt` the scene's ground truth (or None).  seq is None.
    --source lidar: the same protocol with a world that moves: `inputs` is a callable that runs INSIDE the captured step and
        returns ((bevs, trans, num_agent), gt) of the frame (lidar.Sequence.step(): a replay advances the world, nothing is
        uploaded), `refresh(frame)` is called for its effect (it seeks the sequence).  --detections truth feeds that gt's
        boxes to the tracker with score 1 and builds no Detector.
    behind(tracks, gt) runs behind sort.update() inside the captured step (None: the step returns the tracks).  The
    tracker's reset() follows the capture; whatever `behind` counts is the tool's to reset.  step.detector is the Detector
    the step runs, or None."""
    seq = None
    detector = None
    if args.source == "boxes":
        seq = make_track_sequence(args.frames, agents_of(args) * args.batch, seed=args.seed, truth=truth)
        static = {part: {key: torch.from_numpy(seq[0][part][key]).cuda() for key in PARTS[part]}
                  for part in ((0, 2) if truth else (0,))}

        def load(frame):
            for part, rows in static.items():
                for key in rows:
                    rows[key].copy_(torch.from_numpy(seq[frame][part][key]))

        gt = static.get(2)
    else:
        truth_dets = getattr(args, "detections", "net") == "truth"
        detector = None if truth_dets else detector_from_args(args, config)
        inputs, refresh, gt = net_scene()
        moving = callable(inputs)

        def load(frame):
            if refresh is None:
                return
            if moving:
                refresh(frame)
            else:
                for dst, src in zip(inputs, refresh(frame)):
                    dst.copy_(src)

        def detections(frame_inputs, frame_gt):
            if truth_dets:
                return {"boxes": frame_gt["boxes"], "scores": torch.ones_like(frame_gt["ids"], dtype=torch.float32),
                        "count": frame_gt["count"]}
            return detector(*frame_inputs)

    def run():
        if args.source == "boxes":
            dets, frame_gt = static[0], gt
        else:
            frame_inputs, frame_gt = inputs() if moving else (inputs, gt)
            dets = detections(frame_inputs, frame_gt)
        tracks = sort.update(dets)
        return tracks if behind is None else behind(tracks, frame_gt)

    step = graph.GraphedStep(run)
    step.detector = detector           # the step's Detector, or None (--source boxes, --detections truth)
    sort.reset()                       # the warm-up runs of the capture advanced the tracker
    return step, load, seq
