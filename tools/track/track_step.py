"""The captured per-frame step of the track tools (sort_codet.py, eval_sort.py): detections -> tracking.Sort.update() ->
whatever the tool runs behind it, as ONE graph (graph.GraphedStep), for both --source modes."""
import torch

from disconet_amd import graph
from disconet_amd.synthetic import make_track_sequence
from codet_common import agents_of, detector_from_args

PARTS = {0: ("boxes", "scores", "count"), 2: ("boxes", "ids", "count")}      # a frame of make_track_sequence: detections, ..., truth


def build_step(args, config, sort, net_scene, behind=None, truth=False):
    """-> (step, load, seq): per frame the tool calls load(frame), then step().

    --source boxes: seq = make_track_sequence(truth=truth); static device tensors of the detections (with truth, of the
        ground truth too) that load(frame) copies the frame's rows into.
    --source net: the Detector of the flags on net_scene()'s (inputs, refresh, gt): `inputs` the static device tensors
        (bevs, trans, num_agent), `refresh(frame)` their fresh values for load(frame) to copy in (None: a standing scene),
        `gt` the scene's ground truth (or None).  seq is None.
    behind(tracks, gt) runs behind sort.update() inside the captured step (None: the step returns the tracks).  The
    tracker's reset() follows the capture; whatever `behind` counts is the tool's to reset."""
    seq = None
    if args.source == "boxes":
        seq = make_track_sequence(args.frames, agents_of(args) * args.batch, seed=args.seed, truth=truth)
        static = {part: {key: torch.from_numpy(seq[0][part][key]).cuda() for key in PARTS[part]}
                  for part in ((0, 2) if truth else (0,))}

        def load(frame):
            for part, rows in static.items():
                for key in rows:
                    rows[key].copy_(torch.from_numpy(seq[frame][part][key]))

        def detections():
            return static[0]

        gt = static.get(2)
    else:
        detector = detector_from_args(args, config)
        inputs, refresh, gt = net_scene()

        def load(frame):
            if refresh is not None:
                for dst, src in zip(inputs, refresh(frame)):
                    dst.copy_(src)

        def detections():
            return detector(*inputs)

    def run():
        tracks = sort.update(detections())
        return tracks if behind is None else behind(tracks, gt)

    step = graph.GraphedStep(run)
    sort.reset()                       # the warm-up runs of the capture advanced the tracker
    return step, load, seq
