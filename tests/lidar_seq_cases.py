"""Cases of the lidar-sequence tests (test_lidar_seq_cpu.py, test_gpu_lidar_seq.py): the hand worlds of dn_lidar_world_step,
the small world of dn_lidar_scan_ids, the generator's worlds with their frames scanned once on the host and shared, and
the geometry the invariants are checked with."""
import functools
import math

import numpy as np

NAN_BITS = 0x7FF8_0000_DEAD_BEEF      # a quiet NaN with a payload: an add would be free to change it, a byte copy is not
CLEARANCE = 0.5


def _row(x, y, yaw=0.0, w=2.0, l=4.5, z_lo=-2.0, z_hi=-0.5):
    return [x, y, w, l, math.sin(yaw), math.cos(yaw), z_lo, z_hi]


def _agents(rng, S, A):
    yaw = rng.uniform(-math.pi, math.pi, (S, A))
    agent0 = np.stack([rng.uniform(-30, 30, (S, A)), rng.uniform(-30, 30, (S, A)), np.sin(yaw), np.cos(yaw)], -1)
    return agent0, rng.uniform(-1.0, 1.0, (S, A, 2))


def world_cases():
    """name -> (world, the cursor [S] int32 at the first call)"""
    rng = np.random.RandomState(154)
    out = {}

    def make(S, K, A, counts):
        yaw = rng.uniform(-math.pi, math.pi, (S, K))
        solids0 = np.stack([rng.uniform(-40, 40, (S, K)), rng.uniform(-40, 40, (S, K)), rng.uniform(1.6, 2.4, (S, K)),
                            rng.uniform(3.5, 5.5, (S, K)), np.sin(yaw), np.cos(yaw), np.full((S, K), -2.0),
                            np.full((S, K), -0.5)], -1).reshape(S, K, 8)
        agent0, agent_vel = _agents(rng, S, A)
        return {"solids0": solids0, "solid_vel": rng.uniform(-1.0, 1.0, (S, K, 2)),
                "solid_count": np.asarray(counts, dtype=np.int32), "agent0": agent0, "agent_vel": agent_vel}

    main = make(2, 5, 3, [3, 5])
    main["solids0"][0, 3:] = np.array([NAN_BITS], dtype=np.uint64).view(np.float64)[0]      # beyond scene 0's count
    main["solids0"][0, 4, 2] = 7.25                                                         # ... and one row with a number
    out["main"] = (main, np.array([0, 7], dtype=np.int32))
    out["no_solids"] = (make(2, 0, 2, [0, 0]), np.array([3, 0], dtype=np.int32))
    out["full_block"] = (make(1, 256, 2, [256]), np.array([11], dtype=np.int32))
    out["one_agent"] = (make(2, 4, 1, [4, 2]), np.array([0, 1], dtype=np.int32))
    near = make(2, 3, 4, [3, 1])                              # sensors within 4 m of the origin, at most 0.2 m a frame: every
    near["agent0"][..., :2] = rng.uniform(-4.0, 4.0, (2, 4, 2))      # relative translation over frames -7 .. 7 is below 16 m
    near["agent_vel"] = rng.uniform(-0.2, 0.2, (2, 4, 2))
    out["near"] = (near, np.array([0, -7], dtype=np.int32))
    out["negative_cursor"] = (make(2, 6, 2, [6, 9]), np.array([-5, -1], dtype=np.int32))    # 9 > K: clamped
    return out


def scan_world():
    """(args, kw) of lidar.scan / host_scan(ids=True): 2 agents (the second 6 m to the side, turned), 8 beams x 256
    azimuths, 12 solids -- 10 cars, the last two rows occluders.  Car 3 is outside the extents (x = 90 of 80); car 7
    stands behind occluder 10 and gets 2 returns from the two agents together, fewer than min_points; car 5, 70 m away, gets exactly min_points = 5 and is
    kept (the test asserts these counts).  G = 4 is smaller than the kept count."""
    from disconet_amd import lidar
    cars = [_row(10, 0), _row(-12, 3, 0.4), _row(6, -9, 1.2), _row(90, 0), _row(-8, -8, 2.0), _row(70, 20, 0.3),
            _row(15, 12, -0.7), _row(28, 0.5), _row(-20, -15, 0.9), _row(3, 14, 1.5)]
    blocks = [_row(20, 0.5, 0.0, 4.0, 4.0, -2.0, 1.5), _row(-15, 14, 0.0, 4.0, 4.0, -2.0, 1.5)]
    solids = np.asarray([cars + blocks], dtype=np.float64)
    pose = np.zeros((1, 2, 4, 4), dtype=np.float64)
    for a, (x, y, yaw) in enumerate(((0.0, 0.0, 0.0), (2.0, 6.0, 0.3))):
        c, s = math.cos(yaw), math.sin(yaw)
        pose[0, a] = [[c, s, 0, -(c * x + s * y)], [-s, c, 0, s * x - c * y], [0, 0, 1, 0], [0, 0, 0, 1]]
    args = (solids, np.array([12], dtype=np.int32), np.array([10], dtype=np.int32), pose, np.array([2], dtype=np.int32),
            lidar.beam_table(8, 256))
    return args, dict(min_points=5, half_extent=80.0, max_range=100.0)


def corners(row, grow=0.0):
    """the footprint's corners [4, 2]: w along the heading (cos, sin), l across it, both half sizes grown by `grow`"""
    x, y, w, l, s, c = (float(v) for v in row[:6])
    hw, hl = w / 2.0 + grow, l / 2.0 + grow
    loc = np.array([[hw, hl], [hw, -hl], [-hw, -hl], [-hw, hl]])
    return np.stack([x + loc[:, 0] * c - loc[:, 1] * s, y + loc[:, 0] * s + loc[:, 1] * c], 1)


def footprints_overlap(a, b, grow=0.0):
    """rotated separating-axis test of two rows' footprints, each grown by `grow` on every side.  Two footprints whose
    forms grown by CLEARANCE / 2 do not overlap are at least CLEARANCE apart (each grown form holds the disc sum)."""
    ca, cb = corners(a, grow), corners(b, grow)
    for row in (a, b):
        s, c = float(row[4]), float(row[5])
        for ax in ((c, s), (-s, c)):
            pa, pb = ca @ np.asarray(ax), cb @ np.asarray(ax)
            if pa.max() < pb.min() or pb.max() < pa.min():
                return False
    return True


def world_at(world, f):
    """(solids [n, 8] of the live rows, sensors [A, 2]) of a make_lidar_world scene at frame f"""
    from disconet_amd import lidar
    w = lidar.host_world_step(world, f)
    n = int(world["solid_count"][0])
    xy = world["agent0"][0, :, :2] + float(f) * world["agent_vel"][0]
    return w["solids"][0, :n], xy


@functools.lru_cache(maxsize=None)
def generated(num_agent, frames, seed):
    """(world, sequence (host only), per frame {"gt", "gt_own_hits"}) of make_lidar_world at 256 x 256 with the tools'
    padding -- scanned once on the host, shared by the tests, and left unchanged"""
    from disconet_amd import Config, lidar
    from disconet_amd.synthetic import make_lidar_world
    world = make_lidar_world(num_agent, 256, seed, 0, frames, rows=128)
    seq = lidar.Sequence(world, Config(map_hw=256), gt_rows=128, device=None)
    steps = []
    for f in range(frames):
        r = seq.host_step(f)
        steps.append({"gt": r["gt"], "gt_own_hits": r["gt_own_hits"]})
    return world, seq, steps


def existence_counts(steps, num_agent, min_points=5):
    """per agent (identities that appear after frame 0, that disappear before the last frame, that had fewer than min_points
    returns of the ego's own in some frame while they were ground truth)"""
    frames = len(steps)
    out = []
    for a in range(num_agent):
        seen = {}
        for f, st in enumerate(steps):
            c = int(st["gt"]["count"][a])
            for ident, own in zip(st["gt"]["ids"][a, :c], st["gt_own_hits"][a, :c]):
                seen.setdefault(int(ident), []).append((f, int(own)))
        out.append((sum(1 for v in seen.values() if v[0][0] > 0), sum(1 for v in seen.values() if v[-1][0] < frames - 1),
                    sum(1 for v in seen.values() if any(own < min_points for _, own in v))))
    return out


def host_mot(steps, scale=4.0, permute_ids=False):
    """HostSort fed the ground-truth boxes as detections (the tools' tracker defaults), scored by HostClearMot against the
    ground truth with its ids -> (figures, the tracking lines as eval_sort.py prints them).  permute_ids: every frame's
    valid ids shuffled among its rows (seeded) -- ids that mean nothing, which the metric must see."""
    from disconet_amd import tracking
    sort = tracking.HostSort(max_age=1, min_hits=3, iou_threshold=0.3, scale=scale, max_tracks=128)
    mot = tracking.HostClearMot(1, iou_threshold=0.5, scale=scale, max_gt_ids=256)
    rng = np.random.RandomState(7)
    for st in steps:
        gt = st["gt"]
        if permute_ids:
            ids = gt["ids"].copy()
            for img in range(ids.shape[0]):
                c = int(gt["count"][img])
                ids[img, :c] = rng.permutation(ids[img, :c])
            gt = dict(gt, ids=ids)
        det = {"boxes": gt["boxes"], "scores": np.ones(gt["ids"].shape, dtype=np.float32), "count": gt["count"]}
        mot.update(sort.update(det), gt)
    figures = mot.compute()
    lines = [tracking.mot_line("agent %d" % a, row) for a, row in enumerate(figures["per_agent"])]
    return figures, lines + [tracking.mot_line("overall", figures["overall"])]
