"""Shared inputs of the lidar tests (tests/test_lidar_host_cpu.py, tests/test_gpu_lidar.py): hand cases of the scan rule
as lidar.scan / lidar.host_scan arguments, each built once."""
import functools
import math

import numpy as np

from disconet_amd import lidar

HALF = 32.0


def box(x, y, w=2.0, l=4.0, yaw=0.0, z_lo=-1.0, z_hi=1.0):
    return [x, y, w, l, math.sin(yaw), math.cos(yaw), z_lo, z_hi]


def make(scenes, dirs, agents=1, live=None, objects=None, k=None, nan_pad=False, **kw):
    """scenes: per scene a list of solid rows -> (args, kw) of lidar.scan / lidar.host_scan"""
    S = len(scenes)
    K = max([len(s) for s in scenes] + [0]) if k is None else int(k)
    solids = np.full((S, K, 8), np.nan if nan_pad else 0.0, dtype=np.float64)
    for i, rows in enumerate(scenes):
        if len(rows):
            solids[i, :len(rows)] = np.asarray(rows, dtype=np.float64)
    count = np.array([len(s) for s in scenes], dtype=np.int32)
    objects = count.copy() if objects is None else np.asarray(objects, dtype=np.int32)
    live = np.full(S, agents, dtype=np.int32) if live is None else np.asarray(live, dtype=np.int32)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    kw.setdefault("half_extent", HALF)
    return (solids, count, objects, lidar.sensor_from_world(S, agents), live, dirs), kw


FAN = lidar.beam_table(3, 37, -5.0, 5.0)                 # R = 111: neither a wave nor a block multiple
DOWN = [math.cos(math.radians(-30.0)), 0.0, math.sin(math.radians(-30.0))]


def _random_solids(n, seed):
    rng = np.random.RandomState(seed)
    rows = []
    while len(rows) < n:
        x, y = rng.uniform(-30.0, 30.0, 2)
        if math.hypot(x, y) < 5.0 or math.hypot(x - 6.0 * math.cos(0.7), y - 6.0 * math.sin(0.7)) < 5.0:
            continue
        rows.append(box(x, y, rng.uniform(1.6, 2.4), rng.uniform(3.5, 5.5), rng.uniform(-math.pi, math.pi), -2.0,
                        rng.uniform(-0.5, 1.5)))
    return rows


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (args, kw)"""
    c = {}
    c["dead_ahead"] = make([[box(10.0, 0.0)]], [[1.0, 0.0, 0.0]], min_points=1)
    c["two_in_line"] = make([[box(10.0, 0.0), box(20.0, 0.0)]], FAN, min_points=1)
    c["zero_component"] = make([[box(5.0, 10.0), box(0.0, 10.0)]], [[0.0, 1.0, 0.0]], min_points=1)
    c["sensor_inside"] = make([[box(0.0, 0.0, 4.0, 4.0), box(10.0, 0.0)]], FAN, min_points=1)
    c["range_short"] = make([[box(10.0, 0.0)]], [[1.0, 0.0, 0.0]], max_range=8.5, min_points=1)
    c["range_exact"] = make([[box(10.0, 0.0)]], [[1.0, 0.0, 0.0]], max_range=9.0, min_points=1)
    c["ground_kept"] = make([[box(10.0, 0.0)]], [DOWN, [1.0, 0.0, 0.0]], keep_ground=True, min_points=1)
    c["ground_dropped"] = make([[box(10.0, 0.0)]], [DOWN, [1.0, 0.0, 0.0]], keep_ground=False, min_points=1)
    c["tie"] = make([[box(10.0, 0.0), box(10.0, 0.0)]], FAN, min_points=1)
    c["nan_padding"] = make([[box(10.0, 0.0), box(0.0, 10.0)]], FAN, k=4, nan_pad=True, min_points=1)
    c["no_padding"] = make([[box(10.0, 0.0), box(0.0, 10.0)]], FAN, min_points=1)
    c["padded_agents"] = make([[box(10.0, 0.0), box(0.0, 10.0)], [box(-10.0, 3.0)]], FAN, agents=3, live=[3, 1], min_points=1)
    # ---- the ground-truth rule ----
    inside = float(np.nextafter(HALF, 0.0))
    c["strict_extents"] = make([[box(HALF, 0.0), box(inside, 8.0), box(0.0, -HALF), box(3.0, -inside)]], FAN, min_points=0)
    hidden = [box(16.0, 0.0, z_lo=-2.0, z_hi=-0.5), box(10.0, 0.0, 4.0, 4.0, z_lo=-2.0, z_hi=1.5)]
    wide = lidar.beam_table(16, 256)
    c["seen_by_a_padded_agent"] = make([hidden], wide, agents=2, live=[1], objects=[1], min_points=5)
    c["seen_by_a_live_agent"] = make([hidden], wide, agents=2, live=[2], objects=[1], min_points=5)
    four = [box(10.0, 0.0), box(40.0, 20.0), box(0.0, 10.0), box(-10.0, 0.0)]
    c["compaction"] = make([four], wide, min_points=1, gt_rows=4)
    c["fewer_rows_than_solids"] = make([four + [box(0.0, -10.0)]], wide, objects=[3], min_points=1, gt_rows=3)
    c["no_objects"] = make([four], FAN, objects=[0], min_points=1)
    # ---- shapes ----
    c["no_solids"] = make([[]], FAN, k=0, keep_ground=True)
    c["one_ray"] = make([[box(10.0, 0.0)]], [[1.0, 0.0, 0.0]], keep_ground=True, min_points=1)
    c["most_solids"] = make([_random_solids(lidar.MAX_SOLIDS, 5)], FAN, agents=2, min_points=1, gt_rows=lidar.MAX_SOLIDS)
    c["several_blocks"] = make([_random_solids(20, 6), _random_solids(7, 7)], lidar.beam_table(5, 157), agents=3, live=[3, 1],
                               objects=[12, 7], keep_ground=True, min_points=2, gt_rows=12)
    return c


def jitter_for(args, seed=11):
    """[A*S, R] float32 range jitter of at most 5 cm for a case's arguments"""
    S, A, R = args[0].shape[0], args[3].shape[1], args[5].shape[0]
    return np.random.RandomState(seed).uniform(-0.05, 0.05, (A * S, R)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host(name, jitter=False):
    """host_scan of a case, computed once; nobody writes into it"""
    args, kw = cases()[name]
    return lidar.host_scan(*args, range_jitter=jitter_for(args) if jitter else None, **kw)


@functools.lru_cache(maxsize=None)
def property_scene(seed):
    """the issue's property scene: 5 agents, 256 x 256, the defaults, with the teacher's view"""
    from disconet_amd.synthetic import make_lidar_scene_batch
    return make_lidar_scene_batch(1, 5, 256, seed=seed, teacher=True)
