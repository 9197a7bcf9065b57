"""Shared cases of tests/test_holistic_host_cpu.py and tests/test_gpu_holistic.py.  TEST infrastructure: the scenes, the
crafted cloud whose points sit on voxel faces after the transform, and the two wrong evaluations of the transform that
the crafted cloud tells from the contract of include/disconet_hip.h :: dn_voxelize_views."""
import functools

import numpy as np
import torch

SCENE_64 = dict(batch_size=2, num_agent=3, map_hw=64, seed=5, boxes_per_scene=8)
OWN_CELLS_64 = (1599, 1588, 833, 1085, 439, 631)
HOLISTIC_CELLS_64 = (1767, 1720, 1022, 1280, 569, 767)


def cfg(hw):
    from disconet_amd import Config
    return Config(map_hw=hw)


@functools.lru_cache(maxsize=None)
def scene(batch_size, num_agent, map_hw, seed, boxes_per_scene):
    """host scene + its host holistic views (computed once per process; callers do not write into them)"""
    from disconet_amd.synthetic import make_box_scene_batch
    return make_box_scene_batch(batch_size, num_agent, map_hw, seed=seed, boxes_per_scene=boxes_per_scene, teacher=True)


def scene_64():
    return scene(**SCENE_64)


def crafted_pose():
    from disconet_amd.synthetic import make_trans_matrices
    return make_trans_matrices(1, 3, jitter_seed=7)[0, 0, 2].numpy().copy()


@functools.lru_cache(maxsize=None)
def _near_face_cloud(hw, n, seed):
    T = crafted_pose()
    c = cfg(hw)
    ext = np.asarray(c.area_extents, dtype=np.float64)
    vs = np.asarray(c.voxel_size, dtype=np.float64)
    rng = np.random.RandomState(seed)
    tgt = rng.uniform(ext[:, 0], ext[:, 1], size=(n, 3))
    axis = rng.randint(0, 3, size=n)
    rows = np.arange(n)
    tgt[rows, axis] = np.round(tgt[rows, axis] / vs[axis]) * vs[axis]          # one coordinate exactly on a voxel face
    inv = np.linalg.inv(T.astype(np.float64))
    src = (tgt @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    parts = [src]
    for toward in (np.float32(np.inf), np.float32(-np.inf)):
        p = src
        for _ in range(3):
            p = np.nextafter(p, toward)
            parts.append(p)
    return np.ascontiguousarray(np.concatenate(parts, 0))


def near_face_cloud(T, hw, n=4096, seed=0):
    """7 * n points [., 3] float32 that `T` carries onto (or within three float32 steps of) a voxel face of the hw map:
    n targets uniform in the extents, one random axis of each snapped to round(c / voxel) * voxel, carried through inv(T)
    in float64 and rounded to float32, plus the copies 1, 2 and 3 float32 steps (np.nextafter, every coordinate) to either
    side.  T must be crafted_pose() (the cloud is cached per (hw, n, seed))."""
    assert np.array_equal(np.asarray(T), crafted_pose())
    return _near_face_cloud(hw, n, seed)


def coords_contract(pts, T):
    from disconet_amd.holistic import transform_cloud
    return transform_cloud(pts, T)


def coords_float32_arithmetic(pts, T):
    """the transform evaluated in float32: same order of the sums, every product and sum rounded to float32"""
    p = np.asarray(pts, dtype=np.float32)
    T = np.asarray(T, dtype=np.float32)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)


def coords_float64_unrounded(pts, T):
    """the float64 sums of the contract WITHOUT the rounding to float32"""
    p = np.asarray(pts, dtype=np.float32).astype(np.float64)
    T = np.asarray(T, dtype=np.float32).astype(np.float64)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)


def cells(coords, hw):
    """the voxel rule on coordinates of either precision -> linear cell index per point, -1 = dropped"""
    c = cfg(hw)
    ext = np.asarray(c.area_extents, dtype=np.float64)
    vs = np.asarray(c.voxel_size, dtype=np.float64)
    dims = [int(v) for v in c.map_dims]
    keep = np.ones(len(coords), dtype=bool)
    for d in range(3):
        keep &= (ext[d, 0] < coords[:, d]) & (coords[:, d] < ext[d, 1])
    q = np.zeros((len(coords), 3), dtype=np.int64)
    q[keep] = (np.floor(coords[keep] / vs) - np.floor(ext[:, 0] / vs)).astype(np.int64)
    lin = (q[:, 0] * dims[1] + q[:, 1]) * dims[2] + q[:, 2]
    return np.where(keep, lin, -1)


def grid_of(cell, hw):
    dims = [int(v) for v in cfg(hw).map_dims]
    g = np.zeros(dims[0] * dims[1] * dims[2], dtype=np.float32)
    g[cell[cell >= 0]] = 1.0
    return g.reshape(dims)


def device_scene_views(s, batch, agents, hw, live=None, **kw):
    """holistic.holistic_views on a host scene dict's clouds and poses"""
    from disconet_amd import holistic
    live = [agents] * batch if live is None else live
    return holistic.holistic_views(s["points"], s["trans_matrices"].cuda(), live, batch, cfg(hw), **kw)


def single_source(pts, T, hw, want=("dense", "bits")):
    """ops.voxelize_views of one cloud (device tensor) as one source of one view under pose T (None: pose -1)"""
    from disconet_amd import ops
    c = cfg(hw)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
    poses = torch.as_tensor(np.asarray(T if T is not None else np.eye(4), dtype=np.float32)).cuda().reshape(1, 4, 4)
    return ops.voxelize_views(pts, i32([0]), i32([pts.shape[0]]), i32([0]), i32([-1 if T is None else 0]), poses, 1,
                              pts.shape[0], c.voxel_size, c.area_extents, c.map_dims, want=want)
