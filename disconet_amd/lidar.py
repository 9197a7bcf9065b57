"""Occlusion-aware lidar scenes: a spinning lidar's rays cast from every agent's pose against the scene's solids (boxes with
a z range), the nearest hit kept, and the ground truth that somebody in the scene can see -- on the GPU in one call (scan,
C ABI dn_lidar_scan: graph-capturable, no host read) and as the numpy / float64 statement of the same rule (host_scan), which
the device equals in every byte.  include/disconet_hip.h states the rule in full.  It is this project's own sensor model: the
reference ships CARLA recordings, not a simulator.

The cloud goes to the voxeliser that already exists: scan()["cloud"] is holistic.pack_clouds' form, so
holistic.holistic_views(cloud, ..., own=True) yields bev_seq and bev_seq_teacher in one more launch; a miss is a row of NaNs,
which the voxeliser's strict extent test drops.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .ops import _need_gpu, _ptr, _stream

MAX_SOLIDS = 256                  # DN_LIDAR_MAX_SOLIDS of include/disconet_hip.h
MAX_RANGE = 80.0                  # defaults of scan / host_scan (m)
GROUND_Z = -2.0                   # the floor of synthetic.BOX_Z: the sensor sits 2 m above the ground
_NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def beam_table(beams=32, azimuths=1024, elev_lo_deg=-30.0, elev_hi_deg=10.0):
    """Unit ray directions of a spinning lidar in the sensor frame, [beams * azimuths, 3] float64: beam b (elevation
    linspace(elev_lo_deg, elev_hi_deg, beams)[b]) at azimuth 2 pi j / azimuths is row b * azimuths + j =
    (cos e cos az, cos e sin az, sin e).  The only sines and cosines of the sensor model: the device reads this table."""
    elev = np.deg2rad(np.linspace(float(elev_lo_deg), float(elev_hi_deg), int(beams)))
    az = 2.0 * math.pi * np.arange(int(azimuths), dtype=np.float64) / float(azimuths)
    e, a = np.meshgrid(elev, az, indexing="ij")
    return np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], -1).reshape(-1, 3)


def sensor_from_world(batch_size, num_agent):
    """[S, A, 4, 4] float64: np.linalg.inv(synthetic.agent_pose(a)) for every scene -- the scan's pose input."""
    from .synthetic import agent_pose
    inv = np.stack([np.linalg.inv(agent_pose(a)) for a in range(int(num_agent))], 0)
    return np.broadcast_to(inv[None], (int(batch_size),) + inv.shape).copy()


def _host(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def _shapes(solids, solid_count, object_count, pose, num_agent, dirs, jitter, gt_rows):
    if len(solids.shape) != 3 or solids.shape[2] != 8:
        raise ValueError("solids %s: [S, K, 8] is expected" % (tuple(solids.shape),))
    S, K = int(solids.shape[0]), int(solids.shape[1])
    if len(pose.shape) != 4 or int(pose.shape[0]) != S or tuple(pose.shape[2:]) != (4, 4):
        raise ValueError("sensor_from_world %s: [S = %d, A, 4, 4] is expected" % (tuple(pose.shape), S))
    A = int(pose.shape[1])
    if len(dirs.shape) != 2 or dirs.shape[1] != 3 or dirs.shape[0] < 1:
        raise ValueError("dirs %s: [R >= 1, 3] is expected" % (tuple(dirs.shape),))
    R = int(dirs.shape[0])
    for name, t in (("solid_count", solid_count), ("object_count", object_count), ("num_agent", num_agent)):
        if tuple(t.shape) != (S,):
            raise ValueError("%s %s: [S = %d] is expected" % (name, tuple(t.shape), S))
    if jitter is not None and tuple(jitter.shape) != (A * S, R):
        raise ValueError("range_jitter %s: [A*S = %d, R = %d] is expected" % (tuple(jitter.shape), A * S, R))
    if S < 1 or A < 1:
        raise ValueError("S = %d scenes, A = %d agents: both must be >= 1" % (S, A))
    G = max(1, K) if gt_rows is None else int(gt_rows)
    if G < 1:
        raise ValueError("gt_rows = %d, must be >= 1" % G)
    return S, A, K, R, G


def _check_objects(object_count, G):
    most = int(np.max(object_count)) if len(object_count) else 0
    if most > G:
        raise ValueError("object_count = %d is more than the %d ground-truth rows (gt_rows)" % (most, G))


def _frame(T, rows):
    """synthetic.boxes_in_agent_frame's expressions on T = sensor_from_world[s][a]: (cx, cy, sin, cos) of the rows"""
    x, y, sn, cs = rows[:, 0], rows[:, 1], rows[:, 4], rows[:, 5]
    cx = (T[0, 0] * x + T[0, 1] * y) + T[0, 3]
    cy = (T[1, 0] * x + T[1, 1] * y) + T[1, 3]
    s = T[1, 0] * cs + T[1, 1] * sn
    c = T[0, 0] * cs + T[0, 1] * sn
    return cx, cy, s, c


def _slab(lo, hi, o, e, tmin, tmax, ok):
    """one axis of the slab test over all rays (e [R]); an exactly zero e makes no division"""
    zero = e == 0.0
    with np.errstate(all="ignore"):
        t0, t1 = (lo - o) / e, (hi - o) / e
    tn = np.where(zero, -np.inf, np.minimum(t0, t1))
    tf = np.where(zero, np.inf, np.maximum(t0, t1))
    inside = bool(lo <= o <= hi)
    return np.maximum(tmin, tn), np.minimum(tmax, tf), ok & (~zero | inside)


def host_scan(solids, solid_count, object_count, sensor_from_world, num_agent, dirs, range_jitter=None, max_range=MAX_RANGE,
              ground_z=GROUND_Z, keep_ground=False, min_points=5, half_extent=32.0, gt_rows=None):
    """The numpy / float64 statement of dn_lidar_scan (include/disconet_hip.h), vectorised over the rays: the same inputs
    as host arrays -> {"points" [A*S, R, 4] float32, "hit" [A*S, R] int32, "solid_hits" [A*S, K] int32, "gt_boxes"
    [A*S, G, 6] float32, "gt_count" [A*S] int32, "gt_own_hits" [A*S, G] int32} (numpy).  Every product, sum and quotient
    is one float64 operation in the order the header writes it."""
    solids = _host(solids, np.float64)
    pose = _host(sensor_from_world, np.float64)
    dirs = _host(dirs, np.float64)
    solid_count, object_count, num_agent = (_host(v, np.int32) for v in (solid_count, object_count, num_agent))
    jitter = None if range_jitter is None else _host(range_jitter, np.float32)
    S, A, K, R, G = _shapes(solids, solid_count, object_count, pose, num_agent, dirs, jitter, gt_rows)
    if K > MAX_SOLIDS:
        raise ValueError("K = %d solids, at most %d" % (K, MAX_SOLIDS))
    _check_objects(object_count, G)
    max_range, ground_z, half_extent = float(max_range), float(ground_z), float(half_extent)
    n_img = A * S
    points = np.full((n_img, R, 4), _NAN32, dtype=np.float32)
    hit = np.full((n_img, R), -2, dtype=np.int32)
    solid_hits = np.zeros((n_img, K), dtype=np.int32)
    dx, dy, dz = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    for a in range(A):
        for s in range(S):
            if a >= int(num_agent[s]):
                continue                                        # a padded agent: all misses, zero counts
            img = a * S + s
            n = min(max(int(solid_count[s]), 0), K)
            rows = solids[s, :n]
            cx, cy, sn, cs = _frame(pose[s, a], rows)
            best = np.full(R, np.inf)
            best_k = np.full(R, -2, dtype=np.int32)
            for k in range(n):
                c, sk = cs[k], sn[k]
                mx, my = -cx[k], -cy[k]
                ox, oy = mx * c + my * sk, my * c - mx * sk
                ex, ey = dx * c + dy * sk, dy * c - dx * sk
                hw, hl = rows[k, 2] / 2.0, rows[k, 3] / 2.0
                tmin, tmax, ok = np.full(R, -np.inf), np.full(R, np.inf), np.ones(R, dtype=bool)
                tmin, tmax, ok = _slab(-hw, hw, ox, ex, tmin, tmax, ok)
                tmin, tmax, ok = _slab(-hl, hl, oy, ey, tmin, tmax, ok)
                tmin, tmax, ok = _slab(rows[k, 6], rows[k, 7], 0.0, dz, tmin, tmax, ok)
                win = ok & (0.0 < tmin) & (tmin <= tmax) & (tmin <= max_range) & (tmin < best)
                best = np.where(win, tmin, best)
                best_k = np.where(win, np.int32(k), best_k)
            down = dz < 0.0
            with np.errstate(all="ignore"):
                tg = np.where(down, ground_z / np.where(down, dz, -1.0), np.inf)
            win = down & (0.0 < tg) & (tg <= max_range) & (tg < best)
            best = np.where(win, tg, best)
            best_k = np.where(win, np.int32(-1), best_k)
            if not keep_ground:
                best_k = np.where(best_k == -1, np.int32(-2), best_k)
            got = best_k != -2
            t = best[got] + jitter[img, got].astype(np.float64) if jitter is not None else best[got]
            with np.errstate(all="ignore"):
                points[img, got, 0] = (t * dx[got]).astype(np.float32)
                points[img, got, 1] = (t * dy[got]).astype(np.float32)
                points[img, got, 2] = (t * dz[got]).astype(np.float32)
            points[img, got, 3] = (best_k[got] >= 0).astype(np.float32)
            hit[img] = best_k
            if K:
                solid_hits[img] = np.bincount(best_k[best_k >= 0], minlength=K)[:K].astype(np.int32)
    gt_boxes = np.zeros((n_img, G, 6), dtype=np.float32)
    gt_count = np.zeros(n_img, dtype=np.int32)
    gt_own = np.zeros((n_img, G), dtype=np.int32)
    for a in range(A):
        for s in range(S):
            live = min(max(int(num_agent[s]), 0), A)
            if a >= live:
                continue
            img = a * S + s
            n = min(max(int(object_count[s]), 0), min(max(int(solid_count[s]), 0), K))
            rows = solids[s, :n]
            cx, cy, sn, cs = _frame(pose[s, a], rows)
            seen = solid_hits[[j * S + s for j in range(live)], :n].sum(0)
            keep = np.nonzero((np.abs(cx) < half_extent) & (np.abs(cy) < half_extent) & (seen >= int(min_points)))[0][:G]
            box = np.stack([cx[keep], cy[keep], rows[keep, 2], rows[keep, 3], sn[keep], cs[keep]], 1)
            gt_boxes[img, :len(keep)] = box.astype(np.float32)
            gt_count[img] = len(keep)
            gt_own[img, :len(keep)] = solid_hits[img, keep]
    return {"points": points, "hit": hit, "solid_hits": solid_hits, "gt_boxes": gt_boxes, "gt_count": gt_count,
            "gt_own_hits": gt_own}


def _dev(x, dtype, device):
    if isinstance(x, torch.Tensor) and x.is_cuda:
        if x.dtype != dtype or not x.is_contiguous():
            raise _lib.DnError("lidar.scan: a device input must be contiguous %s (got %s, contiguous=%s)"
                               % (dtype, x.dtype, x.is_contiguous()))
        return x
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    return t.to(dtype).contiguous().to(device)


def scan(solids, solid_count, object_count, sensor_from_world, num_agent, dirs, range_jitter=None, max_range=MAX_RANGE,
         ground_z=GROUND_Z, keep_ground=False, min_points=5, half_extent=32.0, gt_rows=None, device="cuda"):
    """dn_lidar_scan on torch's current stream: solids [S, K, 8] float64, solid_count / object_count / num_agent [S] int32,
    sensor_from_world [S, A, 4, 4] float64, dirs [R, 3] float64 (beam_table), range_jitter [A*S, R] float32 or None --
    device tensors as they are (nothing is copied and nothing read back: the call can be captured into a graph and replayed
    with the solids changed in place), host arrays uploaded to `device` first.  -> host_scan's dict as device tensors, plus
    "cloud" = (points.view(-1, 4), offsets): holistic.pack_clouds' form, the host offsets arange(A*S + 1) * R, for
    holistic.holistic_views(cloud, ..., own=True).  Raises when object_count > gt_rows; a device object_count cannot be
    read without a wait, so it needs gt_rows >= K (nothing can then be dropped)."""
    known = None if (isinstance(object_count, torch.Tensor) and object_count.is_cuda) else _host(object_count, np.int32)
    first = solids if isinstance(solids, torch.Tensor) and solids.is_cuda else None
    dev = first.device if first is not None else torch.device(device)
    solids = _dev(solids, torch.float64, dev)
    pose = _dev(sensor_from_world, torch.float64, dev)
    dirs = _dev(dirs, torch.float64, dev)
    solid_count, object_count, num_agent = (_dev(v, torch.int32, dev) for v in (solid_count, object_count, num_agent))
    jitter = None if range_jitter is None else _dev(range_jitter, torch.float32, dev)
    _need_gpu(solids, pose, dirs, solid_count, object_count, num_agent, jitter)
    S, A, K, R, G = _shapes(solids, solid_count, object_count, pose, num_agent, dirs, jitter, gt_rows)
    if known is not None:
        _check_objects(known, G)
    elif G < K:
        raise ValueError("gt_rows = %d < K = %d with object_count on the device: pass host counts, or gt_rows >= K" % (G, K))
    n_img = A * S
    out = {"points": torch.empty((n_img, R, 4), dtype=torch.float32, device=dev),
           "hit": torch.empty((n_img, R), dtype=torch.int32, device=dev),
           "solid_hits": torch.empty((n_img, K), dtype=torch.int32, device=dev),
           "gt_boxes": torch.empty((n_img, G, 6), dtype=torch.float32, device=dev),
           "gt_count": torch.empty((n_img,), dtype=torch.int32, device=dev),
           "gt_own_hits": torch.empty((n_img, G), dtype=torch.int32, device=dev)}
    _lib.check(_lib.load().dn_lidar_scan(
        _ptr(solids) if K else None, _ptr(solid_count), _ptr(object_count), _ptr(pose), _ptr(num_agent), _ptr(dirs),
        _ptr(jitter), S, A, K, R, ctypes.c_double(float(max_range)), ctypes.c_double(float(ground_z)), int(bool(keep_ground)),
        int(min_points), ctypes.c_double(float(half_extent)), G, _ptr(out["points"]), _ptr(out["hit"]),
        _ptr(out["solid_hits"]) if K else None, _ptr(out["gt_boxes"]), _ptr(out["gt_count"]), _ptr(out["gt_own_hits"]),
        _stream()), "dn_lidar_scan")
    out["cloud"] = (out["points"].view(-1, 4), np.arange(n_img + 1, dtype=np.int64) * R)
    return out
