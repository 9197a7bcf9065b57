"""Occlusion-aware lidar scenes: a spinning lidar's rays cast from every agent's pose against the scene's solids (boxes with
a z range), the nearest hit kept, and the ground truth that somebody in the scene can see -- on the GPU in one call (scan,
C ABI dn_lidar_scan: graph-capturable, no host read) and as the numpy / float64 statement of the same rule (host_scan), which
the device equals in every byte.  include/disconet_hip.h states the rule in full.  It is this project's own sensor model: the
reference ships CARLA recordings, not a simulator.

The cloud goes to the voxeliser that already exists: scan()["cloud"] is holistic.pack_clouds' form, so
holistic.holistic_views(cloud, ..., own=True) yields bev_seq and bev_seq_teacher in one more launch; a miss is a row of NaNs,
which the voxeliser's strict extent test drops.

Sequences: world_step (dn_lidar_world_step) moves the solids and the sensors to the frame of a cursor that lives on the
device and rebuilds trans_matrices there; host_world_step is its numpy statement.  scan(ids=True) (dn_lidar_scan_ids) names
the solid behind every ground-truth row, one id per car across frames.  Sequence strings them together with the voxeliser:
its step() touches the host nowhere, so a captured step in front of the detector replays frame after frame.
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
              ground_z=GROUND_Z, keep_ground=False, min_points=5, half_extent=32.0, gt_rows=None, ids=False):
    """The numpy / float64 statement of dn_lidar_scan (include/disconet_hip.h), vectorised over the rays: the same inputs
    as host arrays -> {"points" [A*S, R, 4] float32, "hit" [A*S, R] int32, "solid_hits" [A*S, K] int32, "gt_boxes"
    [A*S, G, 6] float32, "gt_count" [A*S] int32, "gt_own_hits" [A*S, G] int32} (numpy).  Every product, sum and quotient
    is one float64 operation in the order the header writes it.  ids: also "gt_ids" [A*S, G] int32 (dn_lidar_scan_ids), the
    solid index k of each kept row, -1 at and beyond the count."""
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
    gt_ids = np.full((n_img, G), -1, dtype=np.int32)
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
            gt_ids[img, :len(keep)] = keep
    out = {"points": points, "hit": hit, "solid_hits": solid_hits, "gt_boxes": gt_boxes, "gt_count": gt_count,
           "gt_own_hits": gt_own}
    if ids:
        out["gt_ids"] = gt_ids
    return out


def _dev(x, dtype, device):
    if isinstance(x, torch.Tensor) and x.is_cuda:
        if x.dtype != dtype or not x.is_contiguous():
            raise _lib.DnError("lidar.scan: a device input must be contiguous %s (got %s, contiguous=%s)"
                               % (dtype, x.dtype, x.is_contiguous()))
        return x
    t = x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    return t.to(dtype).contiguous().to(device)


def scan(solids, solid_count, object_count, sensor_from_world, num_agent, dirs, range_jitter=None, max_range=MAX_RANGE,
         ground_z=GROUND_Z, keep_ground=False, min_points=5, half_extent=32.0, gt_rows=None, device="cuda", ids=False):
    """dn_lidar_scan on torch's current stream: solids [S, K, 8] float64, solid_count / object_count / num_agent [S] int32,
    sensor_from_world [S, A, 4, 4] float64, dirs [R, 3] float64 (beam_table), range_jitter [A*S, R] float32 or None --
    device tensors as they are (nothing is copied and nothing read back: the call can be captured into a graph and replayed
    with the solids changed in place), host arrays uploaded to `device` first.  -> host_scan's dict as device tensors, plus
    "cloud" = (points.view(-1, 4), offsets): holistic.pack_clouds' form, the host offsets arange(A*S + 1) * R, for
    holistic.holistic_views(cloud, ..., own=True).  Raises when object_count > gt_rows; a device object_count cannot be
    read without a wait, so it needs gt_rows >= K (nothing can then be dropped).  ids: dn_lidar_scan_ids, which adds
    "gt_ids" [A*S, G] int32 as host_scan(ids=True) does."""
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
    args = (_ptr(solids) if K else None, _ptr(solid_count), _ptr(object_count), _ptr(pose), _ptr(num_agent), _ptr(dirs),
            _ptr(jitter), S, A, K, R, ctypes.c_double(float(max_range)), ctypes.c_double(float(ground_z)),
            int(bool(keep_ground)), int(min_points), ctypes.c_double(float(half_extent)), G, _ptr(out["points"]),
            _ptr(out["hit"]), _ptr(out["solid_hits"]) if K else None, _ptr(out["gt_boxes"]), _ptr(out["gt_count"]),
            _ptr(out["gt_own_hits"]))
    if ids:
        out["gt_ids"] = torch.empty((n_img, G), dtype=torch.int32, device=dev)
        _lib.check(_lib.load().dn_lidar_scan_ids(*args, _ptr(out["gt_ids"]), _stream()), "dn_lidar_scan_ids")
    else:
        _lib.check(_lib.load().dn_lidar_scan(*args, _stream()), "dn_lidar_scan")
    out["cloud"] = (out["points"].view(-1, 4), np.arange(n_img + 1, dtype=np.int64) * R)
    return out


# ---------------------------------------------------------------------------
# sequences: the world at frame f (dn_lidar_world_step), and the Sequence that scans it frame after frame
# ---------------------------------------------------------------------------
WORLD_KEYS = (("solids0", np.float64), ("solid_vel", np.float64), ("solid_count", np.int32), ("agent0", np.float64),
              ("agent_vel", np.float64))


def _world_shapes(world):
    solids0, vel, count, agent0, avel = (world[k] for k, _ in WORLD_KEYS)
    if len(solids0.shape) != 3 or solids0.shape[2] != 8:
        raise ValueError("solids0 %s: [S, K, 8] is expected" % (tuple(solids0.shape),))
    S, K = int(solids0.shape[0]), int(solids0.shape[1])
    if len(agent0.shape) != 3 or int(agent0.shape[0]) != S or agent0.shape[2] != 4:
        raise ValueError("agent0 %s: [S = %d, A, 4] is expected" % (tuple(agent0.shape), S))
    A = int(agent0.shape[1])
    for name, t, want in (("solid_vel", vel, (S, K, 2)), ("solid_count", count, (S,)), ("agent_vel", avel, (S, A, 2))):
        if tuple(t.shape) != want:
            raise ValueError("%s %s: %s is expected" % (name, tuple(t.shape), want))
    if S < 1 or A < 1:
        raise ValueError("S = %d scenes, A = %d agents: both must be >= 1" % (S, A))
    return S, A, K


def host_world_step(world, f):
    """The numpy / float64 statement of dn_lidar_world_step (include/disconet_hip.h) at frame f (an int for every scene, or
    [S] ints): world = {"solids0" [S, K, 8], "solid_vel" [S, K, 2], "solid_count" [S], "agent0" [S, A, 4] (x, y, sin, cos),
    "agent_vel" [S, A, 2]} -> {"solids" [S, K, 8] float64, "sensor_from_world" [S, A, 4, 4] float64, "trans"
    [S, A, A, 4, 4] float32, "frame" [S] int32 = f + 1: the cursor after the call}.  Every product and sum is one float64
    operation in the order the header writes it; what the header copies as bytes is copied as bytes."""
    w = {k: _host(world[k], dt) for k, dt in WORLD_KEYS}
    S, A, K = _world_shapes(w)
    if K > MAX_SOLIDS:
        raise ValueError("K = %d solids, at most %d" % (K, MAX_SOLIDS))
    frame = np.broadcast_to(np.asarray(f, dtype=np.int32), (S,)).copy()
    solids = w["solids0"].copy()                                # columns 2 .. 7 and the rows beyond the count: bytes
    pose = np.zeros((S, A, 4, 4), dtype=np.float64)
    trans = np.zeros((S, A, A, 4, 4), dtype=np.float32)
    with np.errstate(all="ignore"):
        for s in range(S):
            t = np.float64(frame[s])
            n = min(max(int(w["solid_count"][s]), 0), K)
            solids[s, :n, 0] = w["solids0"][s, :n, 0] + t * w["solid_vel"][s, :n, 0]
            solids[s, :n, 1] = w["solids0"][s, :n, 1] + t * w["solid_vel"][s, :n, 1]
            x = w["agent0"][s, :, 0] + t * w["agent_vel"][s, :, 0]
            y = w["agent0"][s, :, 1] + t * w["agent_vel"][s, :, 1]
            sn, cs = w["agent0"][s, :, 2], w["agent0"][s, :, 3]
            T = pose[s]
            T[:, 0, 0], T[:, 0, 1], T[:, 0, 3] = cs, sn, -((cs * x) + (sn * y))
            T[:, 1, 0], T[:, 1, 1], T[:, 1, 3] = -sn, cs, (sn * x) - (cs * y)
            T[:, 2, 2] = T[:, 3, 3] = 1.0
            for i in range(A):
                Ti = T[i]
                r = np.zeros((A, 4, 4), dtype=np.float64)
                r[:, 0, 0] = Ti[0, 0] * cs + Ti[0, 1] * sn
                r[:, 0, 1] = Ti[0, 1] * cs - Ti[0, 0] * sn
                r[:, 1, 0] = Ti[1, 0] * cs + Ti[1, 1] * sn
                r[:, 1, 1] = Ti[1, 1] * cs - Ti[1, 0] * sn
                r[:, 0, 3] = (Ti[0, 0] * x + Ti[0, 1] * y) + Ti[0, 3]
                r[:, 1, 3] = (Ti[1, 0] * x + Ti[1, 1] * y) + Ti[1, 3]
                r[:, 2, 2] = r[:, 3, 3] = 1.0
                trans[s, i] = r.astype(np.float32)
                trans[s, i, i] = np.eye(4, dtype=np.float32)
    return {"solids": solids, "sensor_from_world": pose, "trans": trans,
            "frame": (frame.astype(np.int64) + 1).astype(np.int32)}


def world_to_device(world, device="cuda"):
    """The world description as the contiguous device tensors world_step reads (tensors already there are kept)."""
    dev = torch.device(device)
    types = {np.float64: torch.float64, np.int32: torch.int32}
    return {k: _dev(world[k], types[dt], dev) for k, dt in WORLD_KEYS}


def world_step(world, frame, out=None):
    """dn_lidar_world_step on torch's current stream: world as host_world_step takes it, but device tensors
    (world_to_device); frame [S] int32 on the device, the cursor, which the call advances by one.  out: {"solids",
    "sensor_from_world", "trans"} to write into (a Sequence's static tensors), else they are allocated.  Nothing is copied
    and nothing read back: a captured call replays frame after frame with nothing uploaded.  -> out."""
    for k, _ in WORLD_KEYS:
        if not (isinstance(world[k], torch.Tensor) and world[k].is_cuda):
            raise _lib.DnError("lidar.world_step needs device tensors (%s); world_to_device makes them" % k)
    w = world_to_device(world, world["agent0"].device)
    S, A, K = _world_shapes(w)
    dev = w["agent0"].device
    frame = _dev(frame, torch.int32, dev)
    if tuple(frame.shape) != (S,):
        raise ValueError("frame %s: [S = %d] is expected" % (tuple(frame.shape), S))
    shapes = {"solids": ((S, K, 8), torch.float64), "sensor_from_world": ((S, A, 4, 4), torch.float64),
              "trans": ((S, A, A, 4, 4), torch.float32)}
    if out is None:
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    for k, (shape, dt) in shapes.items():
        t = out[k]
        if tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError("out[%r] %s %s: contiguous %s %s on %s is expected" % (k, tuple(t.shape), t.dtype, shape, dt, dev))
    _need_gpu(frame, w["solid_count"], w["agent0"], w["agent_vel"], out["sensor_from_world"], out["trans"])
    _lib.check(_lib.load().dn_lidar_world_step(
        _ptr(w["solids0"]) if K else None, _ptr(w["solid_vel"]) if K else None, _ptr(w["solid_count"]), _ptr(w["agent0"]),
        _ptr(w["agent_vel"]), _ptr(frame), S, A, K, _ptr(out["solids"]) if K else None, _ptr(out["sensor_from_world"]),
        _ptr(out["trans"]), _stream()), "dn_lidar_world_step")
    return out


class Sequence:
    """A moving lidar world scanned frame after frame: owns the static device tensors -- the world description (world:
    host_world_step's keys plus "object_count" [S] and "num_agent" [S], synthetic.make_lidar_world's dict), the cursor,
    the frame's solids, poses and trans_matrices, the beam table and holistic.source_ranges -- so that step() touches
    the host nowhere and sits inside a graph.GraphedStep in front of the detector; a replay advances the world by one
    frame with nothing uploaded.

    step(teacher=False) -> {"bev_seq" [A*S, 1, X, Y, Z], "trans_matrices" [S, A, A, 4, 4] float32, "num_agent" [S, A]
    int64, "gt": {"boxes" [A*S, G, 6] float32, "ids" [A*S, G] int32 (the solid's row: one id per car across frames, -1
    beyond the count), "count" [A*S] int32} -- the tracking metrics' form --, "gt_own_hits" [A*S, G] int32} and with
    teacher "bev_seq_teacher".  trans_matrices and num_agent are the Sequence's own tensors, the rest is fresh.
    seek(f) / reset() write the cursor.  host_step(f) is the same dict as numpy arrays from host_world_step, host_scan and
    the host voxeliser; it does not move the cursor.  device = None: a host-only Sequence (host_step alone)."""

    def __init__(self, world, config, beams=32, azimuths=1024, min_points=5, gt_rows=None, device="cuda"):
        from . import holistic
        self.config = config
        self.min_points = int(min_points)
        self.half_extent = float(config.area_extents[0][1])
        self.dirs_host = beam_table(beams, azimuths)
        self.host_world = {k: _host(world[k], dt).copy() for k, dt in WORLD_KEYS}
        self.host_world["object_count"] = _host(world["object_count"], np.int32).copy()
        self.S, self.A, self.K = _world_shapes(self.host_world)
        live = world.get("num_agent")
        self.live = np.full(self.S, self.A, dtype=np.int32) if live is None else _host(live, np.int32).copy()
        self.host_world["num_agent"] = self.live
        self.G = max(1, self.K) if gt_rows is None else int(gt_rows)
        _check_objects(self.host_world["object_count"], self.G)
        self.offsets = np.arange(self.A * self.S + 1, dtype=np.int64) * len(self.dirs_host)
        self.live_host = tuple(int(v) for v in self.live)
        self.device = None
        if device is None:                                      # host_step only
            return
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.world = world_to_device(self.host_world, dev)
        self.object_count = torch.from_numpy(self.host_world["object_count"]).to(dev)
        self.live_dev = torch.from_numpy(self.live).to(dev)
        self.cursor = torch.zeros(self.S, dtype=torch.int32, device=dev)
        S, A, K = self.S, self.A, self.K
        self.state = {"solids": torch.zeros((S, K, 8), dtype=torch.float64, device=dev),
                      "sensor_from_world": torch.zeros((S, A, 4, 4), dtype=torch.float64, device=dev),
                      "trans": torch.zeros((S, A, A, 4, 4), dtype=torch.float32, device=dev)}
        self.dirs = torch.from_numpy(self.dirs_host).to(dev)
        self.num_agent = torch.from_numpy(np.repeat(self.live.astype(np.int64)[:, None], A, 1)).to(dev)
        self.ranges = holistic.source_ranges(self.offsets, self.live_host, A, S, own=True, device=dev)

    def _need_device(self):
        if self.device is None:
            raise _lib.DnError("this lidar.Sequence was made with device = None: host_step() is all it has")

    def seek(self, f):
        """the next step() is frame f (an int for every scene, or [S] ints); one small copy onto the current stream"""
        self._need_device()
        frame = np.broadcast_to(np.asarray(f, dtype=np.int32), (self.S,)).copy()
        self.cursor.copy_(torch.from_numpy(frame))

    def reset(self):
        self.seek(0)

    def _scan_kw(self):
        return dict(min_points=self.min_points, half_extent=self.half_extent, gt_rows=self.G, ids=True)

    def step(self, teacher=False):
        from . import holistic
        self._need_device()
        world_step(self.world, self.cursor, out=self.state)
        res = scan(self.state["solids"], self.world["solid_count"], self.object_count, self.state["sensor_from_world"],
                   self.live_dev, self.dirs, **self._scan_kw())
        views = holistic.holistic_views(res["cloud"], self.state["trans"], self.live_host, self.S, self.config, own=True,
                                        ranges=self.ranges)
        out = {"bev_seq": views["own_dense"], "trans_matrices": self.state["trans"], "num_agent": self.num_agent,
               "gt": {"boxes": res["gt_boxes"], "ids": res["gt_ids"], "count": res["gt_count"]},
               "gt_own_hits": res["gt_own_hits"]}
        if teacher:
            out["bev_seq_teacher"] = views["dense"]
        return out

    def host_step(self, f, teacher=False):
        from . import holistic
        w = host_world_step(self.host_world, f)
        res = host_scan(w["solids"], self.host_world["solid_count"], self.host_world["object_count"], w["sensor_from_world"],
                        self.live, self.dirs_host, **self._scan_kw())
        points = [res["points"][i] for i in range(self.A * self.S)]
        views = holistic.host_holistic_views(points, w["trans"], self.live_host, self.S, self.config, own=True)
        out = {"bev_seq": views["own_dense"], "trans_matrices": w["trans"], "num_agent": np.repeat(
                   self.live.astype(np.int64)[:, None], self.A, 1),
               "gt": {"boxes": res["gt_boxes"], "ids": res["gt_ids"], "count": res["gt_count"]},
               "gt_own_hits": res["gt_own_hits"]}
        if teacher:
            out["bev_seq_teacher"] = views["dense"]
        return out
