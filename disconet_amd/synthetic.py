"""Seeded synthetic collaborative-perception scenes.

There is no V2X-Sim data in this environment, so bench.py and the parity tests
feed both the HIP path and the oracle from this generator:

* voxels: per agent Bernoulli(p) occupancy on (H, W, 13), seed 1234 + agent,
  or a seeded point cloud xyz ~ U(extents) for the voxelizer row;
* poses: agent i at (x, y, yaw) = (6i cos 0.7i, 6i sin 0.7i, 0.15 i);
  trans_matrices[b, i, j] = T_i^-1 T_j (4x4 float32, maps agent j's frame into
  agent i's frame);
* num_agent_tensor[b, :] = number of live agents (padded agents are all-zero).
"""
import math

import numpy as np
import torch


def agent_pose(i):
    x = 6.0 * i * math.cos(0.7 * i)
    y = 6.0 * i * math.sin(0.7 * i)
    yaw = 0.15 * i
    c, s = math.cos(yaw), math.sin(yaw)
    T = np.eye(4, dtype=np.float64)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = c, -s, s, c
    T[0, 3], T[1, 3] = x, y
    return T


def make_trans_matrices(batch_size, num_agent, jitter_seed=None):
    """[B, A, A, 4, 4] float32; entry [b, i, j] = T_i^-1 T_j."""
    poses = [agent_pose(i) for i in range(num_agent)]
    out = np.zeros((batch_size, num_agent, num_agent, 4, 4), dtype=np.float32)
    rng = np.random.RandomState(jitter_seed) if jitter_seed is not None else None
    for b in range(batch_size):
        ps = poses
        if rng is not None:
            ps = []
            for T in poses:
                J = np.eye(4)
                a = rng.uniform(-0.05, 0.05)
                J[0, 0], J[0, 1], J[1, 0], J[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
                J[0, 3], J[1, 3] = rng.uniform(-1, 1, size=2)
                ps.append(T @ J)
        for i in range(num_agent):
            Ti_inv = np.linalg.inv(ps[i])
            for j in range(num_agent):
                out[b, i, j] = (Ti_inv @ ps[j]).astype(np.float32)
    return torch.from_numpy(out)


def make_bevs(batch_size, num_agent, map_hw=256, z=13, p=0.02, live=None):
    """Agent-major occupancy stack [A*B, 1, H, W, Z] float32 (image index =
    agent * B + b, the layout the reference's tools build with torch.cat)."""
    per_agent = []
    for a in range(num_agent):
        g = torch.Generator().manual_seed(1234 + a)
        occ = (torch.rand(batch_size, 1, map_hw, map_hw, z, generator=g) < p).to(torch.float32)
        if live is not None:
            for b in range(batch_size):
                if a >= int(live[b]):
                    occ[b].zero_()
        per_agent.append(occ)
    return torch.cat(per_agent, 0)


def make_scene_batch(batch_size=4, num_agent=5, map_hw=256, live=None, jitter_seed=None):
    """Returns (bevs, trans_matrices, num_agent_tensor) shaped like the
    reference's CoDetModule.step inputs."""
    if live is None:
        live = [num_agent] * batch_size
    bevs = make_bevs(batch_size, num_agent, map_hw, live=live)
    trans = make_trans_matrices(batch_size, num_agent, jitter_seed)
    num_agent_tensor = torch.tensor([[int(n)] * num_agent for n in live], dtype=torch.int64)
    return bevs, trans, num_agent_tensor


def make_point_cloud(n_points=60000, seed=0, extents=((-32.0, 32.0), (-32.0, 32.0), (-3.0, 2.0)),
                     boundary_cases=True):
    """Seeded cloud [N, 4] float32 (x, y, z, intensity).  Slightly over-scans
    the extents so the strict range filter has something to reject, and
    appends points lying exactly on voxel and extent boundaries."""
    rng = np.random.RandomState(seed)
    lo = np.array([e[0] for e in extents]) - 1.0
    hi = np.array([e[1] for e in extents]) + 1.0
    pts = rng.uniform(lo, hi, size=(n_points, 3))
    if boundary_cases:
        vs = np.array([0.25, 0.25, 0.4])
        k = rng.randint(-130, 130, size=(512, 3))
        on_edges = k * vs                      # exactly on voxel boundaries (in fp64)
        ext = np.array([[extents[0][0], 0.1, 0.1], [extents[0][1], 0.1, 0.1],
                        [0.1, extents[1][0], 0.1], [0.1, extents[1][1], 0.1],
                        [0.1, 0.1, extents[2][0]], [0.1, 0.1, extents[2][1]],
                        [np.nextafter(np.float32(extents[0][1]), np.float32(0)), 0.0, 0.0],
                        [np.nextafter(np.float32(extents[0][0]), np.float32(0)), 0.0, 0.0],
                        [0.0, 0.0, np.nextafter(np.float32(extents[2][1]), np.float32(0))],
                        [0.0, 0.0, np.nextafter(np.float32(extents[2][0]), np.float32(0))]])
        pts = np.concatenate([pts, on_edges, ext], 0)
    inten = rng.uniform(0, 1, size=(pts.shape[0], 1))
    return np.concatenate([pts, inten], 1).astype(np.float32)


def randomize_bn_stats(model, seed=7):
    """Random-init checkpoints have trivial BatchNorm statistics; give eval-mode
    BN something to do: mean ~ N(0, 0.1), var ~ U(0.5, 1.5),
    gamma ~ U(0.8, 1.2), beta ~ N(0, 0.05)."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
            n = m.num_features
            m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
            with torch.no_grad():
                m.weight.copy_(torch.rand(n, generator=g) * 0.4 + 0.8)
                m.bias.copy_(torch.randn(n, generator=g) * 0.05)


def make_sparse_scene_batch(batch_size=4, num_agent=5, map_hw=256, z=13, p=0.02):
    """The on-disk form of the reference's samples: per image a sorted [M, 3]
    int32 voxel index list (what V2XSimDet.__getitem__ scatters into the dense
    grid).  Returns (indices [Mtot, 3] int32, offsets [A*B + 1] int32) in the
    agent-major image order, plus the matching dense bevs for checking."""
    bevs = make_bevs(batch_size, num_agent, map_hw, z, p)
    lists, offsets = [], [0]
    for g in range(bevs.shape[0]):
        idx = torch.nonzero(bevs[g, 0]).to(torch.int32)      # row-major = lexsort(x, y, z)
        lists.append(idx)
        offsets.append(offsets[-1] + idx.shape[0])
    return torch.cat(lists, 0).contiguous(), torch.tensor(offsets, dtype=torch.int32), bevs


def make_train_targets(n_images, map_hw=256, anchors=6, code=6, seed=17, p_fg=0.01, p_ignore=0.005):
    """Seeded stand-ins for what V2XSimDet yields next to the voxels (upstream
    V2XSimDet.__getitem__: labels, reg_targets, reg_loss_mask): one-hot (bg, vehicle) labels per
    anchor [N, H*W*A, 2] (an all-zero row = don't care), box-code regression targets
    [N, H, W, A, 1, code] and the positive-anchor mask [N, H, W, A, 1]."""
    g = torch.Generator().manual_seed(seed)
    n = n_images * map_hw * map_hw * anchors
    fg = torch.rand(n, generator=g) < p_fg
    ignore = torch.rand(n, generator=g) < p_ignore
    labels = torch.stack([(~fg).float(), fg.float()], -1)
    labels[ignore & ~fg] = 0
    reg_targets = (torch.randn(n, code, generator=g) * 0.5) * fg[:, None]
    return (labels.view(n_images, -1, 2),
            reg_targets.view(n_images, map_hw, map_hw, anchors, 1, code),
            fg.view(n_images, map_hw, map_hw, anchors, 1))


def make_gt_boxes(n_images, seed=0, max_boxes=64, extent=32.0, min_boxes=None):
    """Seeded ground-truth boxes to score detections against: (gt_boxes [N, max_boxes, 6] float32 = (x, y, w, h, sin,
    cos), gt_count [N] int32), rows >= gt_count zero.  Per image min_boxes (default max_boxes // 2) .. max_boxes
    car-sized boxes, centres ~ U(-extent, extent)^2, yaw ~ U(-pi, pi).  They have nothing to do with the synthetic
    occupancy: an mAP against them checks the plumbing, not the detector."""
    rng = np.random.RandomState(seed)
    lo = max_boxes // 2 if min_boxes is None else int(min_boxes)
    boxes = np.zeros((n_images, max_boxes, 6), dtype=np.float32)
    count = rng.randint(lo, max_boxes + 1, size=n_images).astype(np.int32)
    for i in range(n_images):
        c = int(count[i])
        yaw = rng.uniform(-math.pi, math.pi, c)
        boxes[i, :c, 0:2] = rng.uniform(-extent, extent, (c, 2))
        boxes[i, :c, 2] = rng.uniform(1.6, 2.4, c)
        boxes[i, :c, 3] = rng.uniform(3.5, 5.5, c)
        boxes[i, :c, 4], boxes[i, :c, 5] = np.sin(yaw), np.cos(yaw)
    return torch.from_numpy(boxes), torch.from_numpy(count)


# ---------------------------------------------------------------------------
# scenes whose boxes and occupancy agree: world boxes -> per-agent ground truth and point clouds -> occupancy
# ---------------------------------------------------------------------------
BOX_SCENE_PITCH = 8.0            # grid pitch of the world boxes (m); centres are jittered by at most +-1 m
BOX_Z = (-2.0, -0.5)             # floor and roof of every box (m), inside the extents' (-3, 2)


def _box_points(box, step=0.1):
    """Points on the four sides (four heights) and on the roof of one world box (x, y, w, h, sin, cos): [P, 3] float64.
    The first point is the roof's centre."""
    x, y, w, h, s, c = (float(v) for v in box)
    us = np.arange(-w / 2.0, w / 2.0 + 1e-9, step)
    vs = np.arange(-h / 2.0, h / 2.0 + 1e-9, step)
    zs = np.linspace(BOX_Z[0] + 0.1, BOX_Z[1] - 0.1, 4)
    side = np.concatenate([np.stack([us, np.full_like(us, -h / 2.0)], 1), np.stack([us, np.full_like(us, h / 2.0)], 1),
                           np.stack([np.full_like(vs, -w / 2.0), vs], 1), np.stack([np.full_like(vs, w / 2.0), vs], 1)], 0)
    side = np.concatenate([np.concatenate([side, np.full((len(side), 1), z)], 1) for z in zs], 0)
    ru, rv = np.meshgrid(us[1:-1:2], vs[1:-1:2], indexing="ij")
    roof = np.stack([ru.ravel(), rv.ravel(), np.full(ru.size, BOX_Z[1])], 1)
    loc = np.concatenate([[[0.0, 0.0, BOX_Z[1]]], roof, side], 0)
    out = loc.copy()
    out[:, 0] = loc[:, 0] * c - loc[:, 1] * s + x
    out[:, 1] = loc[:, 0] * s + loc[:, 1] * c + y
    return out


def boxes_in_agent_frame(world_boxes, agent):
    """World boxes [K, 6] float64 under agent_pose(agent)^-1: centre and heading in that agent's frame."""
    T = np.linalg.inv(agent_pose(agent))
    b = np.asarray(world_boxes, dtype=np.float64).reshape(-1, 6)
    out = b.copy()
    out[:, 0] = T[0, 0] * b[:, 0] + T[0, 1] * b[:, 1] + T[0, 3]
    out[:, 1] = T[1, 0] * b[:, 0] + T[1, 1] * b[:, 1] + T[1, 3]
    out[:, 4] = T[1, 0] * b[:, 5] + T[1, 1] * b[:, 4]          # the heading vector (cos, sin) turned by -yaw_agent
    out[:, 5] = T[0, 0] * b[:, 5] + T[0, 1] * b[:, 4]
    return out


def host_occupancy(pts, voxel_size, extents, dims):
    """numpy form of the voxelizer (ops.voxelize_occupy; upstream voxelize_occupy): strict extent filter on the float32
    coordinates, floor(pts / voxel) in float64, shifted by floor(extent_lo / voxel) -> dense [X, Y, Z] float32."""
    pts = np.asarray(pts, dtype=np.float32)
    ext = np.asarray(extents, dtype=np.float64)
    vs = np.asarray(voxel_size, dtype=np.float64)
    keep = np.ones(len(pts), dtype=bool)
    for d in range(3):
        keep &= (ext[d, 0] < pts[:, d]) & (pts[:, d] < ext[d, 1])
    idx = (np.floor(pts[keep, :3] / vs) - np.floor(ext[:, 0] / vs)).astype(np.int64)
    dense = np.zeros(tuple(int(v) for v in dims), dtype=np.float32)
    dense[idx[:, 0], idx[:, 1], idx[:, 2]] = 1.0
    return dense


def make_box_scene_batch(batch_size=1, num_agent=2, map_hw=256, seed=0, boxes_per_scene=24, clutter=200, device=None,
                         teacher=False):
    """Seeded scenes in which the ground truth and the occupancy describe the same boxes.  Per scene up to
    `boxes_per_scene` car-sized world boxes (w ~ U(1.6, 2.4), l ~ U(3.5, 5.5), any yaw) sit on a grid of pitch 8 m over
    agent 0's extents, centres jittered by at most 1 m: two centres are at least 6 m apart, the boxes' circumscribed
    circles (radius <= 3 m) never meet.  Agent i sits at agent_pose(i); its ground truth is the world boxes in its frame
    whose centre is strictly inside the extents, its cloud the points on the boxes' sides and roofs plus `clutter` seeded
    points, both in its frame; the cloud goes through the voxelizer (ops.voxelize_occupy on `device`; device = None: the
    numpy form host_occupancy, tensors stay on the host).  Images are agent-major (image = agent * B + b).  Returns
    {"bev_seq" [A*B, 1, H, W, Z], "trans_matrices", "num_agent" (as make_scene_batch), "gt_boxes" [A*B, boxes_per_scene, 6]
    float32, "gt_count" [A*B] int32 (rows >= count zero), "points": per image [P, 4] float32, "world_boxes": per scene
    [K, 6] float64}.  teacher: also "bev_seq_teacher" [A*B, 1, H, W, Z], the holistic view of every image -- all agents'
    clouds carried into the image's frame by trans_matrices, merged and voxelised (holistic.holistic_views, one launch, on
    `device`; device = None: the numpy form holistic.host_holistic_views)."""
    from .config import Config
    cfg = Config(map_hw=map_hw)
    ext, vs, dims = cfg.area_extents, cfg.voxel_size, cfg.map_dims
    half = float(ext[0][1])
    cells = max(1, int(round(2 * half / BOX_SCENE_PITCH)))
    g = int(boxes_per_scene)
    n_img = num_agent * batch_size
    gt_boxes = np.zeros((n_img, g, 6), dtype=np.float32)
    gt_count = np.zeros(n_img, dtype=np.int32)
    points, world = [None] * n_img, []
    for b in range(batch_size):
        rng = np.random.RandomState((int(seed) * 9973 + b) % (2 ** 31))
        k = min(g, cells * cells)
        cell = rng.permutation(cells * cells)[:k]
        wb = np.zeros((k, 6), dtype=np.float64)
        wb[:, 0] = -half + (cell // cells + 0.5) * (2 * half / cells) + rng.uniform(-1.0, 1.0, k)
        wb[:, 1] = -half + (cell % cells + 0.5) * (2 * half / cells) + rng.uniform(-1.0, 1.0, k)
        wb[:, 2] = rng.uniform(1.6, 2.4, k)
        wb[:, 3] = rng.uniform(3.5, 5.5, k)
        yaw = rng.uniform(-math.pi, math.pi, k)
        wb[:, 4], wb[:, 5] = np.sin(yaw), np.cos(yaw)
        world.append(wb)
        cloud = np.concatenate([_box_points(row) for row in wb], 0) if k else np.zeros((0, 3))
        for a in range(num_agent):
            img = a * batch_size + b
            mine = boxes_in_agent_frame(wb, a)
            kept = mine[(np.abs(mine[:, 0]) < half) & (np.abs(mine[:, 1]) < half)]
            gt_boxes[img, :len(kept)] = kept.astype(np.float32)
            gt_count[img] = len(kept)
            T = np.linalg.inv(agent_pose(a))
            pts = cloud.copy()
            pts[:, 0] = T[0, 0] * cloud[:, 0] + T[0, 1] * cloud[:, 1] + T[0, 3]
            pts[:, 1] = T[1, 0] * cloud[:, 0] + T[1, 1] * cloud[:, 1] + T[1, 3]
            noise = rng.uniform([-half, -half, ext[2][0]], [half, half, ext[2][1]], size=(int(clutter), 3))
            pts = np.concatenate([pts, noise], 0)
            points[img] = np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1))], 1).astype(np.float32)
    if device is None:
        bevs = torch.from_numpy(np.stack([host_occupancy(p, vs, ext, dims) for p in points], 0))[:, None]
    else:
        from . import ops
        bevs = torch.stack([ops.voxelize_occupy(torch.from_numpy(p).to(device), vs, ext, dims) for p in points], 0)[:, None]
    trans = make_trans_matrices(batch_size, num_agent)
    na = torch.tensor([[num_agent] * num_agent for _ in range(batch_size)], dtype=torch.int64)
    out = {"bev_seq": bevs, "trans_matrices": trans, "num_agent": na, "gt_boxes": torch.from_numpy(gt_boxes),
           "gt_count": torch.from_numpy(gt_count)}
    if device is not None:
        out = {k: v.to(device) for k, v in out.items()}
    if teacher:
        from . import holistic
        live = [num_agent] * batch_size
        if device is None:
            out["bev_seq_teacher"] = torch.from_numpy(holistic.host_holistic_views(points, trans, live, batch_size, cfg)["dense"])
        else:
            out["bev_seq_teacher"] = holistic.holistic_views(points, out["trans_matrices"], live, batch_size, cfg,
                                                             device=device)["dense"]
    out["points"], out["world_boxes"] = points, world
    return out


# ---------------------------------------------------------------------------
# the same cars seen by a sensor model: ray-cast scans, occluders, the ground truth that somebody can see (lidar.py)
# ---------------------------------------------------------------------------
LIDAR_KEEP_OUT = 4.0             # a car whose centre is within this of a sensor is dropped (m)
LIDAR_OCCLUDER = (4.0, 4.0, -2.0, 1.5)      # w, l, z_lo, z_hi of an occluder (m), yaw 0
LIDAR_OCCLUDER_MARGIN = 1.5      # an occluder's footprint grown by this holds no sensor (m)


def lidar_world_solids(num_agent, map_hw, seed, scene, boxes_per_scene, occluders):
    """The solids of scene `scene` of make_lidar_scene_batch: (rows [n, 8] float64 = (x, y, w, l, sin, cos, z_lo, z_hi), the
    number of cars among them -- the first rows).  The cars are make_box_scene_batch's world boxes of the same seed (the
    RNG draws come in the same order) minus those whose centre is within LIDAR_KEEP_OUT of a sensor; up to `occluders`
    occluders follow on the grid cells the cars did not take, in the permutation's order, skipping a cell whose occluder
    footprint grown by LIDAR_OCCLUDER_MARGIN holds a sensor."""
    from .config import Config
    half = float(Config(map_hw=map_hw).area_extents[0][1])
    cells = max(1, int(round(2 * half / BOX_SCENE_PITCH)))
    rng = np.random.RandomState((int(seed) * 9973 + int(scene)) % (2 ** 31))
    k = min(int(boxes_per_scene), cells * cells)
    perm = rng.permutation(cells * cells)
    cell = perm[:k]
    wb = np.zeros((k, 8), dtype=np.float64)
    wb[:, 0] = -half + (cell // cells + 0.5) * (2 * half / cells) + rng.uniform(-1.0, 1.0, k)
    wb[:, 1] = -half + (cell % cells + 0.5) * (2 * half / cells) + rng.uniform(-1.0, 1.0, k)
    wb[:, 2] = rng.uniform(1.6, 2.4, k)
    wb[:, 3] = rng.uniform(3.5, 5.5, k)
    yaw = rng.uniform(-math.pi, math.pi, k)
    wb[:, 4], wb[:, 5] = np.sin(yaw), np.cos(yaw)
    wb[:, 6], wb[:, 7] = BOX_Z
    sensors = np.array([agent_pose(a)[:2, 3] for a in range(num_agent)], dtype=np.float64).reshape(-1, 2)
    far = np.ones(k, dtype=bool)
    for sx, sy in sensors:
        far &= np.hypot(wb[:, 0] - sx, wb[:, 1] - sy) > LIDAR_KEEP_OUT
    cars = wb[far]
    w, l, z_lo, z_hi = LIDAR_OCCLUDER
    rows = []
    for c in perm[k:]:
        if len(rows) >= int(occluders):
            break
        x = -half + (c // cells + 0.5) * (2 * half / cells)
        y = -half + (c % cells + 0.5) * (2 * half / cells)
        if any(abs(sx - x) <= w / 2.0 + LIDAR_OCCLUDER_MARGIN and abs(sy - y) <= l / 2.0 + LIDAR_OCCLUDER_MARGIN
               for sx, sy in sensors):
            continue
        rows.append([x, y, w, l, 0.0, 1.0, z_lo, z_hi])
    return np.concatenate([cars, np.asarray(rows, dtype=np.float64).reshape(-1, 8)], 0), len(cars)


def make_lidar_scene_batch(batch_size=1, num_agent=2, map_hw=256, seed=0, boxes_per_scene=24, occluders=10, beams=32,
                           azimuths=1024, min_points=5, keep_ground=False, device=None, teacher=False, gt_rows=None):
    """make_box_scene_batch's scenes seen through a sensor model (lidar.py; include/disconet_hip.h states the rule): the
    same world cars (lidar_world_solids) with z from BOX_Z, plus up to `occluders` tall blocks; agent i at agent_pose(i)
    casts beams x azimuths rays (lidar.beam_table, -30 .. +10 degrees) and keeps each ray's nearest return, so a car
    behind a block or another car is absent from that agent's cloud, present in a neighbour's and in the teacher's holistic
    view.  The ground truth of an image is the cars whose centre is strictly inside the extents AND on which the scene's
    agents together have at least `min_points` returns.  Returns make_box_scene_batch's keys with the same shapes and
    meaning ("points": per image the scan's [beams * azimuths, 4] rows, a miss a row of NaNs; "world_boxes": per scene the
    cars [K, 6] float64), plus "gt_own_hits" [A*B, boxes_per_scene] int32 (the image's own returns on each ground-truth
    row), "solid_hits" [A*B, boxes_per_scene + occluders] int32 and "world_solids": per scene [n, 8] float64.
    The occluders stand on the grid cells that the cars left free: boxes_per_scene at or above the grid's cell count (64 at
    map_hw = 256) leaves none.  gt_rows (default boxes_per_scene, and not below it) pads "gt_boxes" and "gt_own_hits" to that
    many rows for a caller whose metric wants a fixed width, without adding cars.
    device = None: lidar.host_scan, host_occupancy and holistic.host_holistic_views, tensors stay on the host; else
    lidar.scan and one holistic.holistic_views(own=True) launch on `device`."""
    from . import holistic, lidar
    from .config import Config
    cfg = Config(map_hw=map_hw)
    ext, vs, dims = cfg.area_extents, cfg.voxel_size, cfg.map_dims
    g = int(boxes_per_scene)
    rows_out = g if gt_rows is None else int(gt_rows)
    if rows_out < g:
        raise ValueError("gt_rows = %d is below boxes_per_scene = %d" % (rows_out, g))
    K = g + int(occluders)
    solids = np.zeros((batch_size, K, 8), dtype=np.float64)
    solid_count = np.zeros(batch_size, dtype=np.int32)
    object_count = np.zeros(batch_size, dtype=np.int32)
    world, world_solids = [], []
    for b in range(batch_size):
        rows, cars = lidar_world_solids(num_agent, map_hw, seed, b, g, occluders)
        solids[b, :len(rows)] = rows
        solid_count[b], object_count[b] = len(rows), cars
        world.append(rows[:cars, :6].copy())
        world_solids.append(rows)
    args = (solids, solid_count, object_count, lidar.sensor_from_world(batch_size, num_agent),
            np.full(batch_size, num_agent, dtype=np.int32), lidar.beam_table(beams, azimuths))
    kw = dict(keep_ground=keep_ground, min_points=min_points, half_extent=float(ext[0][1]), gt_rows=rows_out)
    trans = make_trans_matrices(batch_size, num_agent)
    na = torch.tensor([[num_agent] * num_agent for _ in range(batch_size)], dtype=torch.int64)
    live = [num_agent] * batch_size
    keys = ("gt_boxes", "gt_count", "gt_own_hits", "solid_hits")
    if device is None:
        res = lidar.host_scan(*args, **kw)
        points = [res["points"][i] for i in range(num_agent * batch_size)]
        out = {"bev_seq": torch.from_numpy(np.stack([host_occupancy(p, vs, ext, dims) for p in points], 0))[:, None],
               "trans_matrices": trans, "num_agent": na}
        out.update({k: torch.from_numpy(res[k]) for k in keys})
        if teacher:
            out["bev_seq_teacher"] = torch.from_numpy(holistic.host_holistic_views(points, trans, live, batch_size, cfg)["dense"])
    else:
        res = lidar.scan(*args, device=device, **kw)
        points = list(res["points"].unbind(0))
        out = {"trans_matrices": trans.to(device), "num_agent": na.to(device)}
        views = holistic.holistic_views(res["cloud"], out["trans_matrices"], live, batch_size, cfg, own=True, device=device)
        out["bev_seq"] = views["own_dense"]
        out.update({k: res[k] for k in keys})
        if teacher:
            out["bev_seq_teacher"] = views["dense"]
    out["points"], out["world_boxes"], out["world_solids"] = points, world, world_solids
    return out


# ---------------------------------------------------------------------------
# a world that moves: the frame-0 description of a lidar sequence (lidar.world_step / lidar.Sequence)
# ---------------------------------------------------------------------------
LIDAR_LANES = ((-2.5, 1.0), (2.5, -1.0), (-7.5, 1.0), (7.5, -1.0))   # (y, direction along x)
LIDAR_LANE_PITCH = 10.0          # slots along a lane (m), jittered by at most +-1.5 m
LIDAR_LANE_SPEED = (0.3, 0.8)    # a lane's speed is uniform in this range (m per frame)
LIDAR_LANE_REACH = 60.0          # slots cover x in [-60, 60]
LIDAR_PARK_Y = 13.5              # the two bands of parked cars and occluders, y = +-13.5
LIDAR_PARK_PITCH = 9.0           # slots along a band (m), jittered by at most +-1 m: two 5.5 m cars at any yaw (circumscribed
                                 # radius < 3.01 m) then keep 7 - 6.02 > 0.5 m between their footprints
LIDAR_CLEARANCE = 0.5            # no two footprints come closer than this in any frame (m)


def make_lidar_world(num_agent=2, map_hw=256, seed=0, scene=0, frames=40, fill=0.8, park_fill=0.8, occluder_share=0.4,
                     van_share=0.2, rows=None):
    """The seeded description of one moving world, scene `scene` of sequence seed `seed`: lidar.host_world_step's arrays with
    S = 1 -- "solids0" [1, K, 8] float64 (dn_lidar_scan's rows at frame 0), "solid_vel" [1, K, 2], "solid_count" [1],
    "agent0" [1, A, 4] (x, y, sin, cos), "agent_vel" [1, A, 2] (metres per frame) -- plus "object_count" [1] (the cars: the
    first rows, the occluders follow), "num_agent" [1] and "world": {"frames", "lanes": per lane (y, direction, speed),
    "agent_lane", "half_extent"}.  rows: K, the solids padded with zero rows beyond the count (default: the count), so that
    worlds of several seeds share one shape.

    Four lanes run parallel to x (LIDAR_LANES: y = +-2.5 and +-7.5, traffic on the right), each with one speed ~
    U(LIDAR_LANE_SPEED) m per frame; slots every LIDAR_LANE_PITCH over +-LIDAR_LANE_REACH, jittered by +-1.5 m, are filled
    with probability `fill`: a share `van_share` of them with a moving LIDAR_OCCLUDER block (a van: it hides the lanes and
    the band behind it from one side of the road while an agent on the other side still sees them), the rest with a car,
    its long side (l) along x: the heading (cos, sin) = (0, direction), as w lies along the heading.  Agent a rides in
    lane a % 4 in a slot of its own (a sensor, not a solid), heading along its travel, in the free slot that brings it
    nearest x = 0 at the middle frame; the first two ride in the two central lanes.  Parked cars at any yaw and standing
    LIDAR_OCCLUDER blocks (a share `occluder_share` of the `park_fill` filled slots) stand in the two bands y =
    +-LIDAR_PARK_Y; nothing moves behind a band, where every agent's view would be shadowed at once and a car would come
    and go from the ground truth.  For every frame (nothing depends on f: a lane shares one velocity) footprints keep
    LIDAR_CLEARANCE: along a lane 10 - 3 - 5.5 m, across lanes 5 - 4 m (two vans), lane to band 6 - 2 - 3.01 m, along a
    band 9 - 2 - 6.02 m; a sensor is 7 m or more from a car centre in its lane and 5 m from one in another (LIDAR_KEEP_OUT
    is 4), and 5 - 2 m or more from an occluder's footprint (LIDAR_OCCLUDER_MARGIN is 1.5).  The occluders' rows carry a
    velocity too: a van's is its lane's."""
    from .config import Config
    A, frames = int(num_agent), int(frames)
    if A < 1 or frames < 1:
        raise ValueError("num_agent = %d, frames = %d: both must be >= 1" % (A, frames))
    rng = np.random.RandomState((int(seed) * 9973 + int(scene) * 131 + 7) % (2 ** 31))
    slots = np.arange(-LIDAR_LANE_REACH, LIDAR_LANE_REACH + 1e-9, LIDAR_LANE_PITCH)
    lanes, cars, vel, blocks, block_vel = [], [], [], [], []
    ow, ol, oz_lo, oz_hi = LIDAR_OCCLUDER
    agent0 = np.zeros((A, 4), dtype=np.float64)
    agent_vel = np.zeros((A, 2), dtype=np.float64)
    riders = {}
    for a in range(A):
        riders.setdefault(a % len(LIDAR_LANES), []).append(a)
    for lane, (y, direction) in enumerate(LIDAR_LANES):
        speed = float(rng.uniform(*LIDAR_LANE_SPEED))
        x = slots + rng.uniform(-1.5, 1.5, len(slots))
        filled = rng.uniform(0.0, 1.0, len(slots)) < fill
        w = rng.uniform(1.6, 2.4, len(slots))
        l = rng.uniform(3.5, 5.5, len(slots))
        van = rng.uniform(0.0, 1.0, len(slots)) < van_share
        lanes.append((y, direction, speed))
        taken = set()
        for a in riders.get(lane, ()):                         # the free slot nearest to where the middle frame is at x = 0
            want = -direction * speed * (frames - 1) / 2.0
            order = [int(i) for i in np.argsort(np.abs(slots - want), kind="stable") if int(i) not in taken]
            taken.add(order[0])
            agent0[a] = (x[order[0]], y, 0.0, direction)       # yaw 0 or pi: sin exactly 0
            agent_vel[a] = (direction * speed, 0.0)
        for i in range(len(slots)):
            if filled[i] and i not in taken and van[i]:
                blocks.append([x[i], y, ow, ol, 0.0, 1.0, oz_lo, oz_hi])
                block_vel.append([direction * speed, 0.0])
            elif filled[i] and i not in taken:
                cars.append([x[i], y, w[i], l[i], direction, 0.0, BOX_Z[0], BOX_Z[1]])
                vel.append([direction * speed, 0.0])
    park = np.arange(-LIDAR_LANE_REACH, LIDAR_LANE_REACH + 1e-9, LIDAR_PARK_PITCH)
    for y in (-LIDAR_PARK_Y, LIDAR_PARK_Y):
        x = park + rng.uniform(-1.0, 1.0, len(park))
        filled = rng.uniform(0.0, 1.0, len(park)) < park_fill
        block = rng.uniform(0.0, 1.0, len(park)) < occluder_share
        w = rng.uniform(1.6, 2.4, len(park))
        l = rng.uniform(3.5, 5.5, len(park))
        yaw = rng.uniform(-math.pi, math.pi, len(park))
        for i in range(len(park)):
            if not filled[i]:
                continue
            if block[i]:
                blocks.append([x[i], y, ow, ol, 0.0, 1.0, oz_lo, oz_hi])
                block_vel.append([0.0, 0.0])
            else:
                cars.append([x[i], y, w[i], l[i], math.sin(yaw[i]), math.cos(yaw[i]), BOX_Z[0], BOX_Z[1]])
                vel.append([0.0, 0.0])
    n = len(cars) + len(blocks)
    K = n if rows is None else int(rows)
    if K < n:
        raise ValueError("rows = %d is below the world's %d solids" % (K, n))
    solids0 = np.zeros((1, K, 8), dtype=np.float64)
    solid_vel = np.zeros((1, K, 2), dtype=np.float64)
    solids0[0, :n] = np.asarray(cars + blocks, dtype=np.float64).reshape(-1, 8)
    solid_vel[0, :n] = np.asarray(vel + block_vel, dtype=np.float64).reshape(-1, 2)
    return {"solids0": solids0, "solid_vel": solid_vel, "solid_count": np.array([n], dtype=np.int32),
            "object_count": np.array([len(cars)], dtype=np.int32), "agent0": agent0[None], "agent_vel": agent_vel[None],
            "num_agent": np.array([A], dtype=np.int32),
            "world": {"frames": frames, "lanes": lanes, "agent_lane": [a % len(LIDAR_LANES) for a in range(A)],
                      "half_extent": float(Config(map_hw=map_hw).area_extents[0][1])}}


def make_lidar_world_batch(batch_size=1, num_agent=2, map_hw=256, seed=0, frames=40, rows=None, **kw):
    """make_lidar_world's scenes 0 .. batch_size - 1 of one seed as one description with S = batch_size, the solids padded
    to a common K (`rows`, default the largest count); "world" is the list of the scenes' metadata."""
    worlds = [make_lidar_world(num_agent, map_hw, seed, b, frames, **kw) for b in range(int(batch_size))]
    K = max(int(w["solid_count"][0]) for w in worlds) if rows is None else int(rows)
    worlds = [make_lidar_world(num_agent, map_hw, seed, b, frames, rows=K, **kw) for b in range(int(batch_size))]
    out = {k: np.concatenate([w[k] for w in worlds], 0) for k in worlds[0] if k != "world"}
    out["world"] = [w["world"] for w in worlds]
    return out


# ---------------------------------------------------------------------------
# labelled scenes for the seg variant: the world boxes above as per-pixel classes
# ---------------------------------------------------------------------------
SEG_CLASS_CAR, SEG_CLASS_LONG = 1, 2      # everything else is class 0; SegDiscoNet's other five classes never occur
SEG_IGNORE = -100                         # nn.CrossEntropyLoss's ignore_index


def seg_pixel_centres(cfg):
    """(xs [H], ys [W]) float64: the centre of every BEV pixel under the voxeliser's index convention -- index
    i = floor(x / voxel) - floor(extent_lo / voxel), so pixel i spans [(i + lo) voxel, (i + lo + 1) voxel) and its centre
    is (i + lo + 0.5) * voxel with lo = floor(extent_lo / voxel).  H is the x index, W the y index (bev_seq's layout)."""
    out = []
    for d in range(2):
        vs = float(cfg.voxel_size[d])
        lo = math.floor(float(cfg.area_extents[d][0]) / vs)
        out.append((np.arange(int(cfg.map_dims[d]), dtype=np.float64) + lo + 0.5) * vs)
    return out[0], out[1]


def make_seg_scene_batch(batch_size=1, num_agent=2, map_hw=256, seed=0, boxes_per_scene=24, clutter=200, device=None,
                         ignore_border=0):
    """Seeded scenes whose per-pixel labels and occupancy describe the same boxes (make_box_scene_batch's scenes with a
    second population and label maps).  Per scene up to `boxes_per_scene` world boxes (x, y, w, h, sin, cos) sit on the
    grid of pitch 8 m over agent 0's extents, centres jittered by at most 1 m, any yaw.  Box k with k % 3 == 1 is a long
    vehicle (w ~ U(2.6, 3.2), h ~ U(10, 13): about 3 m x 12 m), class 2; every other box is car-sized (w ~ U(1.6, 2.4),
    h ~ U(3.5, 5.5)), class 1; everything else is class 0.  Long vehicles may reach into a neighbour's cell: the rule
    below says who wins.  Agent i sits at agent_pose(i); its cloud is the points on the boxes' sides and roofs
    (_box_points) plus `clutter` seeded points, in its frame, put through the voxeliser, whose strict extent filter
    keeps what the agent sees (ops.voxelize_occupy on `device`; device = None: host_occupancy, tensors stay on the host).

    Labels, per image (image = agent * B + b), in float64: pixel (i, j) has the centre (xs[i], ys[j]) of
    seg_pixel_centres.  With the world boxes carried into the agent's frame by boxes_in_agent_frame, dx = xs[i] - x,
    dy = ys[j] - y, u = dx * cos + dy * sin, v = dy * cos - dx * sin, box k CONTAINS the centre iff |u| <= w / 2 and
    |v| <= h / 2 -- the edges belong to the box.  The pixel takes the class of the LOWEST-index box that contains its
    centre, else 0.  ignore_border = k > 0 then writes -100 into the k outermost rows and columns on every side.

    Returns {"bev_seq" [A*B, Z, H, W] float32 (the NCHW-shaped view of the voxeliser's [H, W, Z] maps that
    SegModule.step / evaluate read), "trans_matrices", "num_agent" (as make_scene_batch), "labels" [A*B, H, W] int64,
    "world_boxes": per scene [K, 6] float64, "world_classes": per scene [K] int64, "points": per image [P, 4] float32}."""
    from .config import Config
    cfg = Config(map_hw=map_hw)
    ext, vs, dims = cfg.area_extents, cfg.voxel_size, cfg.map_dims
    half = float(ext[0][1])
    cells = max(1, int(round(2 * half / BOX_SCENE_PITCH)))
    n_img = num_agent * batch_size
    xs, ys = seg_pixel_centres(cfg)
    labels = np.zeros((n_img, dims[0], dims[1]), dtype=np.int64)
    points, world, world_cls = [None] * n_img, [], []
    for b in range(batch_size):
        rng = np.random.RandomState((int(seed) * 9973 + b) % (2 ** 31))
        k = min(int(boxes_per_scene), cells * cells)
        cell = rng.permutation(cells * cells)[:k]
        long_one = np.arange(k) % 3 == 1
        wb = np.zeros((k, 6), dtype=np.float64)
        wb[:, 0] = -half + (cell // cells + 0.5) * (2 * half / cells) + rng.uniform(-1.0, 1.0, k)
        wb[:, 1] = -half + (cell % cells + 0.5) * (2 * half / cells) + rng.uniform(-1.0, 1.0, k)
        wb[:, 2] = np.where(long_one, rng.uniform(2.6, 3.2, k), rng.uniform(1.6, 2.4, k))
        wb[:, 3] = np.where(long_one, rng.uniform(10.0, 13.0, k), rng.uniform(3.5, 5.5, k))
        yaw = rng.uniform(-math.pi, math.pi, k)
        wb[:, 4], wb[:, 5] = np.sin(yaw), np.cos(yaw)
        cls = np.where(long_one, SEG_CLASS_LONG, SEG_CLASS_CAR).astype(np.int64)
        world.append(wb)
        world_cls.append(cls)
        cloud = np.concatenate([_box_points(row) for row in wb], 0) if k else np.zeros((0, 3))
        for a in range(num_agent):
            img = a * batch_size + b
            mine = boxes_in_agent_frame(wb, a)
            for j in range(k - 1, -1, -1):                  # highest index first: the lowest index is written last and wins
                x, y, w, h, s, c = mine[j]
                dx, dy = (xs - x)[:, None], (ys - y)[None, :]
                u, v = dx * c + dy * s, dy * c - dx * s
                labels[img][(np.abs(u) <= w / 2.0) & (np.abs(v) <= h / 2.0)] = cls[j]
            T = np.linalg.inv(agent_pose(a))
            pts = cloud.copy()
            pts[:, 0] = T[0, 0] * cloud[:, 0] + T[0, 1] * cloud[:, 1] + T[0, 3]
            pts[:, 1] = T[1, 0] * cloud[:, 0] + T[1, 1] * cloud[:, 1] + T[1, 3]
            noise = rng.uniform([-half, -half, ext[2][0]], [half, half, ext[2][1]], size=(int(clutter), 3))
            pts = np.concatenate([pts, noise], 0)
            points[img] = np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1))], 1).astype(np.float32)
    kb = int(ignore_border)
    if kb > 0:
        frame = np.ones(labels.shape[1:], dtype=bool)
        frame[kb:labels.shape[1] - kb, kb:labels.shape[2] - kb] = False
        labels[:, frame] = SEG_IGNORE
    if device is None:
        bevs = torch.from_numpy(np.stack([host_occupancy(p, vs, ext, dims) for p in points], 0))
    else:
        from . import ops
        bevs = torch.stack([ops.voxelize_occupy(torch.from_numpy(p).to(device), vs, ext, dims) for p in points], 0)
    trans = make_trans_matrices(batch_size, num_agent)
    na = torch.tensor([[num_agent] * num_agent for _ in range(batch_size)], dtype=torch.int64)
    out = {"bev_seq": bevs.permute(0, 3, 1, 2), "trans_matrices": trans, "num_agent": na, "labels": torch.from_numpy(labels)}
    if device is not None:
        out = {key: value.to(device) for key, value in out.items()}
    out["world_boxes"], out["world_classes"], out["points"] = world, world_cls, points
    return out


# ---------------------------------------------------------------------------
# detection sequences for the tracker (tracking.Sort / HostSort)
# ---------------------------------------------------------------------------
def make_track_sequence(frames, n_images, seed=0, objects=6, width=None, noise=0.05, p_miss=0.1, false_positives=1,
                        extent=24.0, speed=0.4, spread=0.05, truth=False):
    """Seeded detections of moving boxes, frame by frame: per image `objects` car-sized boxes (w ~ U(1.6, 2.4),
    l ~ U(3.5, 5.5), any yaw) start on a grid of pitch 8 m (centres jittered by at most 1 m) and move at constant
    velocity -- a flow of at most `speed` m per frame shared by the image plus at most `spread` m per frame of their own,
    so that two of them never come close in a few dozen frames.  Every frame, every object is detected with probability
    1 - p_miss at its true box plus N(0, noise) m on the centre and N(0, noise / 2) m on the size, with a score in
    (0.5, 1); `false_positives` boxes per frame are drawn uniformly over the extent with a score in (0.1, 0.5).  Rows are
    the objects in identity order, then the false positives.  Returns a list of `frames` pairs (det, ident):
    det = postprocess.pad_detections' dict {"boxes" [N, K, 6] float32, "scores" [N, K] float32, "count" [N] int32} (numpy;
    K = `width`, default objects + false_positives, at least 1), ident [N, K] int32 = the true identity of each row
    (0 .. objects - 1), -1 for a false positive and for the padding.
    With truth=True the list holds triples (det, ident, gt): gt = {"boxes" [N, G, 6] float32, "ids" [N, G] int32, "count"
    [N] int32} (G = max(objects, 1)), the noise-free boxes of ALL objects that frame in identity order, ids
    0 .. objects - 1 -- what tracking.ClearMot takes as ground truth.  They follow from the start / velocity / size / yaw
    already drawn: no extra random draw, so det and ident are the same arrays either way."""
    from .postprocess import pad_boxes, pad_detections
    rng = np.random.RandomState(int(seed))
    k = max(1, int(objects) + int(false_positives)) if width is None else int(width)
    cells = max(1, int(2 * extent // 8.0))
    if objects > cells * cells:
        raise ValueError("%d objects do not fit the %d x %d grid of pitch 8 m over +-%g m" % (objects, cells, cells, extent))
    start, vel, size, yaw = [], [], [], []
    for _ in range(n_images):
        cell = rng.permutation(cells * cells)[:objects]
        xy = np.stack([(cell // cells + 0.5) * 8.0 - cells * 4.0, (cell % cells + 0.5) * 8.0 - cells * 4.0], 1)
        start.append(xy + rng.uniform(-1.0, 1.0, (objects, 2)))
        flow = rng.uniform(-speed, speed, 2) / math.sqrt(2.0)
        vel.append(flow[None, :] + rng.uniform(-spread, spread, (objects, 2)) / math.sqrt(2.0))
        size.append(np.stack([rng.uniform(1.6, 2.4, objects), rng.uniform(3.5, 5.5, objects)], 1))
        yaw.append(rng.uniform(-math.pi, math.pi, objects))
    out = []
    for f in range(int(frames)):
        boxes, scores, idents = [], [], []
        for i in range(n_images):
            seen = rng.uniform(size=objects) >= p_miss
            n_seen = int(seen.sum())
            b = np.zeros((n_seen + int(false_positives), 6), dtype=np.float64)
            b[:n_seen, 0:2] = (start[i] + f * vel[i])[seen] + noise * rng.standard_normal((n_seen, 2))
            b[:n_seen, 2:4] = size[i][seen] + 0.5 * noise * rng.standard_normal((n_seen, 2))
            b[:n_seen, 4], b[:n_seen, 5] = np.sin(yaw[i][seen]), np.cos(yaw[i][seen])
            fy = rng.uniform(-math.pi, math.pi, int(false_positives))
            b[n_seen:, 0:2] = rng.uniform(-extent, extent, (int(false_positives), 2))
            b[n_seen:, 2] = rng.uniform(1.6, 2.4, int(false_positives))
            b[n_seen:, 3] = rng.uniform(3.5, 5.5, int(false_positives))
            b[n_seen:, 4], b[n_seen:, 5] = np.sin(fy), np.cos(fy)
            s = np.concatenate([rng.uniform(0.5, 1.0, n_seen), rng.uniform(0.1, 0.5, int(false_positives))])
            ident = np.concatenate([np.nonzero(seen)[0], np.full(int(false_positives), -1)])
            boxes.append(b[:k])
            scores.append(s[:k])
            idents.append(ident[:k])
        det = pad_detections(boxes, scores, k)
        ident = np.full((n_images, k), -1, dtype=np.int32)
        for i, row in enumerate(idents):
            ident[i, :len(row)] = row
        if not truth:
            out.append((det, ident))
            continue
        true = []
        for i in range(n_images):
            b = np.zeros((int(objects), 6), dtype=np.float64)
            b[:, 0:2] = start[i] + f * vel[i]
            b[:, 2:4] = size[i]
            b[:, 4], b[:, 5] = np.sin(yaw[i]), np.cos(yaw[i])
            true.append(b)
        gt_boxes, gt_count = pad_boxes(true, max(1, int(objects)))
        gt_ids = np.zeros((n_images, max(1, int(objects))), dtype=np.int32)
        gt_ids[:, :int(objects)] = np.arange(int(objects), dtype=np.int32)[None, :]
        out.append((det, ident, {"boxes": gt_boxes, "ids": gt_ids, "count": gt_count}))
    return out
