"""The distillation teacher's holistic view: every agent's point cloud merged into each ego's frame and voxelised (what
the reference's dataset builder stores per sample as bev_seq_teacher), here from clouds and poses on the GPU in one
launch for the whole batch (ops.voxelize_views, dn_voxelize_views) -- with the students' own views from the same launch
when asked for.

The rule (include/disconet_hip.h states it in full): the view of ego i of scene b is the union over the live agents j of
cloud (j, b) carried by trans_matrices[b, i, j] (agent j's frame -> agent i's frame), the ego's own cloud taken as it is;
a carried coordinate is float32(((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]) summed in float64, and the float32
coordinates go through the voxelizer's rule.  host_holistic_views is the numpy reference of the same rule.  The upstream
builder's own merge is not pinned (its source is not among what this project was written from): the rule is this
project's.
"""
import numpy as np
import torch

from . import _lib, ops

_SRC_CACHE = {}      # (live counts, A, B, ego range, own, device) -> the device index tensors of view_sources (no poses, no clouds in them)


def _live_counts(num_agent, batch):
    """the [B] live-agent counts as host ints, from a list / array / tensor [B] or the reference's num_agent tensor
    [B, A] (column 0).  A device tensor is copied to the host (the one wait of this module): pass host counts to avoid it."""
    t = num_agent
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    t = np.asarray(t)
    if t.ndim == 2:
        t = t[:, 0]
    if t.ndim != 1 or len(t) < batch:
        raise ValueError("num_agent %s: [B] counts or the [B, A] tensor are expected (B = %d)" % (t.shape, batch))
    return tuple(int(v) for v in t[:batch])


def view_sources(num_agent_cpu, agents, batch, ego_first=0, ego_count=None, own=False):
    """The host-side source lists of the holistic views, in the reference's loop order (train._fusion_index_lists: for b,
    for ego i in [ego_first, ego_first + ego_count), sources j = 0 .. n_b - 1): -> {"src_image": the agent-major image
    j * B + b whose cloud the source reads, "src_view": (i - ego_first) * B + b -- agent-major over THIS rank's egos, the
    bev_seq_teacher layout CoDetModule documents for an AgentShard --, "src_pose": -1 for j == i (the ego's own cloud is
    not transformed), else (b * A + i) * A + j into trans_matrices.reshape(-1, 4, 4), "n_views"}.  A padded ego
    (i >= n_b) has no sources: its view is all zero.  own: another E * B single-source views follow (view E * B +
    (i - ego_first) * B + b = cloud (i, b) as it is; a padded ego again none), the students' own views."""
    A, B = int(agents), int(batch)
    E = A - ego_first if ego_count is None else int(ego_count)
    if A < 1 or B < 1 or ego_first < 0 or E < 0 or ego_first + E > A:
        raise ValueError("view_sources: agents %d, batch %d, egos [%d, %d)" % (A, B, ego_first, ego_first + E))
    counts = [int(num_agent_cpu[b]) for b in range(B)]
    if any(n < 0 or n > A for n in counts):
        raise ValueError("view_sources: live counts %s of %d agents" % (counts, A))
    image, view, pose = [], [], []
    for b in range(B):
        for i in range(ego_first, min(ego_first + E, counts[b])):
            for j in range(counts[b]):
                image.append(j * B + b)
                view.append((i - ego_first) * B + b)
                pose.append(-1 if j == i else (b * A + i) * A + j)
    if own:
        for b in range(B):
            for i in range(ego_first, min(ego_first + E, counts[b])):
                image.append(i * B + b)
                view.append(E * B + (i - ego_first) * B + b)
                pose.append(-1)
    return {"src_image": image, "src_view": view, "src_pose": pose, "n_views": E * B * (2 if own else 1)}


def _device_sources(counts, agents, batch, ego_first, ego_count, own, device):
    key = (counts, agents, batch, ego_first, ego_count, bool(own), str(device))
    hit = _SRC_CACHE.get(key)
    if hit is None:
        if len(_SRC_CACHE) > 64:
            _SRC_CACHE.clear()
        src = view_sources(counts, agents, batch, ego_first, ego_count, own)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=device)      # noqa: E731
        hit = dict(src, d_view=i32(src["src_view"]), d_pose=i32(src["src_pose"]),
                   d_image=torch.tensor(src["src_image"], dtype=torch.long, device=device),
                   d_next=torch.tensor([k + 1 for k in src["src_image"]], dtype=torch.long, device=device))
        _SRC_CACHE[key] = hit
    return hit


def _ranges_of(src, offsets, dev):
    off = torch.from_numpy(offsets.astype(np.int32)).to(dev)
    begin = off[src["d_image"]].contiguous()
    sizes = np.diff(offsets)
    return {"src": src, "begin": begin, "count": (off[src["d_next"]] - begin).contiguous(),
            "max_count": int(sizes[src["src_image"]].max()) if len(src["src_image"]) else 0}


def source_ranges(offsets, num_agent, agents, batch_size, ego_first=0, ego_count=None, own=False, device="cuda"):
    """The device index tensors that holistic_views derives from the clouds' sizes and the live counts, made once and OWNED
    BY THE CALLER: offsets [A*B + 1] (pack_clouds' / lidar.scan's host offsets), num_agent as holistic_views takes it.
    Pass the result as holistic_views(..., ranges=...) with the same offsets, counts, egos and `own`: that call uploads
    nothing and holds no tensor that a module cache could drop, so it can be captured into a graph.  Keep the result alive
    as long as the graph: the graph reads these tensors at every replay."""
    A, B = int(agents), int(batch_size)
    offsets = np.asarray(offsets, dtype=np.int64)
    if len(offsets) != A * B + 1:
        raise ValueError("%d clouds for %d agents x %d scenes" % (len(offsets) - 1, A, B))
    counts = _live_counts(num_agent, B)
    E = A - ego_first if ego_count is None else int(ego_count)
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    src = view_sources(counts, A, B, int(ego_first), E, own)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)      # noqa: E731
    src = dict(src, d_view=i32(src["src_view"]), d_pose=i32(src["src_pose"]),
               d_image=torch.tensor(src["src_image"], dtype=torch.long, device=dev),
               d_next=torch.tensor([k + 1 for k in src["src_image"]], dtype=torch.long, device=dev))
    return dict(_ranges_of(src, offsets, dev), key=(counts, A, B, int(ego_first), E, bool(own), offsets.tobytes()))


def pack_clouds(points, device):
    """points: the per-image list of clouds [P_k, >= 3] (numpy arrays or tensors, agent-major: image = agent * B + b), all
    with the same number of columns -> (the concatenated float32 device tensor [P_total, columns], the host offsets
    [len(points) + 1] int64: image k owns the rows offsets[k] .. offsets[k + 1])."""
    if not len(points):
        raise ValueError("pack_clouds: no clouds")
    cols = {int(p.shape[1]) if len(p.shape) == 2 else -1 for p in points}
    if len(cols) != 1 or min(cols) < 3:
        raise ValueError("pack_clouds: every cloud must be [P, C] with one C >= 3 (got C in %s)" % sorted(cols))
    offsets = np.zeros(len(points) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([int(p.shape[0]) for p in points])
    if offsets[-1] >= 2 ** 31:
        raise ValueError("pack_clouds: %d points; the source lists are int32" % offsets[-1])
    if all(isinstance(p, torch.Tensor) for p in points):
        pts = torch.cat([p.to(device=device, dtype=torch.float32) for p in points], 0).contiguous()
    else:
        host = np.concatenate([p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p) for p in points], 0)
        pts = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(device)
    return pts, offsets


def holistic_views(points, trans_matrices, num_agent, batch_size, config, ego_first=0, ego_count=None, want=("dense",),
                   own=False, device="cuda", ranges=None):
    """points: per image [P_k, >= 3] (pack_clouds' input), or pack_clouds' result (pts, offsets) for a caller that keeps
    its clouds on the device; trans_matrices [B, A, A, 4, 4]; num_agent: the live counts [B] (host ints: nothing waits for
    the device) or the reference's [B, A] tensor; config: voxel_size / area_extents / map_dims (disconet_amd.Config).
    -> {"dense": [E*B, 1, X, Y, Z] float32 -- data["bev_seq_teacher"] of CoDetModule.step for the egos [ego_first,
    ego_first + ego_count), agent-major --, "bits": the same as an ops.SpTensor(bits=True)}, the keys of `want`; with own
    also "own_dense" / "own_bits", the egos' own views (data["bev_seq"]), written by the same launch.
    ranges: source_ranges' result for these offsets, counts and egos -- the call then uploads nothing and reads no module
    cache, which is what a caller that captures it into a graph needs (and it must keep `ranges` as long as the graph)."""
    B = int(batch_size)
    A = int(trans_matrices.shape[1])
    if trans_matrices.dim() != 5 or tuple(trans_matrices.shape[2:]) != (A, 4, 4) or trans_matrices.shape[0] < B:
        raise ValueError("trans_matrices %s: [B, A, A, 4, 4] is expected" % (tuple(trans_matrices.shape),))
    if isinstance(points, tuple) and len(points) == 2 and isinstance(points[0], torch.Tensor) and points[0].dim() == 2:
        pts, offsets = points
        offsets = np.asarray(offsets, dtype=np.int64)
    else:
        pts, offsets = pack_clouds(points, device)
    if len(offsets) != A * B + 1:
        raise ValueError("%d clouds for %d agents x %d scenes" % (len(offsets) - 1, A, B))
    dev = pts.device
    counts = _live_counts(num_agent, B)
    E = A - ego_first if ego_count is None else int(ego_count)
    key = (counts, A, B, int(ego_first), E, bool(own), offsets.tobytes())
    if ranges is not None and (ranges["key"] != key or ranges["begin"].device != dev):
        raise ValueError("holistic_views: `ranges` was made for other clouds, live counts, egos or another device")
    src = ranges["src"] if ranges is not None else _device_sources(counts, A, B, int(ego_first), E, own, dev)
    if ranges is None:
        ranges = _ranges_of(src, offsets, dev)
    begin, count, max_count = ranges["begin"], ranges["count"], ranges["max_count"]
    poses = trans_matrices.to(device=dev, dtype=torch.float32).contiguous()
    res = ops.voxelize_views(pts, begin, count, src["d_view"], src["d_pose"], poses, src["n_views"], max_count,
                             config.voxel_size, config.area_extents, config.map_dims, want=want)
    if not own:
        return res
    n = E * B
    out = {}
    if "dense" in res:
        out["dense"], out["own_dense"] = res["dense"][:n], res["dense"][n:]
    if "bits" in res:
        b = res["bits"]
        out["bits"] = ops.SpTensor(n, b.h, b.w, b.c, data=b.data[:n], bits=True)
        out["own_bits"] = ops.SpTensor(n, b.h, b.w, b.c, data=b.data[n:], bits=True)
    return out


def transform_cloud(pts, T):
    """numpy statement of the transform: pts [P, >= 3] float32, T [4, 4] float32 -> [P, 3] float32 =
    float32(((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]), every operand widened to float64, summed in that order."""
    p = np.asarray(pts, dtype=np.float32)[:, :3].astype(np.float64)
    T = np.asarray(T, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):         # inf * 0 and inf - inf are NaN, as on the device: the voxel rule drops them
        c = [((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)]
        return np.stack(c, 1).astype(np.float32)


def host_holistic_views(points, trans_matrices, num_agent, batch_size, config, ego_first=0, ego_count=None, own=False):
    """numpy reference of holistic_views: the same sources (view_sources), transform_cloud, the clouds of a view merged,
    synthetic.host_occupancy -> {"dense" [E*B, 1, X, Y, Z] float32 numpy (and "own_dense" with own)}."""
    from .synthetic import host_occupancy
    B = int(batch_size)
    trans = trans_matrices.detach().cpu().numpy() if isinstance(trans_matrices, torch.Tensor) else np.asarray(trans_matrices)
    A = int(trans.shape[1])
    if len(points) != A * B:
        raise ValueError("%d clouds for %d agents x %d scenes" % (len(points), A, B))
    poses = np.asarray(trans, dtype=np.float32).reshape(-1, 4, 4)
    src = view_sources(_live_counts(num_agent, B), A, B, ego_first, ego_count, own)
    clouds = [[] for _ in range(src["n_views"])]
    for image, view, pose in zip(src["src_image"], src["src_view"], src["src_pose"]):
        p = points[image]
        p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
        clouds[view].append(np.asarray(p, dtype=np.float32)[:, :3] if pose < 0 else transform_cloud(p, poses[pose]))
    dims = tuple(int(v) for v in config.map_dims)
    dense = np.zeros((src["n_views"], 1) + dims, dtype=np.float32)
    for v, parts in enumerate(clouds):
        if parts:
            dense[v, 0] = host_occupancy(np.concatenate(parts, 0), config.voxel_size, config.area_extents, dims)
    if not own:
        return {"dense": dense}
    n = src["n_views"] // 2
    return {"dense": dense[:n], "own_dense": dense[n:]}
