"""dn_voxelize_views / holistic.holistic_views on the MI355X against the numpy reference holistic.host_holistic_views
and against the shipped voxeliser.  Every comparison is bit for bit (np.array_equal / torch.equal): the arithmetic of the
transform is a contract (include/disconet_hip.h), float64 sums in a fixed order rounded once to float32, and
tests/test_holistic_host_cpu.py shows that the crafted cloud used here tells it from float32 arithmetic and from
unrounded float64 coordinates.  Then one real distillation step on the views, and the training tool's KD form."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import holistic_cases as H
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def _views(s, batch, agents, hw, **kw):
    kw.setdefault("want", ("dense", "bits"))
    return H.device_scene_views(s, batch, agents, hw, **kw)


def _check_pair(out, host_dense, what):
    d, b = out["dense"], out["bits"]
    assert d.dtype == torch.float32 and tuple(d.shape) == host_dense.shape, what
    assert np.array_equal(d.cpu().numpy(), host_dense), what
    assert b.bits and b.data.dtype == torch.int32 and b.shape == (d.shape[0],) + tuple(d.shape[2:]), what
    assert torch.equal(b.nhwc(), d[:, 0]), what


# ---- against the host reference ----------------------------------------------------------------------------------------
def test_device_equals_host_on_the_64_map_scene():
    s = H.scene_64()
    _check_pair(_views(s, 2, 3, 64), s["bev_seq_teacher"].numpy(), "64")


def test_device_equals_host_at_128():
    s = H.scene(1, 3, 128, 1, 16)
    _check_pair(_views(s, 1, 3, 128), s["bev_seq_teacher"].numpy(), "128")


def test_ragged_batch_padded_views_are_zero():
    from disconet_amd.holistic import host_holistic_views
    s = H.scene_64()
    host = host_holistic_views(s["points"], s["trans_matrices"], [3, 2], 2, H.cfg(64))["dense"]
    assert not host[2 * 2 + 1].any() and all(host[v].any() for v in (0, 1, 2, 3, 4))
    assert not np.array_equal(host[1], s["bev_seq_teacher"].numpy()[1])          # scene 1 lost agent 2's cloud
    out = _views(s, 2, 3, 64, live=[3, 2])
    _check_pair(out, host, "ragged")
    # the [B, A] tensor form of the counts gives the same
    na = torch.tensor([[3] * 3, [2] * 3])
    assert torch.equal(_views(s, 2, 3, 64, live=na)["dense"], out["dense"])


def test_ego_range_equals_the_rows_of_the_full_result():
    s = H.scene_64()
    full = _views(s, 2, 3, 64)
    part = _views(s, 2, 3, 64, ego_first=1, ego_count=2)
    assert torch.equal(part["dense"], full["dense"][2:6]) and torch.equal(part["bits"].data, full["bits"].data[2:6])


def test_own_views_from_the_same_launch():
    from disconet_amd import ops
    s = H.scene_64()
    c = H.cfg(64)
    out = _views(s, 2, 3, 64, own=True)
    _check_pair({"dense": out["dense"], "bits": out["bits"]}, s["bev_seq_teacher"].numpy(), "holistic beside own")
    _check_pair({"dense": out["own_dense"], "bits": out["own_bits"]}, s["bev_seq"].numpy(), "own")
    for k, p in enumerate(s["points"]):
        one = ops.voxelize_occupy(torch.from_numpy(p).cuda(), c.voxel_size, c.area_extents, c.map_dims)
        assert torch.equal(out["own_dense"][k, 0], one), k


# ---- the crafted cloud ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [64, 128])
def test_crafted_cloud_under_the_contract(hw):
    from disconet_amd import ops
    from disconet_amd.synthetic import host_occupancy
    T = H.crafted_pose()
    pts = H.near_face_cloud(T, hw)
    c = H.cfg(hw)
    dev = torch.from_numpy(pts).cuda()
    host = host_occupancy(H.coords_contract(pts, T), c.voxel_size, c.area_extents, c.map_dims)
    out = H.single_source(dev, T, hw)
    _check_pair(out, host[None, None], "crafted %d" % hw)
    wrong = H.grid_of(H.cells(H.coords_float32_arithmetic(pts, T), hw), hw)
    print("map %d: the device's grid differs from the float32-arithmetic grid in %d cells" % (
        hw, int((out["dense"][0, 0].cpu().numpy() != wrong).sum())))
    # pose -1: the same cloud as it is, bit for bit the shipped voxeliser
    plain = H.single_source(dev, None, hw)
    assert torch.equal(plain["dense"][0, 0], ops.voxelize_occupy(dev, c.voxel_size, c.area_extents, c.map_dims))
    assert torch.equal(plain["bits"].nhwc()[0], plain["dense"][0, 0])


# ---- against the shipped voxeliser -------------------------------------------------------------------------------------
def test_views_equal_the_shipped_voxeliser_on_host_merged_clouds():
    from disconet_amd import ops
    from disconet_amd.holistic import transform_cloud, view_sources
    s = H.scene_64()
    c = H.cfg(64)
    out = _views(s, 2, 3, 64, want=("dense",))
    src = view_sources([3, 3], 3, 2)
    poses = s["trans_matrices"].numpy().reshape(-1, 4, 4)
    for v in range(6):
        parts = [s["points"][i][:, :3] if p < 0 else transform_cloud(s["points"][i], poses[p])
                 for i, vv, p in zip(src["src_image"], src["src_view"], src["src_pose"]) if vv == v]
        merged = torch.from_numpy(np.ascontiguousarray(np.concatenate(parts, 0))).cuda()
        assert torch.equal(out["dense"][v, 0], ops.voxelize_occupy(merged, c.voxel_size, c.area_extents, c.map_dims)), v


# ---- edge inputs -----------------------------------------------------------------------------------------------------------
def _raw(pts, begin, count, view, pose, poses, n_views, hw=64, want=("dense", "bits"), max_count=None):
    from disconet_amd import ops
    c = H.cfg(hw)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
    mc = max(count or [0]) if max_count is None else max_count
    return ops.voxelize_views(pts, i32(begin), i32(count), i32(view), i32(pose), poses, n_views, mc, c.voxel_size,
                              c.area_extents, c.map_dims, want=want)


def _scene_raw():
    """the 64-map scene as raw launch arguments (pts, lists, poses)"""
    from disconet_amd.holistic import pack_clouds, view_sources
    s = H.scene_64()
    pts, off = pack_clouds(s["points"], "cuda")
    src = view_sources([3, 3], 3, 2)
    begin = [int(off[i]) for i in src["src_image"]]
    count = [int(off[i + 1] - off[i]) for i in src["src_image"]]
    return s, pts, begin, count, src["src_view"], src["src_pose"], s["trans_matrices"].cuda().reshape(-1, 4, 4).contiguous()


def test_empty_inputs_give_zeros():
    from disconet_amd.holistic import holistic_views
    s, pts, begin, count, view, pose, poses = _scene_raw()
    out = _raw(pts, [], [], [], [], poses, 3)                                           # n_src == 0
    assert not out["dense"].any() and not out["bits"].data.any() and tuple(out["dense"].shape) == (3, 1, 64, 64, 13)
    out = _raw(pts, [0, 5], [0, 0], [0, 1], [-1, 0], poses, 2)                         # sources without points
    assert not out["dense"].any() and not out["bits"].data.any()
    out = _raw(pts, begin[:3], count[:3], view[:3], pose[:3], poses, 6)                 # views 1..5 have no sources
    assert out["dense"][0].any() and not out["dense"][1:].any() and not out["bits"].data[1:].any()
    empty = [np.zeros((0, 4), np.float32)] * 6
    out = holistic_views(empty, s["trans_matrices"], [3, 3], 2, H.cfg(64), want=("dense", "bits"))
    assert not out["dense"].any() and not out["bits"].data.any()


def test_a_source_that_points_outside_its_buffers_writes_nothing():
    """The lists live on the device, so the kernel is what refuses them.  Every buffer handed over here is a slice of a
    larger allocation: the bad indices stay inside memory this test owns, and the bytes around the outputs are checked."""
    from disconet_amd import ops
    s, pts, begin, count, view, pose, poses = _scene_raw()
    c = H.cfg(64)
    inner = pts[16:pts.shape[0] - 16]                       # rows -1 and n + 4 of `inner` exist in `pts`
    n = inner.shape[0]
    dense = torch.full((4, 1, 64, 64, 13), 7.0, device="cuda")
    words = torch.full((4, 64, 64), 7, dtype=torch.int32, device="cuda")
    out = {"dense": dense[1:2], "bits": ops.SpTensor(1, 64, 64, 13, data=words[1:2], bits=True)}
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
    #            good  past the end  view 1 of 1  view -1  pose 2 of 2  pose -2  begin -1  count -1
    lists = [i32(v) for v in ([0, n - 4, 0, 0, 0, 0, -1, 0], [8, 8, 8, 8, 8, 8, 8, -1], [0, 0, 1, -1, 0, 0, 0, 0],
                              [-1, -1, -1, -1, 2, -2, -1, -1])]
    ops.voxelize_views(inner, *lists, poses[:2], 1, 8, c.voxel_size, c.area_extents, c.map_dims, want=("dense", "bits"), out=out)
    only = _raw(inner, [0], [8], [0], [-1], poses[:2], 1)
    assert torch.equal(dense[1:2], only["dense"]) and torch.equal(words[1:2], only["bits"].data)
    assert bool((dense[0] == 7).all()) and bool((dense[2:] == 7).all()) and bool((words[0] == 7).all()) and bool((words[2:] == 7).all())


def test_duplicated_and_reversed_sources_and_both_strides_write_the_same_bytes():
    s, pts, begin, count, view, pose, poses = _scene_raw()
    ref = _raw(pts, begin, count, view, pose, poses, 6)
    _check_pair(ref, s["bev_seq_teacher"].numpy(), "raw lists")
    rev = _raw(pts, begin[::-1], count[::-1], view[::-1], pose[::-1], poses, 6)
    dup = _raw(pts, begin + begin[:5], count + count[:5], view + view[:5], pose + pose[:5], poses, 6)
    small_grid = _raw(pts, begin, count, view, pose, poses, 6, max_count=1)            # max_count only sizes the grid
    xyz = _raw(pts[:, :3].contiguous(), begin, count, view, pose, poses, 6)            # pt_stride 3 against 4
    assert pts.shape[1] == 4
    for other in (rev, dup, small_grid, xyz):
        assert torch.equal(other["dense"], ref["dense"]) and torch.equal(other["bits"].data, ref["bits"].data)
    for want in (("dense",), ("bits",)):
        one = _raw(pts, begin, count, view, pose, poses, 6, want=want)
        assert tuple(one) == want
        assert torch.equal(one[want[0]] if want[0] == "dense" else one["bits"].data,
                           ref["dense"] if want[0] == "dense" else ref["bits"].data)


def test_nan_and_inf_points_are_dropped():
    from disconet_amd.holistic import transform_cloud
    from disconet_amd.synthetic import host_occupancy
    T = H.crafted_pose()
    c = H.cfg(64)
    good = H.near_face_cloud(T, 64)[:512]
    bad = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 0], [0, 0, np.inf],
                    [np.inf, np.inf, 0], [3e38, 3e38, 0], [-3e38, 3e38, 0]], np.float32)
    both = np.concatenate([bad, good, bad], 0)
    dev = torch.from_numpy(both).cuda()
    for pose in (T, None):
        coords = transform_cloud(both, T) if pose is not None else both
        want = host_occupancy(coords, c.voxel_size, c.area_extents, c.map_dims)
        clean = host_occupancy(transform_cloud(good, T) if pose is not None else good, c.voxel_size, c.area_extents, c.map_dims)
        assert np.array_equal(want, clean)
        _check_pair(H.single_source(dev, pose, 64), want[None, None], "nan / inf")


def test_33_height_bins_with_bits_raise():
    from disconet_amd import _lib, ops
    pts = torch.zeros((4, 3), device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
    args = (pts, i32([0]), i32([4]), i32([0]), i32([-1]), torch.eye(4, device="cuda")[None], 1, 4, (0.25, 0.25, 0.4),
            ((-8.0, 8.0), (-8.0, 8.0), (-3.0, 9.9)), (64, 64, 33))
    with pytest.raises(_lib.DnError, match="33 height bins"):
        ops.voxelize_views(*args, want=("dense", "bits"))
    out = ops.voxelize_views(*args, want=("dense",))                     # the dense grid alone has no such limit
    assert tuple(out["dense"].shape) == (1, 1, 64, 64, 33) and int(out["dense"].sum()) == 1


# ---- repeatability and capture -----------------------------------------------------------------------------------------
def test_two_runs_and_a_graph_replay_write_the_same_bytes():
    s, pts, begin, count, view, pose, poses = _scene_raw()
    from disconet_amd import ops
    c = H.cfg(64)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
    lists = [i32(v) for v in (begin, count, view, pose)]
    run = lambda: ops.voxelize_views(pts, *lists, poses, 6, max(count), c.voxel_size, c.area_extents, c.map_dims,   # noqa: E731
                                     want=("dense", "bits"))
    flat = lambda o: {"dense": o["dense"], "bits": o["bits"].data}                                                   # noqa: E731
    first, second = flat(run()), flat(run())
    for k in first:
        assert torch.equal(first[k].view(torch.uint8), second[k].view(torch.uint8)), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = flat(run())
    for k in captured:
        captured[k].view(torch.uint8).fill_(0xCD)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(first[k].view(torch.uint8), captured[k].view(torch.uint8)), k


def test_box_scene_with_teacher_on_the_gpu_equals_the_host_form():
    from disconet_amd.synthetic import make_box_scene_batch
    dev = make_box_scene_batch(1, 2, 128, seed=2, boxes_per_scene=16, teacher=True, device="cuda")
    host = H.scene(1, 2, 128, 2, 16)
    keys = [k for k, v in host.items() if isinstance(v, torch.Tensor)]
    assert "bev_seq_teacher" in keys and len(keys) == 6
    for k in keys:
        assert dev[k].is_cuda and dev[k].dtype == host[k].dtype and torch.equal(dev[k].cpu(), host[k]), k


# ---- one real distillation step ---------------------------------------------------------------------------------------------
def test_one_kd_step_on_the_holistic_views():
    """tests/assign_train_case.py's size (128 x 128, 2 agents, batch 1): CoDetModule.step(kd_flag = 1) with bev_seq_teacher
    from the one-launch call and targets from assign_targets; the same step with bev_seq_teacher uploaded from
    host_holistic_views gives the same losses to the 1e-12 relative bar tests/test_gpu_assign.py takes from
    tests/test_gpu_train_step.py (the loss scalars are sums by f64 atomics: their last bits are not repeatable run to run)."""
    from disconet_amd import CoDetModule, Config, DiscoNet, TeacherNet, holistic, postprocess as P, targets as T
    from tests import assign_train_case as TC
    cfg = Config(map_hw=TC.HW)
    torch.manual_seed(0)
    model = DiscoNet(cfg, kd_flag=1, num_agent=TC.AGENTS).cuda()
    teacher = TeacherNet(cfg).cuda().eval()
    module = CoDetModule(model, teacher, cfg, None, kd_flag=1)
    scene = TC.scene(device="cuda")
    live = [TC.AGENTS] * TC.BATCH
    view = holistic.holistic_views(scene["points"], scene["trans_matrices"], live, TC.BATCH, cfg)["dense"]
    assert tuple(view.shape) == tuple(scene["bev_seq"].shape) and bool((view >= scene["bev_seq"]).all())
    assert int(view.sum()) > int(scene["bev_seq"].sum())
    data = {k: scene[k] for k in ("bev_seq", "trans_matrices", "num_agent")}
    data.update(T.assign_targets(P.make_anchors(cfg), scene["gt_boxes"], scene["gt_count"]))
    data["kd_weight"] = 1e5
    direct = module.step(dict(data, bev_seq_teacher=view), TC.BATCH, update=False)
    host = holistic.host_holistic_views(scene["points"], scene["trans_matrices"], live, TC.BATCH, cfg)["dense"]
    uploaded = torch.from_numpy(host).cuda()
    through_host = module.step(dict(data, bev_seq_teacher=uploaded), TC.BATCH, update=False)
    print("losses", direct, "with the host's view", through_host)
    assert set(direct) == {"loss", "cls_loss", "loc_loss", "kd_loss"}
    assert all(np.isfinite(v) for v in direct.values()) and direct["kd_loss"] > 0
    for k in direct:
        assert abs(direct[k] - through_host[k]) <= 1e-12 * abs(direct[k]), k
    assert torch.equal(uploaded, view)
    # the step's own conversion of the view (TeacherNet's encoder input) is a view of the tensor the call wrote
    assert teacher._enc_input(view).data_ptr() == view.data_ptr()


# ---- the training tool ------------------------------------------------------------------------------------------------------
def test_cli_kd_training_on_box_scenes(tmp_path):
    train = os.path.join(ROOT, "tools", "det", "train_codet.py")
    r = subprocess.run([sys.executable, train, "--com", "disco", "--targets", "boxes", "--kd_flag", "1", "--nepoch", "1",
                        "--steps_per_epoch", "2", "--num_agent", "2", "--batch", "1", "--logpath", str(tmp_path)], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout[-600:])
    import re
    assert "epoch 1: mean loss" in r.stdout and re.search(r"kd_loss [0-9.]+", r.stdout), r.stdout
    assert r.stdout.lstrip().startswith("teacher: no --resume_teacher")
    assert (tmp_path / "epoch_1.pth").exists()
