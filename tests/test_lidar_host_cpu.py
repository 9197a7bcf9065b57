"""The lidar sensor model without a GPU: the library's entry point, lidar.host_scan (the numpy statement of the contract in
include/disconet_hip.h) on hand cases whose answers are known, the visible-ground-truth rule, synthetic.make_lidar_scene_batch
and its occlusion property, and the tools' --scene flag."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import lidar_cases as LC
from tests.conftest import ROOT

NAN_ROW = np.full(4, np.nan, dtype=np.float32).tobytes()


def test_library_exports_the_entry_point():
    from disconet_amd import _lib
    lib = _lib.load()
    assert lib.dn_lidar_scan is not None and lib.dn_version() >= 152
    import disconet_amd
    assert disconet_amd.lidar.MAX_SOLIDS == 256 and "lidar" in disconet_amd.__all__


def test_library_refuses_bad_arguments_without_a_gpu():
    from disconet_amd import _lib
    lib = _lib.load()
    p = 256                                              # a non-null, 16-byte aligned address that is never dereferenced
    good = dict(solids=p, solid_count=p, object_count=p, pose=p, num_agent=p, dirs=p, jitter=None, S=1, A=1, K=4, R=8,
                max_range=80.0, ground_z=-2.0, keep_ground=0, min_points=5, half=32.0, G=4, points=p, hit=p, solid_hits=p,
                gt_boxes=p, gt_count=p, gt_own=p)
    for bad in (dict(K=257), dict(K=-1), dict(R=0), dict(S=0), dict(A=0), dict(G=0), dict(solids=None), dict(dirs=None),
                dict(points=None), dict(gt_count=None), dict(num_agent=None), dict(max_range=0.0), dict(half=float("nan")),
                dict(ground_z=float("inf"))):
        a = dict(good, **bad)
        rc = lib.dn_lidar_scan(*[a[k] for k in good], None)
        assert rc == -1 and lib.dn_last_error(), bad       # DN_ERR_ARG, decided on the host


def test_beam_table_is_unit_and_ordered():
    from disconet_amd import lidar
    d = lidar.beam_table(4, 8, -30.0, 10.0)
    assert d.shape == (32, 3) and d.dtype == np.float64
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-15)
    assert math.isclose(d[0, 2], math.sin(math.radians(-30.0))) and math.isclose(d[-1, 2], math.sin(math.radians(10.0)))
    assert d[0, 1] == 0.0 and d[2, 0] == pytest.approx(0.0, abs=1e-16)      # beam 0: azimuth 0, then a quarter turn


# ---- hand cases ----------------------------------------------------------------------------------------------------------------
def test_box_dead_ahead_is_hit_at_its_near_face_exactly():
    r = LC.host("dead_ahead")
    assert r["hit"].tolist() == [[0]] and r["solid_hits"].tolist() == [[1]]
    assert r["points"][0, 0].tolist() == [9.0, 0.0, 0.0, 1.0]              # t = cx - w / 2, two zero direction components
    assert r["gt_count"].tolist() == [1] and r["gt_boxes"][0, 0].tolist() == [10.0, 0.0, 2.0, 4.0, 0.0, 1.0]
    assert r["gt_own_hits"].tolist() == [[1]]


def test_the_farther_of_two_boxes_in_line_gets_no_return():
    r = LC.host("two_in_line")
    assert r["solid_hits"][0, 0] >= 3 and r["solid_hits"][0, 1] == 0
    assert set(np.unique(r["hit"]).tolist()) == {-2, 0}
    assert r["gt_count"].tolist() == [1]                                   # nobody sees the far one


def test_a_zero_direction_component_makes_no_division():
    r = LC.host("zero_component")                                          # d = (0, 1, 0): box 0 at x = 5 is passed by
    assert r["hit"].tolist() == [[1]] and r["points"][0, 0].tolist() == [0.0, 8.0, 0.0, 1.0]
    assert np.isfinite(r["points"]).all()


def test_a_sensor_inside_a_solid_gets_nothing_from_it():
    r = LC.host("sensor_inside")
    assert r["solid_hits"][0, 0] == 0 and r["solid_hits"][0, 1] >= 3


def test_max_range_cuts_returns_off():
    assert LC.host("range_short")["hit"].tolist() == [[-2]]
    assert LC.host("range_short")["points"][0, 0].tobytes() == NAN_ROW
    assert LC.host("range_exact")["hit"].tolist() == [[0]]                 # tmin <= max_range: equality is a return


def test_ground_kept_and_dropped():
    kept, dropped = LC.host("ground_kept"), LC.host("ground_dropped")
    assert kept["hit"].tolist() == [[-1, 0]] and dropped["hit"].tolist() == [[-2, 0]]
    t = -2.0 / LC.DOWN[2]
    want = [np.float32(t * LC.DOWN[0]), 0.0, np.float32(t * LC.DOWN[2]), 0.0]
    assert kept["points"][0, 0].tolist() == want and abs(float(kept["points"][0, 0, 2]) + 2.0) < 1e-6
    assert dropped["points"][0, 0].tobytes() == NAN_ROW
    assert kept["points"][0, 1].tobytes() == dropped["points"][0, 1].tobytes()
    assert kept["solid_hits"].tolist() == dropped["solid_hits"].tolist() == [[1]]


def test_a_tie_goes_to_the_lower_index():
    r = LC.host("tie")
    assert r["solid_hits"][0, 0] >= 3 and r["solid_hits"][0, 1] == 0


def test_nan_in_padded_rows_changes_nothing():
    a, b = LC.host("nan_padding"), LC.host("no_padding")
    for k in ("points", "hit", "gt_count"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["solid_hits"][:, :2].tolist() == b["solid_hits"].tolist() and not a["solid_hits"][:, 2:].any()
    assert a["gt_boxes"][:, :2].tobytes() == b["gt_boxes"].tobytes() and not a["gt_boxes"][:, 2:].any()


def test_a_padded_agents_image_is_all_misses():
    r = LC.host("padded_agents")                                           # S = 2, A = 3, live [3, 1]: image a * 2 + s
    for img in (3, 5):                                                     # agents 1 and 2 of scene 1
        assert (r["hit"][img] == -2).all() and not r["solid_hits"][img].any() and r["gt_count"][img] == 0
        assert r["points"][img].tobytes() == NAN_ROW * r["hit"].shape[1]
    for img in (0, 1, 2, 4):
        assert (r["hit"][img] >= 0).any()


def test_jitter_moves_a_point_along_its_ray():
    args, kw = LC.cases()["two_in_line"]
    plain, moved = LC.host("two_in_line"), LC.host("two_in_line", True)
    j = LC.jitter_for(args)
    assert plain["hit"].tobytes() == moved["hit"].tobytes() and plain["solid_hits"].tobytes() == moved["solid_hits"].tobytes()
    got = plain["hit"][0] >= 0
    step = moved["points"][0, got, :3].astype(np.float64) - plain["points"][0, got, :3].astype(np.float64)
    assert np.allclose(step, j[0, got, None].astype(np.float64) * args[5][got], atol=5e-6)      # two float32 roundings at |p| < 32
    assert np.abs(step).max() > 0.01


# ---- the ground-truth rule -------------------------------------------------------------------------------------------------------
def test_the_extents_test_is_strict():
    r = LC.host("strict_extents")                                          # min_points = 0: the extents alone decide
    inside = np.float32(np.nextafter(LC.HALF, 0.0))
    assert r["gt_count"].tolist() == [2]
    assert r["gt_boxes"][0, 0, :2].tolist() == [inside, 8.0] and r["gt_boxes"][0, 1, :2].tolist() == [3.0, -inside]


def test_min_points_is_counted_over_the_live_agents_only():
    padded, live = LC.host("seen_by_a_padded_agent"), LC.host("seen_by_a_live_agent")
    assert live["solid_hits"][0, 0] == 0 and live["solid_hits"][1, 0] >= 5     # hidden from agent 0, seen by agent 1
    assert padded["gt_count"].tolist() == [0, 0] and not padded["solid_hits"][1].any()
    assert live["gt_count"].tolist() == [1, 1]
    assert live["gt_own_hits"][:, 0].tolist() == [0, int(live["solid_hits"][1, 0])]
    assert live["gt_boxes"][0, 0, :4].tolist() == [16.0, 0.0, 2.0, 4.0]
    from disconet_amd.synthetic import boxes_in_agent_frame
    want = boxes_in_agent_frame(np.array([[16.0, 0.0, 2.0, 4.0, 0.0, 1.0]]), 1)[0].astype(np.float32)
    assert live["gt_boxes"][1, 0].tobytes() == want.tobytes()


def test_compaction_keeps_the_order_and_zeroes_the_rest():
    r = LC.host("compaction")
    assert r["gt_count"].tolist() == [3]
    assert r["gt_boxes"][0, :3, :2].tolist() == [[10.0, 0.0], [0.0, 10.0], [-10.0, 0.0]]
    assert not r["gt_boxes"][0, 3:].any() and not r["gt_own_hits"][0, 3:].any()
    assert r["gt_own_hits"][0, :3].tolist() == r["solid_hits"][0, [0, 2, 3]].tolist()
    few = LC.host("fewer_rows_than_solids")                                # G = 3 < K = 5, three objects, two of them kept
    assert few["gt_count"].tolist() == [2] and few["gt_boxes"].shape == (1, 3, 6) and not few["gt_boxes"][0, 2:].any()
    assert LC.host("no_objects")["gt_count"].tolist() == [0]


def test_more_objects_than_rows_raises():
    from disconet_amd import lidar
    args, kw = LC.cases()["compaction"]
    with pytest.raises(ValueError, match="object_count = 4 is more than the 3 ground-truth rows"):
        lidar.host_scan(*args, **dict(kw, gt_rows=3))


# ---- the scenes ------------------------------------------------------------------------------------------------------------------
def test_scene_is_repeatable_and_shaped_like_the_box_scene():
    from disconet_amd.synthetic import make_box_scene_batch, make_lidar_scene_batch
    kw = dict(batch_size=2, num_agent=2, map_hw=64, seed=3, boxes_per_scene=6, teacher=True)
    a, b = make_lidar_scene_batch(beams=8, azimuths=64, **kw), make_lidar_scene_batch(beams=8, azimuths=64, **kw)
    ref = make_box_scene_batch(**kw)
    for k, v in ref.items():
        if isinstance(v, torch.Tensor):
            assert a[k].shape == v.shape and a[k].dtype == v.dtype, k
            assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), k
    assert set(a) == set(ref) | {"gt_own_hits", "solid_hits", "world_solids"}
    assert len(a["points"]) == 4 and a["points"][0].shape == (8 * 64, 4) and a["points"][0].dtype == np.float32
    assert a["gt_own_hits"].shape == (4, 6) and a["gt_own_hits"].dtype == torch.int32
    other = make_lidar_scene_batch(beams=8, azimuths=64, **dict(kw, seed=4))
    assert other["bev_seq"].numpy().tobytes() != a["bev_seq"].numpy().tobytes()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_cars_are_the_box_scenes_and_no_sensor_is_inside_a_solid(seed):
    from disconet_amd.synthetic import agent_pose, lidar_world_solids, make_box_scene_batch
    rows, cars = lidar_world_solids(5, 256, seed, 0, 24, 10)
    world = make_box_scene_batch(1, 1, 256, seed=seed, clutter=0)["world_boxes"][0]
    have = {r[:6].tobytes() for r in rows[:cars]}
    assert have <= {w.tobytes() for w in world} and cars >= len(world) - 5
    assert len(rows) - cars == 10 and (rows[cars:, 2:8] == [4.0, 4.0, 0.0, 1.0, -2.0, 1.5]).all()
    for a in range(5):
        sx, sy = agent_pose(a)[:2, 3]
        dx, dy = sx - rows[:, 0], sy - rows[:, 1]
        u, v = dx * rows[:, 5] + dy * rows[:, 4], dy * rows[:, 5] - dx * rows[:, 4]
        assert not ((np.abs(u) <= rows[:, 2] / 2) & (np.abs(v) <= rows[:, 3] / 2)).any()
        assert (np.hypot(dx[:cars], dy[:cars]) > 4.0).all()


def _hidden_pairs(scene, min_points=5):
    own, count = scene["gt_own_hits"].numpy(), scene["gt_count"].numpy()
    return [(i, g) for i in range(len(count)) for g in range(int(count[i])) if own[i, g] < min_points]


def test_some_ground_truth_is_seen_only_through_collaboration():
    """The property the scenes exist for: (image, ground-truth row) pairs with fewer than min_points returns of their own
    (kept because the scene's agents together have enough).  The float64 prototype of the rule found 31 over seeds 0..3,
    at least one in every seed; lidar.host_scan finds [4, 16, 8, 3] = 31."""
    found = [len(_hidden_pairs(LC.property_scene(seed))) for seed in range(4)]
    print("pairs with gt_own_hits < min_points, seeds 0..3:", found)
    assert min(found) >= 1 and sum(found) >= 10, found


def _voxels_meeting(cfg, gt_row, z_lo, z_hi):
    """index arrays (i, j, z) of the voxels that meet the box: centre within the footprint grown by half a voxel diagonal,
    height bin overlapping [z_lo, z_hi]"""
    from disconet_amd.synthetic import seg_pixel_centres
    xs, ys = seg_pixel_centres(cfg)
    x, y, w, l, s, c = (float(v) for v in gt_row)
    grow = 0.5 * math.hypot(cfg.voxel_size[0], cfg.voxel_size[1])
    dx, dy = (xs - x)[:, None], (ys - y)[None, :]
    u, v = dx * c + dy * s, dy * c - dx * s
    i, j = np.nonzero((np.abs(u) <= w / 2 + grow) & (np.abs(v) <= l / 2 + grow))
    vz, z0 = float(cfg.voxel_size[2]), float(cfg.area_extents[2][0])
    bins = np.arange(int(math.floor((z_lo - z0) / vz)), int(math.floor((z_hi - z0) / vz)) + 1)
    return np.repeat(i, len(bins)), np.repeat(j, len(bins)), np.tile(bins, len(i))


def test_a_hidden_box_is_absent_from_the_own_view_and_present_in_the_teachers():
    """Pairs with no return of their own at all (a pair with one to four returns has those points in its own view): no
    occupied voxel of bev_seq meets the box, at least one of bev_seq_teacher does."""
    from disconet_amd import Config
    from disconet_amd.synthetic import BOX_Z
    cfg = Config(map_hw=256)
    checked = 0
    for seed in range(4):
        scene = LC.property_scene(seed)
        own = scene["gt_own_hits"].numpy()
        for img, g in _hidden_pairs(scene):
            if own[img, g] != 0:
                continue
            i, j, z = _voxels_meeting(cfg, scene["gt_boxes"][img, g].numpy(), *BOX_Z)
            assert len(i) and not scene["bev_seq"][img, 0].numpy()[i, j, z].any(), (seed, img, g)
            assert scene["bev_seq_teacher"][img, 0].numpy()[i, j, z].any(), (seed, img, g)
            checked += 1
    assert checked >= 4


# ---- the tools -------------------------------------------------------------------------------------------------------------------
def _tool(rel):
    spec = importlib.util.spec_from_file_location("lidar_tool_" + rel.replace("/", "_").replace(".py", ""),
                                                  os.path.join(ROOT, "tools", rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("rel, parser", [("det/train_codet.py", "build_parser"), ("det/eval_codet.py", "build_eval_parser"),
                                         ("det/detect_codet.py", "build_detect_parser"),
                                         ("det/visualize_codet.py", "build_vis_parser")])
def test_tools_take_scene_lidar_and_still_refuse_v2v(rel, parser):
    mod = _tool(rel)
    ap = getattr(mod, parser)()
    assert ap.parse_known_args([])[0].scene == "boxes"
    assert ap.parse_known_args(["--scene", "lidar"])[0].scene == "lidar"
    with pytest.raises(SystemExit):
        ap.parse_known_args(["--scene", "fog"])
    with pytest.raises(SystemExit, match=r"disco \| sum \| mean \| max"):
        mod.main(["--com", "v2v", "--scene", "lidar"])


def test_the_tools_lidar_scenes_have_occluders_and_hidden_boxes():
    """The det tools ask their box scenes for 64 cars, which is every grid cell at 256 x 256 and would leave no occluder a
    cell: codet_common.lidar_scene, the one place the tools build a lidar scene, keeps 24 cars and pads the ground truth
    to the tool's 64 rows.  At the tools' default of 5 agents its scenes are the property scenes; at the README recipe's 2
    agents every scene still has its ten occluders, and boxes hidden from an ego exist (seeds 0 .. 3: 0, 4, 0, 1)."""
    _tool("det/eval_codet.py")                                             # (puts tools/det on the path, as every tool does)
    import codet_common
    for seed in range(4):
        scene, ref = codet_common.lidar_scene(1, 5, 256, seed, 64, device=None), LC.property_scene(seed)
        assert scene["gt_boxes"].shape == (5, 64, 6) and scene["gt_own_hits"].shape == (5, 64)
        assert torch.equal(scene["gt_boxes"][:, :24], ref["gt_boxes"]) and not scene["gt_boxes"][:, 24:].any()
        assert torch.equal(scene["gt_count"], ref["gt_count"]) and torch.equal(scene["gt_own_hits"][:, :24], ref["gt_own_hits"])
        assert torch.equal(scene["bev_seq"], ref["bev_seq"])
        assert len(scene["world_solids"][0]) - len(scene["world_boxes"][0]) == 10
    hidden = []
    for seed in range(4):
        scene = codet_common.lidar_scene(1, 2, 256, seed, 64, device=None)
        assert len(scene["world_solids"][0]) - len(scene["world_boxes"][0]) == 10, seed
        hidden.append(len(_hidden_pairs(scene)))
    print("the recipe's scenes (2 agents), pairs with gt_own_hits < min_points, seeds 0..3:", hidden)
    assert sum(hidden) >= 1, hidden


def test_more_cars_than_free_cells_leave_no_occluder_and_gt_rows_only_pads():
    from disconet_amd.synthetic import lidar_world_solids, make_lidar_scene_batch
    rows, cars = lidar_world_solids(2, 256, 0, 0, 64, 10)                  # 64 cars on 64 cells: documented, no occluder
    assert len(rows) == cars
    with pytest.raises(ValueError, match="gt_rows = 4 is below boxes_per_scene = 6"):
        make_lidar_scene_batch(1, 2, 64, boxes_per_scene=6, gt_rows=4, beams=4, azimuths=16)


def test_source_ranges_are_checked_against_the_call():
    from disconet_amd import Config, holistic
    r = holistic.source_ranges(np.arange(5) * 8, [2, 2], 2, 2, own=True, device="cpu")
    assert r["max_count"] == 8 and r["begin"].tolist() == [0, 16, 0, 16, 8, 24, 8, 24, 0, 16, 8, 24]
    assert r["count"].tolist() == [8] * 12 and r["src"]["n_views"] == 8
    pts = torch.zeros((32, 4))
    trans = torch.zeros((2, 2, 2, 4, 4))
    with pytest.raises(ValueError, match="`ranges` was made for other clouds"):
        holistic.holistic_views((pts, np.arange(5) * 8), trans, [2, 1], 2, Config(map_hw=64), own=True, ranges=r)
    with pytest.raises(ValueError, match="`ranges` was made for other clouds"):
        holistic.holistic_views((pts, np.arange(5) * 8), trans, [2, 2], 2, Config(map_hw=64), own=False, ranges=r)


def test_scene_lidar_needs_box_targets_and_scene_ground_truth():
    with pytest.raises(SystemExit, match="--scene lidar needs --targets boxes"):
        _tool("det/train_codet.py").main(["--scene", "lidar"])
    with pytest.raises(SystemExit, match="--scene lidar needs --gt scene"):
        _tool("det/eval_codet.py").main(["--scene", "lidar"])
