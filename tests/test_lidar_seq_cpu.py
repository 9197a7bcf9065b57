"""Lidar sequences without a GPU: the two entry points and their refusals, lidar.host_world_step (the numpy statement of
dn_lidar_world_step in include/disconet_hip.h) against linear algebra, host_scan(ids=True), the invariants and the
existence counts of synthetic.make_lidar_world over every frame, the tracker on oracle detections, and the tools' flags."""
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import lidar_seq_cases as SC
from tests.conftest import ROOT


def _tool(rel):
    spec = importlib.util.spec_from_file_location("tool_" + os.path.basename(rel)[:-3], os.path.join(ROOT, "tools", rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_declares_and_library_exports_both_entry_points():
    from disconet_amd import _lib
    with open(os.path.join(ROOT, "include", "disconet_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    assert lib.dn_version() >= 154
    for name in ("dn_lidar_world_step", "dn_lidar_scan_ids"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert getattr(lib, name) is not None and name in _lib.SIGNATURES


def test_world_step_refuses_bad_arguments_without_a_gpu():
    from disconet_amd import _lib
    lib = _lib.load()
    p = 256                                              # a non-null address that is never dereferenced
    good = dict(solids0=p, solid_vel=p, solid_count=p, agent0=p, agent_vel=p, frame=p, S=1, A=2, K=4, solids=p, pose=p,
                trans=p)
    for bad in (dict(K=257), dict(K=-1), dict(S=0), dict(A=0), dict(solids0=None), dict(solid_vel=None), dict(solids=None),
                dict(solid_count=None), dict(agent0=None), dict(agent_vel=None), dict(frame=None), dict(pose=None),
                dict(trans=None)):
        a = dict(good, **bad)
        rc = lib.dn_lidar_world_step(*[a[k] for k in good], None)
        assert rc == -1 and lib.dn_last_error(), bad       # DN_ERR_ARG, decided on the host


def test_scan_ids_refuses_bad_arguments_without_a_gpu():
    from disconet_amd import _lib
    lib = _lib.load()
    p = 256
    good = dict(solids=p, solid_count=p, object_count=p, pose=p, num_agent=p, dirs=p, jitter=None, S=1, A=1, K=4, R=8,
                max_range=80.0, ground_z=-2.0, keep_ground=0, min_points=5, half=32.0, G=4, points=p, hit=p, solid_hits=p,
                gt_boxes=p, gt_count=p, gt_own=p, gt_ids=p)
    for bad in (dict(gt_ids=None), dict(K=257), dict(R=0), dict(G=0), dict(solids=None), dict(gt_count=None),
                dict(half=float("nan"))):
        a = dict(good, **bad)
        rc = lib.dn_lidar_scan_ids(*[a[k] for k in good], None)
        assert rc == -1 and lib.dn_last_error(), bad


def _pose_matrix(x, y, sn, cs):
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1], T[0, 3], T[1, 3] = cs, -sn, sn, cs, x, y
    return T


def test_host_world_step_is_the_inverse_pose_and_the_relative_pose():
    from disconet_amd import lidar
    world, cursor = SC.world_cases()["main"]
    w0 = lidar.host_world_step(world, 0)
    assert w0["solids"].tobytes() == world["solids0"].tobytes()            # frame 0: nothing has moved, bytes and all
    for f in (cursor, 5, -3):
        w = lidar.host_world_step(world, f)
        frame = np.broadcast_to(np.asarray(f), (2,))
        assert w["frame"].tolist() == [int(v) + 1 for v in frame] and w["trans"].dtype == np.float32
        for s in range(2):
            n = int(world["solid_count"][s])
            moved = world["solids0"][s, :n, :2] + float(frame[s]) * world["solid_vel"][s, :n]
            assert np.array_equal(w["solids"][s, :n, :2], moved)
            assert w["solids"][s, :, 2:].tobytes() == world["solids0"][s, :, 2:].tobytes()
            xy = world["agent0"][s, :, :2] + float(frame[s]) * world["agent_vel"][s]
            T = [_pose_matrix(xy[a, 0], xy[a, 1], world["agent0"][s, a, 2], world["agent0"][s, a, 3]) for a in range(3)]
            for i in range(3):
                assert np.abs(w["sensor_from_world"][s, i] - np.linalg.inv(T[i])).max() < 1e-12
                assert w["trans"][s, i, i].tobytes() == np.eye(4, dtype=np.float32).tobytes()      # +0.0 and 1.0, exactly
                for j in range(3):
                    # this world's translations reach 100 m, where float32 is spaced 7.6e-6: the rotation block is held to
                    # 1e-6, a translation to one float32 step of the rounded product (the world below holds all to 1e-6)
                    want = np.linalg.inv(T[i]) @ T[j]
                    got = w["trans"][s, i, j]
                    rot = np.ones((4, 4), dtype=bool)
                    rot[:2, 3] = False
                    assert np.abs(got - want)[rot].max() <= 1e-6, (f, s, i, j)
                    if i != j:                        # (the diagonal is the exact identity, checked above)
                        near = want[:2, 3].astype(np.float32)
                        assert (np.abs(got[:2, 3].astype(np.float64) - near) <= np.spacing(np.abs(near))).all(), (f, s, i, j)


def test_trans_is_within_1e_6_of_the_matrix_product():
    """trans[i][j] against inv(T_i) @ T_j, every entry within 1e-6 absolute, on a world whose sensors stay within 5.4 m of
    the origin: a relative translation is then below 16 m, where float32 is spaced 9.5e-7 and its rounding is below 4.8e-7."""
    from disconet_amd import lidar
    world, _ = SC.world_cases()["near"]
    A = world["agent0"].shape[1]
    for f in (0, 3, 7, -7):
        w = lidar.host_world_step(world, f)
        for s in range(world["agent0"].shape[0]):
            xy = world["agent0"][s, :, :2] + float(f) * world["agent_vel"][s]
            assert np.abs(xy).max() <= 5.4
            T = [_pose_matrix(xy[a, 0], xy[a, 1], world["agent0"][s, a, 2], world["agent0"][s, a, 3]) for a in range(A)]
            for i in range(A):
                assert np.abs(w["sensor_from_world"][s, i] - np.linalg.inv(T[i])).max() < 1e-12
                for j in range(A):
                    want = np.linalg.inv(T[i]) @ T[j]
                    assert np.abs(want[:2, 3]).max() < 16.0
                    assert np.abs(w["trans"][s, i, j] - want).max() <= 1e-6, (f, s, i, j)


def test_a_nan_row_beyond_the_count_keeps_its_bytes():
    from disconet_amd import lidar
    world, _ = SC.world_cases()["main"]
    want = world["solids0"][0, 3:].tobytes()
    assert np.isnan(world["solids0"][0, 3, 0]) and np.array([SC.NAN_BITS], dtype=np.uint64).tobytes() in want
    for f in (0, 7, -2):
        assert lidar.host_world_step(world, f)["solids"][0, 3:].tobytes() == want
    with pytest.raises(ValueError, match="K = 257 solids"):
        lidar.host_world_step(dict(world, solids0=np.zeros((2, 257, 8)), solid_vel=np.zeros((2, 257, 2))), 0)


def test_host_scan_ids_name_the_kept_solids():
    from disconet_amd import lidar
    args, kw = SC.scan_world()
    plain, full = lidar.host_scan(*args, **kw), lidar.host_scan(*args, ids=True, **kw)
    assert "gt_ids" not in plain and sorted(full) == sorted(list(plain) + ["gt_ids"])
    for k in plain:
        assert plain[k].tobytes() == full[k].tobytes(), k
    ids, count = full["gt_ids"], full["gt_count"]
    assert ids.dtype == np.int32 and ids.shape == (2, 12) and count.min() > 4
    for img in range(2):
        c = int(count[img])
        kept = ids[img, :c]
        assert (np.diff(kept) > 0).all() and (ids[img, c:] == -1).all() and kept.max() < 10       # cars only
        assert 3 not in kept and 7 not in kept and 5 in kept     # outside the extents; too few returns; exactly min_points
        cx, cy, sn, cs = lidar._frame(args[3][0, img], args[0][0, kept])
        box = np.stack([cx, cy, args[0][0, kept, 2], args[0][0, kept, 3], sn, cs], 1).astype(np.float32)
        assert box.tobytes() == full["gt_boxes"][img, :c].tobytes()
        assert np.array_equal(full["gt_own_hits"][img, :c], full["solid_hits"][img, kept])
    assert 0 < full["solid_hits"][:, 7].sum() < 5 == full["solid_hits"][:, 5].sum()
    with pytest.raises(ValueError, match="object_count = 10 is more than the 4"):      # as without ids: the Python surface
        lidar.host_scan(*args, ids=True, gt_rows=4, **kw)                               # never drops a box silently


WORLD_CASES = [(0, 2, 24), (0, 5, 40)]      # seed, agents, frames


@pytest.mark.parametrize("seed, agents, frames", WORLD_CASES)
def test_generated_world_keeps_its_invariants_in_every_frame(seed, agents, frames):
    from disconet_amd.synthetic import LIDAR_KEEP_OUT, LIDAR_OCCLUDER_MARGIN, make_lidar_world
    world = make_lidar_world(agents, 256, seed, 0, frames)
    again = make_lidar_world(agents, 256, seed, 0, frames)
    assert all(np.array_equal(world[k], again[k]) for k in world if k != "world")      # seeded
    n, cars = int(world["solid_count"][0]), int(world["object_count"][0])
    assert world["solids0"].shape == (1, n, 8) and 0 < cars < n and world["agent0"].shape == (1, agents, 4)
    rows0 = world["solids0"][0]
    assert (rows0[:cars, 7] == -0.5).all() and (rows0[cars:, 7] == 1.5).all()          # cars first, occluders follow
    assert (rows0[cars:, 2:4] == 4.0).all() and (rows0[:cars, 2] <= 2.4).all()
    lane = np.abs(world["solid_vel"][0, :cars, 0]) > 0                                  # a moving car's long side (l) lies along x
    assert lane.any() and (np.abs(rows0[:cars][lane, 4]) == 1.0).all() and (rows0[:cars][lane, 5] == 0.0).all()
    assert (np.abs(world["agent0"][0, :2, 1]) == 2.5).all()                            # the first two ride the central lanes
    for f in range(frames):
        rows, sensors = SC.world_at(world, f)
        near = np.abs(rows[:, None, :2] - rows[None, :, :2]).max(-1) < 12.0             # only pairs that could touch
        for i, j in zip(*np.nonzero(np.triu(near, 1))):
            assert not SC.footprints_overlap(rows[i], rows[j], SC.CLEARANCE / 2.0), (f, i, j)
        for sx, sy in sensors:
            assert (np.hypot(rows[:cars, 0] - sx, rows[:cars, 1] - sy) > LIDAR_KEEP_OUT).all(), f
            inside = ((np.abs(rows[cars:, 0] - sx) <= rows[cars:, 2] / 2.0 + LIDAR_OCCLUDER_MARGIN)
                      & (np.abs(rows[cars:, 1] - sy) <= rows[cars:, 3] / 2.0 + LIDAR_OCCLUDER_MARGIN))
            assert not inside.any(), f


def test_the_overlap_test_sees_an_overlap():
    a, b = SC._row(0, 0, 0.0), SC._row(2.2, 0, 0.0)           # w = 2 along x: 0.2 m apart
    assert not SC.footprints_overlap(a, b) and SC.footprints_overlap(a, b, SC.CLEARANCE / 2.0)
    assert SC.footprints_overlap(SC._row(0, 0, 0.7), SC._row(2.5, 2.0, -0.4)) and not SC.footprints_overlap(
        SC._row(0, 0, 0.7), SC._row(6.5, 0, -0.4), SC.CLEARANCE / 2.0)


@pytest.mark.parametrize("seed, agents, frames", WORLD_CASES)
def test_generated_world_has_cars_that_come_go_and_hide(seed, agents, frames):
    """Every agent's ground truth holds at least 3 identities that appear after frame 0, 3 that disappear before the last
    frame and 3 with fewer than min_points = 5 returns of the ego's own in some frame while they were ground truth."""
    world, _, steps = SC.generated(agents, frames, seed)
    counts = SC.existence_counts(steps, agents)
    print("seed %d, %d agents x %d frames: (appear, disappear, seen by others only) per agent %s" % (seed, agents, frames, counts))
    assert all(min(c) >= 3 for c in counts), counts
    for st in steps:                                                    # one id per car: a row's id is its solid's row
        for a in range(agents):
            c = int(st["gt"]["count"][a])
            ids = st["gt"]["ids"][a]
            assert (np.diff(ids[:c]) > 0).all() and (ids[c:] == -1).all() and ids[:c].max(initial=0) < world["object_count"][0]


def test_tracker_on_oracle_detections_switches_no_identity_and_the_metric_sees_wrong_ids():
    _, _, steps = SC.generated(2, 24, 0)
    figures, lines = SC.host_mot(steps)
    print("\n".join(lines))
    assert figures["overall"]["IDSW"] == 0 and figures["overall"]["FP"] == 0 and figures["overall"]["TP"] > 500
    shuffled, _ = SC.host_mot(steps, permute_ids=True)
    assert shuffled["overall"]["IDSW"] > 0 and shuffled["overall"]["TP"] == figures["overall"]["TP"]


def test_sequence_host_step_is_random_access_and_shaped_for_the_metrics():
    from disconet_amd import Config, _lib, lidar
    from disconet_amd.synthetic import make_lidar_world_batch
    world = make_lidar_world_batch(2, 2, 64, seed=3, frames=4)
    assert world["solids0"].shape[0] == 2 and len(world["world"]) == 2 and world["solid_count"].max() == world["solids0"].shape[1]
    seq = lidar.Sequence(world, Config(map_hw=64), beams=4, azimuths=64, gt_rows=8, device=None) if world[
        "object_count"].max() <= 8 else lidar.Sequence(world, Config(map_hw=64), beams=4, azimuths=64, device=None)
    a, b, again = seq.host_step(2), seq.host_step(0, teacher=True), seq.host_step(2)
    G = seq.G
    assert a["bev_seq"].shape == (4, 1, 64, 64, 13) and a["trans_matrices"].shape == (2, 2, 2, 4, 4)
    assert a["num_agent"].tolist() == [[2, 2], [2, 2]] and a["gt"]["boxes"].shape == (4, G, 6)
    assert a["gt"]["ids"].shape == (4, G) and a["gt"]["count"].shape == (4,) and a["gt_own_hits"].shape == (4, G)
    assert "bev_seq_teacher" in b and "bev_seq_teacher" not in a
    assert a["trans_matrices"].tobytes() == again["trans_matrices"].tobytes() != b["trans_matrices"].tobytes()
    assert a["bev_seq"].tobytes() == again["bev_seq"].tobytes()
    with pytest.raises(_lib.DnError, match="device = None"):
        seq.step()


def test_track_tools_take_source_lidar_and_detections():
    for rel, default in (("track/eval_sort.py", "boxes"), ("track/sort_codet.py", "net")):
        mod = _tool(rel)
        args = mod.parse_args([])
        assert args.source == default and args.detections == "net"
        args = mod.parse_args(["--source", "lidar", "--detections", "truth", "--seed", "100"])
        assert (args.source, args.detections, args.seed) == ("lidar", "truth", 100)
        assert mod.parse_args(["--source", "lidar"]).detections == "net"
        with pytest.raises(SystemExit):
            mod.parse_args(["--source", "radar"])
        with pytest.raises(SystemExit):
            mod.parse_args(["--source", "lidar", "--detections", "guess"])
        with pytest.raises(SystemExit, match="--detections truth needs --source lidar"):
            mod.parse_args(["--detections", "truth"])


def test_sequence_frames_needs_lidar_scenes_and_box_targets():
    mod = _tool("det/train_codet.py")
    assert mod.parse_args([]).sequence_frames == 0
    assert mod.parse_args(["--scene", "lidar", "--targets", "boxes", "--sequence_frames", "40"]).sequence_frames == 40
    with pytest.raises(SystemExit, match="--sequence_frames N >= 0, and N > 0 needs --scene lidar --targets boxes"):
        mod.main(["--sequence_frames", "4"])
    with pytest.raises(SystemExit, match="--sequence_frames N >= 0, and N > 0 needs --scene lidar --targets boxes"):
        mod.main(["--sequence_frames", "4", "--targets", "boxes"])
    with pytest.raises(SystemExit, match="needs --targets boxes"):
        mod.main(["--sequence_frames", "4", "--scene", "lidar"])
