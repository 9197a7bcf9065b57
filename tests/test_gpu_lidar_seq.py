"""Lidar sequences on the device against their numpy statements, equal in every byte: dn_lidar_world_step against
lidar.host_world_step over consecutive calls (the cursor advances on the device), dn_lidar_scan_ids against
lidar.host_scan(ids=True), lidar.Sequence.step() captured into one graph against Sequence.host_step(f) replay after
replay, and the tools with --source lidar / --sequence_frames."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lidar_seq_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8))[0]
        raise AssertionError("%s differs in %d bytes, the first at byte %d" % (what, len(bad), bad[0]))


@pytest.mark.parametrize("name", sorted(SC.world_cases()))
def test_world_step_equals_the_host_statement_call_after_call(name):
    from disconet_amd import lidar
    world, cursor = SC.world_cases()[name]
    dev = lidar.world_to_device(world)
    frame = torch.from_numpy(cursor.copy()).cuda()
    out = None
    for call in range(3):
        out = lidar.world_step(dev, frame, out=out)              # the second and third call write into the first's tensors
        host = lidar.host_world_step(world, cursor + call)
        for k in ("solids", "sensor_from_world", "trans"):
            _same(out[k], host[k], "%s, call %d: %s" % (name, call, k))
        _same(frame, host["frame"], "%s, call %d: the cursor" % (name, call))
    assert frame.cpu().tolist() == (cursor + 3).tolist()


def test_world_step_refuses_one_solid_too_many_and_host_tensors():
    from disconet_amd import _lib, lidar
    world, cursor = SC.world_cases()["one_agent"]
    big = dict(world, solids0=np.zeros((2, 257, 8)), solid_vel=np.zeros((2, 257, 2)))
    frame = torch.from_numpy(cursor.copy()).cuda()
    with pytest.raises(_lib.DnError, match="K = 257 solids"):
        lidar.world_step(lidar.world_to_device(big), frame)
    assert frame.cpu().tolist() == cursor.tolist()               # refused on the host: nothing ran
    with pytest.raises(_lib.DnError, match="needs device tensors"):
        lidar.world_step(world, frame)


def test_scan_ids_equals_the_host_statement_and_leaves_the_scan_alone():
    from disconet_amd import _lib, lidar
    from disconet_amd.ops import _ptr, _stream
    import ctypes
    args, kw = SC.scan_world()
    host = lidar.host_scan(*args, ids=True, **kw)
    dev, plain = lidar.scan(*args, ids=True, **kw), lidar.scan(*args, **kw)
    assert "gt_ids" not in plain and sorted(k for k in dev if k != "cloud") == sorted(host)
    for k in host:
        _same(dev[k], host[k], "ids=True: " + k)
        if k != "gt_ids":
            _same(plain[k], host[k], "ids=False: " + k)
    assert int(host["gt_count"].min()) > 4
    # G = 4, smaller than the kept count: the Python surface refuses it (object_count > gt_rows), the entry point keeps the
    # first G rows and reports G -- through the library, against the host's first four rows
    G, n_img, K, R = 4, 2, 12, args[5].shape[0]
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
    out = {"points": torch.empty((n_img, R, 4), dtype=torch.float32, device="cuda"),
           "hit": torch.empty((n_img, R), dtype=torch.int32, device="cuda"),
           "solid_hits": torch.empty((n_img, K), dtype=torch.int32, device="cuda"),
           "gt_boxes": torch.full((n_img, G, 6), 9.0, dtype=torch.float32, device="cuda"),
           "gt_count": torch.empty((n_img,), dtype=torch.int32, device="cuda"),
           "gt_own_hits": torch.full((n_img, G), 9, dtype=torch.int32, device="cuda"),
           "gt_ids": torch.full((n_img, G), 9, dtype=torch.int32, device="cuda")}
    _lib.check(_lib.load().dn_lidar_scan_ids(
        *[_ptr(x) for x in t], None, 1, 2, K, R, ctypes.c_double(kw["max_range"]), ctypes.c_double(lidar.GROUND_Z), 0,
        kw["min_points"], ctypes.c_double(kw["half_extent"]), G, *[_ptr(out[k]) for k in out], _stream()), "dn_lidar_scan_ids")
    assert out["gt_count"].cpu().tolist() == [G, G]
    for k in ("gt_boxes", "gt_own_hits", "gt_ids"):
        _same(out[k], np.ascontiguousarray(host[k][:, :G]), "G = 4: " + k)
    for k in ("points", "hit", "solid_hits"):
        _same(out[k], host[k], "G = 4: " + k)


def _flat(step):
    return {"bev_seq": step["bev_seq"], "trans_matrices": step["trans_matrices"], "num_agent": step["num_agent"],
            "gt_boxes": step["gt"]["boxes"], "gt_ids": step["gt"]["ids"], "gt_count": step["gt"]["count"],
            "gt_own_hits": step["gt_own_hits"], "bev_seq_teacher": step["bev_seq_teacher"]}


def test_sequence_step_replays_frame_after_frame_from_one_graph():
    from disconet_amd import Config, graph, holistic, lidar
    from disconet_amd.synthetic import make_lidar_world
    cfg = Config(map_hw=64)
    world = make_lidar_world(2, 64, 0, 0, 8)
    seq = lidar.Sequence(world, cfg, beams=8, azimuths=256, min_points=2)
    host = [_flat(seq.host_step(f, teacher=True)) for f in range(4)]
    assert sum(int(h["gt_count"].sum()) for h in host) > 0 and host[0]["trans_matrices"].tobytes() != host[1][
        "trans_matrices"].tobytes() and host[0]["bev_seq"].tobytes() != host[3]["bev_seq"].tobytes()
    step = graph.GraphedStep(lambda: seq.step(teacher=True), range_guard=False)
    holistic._SRC_CACHE.clear()          # the graph depends on no module cache: the Sequence owns its index tensors
    seq.reset()                          # the warm-up runs advanced the cursor
    for f in range(4):
        got = _flat(step())
        for k, want in host[f].items():
            _same(got[k], want, "replay %d: %s" % (f, k))
    assert seq.cursor.cpu().tolist() == [4]
    seq.seek(1)
    got = _flat(step())
    for k, want in host[1].items():
        _same(got[k], want, "after seek(1): %s" % k)


def _run(args, timeout):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_eval_sort_on_a_lidar_sequence_with_oracle_detections_equals_the_host():
    out = _run([os.path.join(ROOT, "tools", "track", "eval_sort.py"), "--source", "lidar", "--detections", "truth",
                "--num_agent", "2", "--frames", "12"], 300)
    lines = out.splitlines()
    assert "note: untrained weights" not in out
    for family in ("MOTA", "IDF1", "HOTA"):
        assert sum(1 for ln in lines if ln.startswith("overall: " + family)) == 1, out
    _, _, steps = SC.generated(2, 12, 0)
    figures, want = SC.host_mot(steps)
    assert figures["overall"]["IDSW"] == 0 and figures["overall"]["FP"] == 0 and figures["overall"]["TP"] > 0
    got = [ln for ln in lines if " MOTA " in ln]
    assert got == want, "\n".join(got + want)


def test_eval_sort_on_a_lidar_sequence_runs_the_network():
    out = _run([os.path.join(ROOT, "tools", "track", "eval_sort.py"), "--source", "lidar", "--num_agent", "2", "--frames", "3"],
               300)
    assert "note: untrained weights" in out and "overall: MOTA" in out and "overall: HOTA" in out, out


def test_train_codet_on_lidar_sequences_writes_a_checkpoint(tmp_path):
    logs = str(tmp_path / "logs")
    out = _run([os.path.join(ROOT, "tools", "det", "train_codet.py"), "--scene", "lidar", "--sequence_frames", "4", "--targets",
                "boxes", "--num_agent", "2", "--batch", "1", "--nepoch", "1", "--steps_per_epoch", "2", "--logpath", logs], 300)
    line = [ln for ln in out.splitlines() if ln.startswith("epoch 1: mean loss")]
    assert len(line) == 1 and np.isfinite(float(line[0].split()[4])), out
    assert os.path.getsize(os.path.join(logs, "epoch_1.pth")) > 0


def test_sort_codet_on_a_lidar_sequence_writes_the_tracks_of_oracle_detections(tmp_path):
    logs = str(tmp_path / "tracks")
    out = _run([os.path.join(ROOT, "tools", "track", "sort_codet.py"), "--source", "lidar", "--detections", "truth",
                "--num_agent", "2", "--frames", "5", "--logpath", logs], 300)
    assert "note: untrained weights" not in out and "wrote tracks_agent0.txt, tracks_agent1.txt" in out, out
    from disconet_amd import tracking
    _, _, steps = SC.generated(2, 5, 0)
    sort = tracking.HostSort(max_age=1, min_hits=3, iou_threshold=0.3, scale=4.0, max_tracks=128)
    want = []
    for st in steps:                                                            # the same frames through the host tracker
        gt = st["gt"]
        want.append(sort.update({"boxes": gt["boxes"], "scores": np.ones(gt["ids"].shape, dtype=np.float32),
                                 "count": gt["count"]})["count"].tolist())
    assert sum(sum(c) for c in want) > 0
    reported = [ln for ln in out.splitlines() if ln.startswith("frame ")]
    assert reported == ["frame %d: tracks reported per image %s" % (f + 1, c) for f, c in enumerate(want)], out
    for a in range(2):
        rows = [ln.split(",") for ln in open(os.path.join(logs, "tracks_agent%d.txt" % a)).read().splitlines()]
        assert all(len(r) == 10 for r in rows)
        assert [sum(1 for r in rows if int(r[0]) == f + 1) for f in range(5)] == [c[a] for c in want]
