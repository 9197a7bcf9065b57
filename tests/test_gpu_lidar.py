"""dn_lidar_scan on the device against lidar.host_scan, the numpy statement of the contract: equal in every byte -- the
points with their NaN rows compared as bytes, hit, solid_hits, gt_boxes, gt_count, gt_own_hits -- on the hand cases and
shapes of tests/lidar_cases.py, with and without range jitter; the scene generator on the device against its host form;
the scan, the views and the target assignment captured into one graph; the tools with --scene lidar."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lidar_cases as LC

pytestmark = pytest.mark.gpu

KEYS = ("points", "hit", "solid_hits", "gt_boxes", "gt_count", "gt_own_hits")


def _assert_same(dev, host, what):
    for k in KEYS:
        got = dev[k].cpu().numpy()
        assert got.shape == host[k].shape and got.dtype == host[k].dtype, (what, k, got.shape, got.dtype)
        if got.tobytes() != host[k].tobytes():
            bad = np.nonzero(got.view(np.uint8).reshape(-1) != host[k].view(np.uint8).reshape(-1))[0]
            raise AssertionError("%s: %s differs in %d bytes, the first at byte %d" % (what, k, len(bad), bad[0]))


@pytest.mark.parametrize("jitter", [False, True], ids=["plain", "jitter"])
@pytest.mark.parametrize("name", sorted(LC.cases()))
def test_device_equals_the_host_statement(name, jitter):
    from disconet_amd import lidar
    args, kw = LC.cases()[name]
    dev = lidar.scan(*args, range_jitter=LC.jitter_for(args) if jitter else None, **kw)
    assert dev["cloud"][0].shape == (args[3].shape[1] * args[0].shape[0] * args[5].shape[0], 4)
    assert dev["cloud"][1].tolist() == [i * args[5].shape[0] for i in range(dev["points"].shape[0] + 1)]
    _assert_same(dev, LC.host(name, jitter), name)


def test_one_solid_too_many_is_refused():
    from disconet_amd import _lib, lidar
    args, kw = LC.make([[LC.box(10.0, 0.0)]], LC.FAN, k=lidar.MAX_SOLIDS + 1)
    with pytest.raises(_lib.DnError, match="K = 257 solids"):
        lidar.scan(*args, **kw)
    with pytest.raises(ValueError, match="object_count = 4 is more than the 3"):
        a, k = LC.cases()["compaction"]
        lidar.scan(*a, **dict(k, gt_rows=3))


def test_scene_on_the_device_equals_the_host_form():
    from disconet_amd.synthetic import make_lidar_scene_batch
    kw = dict(batch_size=1, num_agent=2, map_hw=64, seed=1, beams=8, azimuths=128, teacher=True)
    dev, host = make_lidar_scene_batch(device="cuda", **kw), make_lidar_scene_batch(**kw)
    keys = [k for k, v in host.items() if isinstance(v, torch.Tensor)]
    assert "bev_seq_teacher" in keys and len(keys) == 8
    for k in keys:
        assert dev[k].is_cuda and dev[k].dtype == host[k].dtype and dev[k].shape == host[k].shape, k
        assert dev[k].cpu().numpy().tobytes() == host[k].numpy().tobytes(), k
    for d, h in zip(dev["points"], host["points"]):
        assert d.cpu().numpy().tobytes() == h.tobytes()
    assert int(host["bev_seq"].sum()) > 0 and int(host["gt_count"].sum()) > 0


def test_scan_views_and_targets_replay_from_one_graph():
    from disconet_amd import Config, holistic, lidar, postprocess as P, targets as T
    from disconet_amd.synthetic import lidar_world_solids, make_trans_matrices
    cfg = Config(map_hw=64)
    half = float(cfg.area_extents[0][1])
    scenes = [lidar_world_solids(2, 64, seed, 0, 4, 0)[0] for seed in (1, 2, 3)]
    K = 4
    rows = np.zeros((3, 1, K, 8))
    for i, r in enumerate(scenes):
        rows[i, 0, :len(r)] = r
    counts = [torch.tensor([len(r)], dtype=torch.int32, device="cuda") for r in scenes]
    solids = torch.from_numpy(rows[0]).cuda()
    count = counts[0].clone()
    pose = torch.from_numpy(lidar.sensor_from_world(1, 2)).cuda()
    live = torch.tensor([2], dtype=torch.int32, device="cuda")
    dirs = torch.from_numpy(lidar.beam_table(8, 128)).cuda()
    trans = make_trans_matrices(1, 2).cuda()
    anchors = torch.as_tensor(P.make_anchors(cfg)).cuda()
    R = dirs.shape[0]
    ranges = holistic.source_ranges(np.arange(3) * R, [2], 2, 1, own=True)      # owned here, for as long as the graph lives

    def run():
        r = lidar.scan(solids, count, count, pose, live, dirs, half_extent=half, min_points=2, gt_rows=K)
        v = holistic.holistic_views(r["cloud"], trans, [2], 1, cfg, own=True, ranges=ranges)
        t = T.assign_targets(anchors, r["gt_boxes"], r["gt_count"])
        out = {k: r[k] for k in KEYS}
        out.update(bev_seq=v["own_dense"], bev_seq_teacher=v["dense"])
        out.update({"target_" + k: x for k, x in t.items()})
        return out

    def set_scene(i):
        solids.copy_(torch.from_numpy(rows[i]).cuda())
        count.copy_(counts[i])

    eager = []
    for i in range(3):
        set_scene(i)
        eager.append({k: v.clone() for k, v in run().items()})
    assert not torch.equal(eager[1]["bev_seq"], eager[2]["bev_seq"]) and int(eager[1]["gt_count"].sum()) > 0
    set_scene(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    holistic._SRC_CACHE.clear()          # the graph depends on no module cache: the index tensors it reads are `ranges`
    for i in (1, 2):
        set_scene(i)
        for v in captured.values():
            v.view(torch.uint8).fill_(0xCD)
        g.replay()
        torch.cuda.synchronize()
        for k, v in eager[i].items():
            assert torch.equal(v.view(torch.uint8), captured[k].view(torch.uint8)), (i, k)


def _run(args, timeout):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable] + args, cwd=root, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_tools_train_and_evaluate_on_lidar_scenes(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    logs = str(tmp_path / "logs")
    out = _run([os.path.join(root, "tools", "det", "train_codet.py"), "--scene", "lidar", "--targets", "boxes", "--num_agent", "2",
                "--batch", "1", "--nepoch", "1", "--steps_per_epoch", "2", "--logpath", logs], 300)
    line = [ln for ln in out.splitlines() if ln.startswith("epoch 1: mean loss")]
    assert len(line) == 1 and np.isfinite(float(line[0].split()[4])), out
    out = _run([os.path.join(root, "tools", "det", "eval_codet.py"), "--scene", "lidar", "--gt", "scene", "--num_agent", "2",
                "--resume", os.path.join(logs, "epoch_1.pth")], 300)
    assert "overall: mAP@0.5" in out, out
