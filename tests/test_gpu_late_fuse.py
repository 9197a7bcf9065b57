"""`--com late` and `--com lowerbound` on the GPU: postprocess.late_fuse (dn_late_fuse, csrc/detect.hip) against the
contract in numpy, postprocess.host_late_fuse -- the bytes of boxes, scores, source and count, padding included -- its
launch behaviour (refusals, two runs, a captured step with detect(), MeanAP and Sort), the NoFusion model and one training
step against the no-fusion twin of tests/late_cases.py, and the tools end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cases
from tests import late_cases as lc

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # the project's parity bar, as tests/test_gpu_fuse_reduce.py :: test_models_vs_twin takes it


def _dev():
    return torch.device("cuda:0")


def _both(det, trans, live, B, A, **kw):
    """(late_fuse's tensors, host_late_fuse's arrays) of one case, and the assertion that their bytes agree"""
    from disconet_amd.postprocess import host_late_fuse, late_fuse
    dev = _dev()
    got = late_fuse(lc.to_device(det, dev), trans.to(dev), torch.tensor(live, dtype=torch.int32, device=dev), B, A, **kw)
    want = host_late_fuse(det, trans, live, B, A, **kw)
    torch.cuda.synchronize()
    bad = lc.same_bytes(got, want)
    assert not bad, (bad, kw, got["count"].tolist(), want["count"].tolist())
    return got, want


# ---------------------------------------------------------------------------
# a. the device equals the contract, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k_in", [1, 5, 64, 300])
@pytest.mark.parametrize("A,B,live,only_v2i", lc.CONFIGS)
def test_random_rows_equal_the_host(A, B, live, only_v2i, k_in):
    """unsorted rows with many overlaps, ragged counts, with and without the extent filter, the default threshold, one
    that suppresses whatever touches (0) and one that suppresses nothing (2); top_k at its default (k_in: below the
    candidate count wherever two agents are listed) and at 1"""
    trans = lc.trans_of(A, B)
    det = lc.random_rows(A, B, k_in, seed=A * 1000 + B * 100 + k_in)
    n_in = n_out = 0
    for iou_thr, ext in ((0.01, lc.EXTENTS), (0.0, None), (2.0, lc.EXTENTS)):
        got, want = _both(det, trans, live, B, A, iou_thr=iou_thr, extents=ext, only_v2i=only_v2i)
        n_in += int(want["count"].sum())
        n_out += want["count"].size * k_in - int(want["count"].sum())
    assert n_in > 0 and (k_in < 64 or n_out > 0)               # rows were kept, and (from 64 rows on) rows were suppressed
    _both(det, trans, live, B, A, top_k=1, extents=lc.EXTENTS, only_v2i=only_v2i)
    if k_in == 64:                                              # a top_k above k_in: every candidate of the list fits
        got, want = _both(det, trans, live, B, A, top_k=min(1024, A * k_in), iou_thr=2.0, only_v2i=only_v2i)
        assert int(want["count"].max()) > k_in


def test_copies_score_edges_extent_edges_and_ego_ranges():
    A, B = 4, 2
    trans = lc.trans_of(A, B)
    # every agent's copy of six objects: one threshold suppresses every copy, one none
    det = lc.copies(A, B, 6, 8, seed=4, trans=trans)
    got, want = _both(det, trans, [4, 4], B, A, top_k=32)
    assert want["count"].tolist() == [6] * (A * B)
    got, want = _both(det, trans, [4, 4], B, A, top_k=32, iou_thr=2.0)
    assert want["count"].tolist() == [24] * (A * B)
    _both(det, trans, [4, 3], B, A, top_k=5, only_v2i=True)
    # NaN, -0, negative, +-inf, equal scores across agents and within one, counts below 0 and above k_in
    det = lc.plant_score_edges(lc.random_rows(A, B, 12, seed=5), B)
    for live in ([4, 3], [0, 9]):
        for kw in (dict(top_k=48, iou_thr=2.0), dict(top_k=48, iou_thr=2.0, extents=lc.EXTENTS), dict(top_k=7), dict()):
            _both(det, trans, live, B, A, **kw)
            _both(det, trans, live, B, A, only_v2i=True, **kw)
    # rows a few ulps on either side of an extent edge
    det, rows = lc.plant_extent_edge(lc.random_rows(A, B, 40, seed=6, counts="full"), trans, B, ego=1, nbr=2)
    got, want = _both(det, trans, [4, 4], B, A, top_k=160, iou_thr=2.0, extents=lc.EXTENTS)
    kept = set(want["source"][1 * B + 0].tolist())
    assert 0 < sum(2 * 40 + r in kept for r in rows) < len(rows)
    # an ego range is the slice of the full result
    full, _ = _both(det, trans, [4, 3], B, A, extents=lc.EXTENTS)
    part, _ = _both(det, trans, [4, 3], B, A, extents=lc.EXTENTS, ego_first=1, ego_count=2)
    for key in lc.KEYS:
        assert torch.equal(part[key], full[key][B:3 * B]), key
    # an empty agent, all agents empty
    det = lc.random_rows(A, B, 5, seed=8)
    det["count"][1 * B + 0] = 0
    _both(det, trans, [4, 4], B, A)
    got, want = _both(dict(det, count=np.zeros(A * B, dtype=np.int32)), trans, [4, 4], B, A)
    assert not want["count"].any() and bool((got["source"] == -1).all())
    # one agent
    _both(lc.random_rows(1, 3, 7, seed=2), lc.trans_of(1, 3), [1, 0, 4], 3, 1, iou_thr=0.0)


def test_the_limit_eight_agents_of_1024_rows():
    """agents * k_in = 8192 rows in every list (64 KB of sort words), top_k = 1024"""
    A, B, k_in = 8, 1, 1024
    trans = lc.trans_of(A, B)
    det = lc.random_rows(A, B, k_in, seed=81, counts="full")
    got, want = _both(det, trans, [8], B, A, top_k=1024, extents=lc.EXTENTS)
    assert int(want["count"].min()) > 100 and len(set((want["source"][0, :int(want["count"][0])] // k_in).tolist())) == A


# ---------------------------------------------------------------------------
# b. launch behaviour
# ---------------------------------------------------------------------------
def test_refusals_raise_before_any_launch():
    from disconet_amd._lib import DnError
    from disconet_amd.postprocess import late_fuse
    dev = _dev()
    A, B, k = 4, 2, 8
    det = lc.to_device(lc.random_rows(A, B, k, seed=1), dev)
    trans = lc.trans_of(A, B).to(dev)
    na = torch.tensor([4, 3], dtype=torch.int32, device=dev)
    for kw, word in ((dict(top_k=0), "top_k"), (dict(top_k=1025), "top_k"), (dict(iou_thr=float("nan")), "iou_thr"),
                     (dict(iou_thr=-1.0), "iou_thr"), (dict(ego_first=3, ego_count=2), "ego range"),
                     (dict(ego_count=0), "ego range"), (dict(extents=((32.0, -32.0), (-32.0, 32.0))), "extents")):
        with pytest.raises(DnError, match=word):
            late_fuse(det, trans, na, B, A, **kw)
    wide = lc.to_device(lc.random_rows(16, 1, 600, seed=1), dev)
    with pytest.raises(DnError, match="at most 8192"):
        late_fuse(wide, lc.trans_of(16, 1).to(dev), torch.tensor([16], dtype=torch.int32, device=dev), 1, 16)
    with pytest.raises(ValueError, match="images"):
        late_fuse(det, trans, na, B, A + 1)
    with pytest.raises(ValueError, match="trans_matrices"):
        late_fuse(det, trans[:1], na, B, A)
    with pytest.raises(DnError, match="device tensors"):
        late_fuse({key: v.cpu().numpy() for key, v in det.items()}, trans, na, B, A)
    torch.cuda.synchronize()                   # nothing was launched: nothing can have failed


def test_two_runs_and_another_stream_give_the_same_bits():
    from disconet_amd.postprocess import late_fuse
    dev = _dev()
    A, B, k = 5, 2, 64
    det = lc.to_device(lc.random_rows(A, B, k, seed=3), dev)
    trans = lc.trans_of(A, B).to(dev)
    na = torch.tensor([5, 2], dtype=torch.int32, device=dev)
    first = late_fuse(det, trans, na, B, A, extents=lc.EXTENTS)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = late_fuse(det, trans, na, B, A, extents=lc.EXTENTS)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(5):
        again = late_fuse(det, trans, na, B, A, extents=lc.EXTENTS)
        for key in lc.KEYS:
            assert torch.equal(first[key].view(torch.int32), again[key].view(torch.int32)), key
            assert torch.equal(first[key].view(torch.int32), other[key].view(torch.int32)), key


def test_a_captured_step_replays_the_eager_bits():
    """detect() + late_fuse() + MeanAP.update() + Sort.update() as one captured graph, on the heads' outputs of a model case"""
    from disconet_amd import Config, build_model, graph, postprocess as P, tracking
    from disconet_amd.synthetic import make_gt_boxes, randomize_bn_stats
    case = "ragged_a4"
    c = cases.MODEL_CASES[case]
    A, B = c["agents"], c["batch"]
    cfg = Config(map_hw=c["map_hw"])
    torch.manual_seed(0)
    m = build_model("late", cfg, kd_flag=0, num_agent=A)
    randomize_bn_stats(m)
    m.eval().cuda()
    anchors = P.make_anchors(cfg)
    bevs, trans, na = (t.cuda() for t in cases.model_inputs(case))
    na32 = na[:, 0].int().contiguous()
    with torch.no_grad():
        result = m(bevs, trans, na32, B)
    gt_boxes, gt_count = (t.cuda() for t in make_gt_boxes(A * B, seed=0, max_boxes=16))
    metric = P.MeanAP(B, capacity=1 << 14)
    sort = tracking.Sort(max_tracks=64)

    def step():
        det = P.detect(result, anchors, pre_nms_top_k=64)
        fused = P.late_fuse(det, trans, na32, B, A, extents=cfg.area_extents[:2])
        match = metric.update(fused, gt_boxes, gt_count)
        tracks = sort.update(fused)
        return dict(fused, rank=match["rank"], track_count=tracks["count"], det_track=tracks["det_track"])

    eager = {k: v.clone() for k, v in step().items()}
    torch.cuda.synchronize()
    det = P.detect(result, anchors, pre_nms_top_k=64)
    want = P.host_late_fuse(det, trans, na32, B, A, extents=cfg.area_extents[:2])
    assert not lc.same_bytes(eager, want) and int(want["count"].sum()) > 0
    ego0 = want["source"][0, :int(want["count"][0])] // 64                               # ego 0 of scene 0: three live agents
    assert (ego0 == 0).any() and (ego0 != 0).any()                                       # the neighbours' boxes arrived
    sort.reset()
    metric.reset()
    g = graph.GraphedStep(step)
    sort.reset()                                # the warm-up runs of the capture advanced the tracker
    metric.reset()
    rep = g()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(rep[k], eager[k]), k
    g.drain()
    sort.status()
    assert metric.compute()["n_det"] == int(want["count"].sum())


# ---------------------------------------------------------------------------
# c. NoFusion against its twin
# ---------------------------------------------------------------------------
_REF = {}


def _ref_outputs(case):
    if case not in _REF:
        c = cases.MODEL_CASES[case]
        ref = lc.build_nofusion_ref(c["map_hw"], c["agents"], kd_flag=1)
        bevs, trans, na = cases.model_inputs(case)
        with torch.no_grad():
            res, x8, x7, x6, x5, fused = ref(bevs, trans, na, c["batch"])
        _REF[case] = (ref, {"cls": res["cls"], "loc": res["loc"], "x8": x8, "x5": x5, "fused": fused})
    return _REF[case]


@pytest.mark.parametrize("math", ["f32", "f16x3", "sp"])
@pytest.mark.parametrize("case", ["cfg1_f1", "ragged_a4"])
def test_nofusion_vs_twin(case, math):
    """within the project's parity bar of the twin (the oracle, not the code under test), and the same bytes when the
    poses are replaced by another jitter and the live counts by others: nothing of the fusion is read"""
    from disconet_amd import Config, NoFusion, build_model
    from disconet_amd.synthetic import make_trans_matrices
    c = cases.MODEL_CASES[case]
    ref, want = _ref_outputs(case)
    m = build_model("lowerbound", Config(map_hw=c["map_hw"]), kd_flag=1, num_agent=c["agents"]).eval()
    m.conv_math = math
    m.load_state_dict({"module." + k: v for k, v in ref.state_dict().items()})
    m = m.cuda()
    assert type(m) is NoFusion
    bevs, trans, na = cases.model_inputs(case)
    with torch.no_grad():
        res, x8, x7, x6, x5, fused = m(bevs.cuda(), trans.cuda(), na.cuda(), c["batch"])
        other = make_trans_matrices(c["batch"], c["agents"], jitter_seed=12345).cuda()
        res2, x8b, _, _, x5b, fused2 = m(bevs.cuda(), other, torch.ones_like(na).cuda(), c["batch"])
    torch.cuda.synchronize()
    assert not torch.equal(other.cpu(), trans)
    got = {"cls": res["cls"].cpu(), "loc": res["loc"].cpu(), "x8": x8.cpu(), "x5": x5.cpu(), "fused": fused.cpu()}
    again = {"cls": res2["cls"].cpu(), "loc": res2["loc"].cpu(), "x8": x8b.cpu(), "x5": x5b.cpu(), "fused": fused2.cpu()}
    for name in want:
        assert got[name].shape == want[name].shape, name
        err = (got[name] - want[name]).abs().max().item()
        assert err <= TOL, "lowerbound/%s/%s %s max abs err %.3e" % (case, math, name, err)
        assert torch.equal(got[name], again[name]), name


@pytest.mark.parametrize("case", ["cfg1", "ragged_a4"])
def test_one_training_step_vs_twin(case, monkeypatch):
    """as tests/test_gpu_fuse_reduce.py :: test_one_training_step_vs_twin: losses within 2e-5 relative of the twin's fp32
    step, every gradient under the acceptance rule of tests/test_gpu_train_step.py :: _assert_grads, unchanged, against
    the twin's float64 autograd"""
    from disconet_amd import CoDetModule, Config, build_model
    from oracle.train_ref import train_step
    from tests.test_gpu_train_step import _assert_grads, _fp64_grads, _grad_report
    c = cases.TRAIN_CASES[case]
    (bevs, trans, na), (labels, targets, mask) = cases.train_inputs(case)
    ref = lc.build_nofusion_ref(c["map_hw"], c["agents"], kd_flag=0)
    model = build_model("lowerbound", Config(map_hw=c["map_hw"]), kd_flag=0, num_agent=c["agents"])
    model.load_state_dict(ref.state_dict())
    model = model.cuda()
    g64 = _fp64_grads(ref, (bevs, trans, na), (labels, targets, mask), c["batch"], monkeypatch)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    l_ref = train_step(ref, opt, bevs, trans, na, c["batch"], labels, targets, mask)
    mod = CoDetModule(model, lr=1e-3)
    assert type(mod.engine).__name__ == "NoFusionTrainEngine"
    data = {"bev_seq": bevs.cuda(), "trans_matrices": trans.cuda(), "num_agent": na.cuda(),
            "labels": labels.cuda(), "reg_targets": targets.cuda(), "reg_loss_mask": mask.cuda()}
    out = mod.step(data, c["batch"])
    print("\nlowerbound %s: losses %s, twin %s" % (case, out, l_ref))
    assert mod.engine.F["n_warps"] == 0
    assert abs(out["cls_loss"] - l_ref[0]) < 2e-5 * abs(l_ref[0]), (out, l_ref)
    assert abs(out["loc_loss"] - l_ref[1]) < 2e-5 * abs(l_ref[1]), (out, l_ref)
    _assert_grads(_grad_report(g64, ref, mod.engine, model))


def test_training_refuses_distillation_and_an_agent_shard():
    from disconet_amd import CoDetModule, Config, TeacherNet, build_model
    from disconet_amd.sharded import AgentShard
    model = build_model("lowerbound", Config(map_hw=128), kd_flag=0, num_agent=2).cuda()
    with pytest.raises(ValueError, match="DiscoGraph"):
        CoDetModule(model, teacher=TeacherNet(Config(map_hw=128)).cuda(), kd_flag=1)
    shard = AgentShard.__new__(AgentShard)      # (never used: the engine refuses before it looks at it)
    with pytest.raises(NotImplementedError):
        CoDetModule(model, shard=shard)


# ---------------------------------------------------------------------------
# d. the tools
# ---------------------------------------------------------------------------
def _run(args, timeout):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable] + args, cwd=root, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_tools_train_lowerbound_then_evaluate_and_track_late(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    logs = str(tmp_path / "logs")
    out = _run([os.path.join(root, "tools", "det", "train_codet.py"), "--com", "lowerbound", "--targets", "boxes",
                "--num_agent", "2", "--batch", "1", "--nepoch", "1", "--steps_per_epoch", "2", "--logpath", logs], 300)
    assert "epoch 1:" in out
    ck = os.path.join(logs, "epoch_1.pth")
    state = torch.load(ck, map_location="cpu", weights_only=False)
    assert not any(k.startswith("pixel_weighted_fusion") for k in state["model_state_dict"])
    for com in ("lowerbound", "late"):
        out = _run([os.path.join(root, "tools", "det", "eval_codet.py"), "--com", com, "--gt", "scene", "--num_agent", "2",
                    "--resume", ck], 300)
        assert "overall: mAP@0.5" in out, out
    tracks = str(tmp_path / "tracks")
    # (a detector of two steps reports a hundred boxes per frame: 32 rows keep the tracker's 128 slots from running out)
    out = _run([os.path.join(root, "tools", "track", "sort_codet.py"), "--com", "late", "--num_agent", "2", "--frames", "3",
                "--pre_nms_top_k", "32", "--resume", ck, "--logpath", tracks], 300)
    assert sorted(os.listdir(tracks)) == ["tracks_agent0.txt", "tracks_agent1.txt"], out
