"""dn_assign_targets / targets.assign_targets on the MI355X against the numpy reference targets.host_assign_targets:
labels, masks and matched rows exactly, best IoU to 1e-11 (the bar of tests/test_gpu_ap.py: the same fp64 geometry, whose
only freedom is the last bits of hypot and of fused-versus-separate products inside libm), every target element within
one fp32 ulp (a last-bit fp64 difference in hypot or log can move the single rounding to fp32 by one ulp at most); then the
round trip through the detection tail, a real training step, and a training run that moves mAP."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import assign_cases as C
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

IOU_TOL = 1e-11


def _device(anchors, gb, gc, pos=C.POS, neg=C.NEG, force=True):
    from disconet_amd import targets as T
    out = T.assign_targets(torch.as_tensor(anchors).cuda(), torch.as_tensor(gb).cuda(), torch.as_tensor(gc).cuda(), pos, neg,
                           force_match=force, want_match=True)
    h, w, a = anchors.shape[:3]
    n = len(gc)
    assert tuple(out["labels"].shape) == (n, h * w * a, 2) and out["labels"].dtype == torch.float32
    assert tuple(out["reg_targets"].shape) == (n, h, w, a, 1, 6) and out["reg_targets"].dtype == torch.float32
    assert tuple(out["reg_loss_mask"].shape) == (n, h, w, a, 1) and out["reg_loss_mask"].dtype == torch.float32
    assert out["matched_gt"].dtype == torch.int32 and out["best_iou"].dtype == torch.float64
    return out


def _np(out):
    n = out["labels"].shape[0]
    return {"labels": out["labels"].cpu().numpy(), "reg_targets": out["reg_targets"].reshape(n, -1, 6).cpu().numpy(),
            "reg_loss_mask": out["reg_loss_mask"].reshape(n, -1).cpu().numpy(), "matched_gt": out["matched_gt"].cpu().numpy(),
            "best_iou": out["best_iou"].cpu().numpy()}


def _compare(dev, host, what):
    assert np.array_equal(dev["labels"], host["labels"]), what
    assert np.array_equal(dev["reg_loss_mask"], host["reg_loss_mask"]), what
    assert np.array_equal(dev["matched_gt"], host["matched_gt"]), what
    d_iou = float(np.abs(dev["best_iou"] - host["best_iou"]).max())
    a, b = dev["reg_targets"], host["reg_targets"]
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    worst = float((np.abs(a.astype(np.float64) - b) / ulp).max())
    differ = int((a != b).sum())
    print("%s: %d positives, %d don't care; largest |best IoU - host| %.3g; %d of %d target elements differ, by at most "
          "%.3g ulp" % (what, int(host["reg_loss_mask"].sum()), int((host["labels"].sum(-1) == 0).sum()), d_iou, differ,
                        a.size, worst))
    assert d_iou <= IOU_TOL, what
    assert worst <= 1.0, what


@pytest.mark.parametrize("name", ["CROWD_64", "CROWD_128", "GRID_256"])
def test_device_equals_host_reference(name):
    from disconet_amd import targets as T
    hw, counts, seed = getattr(C, name)
    anchors, gb, gc = C.crowd(hw, counts, seed)
    pairs = C.pairs_of(anchors, gb, gc)
    C.assert_margins(pairs, anchors.reshape(-1, 6).shape[0], "%s seed %d" % (name, seed))     # a condition: nothing is filtered
    garbage = C.crowd(hw, counts, seed, garbage=True)[1]
    wide = np.concatenate([garbage, np.full((len(gc), 3, 6), np.nan, np.float32)], 1)          # padding rows full of garbage
    for force in (True, False):
        host = T.host_assign_targets(anchors, gb, gc, C.POS, C.NEG, force_match=force, pairs=pairs)
        if force:
            assert (host["reg_loss_mask"].sum(1)[gc > 0] >= gc[gc > 0]).all()            # every touched box has its anchor
        dev = _np(_device(anchors, gb, gc, force=force))
        _compare(dev, host, "%s force %d" % (name, force))
        assert not dev["labels"][gc == 0, :, 1].any() and (dev["labels"][gc == 0, :, 0] == 1).all()
        padded = _np(_device(anchors, wide, gc, force=force))
        for k in dev:
            assert np.array_equal(dev[k], padded[k]), (name, k)


@pytest.mark.parametrize("force", [False, True])
def test_crafted_exact_cases(force):
    anchors, gb, gc, exp = C.crafted()
    dev = _np(_device(anchors, gb, gc, force=force))
    C.check_crafted(dev, exp[force], gb)


def _lattice_1024():
    """1024 ground-truth rows, each on its own anchor of a 32 x 32 lattice of 2 x 4 anchors at pitch 8 m, shifted by 0,
    1/4, 1/2 or 1 m: IoU exactly 1, 7/9, 3/5, 1/3 -- dyadic geometry, a crafted case (no margins: 3/5 is pos_thr itself)."""
    r = np.random.default_rng(0)
    xs = (np.arange(32) - 15.5) * 8.0
    anchors = np.zeros((32, 32, 1, 6), np.float32)
    anchors[..., 0], anchors[..., 1] = xs[:, None, None], xs[None, :, None]
    anchors[..., 2], anchors[..., 3], anchors[..., 5] = 2.0, 4.0, 1.0
    perm = r.permutation(1024)
    shift = np.asarray([0.0, 0.25, 0.5, 1.0])[r.integers(0, 4, 1024)]
    gb = anchors.reshape(1024, 6)[perm][None].copy()
    gb[0, :, 0] += shift
    iou = {0.0: 1.0, 0.25: 7 / 9, 0.5: 3 / 5, 1.0: 1 / 3}
    return anchors, gb, np.asarray([1024], np.int32), perm, np.asarray([iou[s] for s in shift.tolist()])


def test_limits_g_1024_g_1_and_a_single_image():
    from disconet_amd import targets as T
    anchors, gb, gc, perm, iou = _lattice_1024()
    for force in (True, False):
        host = T.host_assign_targets(anchors, gb, gc, C.POS, C.NEG, force_match=force)
        dev = _np(_device(anchors, gb, gc, force=force))
        _compare(dev, host, "1024 rows force %d" % force)
        assert np.array_equal(dev["best_iou"][0, perm], iou)
        want = np.where((iou >= C.POS) | force, np.arange(1024), -1)
        assert np.array_equal(dev["matched_gt"][0, perm], want)
        assert int((dev["labels"][0].sum(-1) == 0).sum()) == 0              # 1/3 is negative, the rest at or above pos_thr
    # G = 1: one box on one image of the 64 x 64 map
    anchors, gb, gc = C.crowd(64, (1,), 11)
    pairs = C.pairs_of(anchors, gb, gc)
    C.assert_margins(pairs, anchors.reshape(-1, 6).shape[0], "one box")
    host = T.host_assign_targets(anchors, gb, gc, pairs=pairs)
    dev = _np(_device(anchors, gb, gc))
    _compare(dev, host, "one box")
    assert dev["reg_loss_mask"].sum() >= 1


def test_wrong_shapes_are_refused_with_the_shapes_in_the_message():
    from disconet_amd import targets as T
    anchors, gb, gc = C.crowd(64, (1,), 11)
    a, b, c = torch.as_tensor(anchors).cuda(), torch.as_tensor(gb).cuda(), torch.as_tensor(gc).cuda()
    for bad in (b[0], b[0, 0], b[..., :5], b.repeat(2, 1, 1)):
        with pytest.raises(ValueError, match="gt_boxes"):
            T.assign_targets(a, bad, c)
    with pytest.raises(ValueError, match="anchors"):
        T.assign_targets(a.reshape(-1, 6), b, c)


def test_two_runs_and_a_graph_replay_write_the_same_bytes():
    from disconet_amd import targets as T
    hw, counts, seed = C.CROWD_128
    anchors, gb, gc = C.crowd(hw, counts, seed)
    a, b, c = torch.as_tensor(anchors).cuda(), torch.as_tensor(gb).cuda(), torch.as_tensor(gc).cuda()
    run = lambda: T.assign_targets(a, b, c, want_match=True)                          # noqa: E731
    first, second = run(), run()
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
        captured = run()
    for k in captured:
        captured[k].view(torch.uint8).fill_(0xCD)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(first[k].view(torch.uint8), captured[k].view(torch.uint8)), k


# ---- round trip through the shipped detection tail ---------------------------------------------------------------------
def _roundtrip_ap(scene, anchors, **kw):
    from disconet_amd import postprocess as P, targets as T
    t = T.assign_targets(anchors, scene["gt_boxes"], scene["gt_count"], **kw)
    n = scene["gt_boxes"].shape[0]
    pos = t["reg_loss_mask"].reshape(n, -1)
    fg = torch.where(pos > 0, 8.0, -8.0)
    result = {"cls": torch.stack([torch.zeros_like(fg), fg], -1).contiguous(), "loc": t["reg_targets"]}
    det = P.detect(result, anchors, pre_nms_top_k=300, iou_thr=0.01)
    metric = P.MeanAP(batch_size=1)
    metric.update(det, scene["gt_boxes"], scene["gt_count"])
    return metric.compute(), int(pos.sum())


def test_round_trip_through_detect_and_mean_ap():
    from disconet_amd import Config, postprocess as P
    from disconet_amd.synthetic import make_box_scene_batch
    scene = make_box_scene_batch(1, 2, 128, seed=1, boxes_per_scene=16, device="cuda")      # centres >= 6 m apart: IoU 0
    anchors = P.make_anchors(Config(map_hw=128))
    res, n_pos = _roundtrip_ap(scene, anchors, pos_thr=0.6, neg_thr=0.45, force_match=True)
    print("force match: %d positives for %d boxes, AP %r / %r" % (n_pos, res["n_gt"], res["mAP@0.5"], res["mAP@0.7"]))
    assert n_pos >= res["n_gt"] > 0
    assert res["mAP@0.5"] == 1.0 and res["mAP@0.7"] == 1.0
    res, n_pos = _roundtrip_ap(scene, anchors, pos_thr=0.95, neg_thr=0.45, force_match=False)
    print("no force match at pos_thr 0.95: %d positives, AP %r / %r" % (n_pos, res["mAP@0.5"], res["mAP@0.7"]))
    assert n_pos == 0
    assert res["mAP@0.5"] == 0.0 and res["mAP@0.7"] == 0.0


def test_box_scene_on_the_gpu_equals_the_host_form():
    from disconet_amd.synthetic import make_box_scene_batch
    dev = make_box_scene_batch(1, 2, 128, seed=2, boxes_per_scene=16, device="cuda")
    host = make_box_scene_batch(1, 2, 128, seed=2, boxes_per_scene=16)
    for k in ("bev_seq", "trans_matrices", "num_agent", "gt_boxes", "gt_count"):
        assert dev[k].is_cuda and torch.equal(dev[k].cpu(), host[k]), k


# ---- one real step ------------------------------------------------------------------------------------------------------
def _module(lr=1e-3):
    from disconet_amd import CoDetModule, Config, DiscoNet
    from tests import assign_train_case as TC
    cfg = Config(map_hw=TC.HW)
    model = DiscoNet(cfg, kd_flag=0, num_agent=TC.AGENTS)
    model.load_state_dict(TC.ref_model().state_dict())
    model = model.cuda()
    return cfg, model, CoDetModule(model, None, cfg, None, kd_flag=0, lr=lr)


def test_one_training_step_on_assigned_targets():
    """TRAIN_CASES["cfg1"]'s size (128 x 128, 2 agents, batch 1): the step reads the tensors assign_targets returns as they
    are; the same targets after a round trip through the host give the same losses, to the 1e-12 relative bar of
    tests/test_gpu_train_step.py (the loss scalars are sums by f64 atomics: their last bits are not repeatable run to run),
    and hand the step the same bytes."""
    from disconet_amd import postprocess as P, targets as T
    from tests import assign_train_case as TC
    from tests.cases import TRAIN_CASES
    assert (TC.HW, TC.AGENTS, TC.BATCH) == tuple(TRAIN_CASES["cfg1"][k] for k in ("map_hw", "agents", "batch"))
    cfg, model, module = _module()
    scene = TC.scene(device="cuda")
    t = T.assign_targets(P.make_anchors(cfg), scene["gt_boxes"], scene["gt_count"])
    data = {k: scene[k] for k in ("bev_seq", "trans_matrices", "num_agent")}
    direct = module.step(dict(data, **t), TC.BATCH, update=False)
    hosted = {k: v.cpu().clone() for k, v in t.items()}
    through_host = module.step(dict(data, **hosted), TC.BATCH, update=False)
    print("losses", direct, "through the host", through_host)
    assert all(np.isfinite(v) for v in direct.values()) and direct["loc_loss"] > 0 and direct["cls_loss"] > 0
    for k in ("loss", "cls_loss", "loc_loss"):
        assert abs(direct[k] - through_host[k]) <= 1e-12 * abs(direct[k]), k
    for k, v in t.items():           # what the step reads after the round trip is what assign_targets wrote
        assert torch.equal(hosted[k].cuda().view(torch.int32), v.view(torch.int32)), k
    for k, v in t.items():           # the step's own conversion of these tensors is a view: nothing is copied
        assert v.to(device=v.device, dtype=torch.float32).contiguous().data_ptr() == v.data_ptr(), k


# ---- training moves the metric ------------------------------------------------------------------------------------------
# the float64 oracle twin on the same scene, targets, initial weights, learning rate and step count (python -m
# tests.assign_train_case, 268 s on the CPU): AP@0.5 0.0000 untrained, 0.4173 trained; AP@0.7 0.3517 trained
ORACLE_AP50 = 0.4173


def _model_ap(model, scene, anchors, batch):
    from disconet_amd import postprocess as P
    from tests import assign_train_case as TC
    model.eval()
    with torch.no_grad():
        out = model(scene["bev_seq"], scene["trans_matrices"], scene["num_agent"], batch)
    det = P.detect(out[0] if isinstance(out, tuple) else out, anchors, pre_nms_top_k=TC.TOP_K, iou_thr=TC.NMS_IOU)
    metric = P.MeanAP(batch_size=batch)
    metric.update(det, scene["gt_boxes"], scene["gt_count"])
    return metric.compute()


def test_training_moves_the_metric():
    """A fixed 2-agent 128 x 128 box scene (tests/assign_train_case.py: 16 world boxes, 28 ground-truth rows over the two
    images), 120 steps of CoDetModule.step at lr 1e-3 on the targets assign_targets returns, default nn init.
    The float64 oracle twin (oracle model, torch Adam, oracle/train_ref.py losses, host_assign_targets' targets; same
    seeds, step count and learning rate; run on the CPU): mean loss of the first five steps 16236.3, of the last five
    336.3; AP@0.5 0.0000 untrained, 0.4173 trained (AP@0.7 0.3517).  The floor is half the oracle's AP@0.5, 0.2087: the
    split-f16 trajectory drifts a few percent from fp32 in loss and AP over 28 boxes moves in coarse steps, while a detector
    that learnt nothing scores 0.
    MI355X: not recorded here (the test prints the figures)."""
    from disconet_amd import postprocess as P, targets as T
    from tests import assign_train_case as TC
    cfg, model, module = _module(lr=TC.LR)
    scene = TC.scene(device="cuda")
    anchors = P.make_anchors(cfg)
    data = {k: scene[k] for k in ("bev_seq", "trans_matrices", "num_agent")}
    data.update(T.assign_targets(anchors, scene["gt_boxes"], scene["gt_count"]))
    before = _model_ap(model, scene, anchors, TC.BATCH)
    losses = [module.step(data, TC.BATCH)["loss"] for _ in range(TC.STEPS)]
    after = _model_ap(model, scene, anchors, TC.BATCH)
    first, last = float(np.mean(losses[:5])), float(np.mean(losses[-5:]))
    print("mean loss of the first five steps %.4f, of the last five %.4f; AP@0.5 untrained %.4f, trained %.4f (AP@0.7 %.4f); "
          "oracle float64 AP@0.5 %.4f, floor %.4f" % (first, last, before["mAP@0.5"], after["mAP@0.5"], after["mAP@0.7"],
                                                       ORACLE_AP50, 0.5 * ORACLE_AP50))
    assert all(np.isfinite(losses))
    assert last < first
    assert after["mAP@0.5"] > before["mAP@0.5"]
    assert after["mAP@0.5"] >= 0.5 * ORACLE_AP50


def test_cli_train_on_boxes_then_eval_on_the_scenes(tmp_path):
    train = os.path.join(ROOT, "tools", "det", "train_codet.py")
    r = subprocess.run([sys.executable, train, "--com", "disco", "--targets", "boxes", "--nepoch", "1", "--steps_per_epoch", "2",
                        "--num_agent", "2", "--batch", "1", "--logpath", str(tmp_path)], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "epoch 1: mean loss" in r.stdout and (tmp_path / "epoch_1.pth").exists()
    ev = os.path.join(ROOT, "tools", "det", "eval_codet.py")
    r = subprocess.run([sys.executable, ev, "--com", "disco", "--gt", "scene", "--resume", str(tmp_path / "epoch_1.pth"),
                        "--num_agent", "2"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout[-600:])
    import re
    m = re.search(r"overall: mAP@0\.5 ([0-9.]+)  mAP@0\.7 ([0-9.]+)", r.stdout)
    assert m and "the boxes of the scenes" in r.stdout, r.stdout
