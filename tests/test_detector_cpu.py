"""disconet_amd.Detector -- the detector of a `--com` mode with its tail -- and what the det / track command lines share
(tools/det/codet_common.py), on the CPU: the model class per mode, the call path of the tail (stand-ins for
postprocess.detect / late_fuse that record their arguments), the heads rule, the checkpoint round trip and the seeding
contract.  The small map keeps the constructions quick; nothing here runs a kernel."""
import argparse
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

HW, A, B = 32, 3, 2


def _config():
    from disconet_amd import Config
    return Config(map_hw=HW)


def _common():
    here = os.path.join(ROOT, "tools", "det")
    if here not in sys.path:
        sys.path.insert(0, here)
    import codet_common
    return codet_common


def test_detector_builds_the_class_of_the_mode_and_refuses_others():
    from disconet_amd import DET_COM_MODES, Detector, build_model
    cfg = _config()
    for com in DET_COM_MODES:
        det = Detector(com, cfg, A, B, device="cpu")
        assert type(det.model) is type(build_model(com, cfg, kd_flag=0, num_agent=A))
        assert not det.model.training and det.model.agent_num == A
        assert (det.com, det.config, det.num_agent, det.batch_size, det.epoch) == (com, cfg, A, B, None)
        assert det.anchors.device.type == "cpu" and det.anchors.shape[:2] == (HW, HW)
    with pytest.raises(ValueError, match=", ".join(DET_COM_MODES)):
        Detector("v2v", cfg, A, B, device="cpu")


@pytest.fixture
def recorded(monkeypatch):
    """stand-ins on the two calls of Detector.tail: they record their arguments and return a marker"""
    from disconet_amd import detector
    calls = {"detect": [], "late_fuse": []}

    def detect(*a, **kw):
        calls["detect"].append((a, kw))
        return "det marker"

    def late_fuse(*a, **kw):
        calls["late_fuse"].append((a, kw))
        return "fused marker"
    monkeypatch.setattr(detector.postprocess, "detect", detect)
    monkeypatch.setattr(detector.postprocess, "late_fuse", late_fuse)
    return calls


@pytest.mark.parametrize("only_v2i", [False, True])
def test_tail_reaches_late_fuse_for_late_only(recorded, only_v2i):
    from disconet_amd import DET_COM_MODES, Detector
    cfg = _config()
    result, trans, na = {"cls": "c", "loc": "l"}, object(), object()
    for com in DET_COM_MODES:
        det = Detector(com, cfg, A, B, only_v2i=only_v2i, pre_nms_top_k=64, iou_thr=0.05, score_thr=0.3, device="cpu")
        for calls in recorded.values():
            del calls[:]
        out = det.tail(result, trans, na)
        (args, kw), = recorded["detect"]                                       # always, with the three thresholds
        assert args[0] is result and args[1] is det.anchors and len(args) == 2
        assert kw == {"pre_nms_top_k": 64, "iou_thr": 0.05, "score_thr": 0.3}
        if com == "late":
            (args, kw), = recorded["late_fuse"]                                # exactly once
            assert args[0] == "det marker" and args[1] is trans and args[2] is na and args[3:] == (B, A)
            assert set(kw) == {"iou_thr", "only_v2i", "extents"}               # the other arguments at their defaults
            assert kw["iou_thr"] == 0.05 and kw["only_v2i"] is only_v2i
            assert np.array_equal(kw["extents"], cfg.area_extents[:2]) and np.shape(kw["extents"]) == (2, 2)
            assert out == "fused marker"
        else:
            assert recorded["late_fuse"] == [] and out == "det marker"


def test_detect_gets_the_default_thresholds(recorded):
    from disconet_amd import Detector
    Detector("disco", _config(), A, B, device="cpu").tail({}, None, None)
    assert recorded["detect"][0][1] == {"pre_nms_top_k": 300, "iou_thr": 0.01, "score_thr": None}


def test_forward_returns_the_dict_of_a_kd_tuple_and_call_is_tail_of_forward(recorded):
    from disconet_amd import Detector
    from disconet_amd.detector import heads
    det = Detector("late", _config(), A, B, device="cpu")
    result, seen = {"cls": "c", "loc": "l"}, []

    def model(bevs, trans, na, batch_size):
        seen.append((bevs, trans, na, batch_size, torch.is_grad_enabled()))
        return result, "x8", "x7", "x6", "x5", "fused"                         # a kd_flag forward
    det.model = model
    assert det.forward("bevs", "trans", "na") is result
    assert seen == [("bevs", "trans", "na", B, False)]
    det.model = lambda *a: result                                              # kd_flag 0: the dict itself
    assert det.forward("bevs", "trans", "na") is result
    assert heads((result, 1)) is result and heads(result) is result
    assert det("bevs", "trans", "na") == "fused marker"
    assert recorded["detect"][0][0][0] is result and recorded["late_fuse"][0][0][:3] == ("det marker", "trans", "na")


def test_load_checkpoint_round_trip_and_epoch(tmp_path):
    from disconet_amd import Detector, build_model, load_checkpoint
    cfg = _config()
    src = Detector("lowerbound", cfg, A, B, seed=3, device="cpu")
    path = str(tmp_path / "epoch_7.pth")
    torch.save({"epoch": 7, "model_state_dict": src.model.state_dict(), "loss": 0.5}, path)
    torch.manual_seed(11)
    model = build_model("lowerbound", cfg, kd_flag=0, num_agent=A)
    ck = load_checkpoint(model, path)
    assert ck["epoch"] == 7 and ck["loss"] == 0.5 and set(ck) == {"epoch", "model_state_dict", "loss"}
    want = src.model.state_dict()
    assert set(model.state_dict()) == set(want)
    for k, v in model.state_dict().items():
        assert torch.equal(v, want[k]), k
    late = Detector("late", cfg, A, B, resume=path, seed=5, device="cpu")       # the lowerbound checkpoint, as the tools pass it
    assert late.epoch == 7 and not late.model.training
    for k, v in late.model.state_dict().items():
        assert torch.equal(v, want[k]), k
    assert src.epoch is None


def test_same_seed_same_parameters():
    from disconet_amd import Detector
    cfg = _config()
    a, b, c = (Detector("disco", cfg, A, B, seed=s, device="cpu") for s in (0, 0, 1))
    pa, pb, pc = (dict(d.model.state_dict()) for d in (a, b, c))
    assert len(pa) > 10
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    differing = [k for k in pa if not torch.equal(pa[k], pc[k])]
    assert any(k.endswith("weight") for k in differing)
    # the draw does not depend on what the generator did before: the constructor seeds first
    torch.rand(17)
    assert all(torch.equal(pa[k], v) for k, v in Detector("disco", cfg, A, B, seed=0, device="cpu").model.state_dict().items())


def test_require_com_and_agents_of():
    from disconet_amd import COM_MODES, DET_COM_MODES
    common = _common()
    ns = argparse.Namespace
    for modes, pattern in ((DET_COM_MODES, r"disco \| sum \| mean \| max \| lowerbound \| late"),
                           (COM_MODES + ("lowerbound",), r"disco \| sum \| mean \| max")):
        with pytest.raises(SystemExit) as e:
            common.require_com(ns(com="v2v"), modes)
        assert re.search(pattern, str(e.value)) and "built on the MI355X path" in str(e.value)
        for com in modes:
            common.require_com(ns(com=com), modes)
    with pytest.raises(SystemExit):
        common.require_com(ns(com="late"), COM_MODES + ("lowerbound",))
    assert common.agents_of(ns(num_agent=5, rsu=0)) == 5 and common.agents_of(ns(num_agent=5, rsu=1)) == 6


def test_the_flag_helpers_keep_the_defaults():
    common = _common()
    ap = argparse.ArgumentParser()
    common.add_tail_flags(ap, 128)
    common.add_sort_flags(ap)
    a = ap.parse_args([])
    assert (a.pre_nms_top_k, a.iou_thr, a.score_thr) == (128, 0.01, None)
    assert (a.max_age, a.min_hits, a.iou_threshold, a.max_tracks) == (1, 3, 0.3, 128)
    ap = argparse.ArgumentParser()
    common.add_tail_flags(ap, 300)
    assert ap.parse_args(["--score_thr", "0.5"]).pre_nms_top_k == 300
