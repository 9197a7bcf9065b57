"""disconet_amd.Detector on the GPU: the same bits as the sequence the det / track tools used to write out themselves
(seed, build_model, randomize_bn_stats, eval, forward, detect, and late_fuse for `--com late`), as a captured step, and
from a checkpoint.  128 x 128 maps of tests/cases.MODEL_CASES, pre_nms_top_k = 64."""
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu

TOP_K = 64
CASE_OF = {"disco": "cfg1_f0", "max": "cfg1_f0", "lowerbound": "cfg1_f0", "late": "ragged_a4"}     # late: ragged live counts


def _setup(com):
    from disconet_amd import Config
    c = cases.MODEL_CASES[CASE_OF[com]]
    return Config(map_hw=c["map_hw"]), c["agents"], c["batch"], tuple(t.cuda() for t in cases.model_inputs(CASE_OF[com]))


def _written_out(com, seed=0):
    """(the detections, the unfused detections) of the sequence the tools wrote out"""
    from disconet_amd import build_model, postprocess as P
    from disconet_amd.synthetic import randomize_bn_stats
    cfg, A, B, (bevs, trans, na) = _setup(com)
    torch.manual_seed(seed)
    model = build_model(com, cfg, layer=3, kd_flag=0, num_agent=A, compress_level=0, only_v2i=False)
    randomize_bn_stats(model)
    model.eval().cuda()
    anchors = P.make_anchors(cfg)
    with torch.no_grad():
        out = model(bevs, trans, na, B)
    det = unfused = P.detect(out[0] if isinstance(out, tuple) else out, anchors, pre_nms_top_k=TOP_K, iou_thr=0.01,
                             score_thr=None)
    if com == "late":
        det = P.late_fuse(det, trans, na, B, A, iou_thr=0.01, only_v2i=False, extents=cfg.area_extents[:2])
    return det, unfused


def _assert_same_bits(got, want):
    assert sorted(got) == sorted(want)
    for key in want:
        assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), key


@pytest.mark.parametrize("com", ["disco", "max", "lowerbound", "late"])
def test_detector_gives_the_bits_of_the_written_out_sequence(com):
    from disconet_amd import Detector, graph
    cfg, A, B, (bevs, trans, na) = _setup(com)
    want, unfused = _written_out(com)
    assert int(want["count"].sum()) > 0
    if com == "late":                                      # the box-level step did something: equality is not vacuous
        assert not all(torch.equal(want[k], unfused[k]) for k in ("boxes", "scores", "count"))
    detector = Detector(com, cfg, A, B, pre_nms_top_k=TOP_K, seed=0)
    got = detector(bevs, trans, na)
    _assert_same_bits(got, want)
    if com == "late":                                      # the call is capturable: a replay gives the eager bits
        eager = {k: v.clone() for k, v in got.items()}
        step = graph.GraphedStep(lambda: detector(bevs, trans, na))
        replayed = step()
        torch.cuda.synchronize()
        _assert_same_bits(replayed, eager)
        step.drain()


def test_a_resumed_detector_gives_the_bits_of_the_one_that_wrote_the_checkpoint(tmp_path):
    from disconet_amd import Detector
    cfg, A, B, (bevs, trans, na) = _setup("late")
    first = Detector("lowerbound", cfg, A, B, pre_nms_top_k=TOP_K, seed=1)
    path = str(tmp_path / "epoch_4.pth")
    torch.save({"epoch": 4, "model_state_dict": first.model.state_dict()}, path)
    want = first(bevs, trans, na)
    assert int(want["count"].sum()) > 0
    resumed = Detector("lowerbound", cfg, A, B, pre_nms_top_k=TOP_K, resume=path, seed=0)
    assert resumed.epoch == 4
    _assert_same_bits(resumed(bevs, trans, na), want)
    fresh = Detector("lowerbound", cfg, A, B, pre_nms_top_k=TOP_K, seed=0)(bevs, trans, na)      # what seed 0 alone gives
    assert not all(torch.equal(fresh[k], want[k]) for k in want)
