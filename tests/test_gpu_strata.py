"""Stratified AP on the GPU (dn_gt_strata, dn_ap_match_strata behind postprocess.gt_strata / match_ground_truth_strata /
StratifiedAP) against the host statements, in every output byte: rank, best_iou, best_gt, tp, gt_claim, the records, the
state and the strata.  No tolerance anywhere: the cases of tests/strata_cases.py are dyadic and axis-aligned, so every IoU
is one correctly rounded division of exact operands on both sides; AP and recall are compared as float64 bits."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import strata_cases as SC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

MAX_AGENTS = 64


def _cuda(case):
    det = {k: torch.as_tensor(v).cuda() for k, v in case["det"].items()}
    return det, torch.as_tensor(case["gb"]).cuda(), torch.as_tensor(case["gc"]).cuda(), torch.as_tensor(case["st"]).cuda()


def _host(case):
    from disconet_amd import postprocess as P
    match = P.host_match_strata(case["det"], case["gb"], case["gc"], case["st"], case["S"], case["thrs"])
    return match, P.strata_records_from_match(case["det"], match, case["batch"])


def _state(case, frames, capacity=None):
    """the accumulator state the host expects after `frames` = [(match, records), ...]"""
    S = case["S"]
    state = np.zeros(2 + MAX_AGENTS * (S + 1), np.int64)
    for match, rec in frames:
        state[0] += len(rec)
        state[1] |= match["status"]
        counts = SC.agent_counts(match["counts"], case["batch"])
        state[2:2 + counts.size] += counts.ravel()
        if capacity is not None and state[0] > capacity:
            state[1] |= 1
    return state


def _assert_match(got, want):
    for key in ("rank", "best_gt", "tp", "gt_claim"):
        g = got[key].cpu().numpy()
        assert g.dtype == want[key].dtype and np.array_equal(g, want[key]), key
    g = got["best_iou"].cpu().numpy()
    assert g.dtype == np.float64 and g.tobytes() == want["best_iou"].tobytes()


# ---- 1. one update: every output byte -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.NAMES + ("hand",))
def test_update_equals_host_in_every_byte(name):
    from disconet_amd import postprocess as P
    case = SC.hand() if name == "hand" else SC.named(name)
    want, rec = _host(case)
    det, gb, gc, st = _cuda(case)
    m = P.StratifiedAP(case["batch"], case["S"], iou_thrs=case["thrs"], capacity=len(rec) + 7)
    big = torch.full((m.capacity + 64, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    m._allocate("cuda")
    m.records = big[:m.capacity]
    got = m.update(det, gb, gc, st)
    _assert_match(got, want)
    plain = P.match_ground_truth(det, gb, gc, case["thrs"])              # dn_ap_match on the same inputs
    for key in ("best_iou", "best_gt", "rank", "tp"):
        assert torch.equal(got[key], plain[key]), key
    alone = P.match_ground_truth_strata(det, gb, gc, st, case["S"], case["thrs"])      # without an accumulator
    for key in got:
        assert torch.equal(got[key], alone[key]), key
    assert m.records[:len(rec)].cpu().numpy().view(np.uint32).tobytes() == rec.tobytes()
    assert (big[len(rec):] == 0x5a5a5a5a).all()                          # nothing behind the last record, nothing behind the array
    state = m.state.cpu().numpy()
    assert state.tobytes() == _state(case, [(want, rec)]).tobytes()
    assert int(state[1]) == case["status"]
    records, counts, status = m.host_records()
    assert records.tobytes() == rec.tobytes() and status == case["status"]
    assert np.array_equal(counts, SC.agent_counts(want["counts"], case["batch"]))


def test_status_bits_raise_and_a_short_capacity_stays_inside_the_array():
    from disconet_amd import _lib as L
    from disconet_amd import postprocess as P
    for name, word in (("bad_strata", "stratum"), ("nonfinite", "non-finite")):
        case = SC.named(name)
        m = P.StratifiedAP(case["batch"], case["S"], iou_thrs=case["thrs"], capacity=4096)
        m.update(*_cuda(case))
        with pytest.raises(L.DnError, match=word):
            m.compute()
        m.reset()
        assert m.compute()["all"]["n_det"] == 0 and not m.state.cpu().numpy().any()
    case = SC.named("k65_g17_s2")
    want, rec = _host(case)
    m = P.StratifiedAP(case["batch"], case["S"], iou_thrs=case["thrs"], capacity=len(rec) - 2)      # two records short
    big = torch.full((m.capacity + 64, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    m._allocate("cuda")
    m.records = big[:m.capacity]
    m.update(*_cuda(case))
    with pytest.raises(L.DnError, match="capacity"):
        m.compute()
    state = m.state.cpu().numpy()
    assert int(state[0]) == len(rec) and int(state[1]) == 1               # the cursor still counts the two that were dropped
    assert state.tobytes() == _state(case, [(want, rec)], capacity=m.capacity).tobytes()
    assert big[:m.capacity].cpu().numpy().view(np.uint32).tobytes() == rec[:m.capacity].tobytes()
    assert (big[m.capacity:] == 0x5a5a5a5a).all()


# ---- 2. accumulation, reset, captured graph ---------------------------------------------------------------------------------------
def _two_frames():
    a, b = SC.named("k65_g17_s2"), SC.named("bad_strata")               # the same shapes, other data
    b["st"] = np.clip(b["st"], -1, 1)
    b["status"] = 0
    return a, b


def test_two_frames_equal_the_host_and_graph_replays_equal_eager_updates():
    from disconet_amd import graph, postprocess as P
    frames = _two_frames()
    host = [_host(c) for c in frames]
    rec = np.concatenate([h[1] for h in host])
    want_state = _state(frames[0], host)
    eager = P.StratifiedAP(1, 2, capacity=1024)
    for c in frames:
        eager.update(*_cuda(c))
    assert eager.records[:len(rec)].cpu().numpy().view(np.uint32).tobytes() == rec.tobytes()
    assert eager.state.cpu().numpy().tobytes() == want_state.tobytes()
    counts = want_state[2:].reshape(MAX_AGENTS, 3)[:3]
    res = eager.compute()
    want = P.stratified_ap_from_records(rec, counts, 2)
    assert res.keys() == want.keys() and len(res["per_agent"]) == 3
    SC.same_row(res["all"], want["all"])
    for got_row, want_row in zip(res["strata"] + res["per_agent"], want["strata"] + want["per_agent"]):
        SC.same_row(got_row, want_row)
    assert 0.0 < res["strata"][0]["AP@0.7"] < 1.0 and res["all"]["n_left_out"][0] > 0

    static = [t.clone() for t in _flat(_cuda(frames[0]))]

    def load(case):
        for dst, src in zip(static, _flat(_cuda(case))):
            dst.copy_(src)

    metric = P.StratifiedAP(1, 2, capacity=1024)
    step = graph.GraphedStep(lambda: metric.update({"boxes": static[0], "scores": static[1], "count": static[2]},
                                                   static[3], static[4], static[5]), range_guard=False)
    metric.reset()                                       # the warm-up runs and the capture appended records
    for c in frames:
        load(c)
        step()
    step.drain()
    torch.cuda.synchronize()
    assert metric.records[:len(rec)].cpu().numpy().view(np.uint32).tobytes() == rec.tobytes()
    assert metric.state.cpu().numpy().tobytes() == eager.state.cpu().numpy().tobytes()


def _flat(c):
    det, gb, gc, st = c
    return [det["boxes"], det["scores"], det["count"], gb, gc, st]


def test_one_stratum_equals_mean_ap():
    from disconet_amd import postprocess as P
    case = SC.named("s1")
    det, gb, gc, st = _cuda(case)
    m, plain = P.StratifiedAP(1, 1), P.MeanAP(1)
    for _ in range(2):
        m.update(det, gb, gc, st)
        plain.update(det, gb, gc)
    res, want = m.compute(), plain.compute()
    for thr in (0.5, 0.7):
        for row in (res["all"], res["strata"][0]):
            assert np.float64(row["AP@%g" % thr]).view(np.uint64) == np.float64(want["mAP@%g" % thr]).view(np.uint64)
    assert 0.05 < want["mAP@0.7"] < 1.0
    assert res["all"]["n_det"] == want["n_det"] and res["all"]["n_gt"] == want["n_gt"] and res["all"]["n_tp"] == want["n_tp"]
    for got_row, want_row in zip(res["per_agent"], want["per_agent"]):
        assert np.float64(got_row["AP@0.5"]).view(np.uint64) == np.float64(want_row["mAP@0.5"]).view(np.uint64)
        assert got_row["n_gt"] == want_row["n_gt"] and got_row["n_tp"] == want_row["n_tp"]


# ---- 3. gt_strata -------------------------------------------------------------------------------------------------------------------
def test_gt_strata_equals_host_in_every_word():
    from disconet_amd import postprocess as P
    r = np.random.default_rng(0)
    n, g = 3, 300                                          # two 256-column blocks
    gb = r.uniform(-32, 32, (n, g, 6)).astype(np.float32)
    gb[0, :8, 0] = [3.0, 6.0, 12.0, -12.0, 30.0, np.nan, 1.0, np.float32(np.nextafter(np.float32(10.0), np.float32(0)))]
    gb[0, :8, 1] = [4.0, -8.0, 0.0, 16.0, 30.0, 1.0, np.inf, 0.0]
    gb[1, 0, :2] = [3e38, 3e38]                           # finite in float32, far: the squares stay finite in float64
    gc = np.asarray([g, 257, -2], np.int32)
    own = r.integers(0, 12, (n, g)).astype(np.int32)
    own[0, :4] = [0, 4, 5, 6]
    for mode, edges, hits in (("range", (10, 20), None), ("range", (5, 10, 15, 20, 25, 30, 35), None), ("range", (10, 20), own),
                              ("visibility", (5,), own), ("visibility", (1, 5, 9), own)):
        want = P.host_gt_strata(gb, gc, mode, edges, hits)
        got = P.gt_strata(torch.as_tensor(gb).cuda(), torch.as_tensor(gc).cuda(), mode, edges,
                          None if hits is None else torch.as_tensor(hits).cuda())
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (mode, edges)
        assert len(set(want[0].tolist())) == len(edges) + 2 if mode == "range" else True
    want = P.host_gt_strata(gb, gc, "range", (10, 20))
    assert want[0, :8].tolist() == [0, 1, 1, 2, 2, -1, -1, 0] and want[1, 0] == 2 and (want[2] == -1).all() and (want[1, 257:] == -1).all()


# ---- 4. the evaluation tool ---------------------------------------------------------------------------------------------------------
def _tool(*extra):
    tool = os.path.join(ROOT, "tools", "det", "eval_codet.py")
    r = subprocess.run([sys.executable, tool, "--com", "lowerbound", "--scene", "lidar", "--gt", "scene", "--num_agent", "2",
                        "--frames", "2"] + list(extra), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    return r.stdout


def test_eval_codet_prints_one_line_per_stratum_and_the_same_overall_line():
    plain, strata = _tool(), _tool("--strata", "visibility")
    assert "stratum" not in plain
    assert strata.startswith(plain)                                        # the per-agent and overall lines are the same text
    overall = [line for line in strata.splitlines() if line.startswith("overall:")]
    assert len(overall) == 1 and overall[0] in plain.splitlines()
    rows = re.findall(r"^stratum (\d), (.+): AP@0\.5 (\S+)  AP@0\.7 (\S+)  recall (\S+) / (\S+)  \((\d+) ground-truth boxes, "
                      r"detections counted (\d+) / (\d+), left out (\d+) / (\d+)\)$", strata, re.M)
    assert [r[0] for r in rows] == ["0", "1"] and "hidden from the ego" in rows[0][1] and "seen by the ego" in rows[1][1]
    n_gt = int(re.search(r"(\d+) ground-truth boxes", overall[0]).group(1))
    assert int(rows[0][6]) + int(rows[1][6]) == n_gt and int(rows[0][6]) >= 1
