"""Stratified AP without a GPU: postprocess.host_match_strata / strata_records_from_match / stratified_ap_from_records
against the sequential restatement of tests/strata_cases.py (integers equal, floats equal as float64 bits), the hand case,
the S = 1 and partition identities with MeanAP's host path, host_gt_strata's edges, the lidar scenes' hidden boxes, the
evaluation tool's flags and the C ABI's declarations and refusals."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from tests import strata_cases as SC
from tests.conftest import ROOT


def _host(case):
    from disconet_amd import postprocess as P
    match = P.host_match_strata(case["det"], case["gb"], case["gc"], case["st"], case["S"], case["thrs"])
    return match, P.strata_records_from_match(case["det"], match, case["batch"])


# ---- 1. the host functions against the restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.NAMES + ("hand",))
def test_host_match_and_metric_equal_the_restatement(name):
    from disconet_amd import postprocess as P
    case = SC.hand() if name == "hand" else SC.named(name)
    match, rec = _host(case)
    want, records = SC.brute_match(case)
    for key in ("rank", "best_gt", "tp", "gt_claim", "stratum", "reach", "counts"):
        assert np.array_equal(match[key], want[key]), key
    assert match["best_iou"].tobytes() == want["best_iou"].tobytes()
    assert match["status"] == want["status"] == case["status"]
    assert rec.dtype == np.uint32 and rec.tobytes() == SC.record_words(records).tobytes()
    assert len(records) > 0 and any(r[2] for r in records)
    counts = SC.agent_counts(match["counts"], case["batch"])
    got = P.stratified_ap_from_records(rec, counts, case["S"], case["thrs"])
    SC.same_row(got["all"], SC.brute_row(records, counts, case["thrs"], None))
    assert [r["name"] for r in got["strata"]] == ["stratum %d" % s for s in range(case["S"])]
    for s in range(case["S"]):
        SC.same_row(got["strata"][s], SC.brute_row(records, counts, case["thrs"], s))
    assert len(got["per_agent"]) == len(counts)
    for a in range(len(counts)):
        SC.same_row(got["per_agent"][a], SC.brute_row(records, counts, case["thrs"], None, agent=a))


def test_the_cases_hold_what_they_are_for():
    """duplicates on one box, matches in every stratum, don't-care matches, equal scores, every shift"""
    case = SC.named("k65_g17_s2")
    match, rec = _host(case)
    st = (rec[:, 2] >> 8).astype(int) - 1
    reach, tp = rec[:, 2] & 1, rec[:, 1] & 1
    assert set(st[reach == 1]) == {-1, 0, 1}
    assert ((reach == 1) & (tp == 0)).sum() >= 3                       # duplicates
    assert len(np.unique(rec[:, 0])) < len(rec) // 2                   # equal scores
    ious = set(np.round(match["best_iou"][match["best_gt"] >= 0], 6))
    assert ious == {1.0, round(7 / 9, 6), 0.6, round(1 / 3, 6)}
    assert (match["best_gt"][0] == 1).sum() == 0 and (match["best_gt"][0] == 0).sum() > 0     # the copy at column 1 never wins
    wide = SC.named("k257_g17_s8_t8")
    m8, _ = _host(wide)
    assert (m8["rank"][0] >= 0).sum() == 257 and (m8["rank"][1] >= 0).sum() == 0 and m8["counts"][0].sum() == 17
    assert set(range(8)) <= set(m8["stratum"].ravel().tolist())
    assert len({int(v) for v in m8["reach"].ravel()}) >= 4              # the eight thresholds tell the four IoUs apart


# ---- 2. the hand case -------------------------------------------------------------------------------------------------------
def test_hand_case_figures_and_meanap_differs():
    from disconet_amd import postprocess as P
    case = SC.hand()
    match, rec = _host(case)
    res = P.stratified_ap_from_records(rec, SC.agent_counts(match["counts"], 1), 2, (0.5,), names=["near", "far"])
    assert res["strata"][0]["AP@0.5"] == 0.5 and res["strata"][1]["AP@0.5"] == 1.0
    assert res["all"]["AP@0.5"] == 0.5 + 0.5 * (2 / 3)
    assert res["strata"][0]["recall@0.5"] == 1.0 and res["strata"][1]["recall@0.5"] == 1.0 and res["all"]["recall@0.5"] == 1.0
    assert [r["name"] for r in res["strata"]] == ["near", "far"]
    assert [r["n_gt"] for r in res["strata"]] == [1, 1] and res["all"]["n_gt"] == 2
    assert [r["n_left_out"] for r in res["strata"]] == [[2], [3]] and res["all"]["n_left_out"] == [1]
    assert [r["n_counted"] for r in res["strata"]] == [[3], [2]] and res["all"]["n_counted"] == [4]
    s, tp, _ = P.records_from_match(case["det"], match)
    # MeanAP counts C: three boxes, three true positives, five records where "all" has two, two and four.  Its curve
    # is another one -- (1/3, 1), (2/3, 3/4), (1, 3/4) against (1/2, 1), (1, 2/3) -- but the areas happen to be the same
    # number, 1/3 + 1/2 = 1/2 + 1/3 = 5/6: on this case the two metrics differ in their counts and curves, not in the AP.
    mean_ap = P.average_precision_from_records(s, tp[0], 3)
    assert (3, int(tp[0].sum()), len(s)) != (res["all"]["n_gt"], res["all"]["n_tp"][0], res["all"]["n_counted"][0])
    assert (int(tp[0].sum()), len(s)) == (3, 5)
    print("hand case: MeanAP %.17g, all %.17g" % (mean_ap, res["all"]["AP@0.5"]))
    assert int(tp[0].sum()) / 3 == res["all"]["recall@0.5"] == 1.0
    # on A and B alone MeanAP has d4 as a false positive where "all" leaves it out: same AP here too (d4 ranks behind
    # the last true positive), one more detection counted
    two = P.host_match_ground_truth(case["det"], case["gb"], np.asarray([2], np.int32), (0.5,))
    s2, tp2, _ = P.records_from_match(case["det"], two)
    assert len(s2) == 5 and res["all"]["n_counted"] == [4] and int(tp2[0].sum()) == 2


def test_empty_stratum_is_nan_recall_and_zero_ap():
    from disconet_amd import postprocess as P
    case = SC.hand()
    match, rec = _host(case)
    res = P.stratified_ap_from_records(rec, [[1, 1, 0, 1]], 3, (0.5,))          # the same records among three strata
    assert res["strata"][2]["n_gt"] == 0 and res["strata"][2]["AP@0.5"] == 0.0 and math.isnan(res["strata"][2]["recall@0.5"])
    empty = P.stratified_ap_from_records(np.zeros((0, 4), np.uint32), np.zeros((0, 3)), 2)
    assert empty["all"]["AP@0.5"] == 0.0 and empty["per_agent"] == [] and len(empty["strata"]) == 2


# ---- 3. identities with MeanAP's host path ------------------------------------------------------------------------------------
def _mean_ap_host(case):
    from disconet_amd import postprocess as P
    match = P.host_match_ground_truth(case["det"], case["gb"], case["gc"], case["thrs"])
    s, tp, _ = P.records_from_match(case["det"], match)
    n_gt = int(np.clip(case["gc"], 0, case["gb"].shape[1]).sum())
    return [P.average_precision_from_records(s, tp[t], n_gt) for t in range(len(case["thrs"]))], tp, n_gt


def test_one_stratum_equals_meanap_bits():
    from disconet_amd import postprocess as P
    case = SC.named("s1")
    match, rec = _host(case)
    res = P.stratified_ap_from_records(rec, SC.agent_counts(match["counts"], 1), 1, case["thrs"])
    want, tp, n_gt = _mean_ap_host(case)
    for t, thr in enumerate(case["thrs"]):
        assert 0.05 < want[t] < 1.0
        for row in (res["all"], res["strata"][0]):
            assert np.float64(row["AP@%g" % thr]).view(np.uint64) == np.float64(want[t]).view(np.uint64)
            assert row["n_gt"] == n_gt and row["n_tp"][t] == int(tp[t].sum()) and row["n_left_out"][t] == 0


def test_strata_partition_meanap_without_dont_care_boxes():
    from disconet_amd import postprocess as P
    case = SC.named("no_dont_care")
    match, rec = _host(case)
    res = P.stratified_ap_from_records(rec, SC.agent_counts(match["counts"], case["batch"]), case["S"], case["thrs"])
    _, tp, n_gt = _mean_ap_host(case)
    assert sum(r["n_gt"] for r in res["strata"]) == n_gt == res["all"]["n_gt"] and min(r["n_gt"] for r in res["strata"]) > 0
    for t in range(len(case["thrs"])):
        assert sum(r["n_tp"][t] for r in res["strata"]) == int(tp[t].sum()) == res["all"]["n_tp"][t] > 0
        assert res["all"]["n_left_out"][t] == 0


# ---- 4. host_gt_strata ------------------------------------------------------------------------------------------------------------
def test_gt_strata_edges_non_finite_centres_and_rows_beyond_the_count():
    from disconet_amd import postprocess as P
    gb = np.zeros((2, 8, 6), np.float32)
    #            inside     on the edge 10 (6-8-10)   between    on the edge 20   beyond      NaN x        inf y      beyond count
    gb[0, :, 0] = [3.0,      6.0,                      12.0,      -12.0,           30.0,       np.nan,      1.0,       1.0]
    gb[0, :, 1] = [4.0,      -8.0,                     0.0,       16.0,            30.0,       1.0,         np.inf,    1.0]
    gb[1] = gb[0]
    got = P.host_gt_strata(gb, np.asarray([7, 2], np.int32), "range", (10, 20))
    assert got.dtype == np.int32
    assert got[0].tolist() == [0, 1, 1, 2, 2, -1, -1, -1] and got[1].tolist() == [0, 1] + [-1] * 6
    assert P.host_gt_strata(gb, np.asarray([99, -4], np.int32), "range", (10, 20))[:, 7].tolist() == [0, -1]      # counts are clamped
    just_inside = np.nextafter(np.float32(10.0), np.float32(0))
    gb[0, 0, :2] = [just_inside, 0.0]
    assert P.host_gt_strata(gb, np.asarray([1, 0], np.int32), "range", (10, 20))[0, 0] == 0
    own = np.asarray([[0, 4, 5, 6, 19, 20, 7, 7]] * 2, np.int32)
    got = P.host_gt_strata(gb, np.asarray([6, 8], np.int32), "visibility", (5,), own)
    assert got[0].tolist() == [0, 0, 1, 1, 1, 1, -1, -1] and got[1].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    assert P.host_gt_strata(gb, np.asarray([6, 0], np.int32), "visibility", (5, 20), own)[0].tolist() == [0, 0, 1, 1, 1, 2, -1, -1]
    assert P.strata_names("visibility", (5,)) == ["hidden from the ego (< 5 own returns)", "seen by the ego (>= 5 own returns)"]
    assert P.strata_names("range", (10, 20)) == ["< 10 m", "10..20 m", ">= 20 m"]
    for mode, edges in (("range", ()), ("range", (20, 10)), ("range", (0, 5)), ("range", range(1, 9)), ("visibility", (2.5,)),
                        ("visibility", (0,)), ("fog", (1,)), ("range", (math.nan,))):
        with pytest.raises(ValueError):
            P.host_gt_strata(gb, np.asarray([1, 1], np.int32), mode, edges, own)
    with pytest.raises(ValueError):
        P.host_gt_strata(gb, np.asarray([1, 1], np.int32), "visibility", (5,))


def test_hidden_boxes_of_the_tools_lidar_scenes_are_stratum_zero():
    """codet_common.lidar_scene at 5 agents, seeds 0 .. 3, built on the host: stratum 0 at edge 5 holds exactly the (image,
    box) pairs with fewer than 5 own returns, and every seed has one."""
    from disconet_amd import postprocess as P
    _tool()
    import codet_common
    total = 0
    for seed in range(4):
        scene = codet_common.lidar_scene(1, 5, 256, seed, 64, device=None)
        own, count = scene["gt_own_hits"].numpy(), scene["gt_count"].numpy()
        direct = {(i, g) for i in range(len(count)) for g in range(int(count[i])) if own[i, g] < 5}
        st = P.host_gt_strata(scene["gt_boxes"], scene["gt_count"], "visibility", (5,), scene["gt_own_hits"])
        assert {(int(i), int(g)) for i, g in zip(*np.nonzero(st == 0))} == direct and len(direct) >= 1, seed
        assert (st == 1).sum() == int(count.sum()) - len(direct) and (st == -1).sum() == st.size - int(count.sum())
        by_range = P.host_gt_strata(scene["gt_boxes"], scene["gt_count"], "range", (10, 20))
        assert ((by_range >= 0) == (st >= 0)).all() and len(set(by_range[by_range >= 0].tolist())) == 3
        total += len(direct)
    print("hidden (image, box) pairs, seeds 0..3:", total)


# ---- 5. the evaluation tool's flags ---------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("strata_tool_eval_codet", os.path.join(ROOT, "tools", "det", "eval_codet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_codet_takes_strata_flags_and_refuses_visibility_without_lidar():
    mod = _tool()
    ap = mod.build_eval_parser()
    assert ap.parse_args([]).strata == "none" and ap.parse_args([]).strata_edges is None
    args = ap.parse_args(["--strata", "range", "--strata_edges", "5,15,25"])
    assert args.strata == "range" and mod.strata_edges_of(args) == [5.0, 15.0, 25.0]
    assert mod.strata_edges_of(ap.parse_args(["--strata", "range"])) == [10.0, 20.0]
    assert mod.strata_edges_of(ap.parse_args(["--strata", "visibility"])) == [5.0]
    with pytest.raises(SystemExit):
        ap.parse_args(["--strata", "fog"])
    with pytest.raises(SystemExit, match="strata_edges"):
        mod.strata_edges_of(ap.parse_args(["--strata", "range", "--strata_edges", "20,10"]))
    for argv in (["--strata", "visibility"], ["--strata", "visibility", "--scene", "lidar"],
                 ["--strata", "visibility", "--gt", "scene"]):
        with pytest.raises(SystemExit, match=r"--scene lidar.*--gt scene"):
            mod.main(["--com", "disco"] + argv)


# ---- 6. the C ABI -----------------------------------------------------------------------------------------------------------------
NAMES = ("dn_gt_strata", "dn_ap_match_strata_workspace_bytes", "dn_ap_match_strata", "dn_ap_strata_reset")
FAKE = ctypes.c_void_p(0x1000)


def test_header_declares_the_entry_points_and_the_package_exports_the_metric():
    import disconet_amd
    from disconet_amd import _lib
    raw = open(os.path.join(ROOT, "include", "disconet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and getattr(_lib.load(), name) is not None
    assert _lib.load().dn_version() >= 153
    for name in ("StratifiedAP", "gt_strata"):
        assert name in disconet_amd.__all__ and hasattr(disconet_amd, name)
    for name in ("host_gt_strata", "match_ground_truth_strata", "host_match_strata", "strata_records_from_match",
                 "stratified_ap_from_records"):
        assert callable(getattr(disconet_amd.postprocess, name)), name


def _match(n=20, k=300, g=64, thrs=(0.5, 0.7), s=2, ws_bytes=None, null=None, records=FAKE, capacity=1000, state=FAKE,
           n_agents=8, batch=4):
    """dn_ap_match_strata with fake (never dereferenced) device pointers: every refusal happens before a launch."""
    from disconet_amd import _lib
    lib = _lib.load()
    need = lib.dn_ap_match_strata_workspace_bytes(n, k, g, len(thrs), s)
    names = ("boxes", "scores", "count", "gt_boxes", "gt_count", "gt_stratum", "best_iou", "best_gt", "rank", "tp", "ws")
    p = {q: (None if q == null else FAKE) for q in names}
    rc = lib.dn_ap_match_strata(p["boxes"], p["scores"], p["count"], p["gt_boxes"], p["gt_count"], p["gt_stratum"], n, k, g,
                                (ctypes.c_double * len(thrs))(*thrs), len(thrs), s, p["best_iou"], p["best_gt"], p["rank"],
                                p["tp"], None, p["ws"], need if ws_bytes is None else ws_bytes, records, capacity, state,
                                n_agents, batch, None)
    return rc, lib.dn_last_error().decode()


def test_match_strata_refusals_happen_before_a_launch():
    from disconet_amd import _lib
    lib = _lib.load()
    base = lib.dn_ap_match_workspace_bytes(20, 300, 64, 2)
    need = lib.dn_ap_match_strata_workspace_bytes(20, 300, 64, 2, 8)
    assert base < need <= base + 256 * (1 + 20 * 9 * 4 // 256)
    for s in (0, 9, -1):
        assert lib.dn_ap_match_strata_workspace_bytes(20, 300, 64, 2, s) == 0
        rc, msg = _match(s=s)
        assert rc != 0 and "S = " in msg
    assert lib.dn_ap_match_strata_workspace_bytes(20, 1025, 64, 2, 2) == 0
    for null in ("boxes", "gt_stratum", "tp", "ws"):
        rc, msg = _match(null=null)
        assert rc != 0 and "null" in msg
    for kw, word in ((dict(k=1025), "K = "), (dict(g=0), "G = "), (dict(thrs=(0.5, 1.5)), "threshold 1"),
                     (dict(ws_bytes=need - 1, s=8), "dn_ap_match_strata_workspace_bytes"), (dict(capacity=0), "capacity"),
                     (dict(state=None), "null"), (dict(n_agents=4), "agent"), (dict(n=0), "images"),
                     (dict(records=ctypes.c_void_p(0x1008)), "16-byte")):
        rc, msg = _match(**kw)
        assert rc != 0 and word in msg and msg.startswith("ap_match_strata"), (kw, msg)
    for args, word in (((None, 4, 2), "null"), ((FAKE, 0, 2), "agent"), ((FAKE, 4, 9), "S = ")):
        rc = lib.dn_ap_strata_reset(args[0], args[1], args[2], None)
        assert rc != 0 and word in lib.dn_last_error().decode()


def test_gt_strata_refusals_happen_before_a_launch():
    from disconet_amd import _lib
    lib = _lib.load()

    def call(own=FAKE, n=4, g=64, mode=0, edges=(10.0, 20.0), n_edges=None, out=FAKE):
        arr = (ctypes.c_double * max(1, len(edges)))(*edges)
        rc = lib.dn_gt_strata(FAKE, FAKE, own, n, g, mode, arr, len(edges) if n_edges is None else n_edges, out, None)
        return rc, lib.dn_last_error().decode()

    for kw, word in ((dict(out=None), "null"), (dict(n=0), "images"), (dict(g=1025), "G = "), (dict(mode=2), "mode"),
                     (dict(mode=1, own=None, edges=(5.0,)), "gt_own_hits"), (dict(n_edges=0), "edges"),
                     (dict(edges=(1.0,) * 8), "edges"), (dict(edges=(20.0, 10.0)), "ascending"), (dict(edges=(0.0,)), "positive"),
                     (dict(edges=(math.inf,)), "finite"), (dict(mode=1, edges=(2.5,)), "integers"),
                     (dict(mode=1, edges=(0.5,)), "integers")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)


def test_python_entry_points_refuse_what_they_cannot_run():
    import torch

    from disconet_amd import _lib as L
    from disconet_amd import postprocess as P
    case = SC.hand()
    cpu = {k: torch.as_tensor(v) for k, v in case["det"].items()}
    gb, gc, st = (torch.as_tensor(case[q]) for q in ("gb", "gc", "st"))
    m = P.StratifiedAP(batch_size=1, n_strata=2)
    with pytest.raises(L.DnError):
        m.update(cpu, gb, gc, st)
    with pytest.raises(L.DnError):
        P.match_ground_truth_strata(cpu, gb, gc, st, 2)
    with pytest.raises(L.DnError):
        P.gt_strata(case["gb"], case["gc"], "range", (10, 20))            # numpy: host_gt_strata is the host form
    for kw in (dict(n_strata=0), dict(n_strata=9), dict(n_strata=2, names=["one"]), dict(n_strata=2, capacity=0),
               dict(n_strata=2, iou_thrs=(0.0,))):
        with pytest.raises(ValueError):
            P.StratifiedAP(batch_size=1, **kw)
    empty = m.compute()                                                    # nothing accumulated: defined, zero
    assert empty["all"]["AP@0.5"] == 0.0 and empty["per_agent"] == [] and [r["n_gt"] for r in empty["strata"]] == [0, 0]
