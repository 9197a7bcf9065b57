"""mAP without a GPU: the host reference of the GPU matching (postprocess.host_match_ground_truth +
average_precision_from_records) against the oracle's sequential average_precision -- AP equal as float64 bits on the
seeded generator, exact crafted cases -- and the C ABI of dn_ap_match: declared, bound, every refusal before a launch."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import ap_cases as A
from tests.conftest import ROOT


# ---- 1. the parallel restatement equals the oracle's sequential loop, bit for bit ------------------------------------
@pytest.mark.parametrize("pitch", [10.0, 3.5])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_host_reference_equals_oracle_bits(seed, pitch):
    from disconet_amd import postprocess as P
    dets, scs, gts = A.make(seed, pitch=pitch)
    det, gb, gc = A.padded(dets, scs, gts)
    A.assert_margins(det, gb, gc, "seed %d pitch %g" % (seed, pitch))
    match = P.host_match_ground_truth(det, gb, gc, A.THRS)
    got = A.host_ap(det, gb, gc, match=match)
    for t, thr in enumerate(A.THRS):
        want = A.oracle_ap(dets, scs, gts, thr)
        print("seed %d pitch %g t %g: AP %.17g, oracle %.17g, %d true positives of %d records" % (
            seed, pitch, thr, got[t], want, int(match["tp"][t].sum()), int(gc.sum())))
        assert 0.05 < want < 0.9
        assert A.bits(got[t]) == A.bits(want)


# ---- 2. crafted exact cases ------------------------------------------------------------------------------------------
def test_crafted_exact_cases():
    from disconet_amd import postprocess as P
    dets, scs, gts, exp = A.crafted()
    det, gb, gc = A.padded(dets, scs, gts)
    match = P.host_match_ground_truth(det, gb, gc, A.THRS)
    A.check_crafted(match, exp)
    assert match["rank"][2, :3].tolist() == [0, 1, 2]              # equal scores: the lower row first
    assert match["rank"][6, :2].tolist() == [0, 1]
    assert int(gc.sum()) == 12 and int(gc[3]) == 2                  # the image without detections counts in n_gt
    got = A.host_ap(det, gb, gc, match=match)
    for t, thr in enumerate(A.THRS):
        assert A.bits(got[t]) == A.bits(A.oracle_ap(dets, scs, gts, thr))
    # padding wider than the data changes nothing
    det_w, gb_w, gc_w = A.padded(dets, scs, gts, k=70, g=33)
    wide = P.host_match_ground_truth(det_w, gb_w, gc_w, A.THRS)
    A.check_crafted(wide, exp)


def test_no_ground_truth_at_all_is_zero():
    from disconet_amd import postprocess as P
    dets, scs, gts, _ = A.crafted()
    none = [g[:0] for g in gts]
    det, gb, gc = A.padded(dets, scs, none)
    match = P.host_match_ground_truth(det, gb, gc, A.THRS)
    assert (match["best_gt"] == -1).all() and not match["tp"].any()
    assert A.host_ap(det, gb, gc, match=match) == [0.0, 0.0]
    assert A.oracle_ap(dets, scs, none, 0.5) == 0.0
    assert P.average_precision_from_records(np.zeros(0), np.zeros(0), 5) == 0.0


def test_non_finite_scores_are_not_rows_and_unsorted_rows_are_ranked():
    from disconet_amd import postprocess as P
    dets, scs, gts = A.make(0, n_img=3)
    scs[1] = scs[1].copy()
    scs[1][::4] = np.nan
    scs[2] = scs[2].copy()
    scs[2][0] = np.inf
    det, gb, gc = A.padded(dets, scs, gts)
    match = P.host_match_ground_truth(det, gb, gc, A.THRS)
    for img in range(3):
        c = int(det["count"][img])
        ok = np.isfinite(det["scores"][img, :c])
        assert sorted(match["rank"][img, :c][ok].tolist()) == list(range(int(ok.sum())))
        assert (match["rank"][img, :c][~ok] == -1).all() and (match["best_gt"][img, :c][~ok] == -1).all()
        order = np.argsort(match["rank"][img, :c][ok], kind="stable")
        assert (np.diff(det["scores"][img, :c][ok][order]) <= 0).all()
    with pytest.raises(ValueError):
        P.host_match_ground_truth(det, gb, gc, (0.0, 0.5))
    with pytest.raises(ValueError):
        P.host_match_ground_truth(det, gb, gc, (0.5, 1.5))
    with pytest.raises(ValueError):
        P.host_match_ground_truth(det, gb, gc, [0.1] * 9)


def test_make_gt_boxes_is_seeded_and_padded():
    from disconet_amd.synthetic import make_gt_boxes
    b, c = make_gt_boxes(6, seed=3, max_boxes=40)
    b2, c2 = make_gt_boxes(6, seed=3, max_boxes=40)
    assert torch.equal(b, b2) and torch.equal(c, c2)
    assert tuple(b.shape) == (6, 40, 6) and b.dtype == torch.float32 and c.dtype == torch.int32
    assert (c >= 20).all() and (c <= 40).all()
    for i in range(6):
        assert not b[i, int(c[i]):].any() and (b[i, :int(c[i]), 2:4] > 0).all()
    assert not torch.equal(b, make_gt_boxes(6, seed=4, max_boxes=40)[0])


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------------
NAMES = ("dn_ap_match_workspace_bytes", "dn_ap_match", "dn_ap_reset")


def _lib():
    from disconet_amd import _lib
    return _lib.load()


def test_header_declares_ap_entry_points_and_bindings_exist():
    from disconet_amd import _lib
    raw = open(os.path.join(ROOT, "include", "disconet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None
    assert _lib.load().dn_version() >= 136
    assert "mAP stays on the CPU" not in raw
    from disconet_amd.csrc import build
    assert "ap_match.hip" in build.SOURCES and "disconet_amd/csrc/rot_iou_device.h" in build.tree_files()


POINTERS = ("boxes", "scores", "count", "gt_boxes", "gt_count", "iou_thrs", "best_iou", "best_gt", "rank", "tp", "ws")


def _call(n=20, k=300, g=64, thrs=(0.5, 0.7), nt=None, ws_bytes=None, null=None, accumulate=True, capacity=1000,
          state=True, n_agents=8, batch=4):
    """dn_ap_match with fake (never dereferenced) device pointers: every refusal happens before a launch."""
    lib = _lib()
    nt = len(thrs) if nt is None else nt
    need = lib.dn_ap_match_workspace_bytes(n, max(1, min(k, 1024)), max(1, min(g, 1024)), max(1, min(nt, 8)))
    fake = ctypes.c_void_p(0x1000)
    p = {name: (None if name == null else fake) for name in POINTERS}
    arr = None if null == "iou_thrs" else (ctypes.c_double * max(1, len(thrs)))(*thrs)
    rc = lib.dn_ap_match(p["boxes"], p["scores"], p["count"], p["gt_boxes"], p["gt_count"], n, k, g, arr, nt,
                         p["best_iou"], p["best_gt"], p["rank"], p["tp"], p["ws"], need if ws_bytes is None else ws_bytes,
                         fake if accumulate else None, capacity, fake if state else None, n_agents, batch, None)
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("which", POINTERS)
def test_null_pointer_is_refused(which):
    rc, msg = _call(null=which)
    assert rc != 0 and "null" in msg


@pytest.mark.parametrize("k", [0, 1025, -1])
def test_k_out_of_range_is_refused(k):
    rc, msg = _call(k=k)
    assert rc != 0 and "K = " in msg


@pytest.mark.parametrize("g", [0, 1025, -1])
def test_g_out_of_range_is_refused(g):
    rc, msg = _call(g=g)
    assert rc != 0 and "G = " in msg


@pytest.mark.parametrize("nt", [0, 9, -1])
def test_threshold_count_out_of_range_is_refused(nt):
    rc, msg = _call(thrs=(0.5,) * 9, nt=nt)
    assert rc != 0 and "T = " in msg


@pytest.mark.parametrize("thr", [0.0, -0.5, 1.0000001, math.nan, math.inf])
def test_threshold_outside_unit_interval_is_refused(thr):
    rc, msg = _call(thrs=(0.5, thr))
    assert rc != 0 and "threshold 1" in msg
    assert _call(thrs=(1.0, 1e-300), ws_bytes=0)[1].find("workspace") >= 0      # (0, 1] itself passes the threshold check


def test_short_workspace_zero_capacity_and_bad_accumulator_are_refused():
    lib = _lib()
    need = lib.dn_ap_match_workspace_bytes(20, 300, 64, 2)
    assert need >= 20 * 300 * 4 * (8 + 4)               # one (IoU, index) per row and 16-column piece at least
    rc, msg = _call(ws_bytes=need - 1)
    assert rc != 0 and "workspace" in msg
    for cap in (0, -5):
        rc, msg = _call(capacity=cap)
        assert rc != 0 and "capacity" in msg
    rc, msg = _call(state=False)
    assert rc != 0 and "null" in msg
    rc, msg = _call(n_agents=4, batch=4)                # 20 images at batch 4 are 5 agents
    assert rc != 0 and "agent" in msg
    rc, msg = _call(batch=0)
    assert rc != 0 and "agent" in msg
    rc, msg = _call(n=0)
    assert rc != 0 and "images" in msg
    rc, msg = lib.dn_ap_reset(None, 4, None), lib.dn_last_error().decode()
    assert rc != 0 and "null" in msg
    rc, msg = lib.dn_ap_reset(ctypes.c_void_p(0x1000), 0, None), lib.dn_last_error().decode()
    assert rc != 0 and "agent" in msg


def test_workspace_query_refuses_what_the_call_refuses():
    lib = _lib()
    for n, k, g, t in ((0, 300, 64, 2), (70000, 300, 64, 2), (20, 0, 64, 2), (20, 1025, 64, 2), (20, 300, 0, 2),
                       (20, 300, 1025, 2), (20, 300, 64, 0), (20, 300, 64, 9)):
        assert lib.dn_ap_match_workspace_bytes(n, k, g, t) == 0, (n, k, g, t)
    assert lib.dn_ap_match_workspace_bytes(20, 1024, 1024, 8) > 0


def test_python_entry_points_refuse_what_they_cannot_run():
    from disconet_amd import _lib as L
    from disconet_amd import postprocess as P
    dets, scs, gts = A.make(0, n_img=4)
    det, gb, gc = A.padded(dets, scs, gts)
    cpu = {k: torch.as_tensor(v) for k, v in det.items()}
    m = P.MeanAP(batch_size=2)
    with pytest.raises(L.DnError):
        m.update(cpu, torch.as_tensor(gb), torch.as_tensor(gc))
    with pytest.raises(L.DnError):
        P.match_ground_truth(cpu, torch.as_tensor(gb), torch.as_tensor(gc))
    with pytest.raises(L.DnError):
        P.match_ground_truth(det, gb, gc)                      # numpy: host_match_ground_truth is the host form
    with pytest.raises(ValueError):
        P.MeanAP(batch_size=2, iou_thrs=(0.0, 0.5))
    with pytest.raises(ValueError):
        P.MeanAP(batch_size=2, capacity=0)
    with pytest.raises(ValueError):
        P.MeanAP(batch_size=0)
    empty = m.compute()                                        # nothing accumulated: defined, zero
    assert empty["mAP@0.5"] == 0.0 and empty["mAP@0.7"] == 0.0 and empty["n_det"] == 0 and empty["per_agent"] == []
