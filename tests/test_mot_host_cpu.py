"""Tracking evaluation without a GPU: the host reference (tracking.HostClearMot) by hand on a scripted sequence and
against an independent restatement of the CLEAR metrics on scipy's assignment, the generator's ground truth, and the C
ABI of dn_mot_step: declared, bound, every refusal before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import mot_cases as C
from tests.conftest import ROOT

NAMES = ("dn_mot_state_bytes", "dn_mot_reset", "dn_mot_step")


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------
def test_header_declares_mot_entry_points_and_bindings_exist():
    from disconet_amd import _lib, tracking
    from disconet_amd.csrc import build
    raw = open(os.path.join(ROOT, "include", "disconet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None
    lib = _lib.load()
    assert lib.dn_version() >= 143
    assert "mot_eval.hip" in build.SOURCES
    assert lib.dn_mot_state_bytes(20, 256) == tracking.mot_state_bytes(20, 256) == 20 * (64 + 32 * 256)
    for n, ids in ((0, 256), (-1, 256), (65536, 256), (1, 0), (1, 1025), (1, -3)):
        assert lib.dn_mot_state_bytes(n, ids) == 0, (n, ids)


def _step(n=3, m=8, g=8, scale=4.0, thr=0.5, max_gt_ids=256, null=None):
    """dn_mot_step with fake (never dereferenced) device pointers: every refusal happens before a launch."""
    from disconet_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    names = ("rect", "id", "count", "gt_boxes", "gt_ids", "gt_count", "state", "out_match", "out_iou", "out_flags")
    p = {name: (None if name == null else fake) for name in names}
    rc = lib.dn_mot_step(p["rect"], p["id"], p["count"], n, m, p["gt_boxes"], p["gt_ids"], p["gt_count"], g, scale, thr,
                         max_gt_ids, p["state"], p["out_match"], p["out_iou"], p["out_flags"], None)
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "images"), (dict(n=-2), "images"), (dict(m=0), "M = 0"), (dict(m=129), "M = 129"), (dict(g=0), "G = 0"),
    (dict(g=1025), "G = 1025"), (dict(scale=0.0), "scale"), (dict(scale=-4.0), "scale"), (dict(scale=float("nan")), "scale"),
    (dict(scale=float("inf")), "scale"), (dict(thr=float("nan")), "iou_threshold"), (dict(thr=float("inf")), "iou_threshold"),
    (dict(thr=0.0), "iou_threshold"), (dict(thr=-0.5), "iou_threshold"), (dict(thr=1.5), "iou_threshold"),
    (dict(max_gt_ids=0), "max_gt_ids = 0"), (dict(max_gt_ids=1025), "max_gt_ids = 1025")] +
    [(dict(null=name), "null " + name) for name in ("rect", "id", "count", "gt_boxes", "gt_ids", "gt_count", "state",
                                                    "out_match", "out_iou", "out_flags")])
def test_mot_step_refuses_bad_arguments(kw, word):
    rc, msg = _step(**kw)
    assert rc == -1, (kw, rc, msg)            # DN_ERR_ARG
    assert msg.startswith("mot_step:") and word in msg, msg


def test_mot_reset_refuses_bad_arguments():
    from disconet_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    for args in ((None, 3, 256), (fake, 0, 256), (fake, 3, 0), (fake, 3, 1025)):
        assert lib.dn_mot_reset(args[0], args[1], args[2], None) == -1, args
        assert lib.dn_last_error().decode().startswith("mot_reset:")


def test_python_parameters_are_checked():
    from disconet_amd import tracking
    for cls in (tracking.ClearMot, tracking.HostClearMot):
        for kw in (dict(scale=0.0), dict(iou_threshold=float("nan")), dict(iou_threshold=0.0), dict(iou_threshold=1.1),
                   dict(max_gt_ids=0), dict(max_gt_ids=1025)):
            with pytest.raises(ValueError):
                cls(1, **kw)
        with pytest.raises(ValueError):
            cls(0)
    host = tracking.HostClearMot(1)
    tracks, gt = C.scripted_sequence()[0][0]
    with pytest.raises(ValueError):
        host.update(tracks, dict(gt, ids=gt["ids"][:, :2]))


# ---- 2. by hand ------------------------------------------------------------------------------------------------------
def test_scripted_sequence_by_hand():
    from disconet_amd import tracking
    frames, want = C.scripted_sequence()
    host = tracking.HostClearMot(1, iou_threshold=0.5, scale=1.0)
    outs = [host.update(tracks, gt) for tracks, gt in frames]
    C.check_scripted(outs, host.compute(), want)
    assert host.status_words().tolist() == [0]
    buf = host.state_bytes()
    assert len(buf) == tracking.mot_state_bytes(1, 256)
    assert buf[:40].view(np.int64).tolist() == [6, 10, 1, 8, 1] and buf[48:64].view(np.int32).tolist() == [0, 0, 0, 0]
    rec = buf[64:].view(np.int32).reshape(256, 8)
    # last, pst, frames_present, frames_matched, segments
    assert rec[:3, :5].tolist() == [[3, 3, 6, 6, 1], [2, 2, 6, 4, 2], [0, 0, 6, 0, 0]] and not rec[3:].any() and not rec[:, 5:].any()
    host.reset()
    assert not host.state_bytes().any() and len(host.state_bytes()) == len(buf)


def test_status_bits_on_the_host():
    from disconet_amd import _lib, tracking
    box, far = C.rect_box(0.0, 0.0, 4.0, 2.0), C.rect_box(50.0, 0.0, 54.0, 2.0)
    tracks = C.tracks_frame([[(1, (0.0, 0.0, 4.0, 2.0))]])
    cases = {4: [(256, box), (0, far)], 8: [(5, box), (5, far)], 2: [(0, C.T.aligned(2.0, 1.0, 0.0, 2.0)), (1, far)]}
    for bit, rows in cases.items():
        host = tracking.HostClearMot(1, scale=1.0)
        out = host.update(tracks, C.gt_frame([rows]))
        assert host.status_words().tolist() == [bit]
        host.update(tracks, C.gt_frame([[(0, box)]]))
        assert host.status_words().tolist() == [bit]               # sticky
        with pytest.raises(_lib.DnError, match="image 0"):
            host.compute()
        if bit == 8:                                               # the lower row won: matched, the other left no trace
            assert out["match"][0].tolist() == [1, -1, -1, -1] and out["flags"][0].tolist() == [5, 0, 0, 0]
            assert host.state_bytes()[:40].view(np.int64).tolist() == [2, 2, 0, 0, 0]
        else:                                                      # the bad row is no miss: FN counts the valid row only
            assert out["match"][0].tolist() == [-1, -1, -1, -1]
            assert host.state_bytes()[:40].view(np.int64).tolist() == [2, 1, 1, 1, 0]
    host = tracking.HostClearMot(1, scale=1.0)
    many = [(i, C.rect_box(8.0 * i, 0.0, 8.0 * i + 4.0, 2.0)) for i in range(130)]
    host.update(tracks, C.gt_frame([many], g=130))
    assert host.status_words().tolist() == [1]
    assert host.state_bytes()[:40].view(np.int64).tolist() == [1, 1, 0, 127, 0]


# ---- 3. against an independent restatement ---------------------------------------------------------------------------
def _clear_restated(seq, n_images, scale, thr=0.5):
    """CLEAR as the MOT benchmark's kit states it, vectorised numpy and scipy's assignment; shares no code with
    tracking.py.  seq = [(tracks, gt)] -> (TP, FP, FN, IDSW, Frag) summed over the images."""
    from scipy.optimize import linear_sum_assignment
    eps = np.finfo("float").eps
    tp = fp = fn = idsw = 0
    n_ids = 1 + max(int(gt["ids"][i, :gt["count"][i]].max()) for _, gt in seq for i in range(n_images))
    prev_id = np.full((n_images, n_ids), np.nan)              # the last track id an identity was matched to, ever
    prev_step = np.full((n_images, n_ids), np.nan)            # ... in the previous frame only
    segments = np.zeros((n_images, n_ids))
    for tracks, gt in seq:
        for i in range(n_images):
            b = gt["boxes"][i, :gt["count"][i]].astype(np.float64)
            ids = gt["ids"][i, :gt["count"][i]]
            ang = np.arctan2(b[:, 4], b[:, 5])
            ex = (np.abs(b[:, 2] * np.cos(ang)) + np.abs(b[:, 3] * np.sin(ang))) / 2
            ey = (np.abs(b[:, 2] * np.sin(ang)) + np.abs(b[:, 3] * np.cos(ang))) / 2
            g = np.stack([b[:, 0] - ex, b[:, 1] - ey, b[:, 0] + ex, b[:, 1] + ey], 1) * scale
            t = tracks["rect"][i, :tracks["count"][i]]
            tid = tracks["id"][i, :tracks["count"][i]]
            w = np.clip(np.minimum(g[:, None, 2], t[None, :, 2]) - np.maximum(g[:, None, 0], t[None, :, 0]), 0, None)
            h = np.clip(np.minimum(g[:, None, 3], t[None, :, 3]) - np.maximum(g[:, None, 1], t[None, :, 1]), 0, None)
            area = lambda r: (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
            sim = w * h / (area(g)[:, None] + area(t)[None, :] - w * h)
            score = (tid[None, :] == prev_step[i, ids][:, None]) * 1000.0 + sim
            score[sim < thr - eps] = 0
            rows, cols = linear_sum_assignment(-score)
            keep = score[rows, cols] > 0 + eps
            rows, cols = rows[keep], cols[keep]
            mid, mtid = ids[rows], tid[cols]
            before = prev_id[i, mid]
            idsw += int((np.logical_not(np.isnan(before)) & (before != mtid)).sum())
            segments[i, mid] += np.isnan(prev_step[i, mid])
            prev_id[i, mid] = mtid
            prev_step[i, :] = np.nan
            prev_step[i, mid] = mtid
            tp += len(rows)
            fn += len(ids) - len(rows)
            fp += len(tid) - len(rows)
    return tp, fp, fn, idsw, int(np.clip(segments - 1, 0, None).sum())


@pytest.mark.parametrize("seed, kw, prototype", [(1, {}, (219, 9, 69, 3, 15)), (0, dict(p_miss=0.3), (140, 9, 148, 5, 26))])
def test_host_equals_restated_clear(seed, kw, prototype):
    from disconet_amd import tracking
    seq = C.generated_sequence(16, 3, seed, **kw)
    want = _clear_restated(seq, 3, C.SCALE)
    host = tracking.HostClearMot(1, scale=C.SCALE)
    for tracks, gt in seq:
        host.update(tracks, gt)
    got = host.compute()["overall"]
    print("seed %d %s: host %s, restated %s, the issue's prototype %s" % (
        seed, kw, [got[key] for key in ("TP", "FP", "FN", "IDSW", "Frag")], want, prototype))
    assert tuple(got[key] for key in ("TP", "FP", "FN", "IDSW", "Frag")) == want
    assert want[3] >= 1 and want[4] >= 1                       # a condition of the test: switches and fragments both occur
    assert got["TP"] + got["FN"] == 16 * 3 * 6 and 0.0 < got["MOTA"] < 1.0 and 0.5 <= got["MOTP"] <= 1.0
    per_image = host.compute()["per_image"]
    assert sum(c["TP"] for c in per_image) == got["TP"] and sum(c["MT"] + c["PT"] + c["ML"] for c in per_image) == 18


def test_agents_sum_their_images_in_order():
    from disconet_amd import tracking
    seq = C.generated_sequence(16, 3, 1)
    host = tracking.HostClearMot(2, scale=C.SCALE)             # images 0, 1 -> agent 0; image 2 -> agent 1
    for tracks, gt in seq:
        host.update(tracks, gt)
    out = host.compute()
    assert len(out["per_agent"]) == 2 and len(out["per_image"]) == 3
    for key in ("TP", "FP", "FN", "IDSW", "Frag", "MT", "PT", "ML", "frames"):
        assert out["per_agent"][0][key] == out["per_image"][0][key] + out["per_image"][1][key]
        assert out["per_agent"][1][key] == out["per_image"][2][key]
        assert out["overall"][key] == sum(c[key] for c in out["per_image"])
    line = tracking.mot_line("overall", out["overall"])
    assert line.startswith("overall: MOTA ") and " IDSW %d " % out["overall"]["IDSW"] in line


# ---- 4. the generator's ground truth ---------------------------------------------------------------------------------
def test_truth_adds_gt_and_changes_nothing_else():
    from disconet_amd.synthetic import make_track_sequence
    for kw in (dict(), dict(p_miss=0.3, objects=4, false_positives=2, width=9)):
        plain = make_track_sequence(5, 2, seed=7, **kw)
        full = make_track_sequence(5, 2, seed=7, truth=True, **kw)
        objects = kw.get("objects", 6)
        for f in range(5):
            assert len(plain[f]) == 2 and len(full[f]) == 3
            det, ident, gt = full[f]
            assert sorted(det) == sorted(plain[f][0])
            for key in det:
                assert det[key].dtype == plain[f][0][key].dtype and np.array_equal(det[key], plain[f][0][key])
            assert np.array_equal(ident, plain[f][1])
            assert gt["boxes"].shape == (2, objects, 6) and gt["boxes"].dtype == np.float32
            assert gt["ids"].dtype == np.int32 and gt["count"].dtype == np.int32
            assert gt["count"].tolist() == [objects] * 2 and (gt["ids"] == np.arange(objects)[None, :]).all()
    # noise-free detections ARE the ground truth, and it moves at constant velocity
    clean = make_track_sequence(4, 2, seed=7, noise=0.0, p_miss=0.0, false_positives=0, truth=True)
    for det, ident, gt in clean:
        assert np.array_equal(det["boxes"], gt["boxes"]) and np.array_equal(ident, gt["ids"])
    step = [clean[f + 1][2]["boxes"][:, :, :2].astype(np.float64) - clean[f][2]["boxes"][:, :, :2] for f in range(3)]
    np.testing.assert_allclose(step[0], step[2], atol=1e-5)
