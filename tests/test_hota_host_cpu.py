"""HOTA without a GPU: the host reference (tracking.HostHota) by hand on scripted sequences, at the alpha edges, on the
sequence that only the global alignment score decides, against a plain restatement of the evaluation kit's algorithm on
scipy's assignment, and the C ABI of dn_hota_*: declared, bound, every refusal before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import hota_cases as H
from tests import idf_cases as I
from tests import mot_cases as C
from tests.conftest import ROOT

NAMES = ("dn_hota_state_bytes", "dn_hota_work_bytes", "dn_hota_reset", "dn_hota_step", "dn_hota_finish")
BAD_SIZES = ((0, 256, 1024, 256), (-1, 256, 1024, 256), (65536, 256, 1024, 256), (1, 0, 1024, 256), (1, 1025, 1024, 256),
             (1, -3, 1024, 256), (1, 256, 0, 256), (1, 256, 2049, 256), (1, 256, -1, 256), (1, 256, 1024, 0),
             (1, 256, 1024, 4097), (1, 256, 1024, -1))


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------
def test_header_declares_hota_entry_points_and_bindings_exist():
    from disconet_amd import _lib, tracking
    from disconet_amd.csrc import build
    raw = open(os.path.join(ROOT, "include", "disconet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None
    lib = _lib.load()
    assert lib.dn_version() >= 145
    assert "hota_eval.hip" in build.SOURCES
    per = 64 + 8 * 256 * 1024 + 9232 * 256 + 4 * (256 + 1024)
    assert lib.dn_hota_state_bytes(20, 256, 1024, 256) == tracking.hota_state_bytes(20, 256, 1024, 256) == 20 * per
    assert lib.dn_hota_state_bytes(2, 1, 1, 1) == tracking.hota_state_bytes(2, 1, 1, 1) == 2 * (64 + 8 + 9232 + 8)
    assert lib.dn_hota_state_bytes(3, 2, 1, 1) == tracking.hota_state_bytes(3, 2, 1, 1) == 3 * (64 + 16 + 9232 + 16)   # 12 -> 16
    most = 64 + 8 * 1024 * 2048 + 9232 * 4096 + 4 * 3072
    assert lib.dn_hota_state_bytes(3, 1024, 2048, 4096) == tracking.hota_state_bytes(3, 1024, 2048, 4096) == 3 * most
    work = 160 + 160 * 256 + 80 * 256 * 1024                                 # about 20 MB an image at the defaults
    assert lib.dn_hota_work_bytes(20, 256, 1024, 256) == tracking.hota_work_bytes(20, 256, 1024, 256) == 20 * work
    assert 20e6 < work < 22e6
    assert lib.dn_hota_work_bytes(1, 1024, 2048, 4096) == 160 + 160 * 4096 + 80 * 1024 * 2048
    for sizes in BAD_SIZES:
        assert lib.dn_hota_state_bytes(*sizes) == 0, sizes
        assert lib.dn_hota_work_bytes(*sizes) == 0, sizes
    assert tracking.HOTA_SLOT_BYTES == 16 + 4 * 256 + 32 * 256 == 9232


STEP_POINTERS = ("rect", "id", "count", "gt_boxes", "gt_ids", "gt_count", "state", "out_potential")


def _step(n=3, m=8, g=8, scale=4.0, max_gt_ids=256, max_track_ids=1024, max_frames=256, null=None, state=0x1000):
    """dn_hota_step with fake (never dereferenced) device pointers: every refusal happens before a launch."""
    from disconet_amd import _lib
    lib = _lib.load()
    p = {name: (None if name == null else ctypes.c_void_p(state if name == "state" else 0x1000)) for name in STEP_POINTERS}
    rc = lib.dn_hota_step(p["rect"], p["id"], p["count"], n, m, p["gt_boxes"], p["gt_ids"], p["gt_count"], g, scale,
                          max_gt_ids, max_track_ids, max_frames, p["state"], p["out_potential"], None)
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "images"), (dict(n=-2), "images"), (dict(n=65536), "images"), (dict(m=0), "M = 0"), (dict(m=129), "M = 129"),
    (dict(g=0), "G = 0"), (dict(g=1025), "G = 1025"), (dict(scale=0.0), "scale"), (dict(scale=-4.0), "scale"),
    (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"), (dict(max_gt_ids=0), "max_gt_ids = 0"),
    (dict(max_gt_ids=1025), "max_gt_ids = 1025"), (dict(max_track_ids=0), "max_track_ids = 0"),
    (dict(max_track_ids=2049), "max_track_ids = 2049"), (dict(max_frames=0), "max_frames = 0"),
    (dict(max_frames=4097), "max_frames = 4097"), (dict(state=0x1004), "8-byte aligned")] +
    [(dict(null=name), "null " + name) for name in STEP_POINTERS])
def test_hota_step_refuses_bad_arguments(kw, word):
    rc, msg = _step(**kw)
    assert rc == -1, (kw, rc, msg)            # DN_ERR_ARG
    assert msg.startswith("hota_step:") and word in msg, msg


FINISH_POINTERS = ("state", "work", "out_counts", "out_alpha_counts", "out_alpha_sums")


def _finish(n=3, max_gt_ids=256, max_track_ids=1024, max_frames=256, null=None, work=0x1000):
    from disconet_amd import _lib
    lib = _lib.load()
    p = {name: (None if name == null else ctypes.c_void_p(work if name == "work" else 0x1000)) for name in FINISH_POINTERS}
    rc = lib.dn_hota_finish(p["state"], n, max_gt_ids, max_track_ids, max_frames, p["work"], p["out_counts"],
                            p["out_alpha_counts"], p["out_alpha_sums"], None, None)    # out_match may be null
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "images"), (dict(n=-2), "images"), (dict(n=65536), "images"), (dict(max_gt_ids=0), "max_gt_ids = 0"),
    (dict(max_gt_ids=1025), "max_gt_ids = 1025"), (dict(max_track_ids=0), "max_track_ids = 0"),
    (dict(max_track_ids=2049), "max_track_ids = 2049"), (dict(max_frames=0), "max_frames = 0"),
    (dict(max_frames=4097), "max_frames = 4097"), (dict(work=0x1004), "8-byte aligned")] +
    [(dict(null=name), "null " + name) for name in FINISH_POINTERS])
def test_hota_finish_refuses_bad_arguments(kw, word):
    rc, msg = _finish(**kw)
    assert rc == -1, (kw, rc, msg)
    assert msg.startswith("hota_finish:") and word in msg, msg


def test_hota_reset_refuses_bad_arguments():
    from disconet_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    cases = [((None, 3, 256, 1024, 256), "null state")] + [((fake,) + sizes, word) for sizes, word in (
        ((0, 256, 1024, 256), "images"), ((65536, 256, 1024, 256), "images"), ((3, 0, 1024, 256), "max_gt_ids = 0"),
        ((3, 1025, 1024, 256), "max_gt_ids = 1025"), ((3, 256, 0, 256), "max_track_ids = 0"),
        ((3, 256, 2049, 256), "max_track_ids = 2049"), ((3, 256, 1024, 0), "max_frames = 0"),
        ((3, 256, 1024, 4097), "max_frames = 4097"))]
    for args, word in cases:
        assert lib.dn_hota_reset(*(args + (None,))) == -1, args
        msg = lib.dn_last_error().decode()
        assert msg.startswith("hota_reset:") and word in msg, msg


def test_python_parameters_are_checked():
    from disconet_amd import tracking
    for cls in (tracking.Hota, tracking.HostHota):
        for kw in (dict(scale=0.0), dict(scale=float("nan")), dict(max_gt_ids=0), dict(max_gt_ids=1025),
                   dict(max_track_ids=0), dict(max_track_ids=2049), dict(max_frames=0), dict(max_frames=4097)):
            with pytest.raises(ValueError):
                cls(1, **kw)
        with pytest.raises(ValueError):
            cls(0)
        made = cls(2, scale=0.25, max_gt_ids=1024, max_track_ids=2048, max_frames=4096)
        assert (made.batch_size, made.scale, made.max_gt_ids, made.max_track_ids, made.max_frames) == (2, 0.25, 1024, 2048, 4096)
        made = cls(1)
        assert (made.scale, made.max_gt_ids, made.max_track_ids, made.max_frames) == (1.0, 256, 1024, 256)
    host = tracking.HostHota(1, **H.SIZES)
    tracks, gt = C.scripted_sequence()[0][0]
    with pytest.raises(ValueError):
        host.update(tracks, dict(gt, ids=gt["ids"][:, :2]))
    with pytest.raises(ValueError):
        host.update(dict(tracks, rect=tracks["rect"][:, :2]), gt)
    host.update(tracks, gt)
    with pytest.raises(ValueError):
        host.update({key: np.concatenate([tracks[key]] * 2) for key in tracks}, {key: np.concatenate([gt[key]] * 2) for key in gt})
    assert [bit for bit, _ in tracking.HOTA_STATUS_BITS] == [1, 2, 4, 8, 16, 32, 64]
    assert tracking.HOTA_STATUS_BITS[:5] == tracking.IDF_STATUS_BITS
    alphas = tracking.hota_alphas()
    assert len(alphas) == 19 and alphas[2] == 0.15000000000000002 and alphas[9] == 0.5 and alphas[18] == 0.05 * 19


# ---- 2. by hand ------------------------------------------------------------------------------------------------------
def _host_run(frames, **params):
    from disconet_amd import tracking
    host = tracking.HostHota(1, **dict(H.SIZES, scale=1.0, **params))
    outs = [host.update(tracks, gt) for tracks, gt in frames]
    return host, outs


def test_swap_sequence_by_hand():
    host, outs = _host_run(I.swap_sequence()[0])
    H.check_swap(host)
    assert host.status_words().tolist() == [0]
    s2 = 1.0 / 1.5
    assert outs[0]["potential"][0].tolist() == [1.0 / (((1.0 + s2) + 1.0) - 1.0) + s2 / (((1.0 + s2) + s2) - s2), 0.0, 0.0, 0.0]
    assert outs[8]["potential"][0].tolist() == [0.0, 1.0, 0.0, 0.0]
    size = len(host.state_bytes())
    host.reset()
    assert not host.state_bytes().any() and len(host.state_bytes()) == size
    fin = host.finish()
    assert not fin["counts"].any() and not fin["alpha_counts"].any() and not fin["alpha_sums"].any() and not fin["match"].any()


def test_alpha_edges_by_hand():
    host, _ = _host_run([H.alpha_edge_frame()])
    H.check_alpha_edges(host)
    image = host.compute()["per_image"]
    assert image[2]["HOTA"] == 1.0 and image[2]["LocA"] == 1.0 and image[2]["HOTALocA(0)"] == 1.0
    assert image[0]["LocA(0)"] == 0.15 and image[0]["HOTA(0)"] == 1.0
    total = 0.0
    for v in [0.15] * 3 + [1.0] * 16:                                     # LocA is 1.0 where nothing matched
        total = total + v
    assert image[0]["LocA"] == total / 19.0 and image[0]["HOTA"] == 3.0 / 19.0 and image[1]["HOTA"] == 10.0 / 19.0


def test_the_global_alignment_decides():
    from disconet_amd import tracking
    frames = H.alignment_sequence()
    host, _ = _host_run(frames)
    H.check_alignment(host)
    tracks, gt = frames[4]                                                # what a matcher that ranks frame 5 by IoU would keep
    s = tracking._iou_matrix([I.A], tracks["rect"][0, :2])
    assert abs(s[0, 1] - 0.92) < 1e-15 and s[0, 0] == 1.0 / 1.5 and s[0, 1] > s[0, 0]
    by_iou = sum(1 for thr in [a - tracking.HOTA_EPS for a in tracking.hota_alphas()] if not s[0, 1] < thr)
    assert by_iou == 18                                                   # that pair would count at alphas 13..17 as well


def test_iou_matrix_is_iou_rect_element_for_element():
    from disconet_amd import tracking
    rng = np.random.default_rng(0)
    lo = rng.uniform(0.0, 8.0, (40, 2))
    g = np.concatenate([lo, lo + rng.uniform(0.5, 6.0, (40, 2))], 1)
    lo = rng.uniform(0.0, 8.0, (37, 2))
    t = np.concatenate([lo, lo + rng.uniform(0.5, 6.0, (37, 2))], 1)
    t[3, 2], t[5, 0], t[7] = np.nan, np.inf, t[8]
    t[9, 2] = t[9, 0]                                                     # no width
    got = tracking._iou_matrix(g, t)
    for a in range(40):
        for b in range(37):
            want = tracking.iou_rect(g[a], t[b]) if np.isfinite(t[b]).all() else 0.0
            assert got[a, b] == want, (a, b)
    assert got[:, [3, 5, 9]].sum() == 0.0 and (got > 0).sum() > 300
    assert tracking._iou_matrix(np.zeros((0, 4)), t).shape == (0, 37) and tracking._iou_matrix(g, np.zeros((0, 4))).shape == (40, 0)


def test_duplicate_track_id_is_counted_nowhere():
    host, outs = _host_run([H.twice_frame()])
    H.check_twice(outs[0], host)


def test_the_log_fills():
    from disconet_amd import _lib
    frames = I.swap_sequence()[0][:3]
    full, _ = _host_run(frames, max_frames=2)
    two, _ = _host_run(frames[:2], max_frames=2)
    assert full.status_words().tolist() == [32] and two.status_words().tolist() == [0]
    a, b = full.state_bytes(), two.state_bytes()
    assert a[:8].view(np.int64)[0] == 3 and b[:8].view(np.int64)[0] == 2 and np.array_equal(a[8:32], b[8:32])
    assert np.array_equal(a[36:], b[36:])
    fa, fb = full.finish(), two.finish()
    for key in ("alpha_counts", "alpha_sums", "match"):
        assert np.array_equal(C.bits(fa[key]), C.bits(fb[key]))
    assert fa["counts"].tolist() == [[3, 2, 4, 4, 2, 2, 32, 0]] and fb["counts"].tolist() == [[2, 2, 4, 4, 2, 2, 0, 0]]
    with pytest.raises(_lib.DnError, match="image 0.*log was full"):
        full.compute()


@pytest.mark.parametrize("case", range(9))
def test_status_bits_on_the_host(case):
    from disconet_amd import _lib, tracking
    bit, word, frames, params = H.status_cases()[case]
    host = tracking.HostHota(1, scale=1.0, **params)
    host.update(*frames[0])
    if bit != 32:
        assert host.status_words().tolist() == [bit]
    for tracks, gt in frames[1:]:
        host.update(tracks, gt)
    assert host.status_words().tolist() == [bit]                   # alone, and sticky
    assert host.finish()["counts"][0, 6] == bit
    with pytest.raises(_lib.DnError, match="image 0.*" + word):
        host.compute()
    host.reset()
    assert host.status_words().tolist() == [0] and not host.state_bytes().any()


def test_state_layout():
    from disconet_amd import tracking
    g, t, f = 5, 3, 2                                              # 4 (g + t) = 32: no padding; the sizes are not powers of two
    host = tracking.HostHota(1, scale=1.0, max_gt_ids=g, max_track_ids=t, max_frames=f)
    tracks, gt = I.swap_sequence()[0][0]
    host.update(tracks, gt)
    buf = host.state_bytes()
    assert len(buf) == tracking.hota_state_bytes(1, g, t, f) == 64 + 8 * 15 + 9232 * 2 + 32
    assert buf[:32].view(np.int64).tolist() == [1, 1, 2, 2] and not buf[32:64].any()
    pot = buf[64:64 + 120].view(np.float64).reshape(g, t)
    assert np.array_equal(pot, host.potential_matrix(0)) and pot[0, 0] > 0 and pot[0, 1] > 0 and int((pot != 0).sum()) == 2
    slot = buf[184:184 + 9232]
    assert slot[:16].view(np.int32).tolist() == [2, 2, 0, 0]
    assert slot[16:528].view(np.int32)[:3].tolist() == [0, 1, 0] and slot[528:1040].view(np.int32)[:3].tolist() == [1, 2, 0]
    assert slot[1040:5136].view(np.float64)[:9].tolist() == [0.0, 0.0, 1.0, 1.0, 10.0, 0.0, 12.0, 2.0, 0.0]
    assert slot[5136:].view(np.float64)[:9].tolist() == [0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.5, 1.0, 0.0]
    assert not buf[184 + 9232:184 + 2 * 9232].any()                # the second slot is not written yet
    tail = buf[184 + 2 * 9232:].view(np.int32)
    assert tail.tolist() == [1, 1, 0, 0, 0, 1, 1, 0]
    odd = tracking.HostHota(2, scale=1.0, max_gt_ids=2, max_track_ids=1, max_frames=1)      # 4 (g + t) = 12: padded to 16
    odd.update({key: np.concatenate([tracks[key]] * 2) for key in tracks}, {key: np.concatenate([gt[key]] * 2) for key in gt})
    per = 64 + 16 + 9232 + 16
    assert len(odd.state_bytes()) == 2 * per and odd.status_words().tolist() == [16, 16]    # track id 2 > max_track_ids
    assert np.array_equal(odd.state_bytes()[:per], odd.state_bytes()[per:])


# ---- 3. against a plain restatement of the kit's algorithm -----------------------------------------------------------
def _hota_restated(seq, image, scale):
    """HOTA as the MOT benchmark's kit states it, vectorised numpy and scipy's assignment; shares no code with
    tracking.py.  seq = [(tracks, gt)] -> per-alpha arrays TP, FN, FP, loc, assa, assre, asspr, the number of terms of each
    sum, HOTA, and the frames whose optimum is not unique."""
    from scipy.optimize import linear_sum_assignment
    eps = np.finfo("float").eps
    alphas = np.arange(0.05, 0.99, 0.05)
    gt_all = np.unique(np.concatenate([gt["ids"][image, :gt["count"][image]] for _, gt in seq]))
    tr_all = np.unique(np.concatenate([tracks["id"][image, :tracks["count"][image]] for tracks, _ in seq]))
    n_gt, n_tr, n_a = len(gt_all), len(tr_all), len(alphas)
    frames = []
    for tracks, gt in seq:
        b = gt["boxes"][image, :gt["count"][image]].astype(np.float64)
        ids = np.searchsorted(gt_all, gt["ids"][image, :gt["count"][image]])
        ang = np.arctan2(b[:, 4], b[:, 5])
        ex = (np.abs(b[:, 2] * np.cos(ang)) + np.abs(b[:, 3] * np.sin(ang))) / 2
        ey = (np.abs(b[:, 2] * np.sin(ang)) + np.abs(b[:, 3] * np.cos(ang))) / 2
        g = np.stack([b[:, 0] - ex, b[:, 1] - ey, b[:, 0] + ex, b[:, 1] + ey], 1) * scale
        t = tracks["rect"][image, :tracks["count"][image]]
        tid = np.searchsorted(tr_all, tracks["id"][image, :tracks["count"][image]])
        w = np.clip(np.minimum(g[:, None, 2], t[None, :, 2]) - np.maximum(g[:, None, 0], t[None, :, 0]), 0, None)
        h = np.clip(np.minimum(g[:, None, 3], t[None, :, 3]) - np.maximum(g[:, None, 1], t[None, :, 1]), 0, None)
        area = lambda r: (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])
        frames.append((ids, tid, w * h / (area(g)[:, None] + area(t)[None, :] - w * h)))
    potential, gt_seen, tr_seen = np.zeros((n_gt, n_tr)), np.zeros((n_gt, 1)), np.zeros((1, n_tr))
    for ids, tid, sim in frames:
        denom = sim.sum(0)[None, :] + sim.sum(1)[:, None] - sim
        sim_iou = np.zeros_like(sim)
        mask = denom > 0 + eps
        sim_iou[mask] = sim[mask] / denom[mask]
        potential[ids[:, None], tid[None, :]] += sim_iou
        gt_seen[ids] += 1
        tr_seen[0, tid] += 1
    align = potential / (gt_seen + tr_seen - potential)
    tp, fn, fp, loc = np.zeros(n_a), np.zeros(n_a), np.zeros(n_a), np.zeros(n_a)
    matched = [np.zeros((n_gt, n_tr)) for _ in alphas]
    tied = []
    for f, (ids, tid, sim) in enumerate(frames):
        if len(ids) == 0:
            fp += len(tid)
            continue
        if len(tid) == 0:
            fn += len(ids)
            continue
        score = align[ids[:, None], tid[None, :]] * sim
        rows, cols = linear_sum_assignment(-score)
        best = score[rows, cols].sum()
        for r, c in zip(rows, cols):                                # is the optimum unique?  forbid each of its pairs in turn
            if score[r, c] > 0:
                other = score.copy()
                other[r, c] = -1.0
                r2, c2 = linear_sum_assignment(-other)
                if not other[r2, c2].sum() < best - 1e-12:
                    tied.append(f + 1)
        for a, alpha in enumerate(alphas):
            ok = sim[rows, cols] >= alpha - eps
            ar, ac = rows[ok], cols[ok]
            tp[a] += len(ar)
            fn[a] += len(ids) - len(ar)
            fp[a] += len(tid) - len(ar)
            if len(ar):
                loc[a] += sim[ar, ac].sum()
                matched[a][ids[ar], tid[ac]] += 1
    out = {"TP": tp, "FN": fn, "FP": fp, "loc": loc, "tied": tied, "cells": [int((m > 0).sum()) for m in matched]}
    for key, seen in (("assa", None), ("assre", gt_seen), ("asspr", tr_seen)):
        out[key] = np.asarray([np.sum(m * (m / np.maximum(1, gt_seen + tr_seen - m if seen is None else seen)))
                               for m in matched])
    det_a = tp / np.maximum(1, tp + fn + fp)
    out["HOTA"] = float(np.mean(np.sqrt(det_a * out["assa"] / np.maximum(1, tp))))
    return out


# the issue's prototype at scale 4, alphas 0.05 / 0.50 / 0.95: (TP, FN, FP) and HOTA as it quotes it, to four places
PROTOTYPE = [((135, 45, 3), (135, 45, 3), (119, 61, 19), 0.7172), ((141, 39, 3), (141, 39, 3), (128, 52, 16), 0.7825),
             ((136, 44, 3), (136, 44, 3), (127, 53, 12), 0.7500), ((152, 28, 3), (152, 28, 3), (125, 55, 30), 0.8321)]


def test_host_equals_the_kits_algorithm():
    """TP / FN / FP equal at all 19 alphas of all 4 images; every floating sum within (terms - 1) 2^-52 relative, the bound
    for two summation orders of non-negative, identically rounded terms.  The issue's HOTA figures are quoted to four
    places: image 1 is 0.78244968 in HostHota AND in the restatement below (they agree to 3e-16), which the issue prints as
    0.7825, so the quoted figures are held to one unit of their last place."""
    from disconet_amd import tracking
    assert C.SCALE == 4.0                                                # the scale the prototype's figures hold at
    seq = C.generated_sequence(30, 4, 0)
    host = tracking.HostHota(1, scale=C.SCALE)
    for tracks, gt in seq:
        host.update(tracks, gt)
    images = host.compute()["per_image"]
    for image in range(4):
        want, got = _hota_restated(seq, image, C.SCALE), images[image]
        assert want["tied"] == [], "image %d: the optimum of frames %s is not unique" % (image, want["tied"])
        for key in ("TP", "FN", "FP"):
            assert got[key] == want[key].tolist(), (image, key)
        print("image %d: TP %s HOTA %.8f (the kit's form %.8f, the issue's prototype %.4f)" % (
            image, [got["TP"][k] for k in (0, 9, 18)], got["HOTA"], want["HOTA"], PROTOTYPE[image][3]))
        for k in range(19):
            terms = {"loc": got["TP"][k], "assa": want["cells"][k], "assre": want["cells"][k], "asspr": want["cells"][k]}
            for key, n_terms in terms.items():
                bound = max(n_terms - 1, 0) * 2.0 ** -52
                assert abs(got[key][k] - want[key][k]) <= bound * want[key][k], (image, k, key, got[key][k], want[key][k])
        for slot, k in enumerate((0, 9, 18)):
            assert (got["TP"][k], got["FN"][k], got["FP"][k]) == PROTOTYPE[image][slot], (image, k)
        assert abs(got["HOTA"] - want["HOTA"]) < 1e-14 and abs(got["HOTA"] - PROTOTYPE[image][3]) < 1e-4
        assert got["GT_Dets"] == 180 and got["GT_IDs"] == 6


def test_finish_reads_the_state_only():
    from disconet_amd import tracking
    seq = C.generated_sequence(16, 3, 1)
    host, other = tracking.HostHota(1, scale=C.SCALE, **H.SIZES), tracking.HostHota(1, scale=C.SCALE, **H.SIZES)
    for f, (tracks, gt) in enumerate(seq):
        host.update(tracks, gt)
        other.update(tracks, gt)
        if f == 7:
            before = host.state_bytes()
            middle = host.compute()["overall"]
            assert np.array_equal(host.state_bytes(), before) and middle["frames"] == 3 * 8 == middle["logged"]
    assert np.array_equal(host.state_bytes(), other.state_bytes())
    assert host.compute() == other.compute()


# ---- 4. the levels ---------------------------------------------------------------------------------------------------
def test_agents_add_their_images_in_order():
    from disconet_amd import tracking
    seq = C.generated_sequence(16, 3, 1)
    host = tracking.HostHota(2, scale=C.SCALE, **H.SIZES)      # images 0, 1 -> agent 0; image 2 -> agent 1
    for tracks, gt in seq:
        host.update(tracks, gt)
    out = host.compute()
    assert len(out["per_agent"]) == 2 and len(out["per_image"]) == 3
    image, agent, o = out["per_image"], out["per_agent"], out["overall"]
    for key in ("frames", "logged", "GT_Dets", "Dets", "GT_IDs", "IDs"):
        assert agent[0][key] == image[0][key] + image[1][key] and agent[1][key] == image[2][key]
        assert o[key] == sum(c[key] for c in image)
    for k in range(19):
        for key in ("TP", "FN", "FP"):
            assert agent[0][key][k] == image[0][key][k] + image[1][key][k] and o[key][k] == sum(c[key][k] for c in image)
        for key in ("loc", "assa", "assre", "asspr"):
            assert agent[0][key][k] == image[0][key][k] + image[1][key][k]
            assert o[key][k] == (image[0][key][k] + image[1][key][k]) + image[2][key][k]
        tp, fn, fp = o["TP"][k], o["FN"][k], o["FP"][k]
        per = o["per_alpha"]
        assert per["DetA"][k] == tp / (tp + fn + fp) and per["DetRe"][k] == tp / (tp + fn) and per["DetPr"][k] == tp / (tp + fp)
        assert per["AssA"][k] == o["assa"][k] / tp and per["LocA"][k] == o["loc"][k] / tp
        assert per["HOTA"][k] == float(np.sqrt(per["DetA"][k] * per["AssA"][k]))
    mean = 0.0
    for v in o["per_alpha"]["HOTA"]:
        mean = mean + v
    assert o["HOTA"] == mean / 19.0 and o["HOTA(0)"] == o["per_alpha"]["HOTA"][0]
    assert o["HOTALocA(0)"] == o["HOTA(0)"] * o["LocA(0)"] and 0.0 < o["HOTA"] < 1.0
    line = tracking.hota_line("overall", o)
    assert line == ("overall: HOTA %.4f DetA %.4f AssA %.4f DetRe %.4f DetPr %.4f AssRe %.4f AssPr %.4f LocA %.4f HOTA(0) %.4f "
                    "LocA(0) %.4f HOTALocA(0) %.4f Dets %d GT_Dets %d IDs %d GT_IDs %d" % (
                        o["HOTA"], o["DetA"], o["AssA"], o["DetRe"], o["DetPr"], o["AssRe"], o["AssPr"], o["LocA"], o["HOTA(0)"],
                        o["LocA(0)"], o["HOTALocA(0)"], o["Dets"], o["GT_Dets"], o["IDs"], o["GT_IDs"]))
    empty = tracking.hota_figures({"counts": np.zeros((2, 8), dtype=np.int64), "alpha_counts": np.zeros((2, 19, 4), dtype=np.int64),
                                   "alpha_sums": np.zeros((2, 19, 4))}, 1)["overall"]
    assert empty["HOTA"] == 0.0 and empty["DetA"] == 0.0 and empty["AssA"] == 0.0 and empty["LocA"] == 1.0
