"""Identity metrics without a GPU: the host reference (tracking.HostIdentity) by hand on scripted sequences, against an
independent restatement of the evaluation kit's form on scipy's assignment, on seeded matrices whose best assignment a
row-by-row pick misses, and the C ABI of dn_idf_*: declared, bound, every refusal before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import idf_cases as I
from tests import mot_cases as C
from tests.conftest import ROOT

NAMES = ("dn_idf_state_bytes", "dn_idf_reset", "dn_idf_step", "dn_idf_finish")


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------
def test_header_declares_idf_entry_points_and_bindings_exist():
    from disconet_amd import _lib, tracking
    from disconet_amd.csrc import build
    raw = open(os.path.join(ROOT, "include", "disconet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None
    lib = _lib.load()
    assert lib.dn_version() >= 144
    assert "idf_eval.hip" in build.SOURCES
    assert lib.dn_idf_state_bytes(20, 256, 1024) == tracking.idf_state_bytes(20, 256, 1024) == 20 * 1053760
    assert lib.dn_idf_state_bytes(2, 1, 1) == tracking.idf_state_bytes(2, 1, 1) == 2 * 76
    assert lib.dn_idf_state_bytes(3, 1024, 2048) == tracking.idf_state_bytes(3, 1024, 2048) == 3 * (64 + 4 * (3072 + 2 ** 21))
    for n, ids, tids in ((0, 256, 1024), (-1, 256, 1024), (65536, 256, 1024), (1, 0, 1024), (1, 1025, 1024), (1, -3, 1024),
                         (1, 256, 0), (1, 256, 2049), (1, 256, -1)):
        assert lib.dn_idf_state_bytes(n, ids, tids) == 0, (n, ids, tids)


STEP_POINTERS = ("rect", "id", "count", "gt_boxes", "gt_ids", "gt_count", "state", "out_overlaps")


def _step(n=3, m=8, g=8, scale=4.0, thr=0.5, max_gt_ids=256, max_track_ids=1024, null=None):
    """dn_idf_step with fake (never dereferenced) device pointers: every refusal happens before a launch."""
    from disconet_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    p = {name: (None if name == null else fake) for name in STEP_POINTERS}
    rc = lib.dn_idf_step(p["rect"], p["id"], p["count"], n, m, p["gt_boxes"], p["gt_ids"], p["gt_count"], g, scale, thr,
                         max_gt_ids, max_track_ids, p["state"], p["out_overlaps"], None)
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "images"), (dict(n=-2), "images"), (dict(n=65536), "images"), (dict(m=0), "M = 0"), (dict(m=129), "M = 129"),
    (dict(g=0), "G = 0"), (dict(g=1025), "G = 1025"), (dict(scale=0.0), "scale"), (dict(scale=-4.0), "scale"),
    (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"), (dict(thr=float("nan")), "iou_threshold"),
    (dict(thr=float("inf")), "iou_threshold"), (dict(thr=0.0), "iou_threshold"), (dict(thr=-0.5), "iou_threshold"),
    (dict(thr=1.5), "iou_threshold"), (dict(max_gt_ids=0), "max_gt_ids = 0"), (dict(max_gt_ids=1025), "max_gt_ids = 1025"),
    (dict(max_track_ids=0), "max_track_ids = 0"), (dict(max_track_ids=2049), "max_track_ids = 2049")] +
    [(dict(null=name), "null " + name) for name in STEP_POINTERS])
def test_idf_step_refuses_bad_arguments(kw, word):
    rc, msg = _step(**kw)
    assert rc == -1, (kw, rc, msg)            # DN_ERR_ARG
    assert msg.startswith("idf_step:") and word in msg, msg


def _finish(n=3, max_gt_ids=256, max_track_ids=1024, null=None):
    from disconet_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    p = {name: (None if name == null else fake) for name in ("state", "out_counts", "out_match")}
    rc = lib.dn_idf_finish(p["state"], n, max_gt_ids, max_track_ids, p["out_counts"], p["out_match"], None)
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "images"), (dict(n=-2), "images"), (dict(n=65536), "images"), (dict(max_gt_ids=0), "max_gt_ids = 0"),
    (dict(max_gt_ids=1025), "max_gt_ids = 1025"), (dict(max_track_ids=0), "max_track_ids = 0"),
    (dict(max_track_ids=2049), "max_track_ids = 2049"), (dict(null="state"), "null state"),
    (dict(null="out_counts"), "null out_counts"), (dict(null="out_match"), "null out_match")])
def test_idf_finish_refuses_bad_arguments(kw, word):
    rc, msg = _finish(**kw)
    assert rc == -1, (kw, rc, msg)
    assert msg.startswith("idf_finish:") and word in msg, msg


def test_idf_reset_refuses_bad_arguments():
    from disconet_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    for args, word in (((None, 3, 256, 1024), "null state"), ((fake, 0, 256, 1024), "images"), ((fake, -2, 256, 1024), "images"),
                       ((fake, 65536, 256, 1024), "images"), ((fake, 3, 0, 1024), "max_gt_ids = 0"),
                       ((fake, 3, 1025, 1024), "max_gt_ids = 1025"), ((fake, 3, 256, 0), "max_track_ids = 0"),
                       ((fake, 3, 256, 2049), "max_track_ids = 2049")):
        assert lib.dn_idf_reset(args[0], args[1], args[2], args[3], None) == -1, args
        msg = lib.dn_last_error().decode()
        assert msg.startswith("idf_reset:") and word in msg, msg


def test_python_parameters_are_checked():
    from disconet_amd import tracking
    for cls in (tracking.Identity, tracking.HostIdentity):
        for kw in (dict(scale=0.0), dict(iou_threshold=float("nan")), dict(iou_threshold=0.0), dict(iou_threshold=1.1),
                   dict(max_gt_ids=0), dict(max_gt_ids=1025), dict(max_track_ids=0), dict(max_track_ids=2049)):
            with pytest.raises(ValueError):
                cls(1, **kw)
        with pytest.raises(ValueError):
            cls(0)
        made = cls(2, iou_threshold=1.0, scale=0.25, max_gt_ids=1024, max_track_ids=2048)     # the whole product is allowed
        assert (made.batch_size, made.iou_threshold, made.scale, made.max_gt_ids, made.max_track_ids) == (2, 1.0, 0.25, 1024, 2048)
    host = tracking.HostIdentity(1)
    tracks, gt = C.scripted_sequence()[0][0]
    with pytest.raises(ValueError):
        host.update(tracks, dict(gt, ids=gt["ids"][:, :2]))
    with pytest.raises(ValueError):
        host.update(dict(tracks, rect=tracks["rect"][:, :2]), gt)
    host.update(tracks, gt)
    two = {key: np.concatenate([gt[key]] * 2) for key in gt}
    with pytest.raises(ValueError):
        host.update({key: np.concatenate([tracks[key]] * 2) for key in tracks}, two)
    assert [bit for bit, _ in tracking.IDF_STATUS_BITS] == [1, 2, 4, 8, 16]
    assert tracking.IDF_STATUS_BITS[:4] == tracking.MOT_STATUS_BITS


# ---- 2. by hand ------------------------------------------------------------------------------------------------------
def test_scripted_sequence_by_hand():
    from disconet_amd import tracking
    frames, _ = C.scripted_sequence()
    host = tracking.HostIdentity(1, iou_threshold=0.5, scale=1.0)
    outs = [host.update(tracks, gt) for tracks, gt in frames]
    I.check_scripted(outs, host)
    assert host.status_words().tolist() == [0]
    size = len(host.state_bytes())
    host.reset()
    assert not host.state_bytes().any() and len(host.state_bytes()) == size
    assert host.finish()["counts"].tolist() == [[0] * 8] and not host.finish()["match"].any()


def test_swap_by_hand_needs_the_global_assignment():
    from disconet_amd import tracking
    frames, want = I.swap_sequence()
    host = tracking.HostIdentity(1, scale=1.0)
    for tracks, gt in frames:
        host.update(tracks, gt)
    I.check_swap(host, want)
    assert I.greedy_total(np.asarray(want["pairs"])) == 5


def test_the_same_track_id_twice_in_one_frame():
    from disconet_amd import tracking
    host = tracking.HostIdentity(1, scale=1.0)
    I.check_twice(host.update(*I.twice_frame()), host)


def test_finish_reads_the_state_only():
    from disconet_amd import tracking
    seq = C.generated_sequence(16, 3, 1)
    host, other = tracking.HostIdentity(1, scale=C.SCALE), tracking.HostIdentity(1, scale=C.SCALE)
    for f, (tracks, gt) in enumerate(seq):
        host.update(tracks, gt)
        other.update(tracks, gt)
        if f == 7:
            before = host.state_bytes()
            middle = host.compute()["overall"]
            assert np.array_equal(host.state_bytes(), before) and middle["frames"] == 3 * 8
    assert np.array_equal(host.state_bytes(), other.state_bytes())


@pytest.mark.parametrize("case", range(7))
def test_status_bits_on_the_host(case):
    from disconet_amd import _lib, tracking
    bit, word, tracks, gt = I.status_cases()[case]
    host = tracking.HostIdentity(1, scale=1.0)
    out = host.update(tracks, gt)
    assert host.status_words().tolist() == [bit]
    host.update(*I.clean_frame(g=gt["ids"].shape[1]))
    assert host.status_words().tolist() == [bit]                   # sticky
    assert host.finish()["counts"][0, 6] == bit
    with pytest.raises(_lib.DnError, match="image 0.*" + word):
        host.compute()
    header = host.state_bytes()[:24].view(np.int64).tolist()
    if bit == 16:                                                  # the bad row is counted nowhere; the good one is
        assert header == [2, 2, 2] and out["overlaps"][0].tolist() == [1, 0, 0, 0]
        assert int(host.counts_matrix(0).sum()) == 2 and host.counts_matrix(0)[0, 0] == 2
    elif bit == 8:                                                 # the lower row won, the other left no trace
        assert header == [2, 2, 2] and out["overlaps"][0].tolist() == [1, 0, 0, 0]
    elif bit == 1:
        assert header == [2, 129, 2] and out["overlaps"][0, :2].tolist() == [1, 0]
    else:                                                          # the bad row is no ground truth: only the valid one counts
        assert header == [2, 2, 2] and not out["overlaps"].any()
    host.reset()
    assert host.status_words().tolist() == [0] and not host.state_bytes().any()


# ---- 3. against an independent restatement ---------------------------------------------------------------------------
def _identity_restated(seq, image, scale, thr=0.5):
    """The identity metrics as the MOT benchmark's kit states them, vectorised numpy and scipy's assignment; shares no
    code with tracking.py.  seq = [(tracks, gt)] -> (IDTP, IDFP, IDFN, GT_IDs, IDs) of one image."""
    from scipy.optimize import linear_sum_assignment
    eps = np.finfo("float").eps
    gt_all = np.unique(np.concatenate([gt["ids"][image, :gt["count"][image]] for _, gt in seq]))
    tr_all = np.unique(np.concatenate([tracks["id"][image, :tracks["count"][image]] for tracks, _ in seq]))
    n_gt, n_tr = len(gt_all), len(tr_all)
    potential = np.zeros((n_gt, n_tr))
    gt_seen, tr_seen = np.zeros(n_gt), np.zeros(n_tr)
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
        sim = w * h / (area(g)[:, None] + area(t)[None, :] - w * h)
        hit_g, hit_t = np.nonzero(sim >= thr - eps)
        potential[ids[hit_g], tid[hit_t]] += 1
        gt_seen[ids] += 1
        tr_seen[tid] += 1
    size = n_gt + n_tr
    fn_mat, fp_mat = np.zeros((size, size)), np.zeros((size, size))
    fp_mat[n_gt:, :n_tr] = 1e10
    fn_mat[:n_gt, n_tr:] = 1e10
    for i in range(n_gt):
        fn_mat[i, :n_tr] = gt_seen[i]
        fn_mat[i, n_tr + i] = gt_seen[i]
    for j in range(n_tr):
        fp_mat[:n_gt, j] = tr_seen[j]
        fp_mat[n_gt + j, j] = tr_seen[j]
    fn_mat[:n_gt, :n_tr] -= potential
    fp_mat[:n_gt, :n_tr] -= potential
    rows, cols = linear_sum_assignment(fn_mat + fp_mat)
    idfn, idfp = int(fn_mat[rows, cols].sum()), int(fp_mat[rows, cols].sum())
    return int(gt_seen.sum()) - idfn, idfp, idfn, n_gt, n_tr


@pytest.mark.parametrize("seed, kw, prototype", [(1, {}, (212, 16, 76, 0.821705)),
                                                 (0, dict(p_miss=0.3), (132, 17, 156, 0.604119))])
def test_host_equals_the_kits_form(seed, kw, prototype):
    from disconet_amd import tracking
    seq = C.generated_sequence(16, 3, seed, **kw)
    want = np.sum([_identity_restated(seq, image, C.SCALE) for image in range(3)], axis=0).tolist()
    host = tracking.HostIdentity(1, scale=C.SCALE)
    for tracks, gt in seq:
        host.update(tracks, gt)
    got = host.compute()["overall"]
    figures = [got[key] for key in ("IDTP", "IDFP", "IDFN", "GT_IDs", "IDs")]
    print("seed %d %s: host %s IDF1 %.6f, the kit's form %s, the issue's prototype %s" % (
        seed, kw, figures, got["IDF1"], want, prototype))
    assert figures == want
    assert tuple(figures[:3]) == prototype[:3] and round(got["IDF1"], 6) == prototype[3]
    assert got["GT_Dets"] == 16 * 3 * 6 and got["Dets"] == figures[0] + figures[1]


def test_long_sequence_identities_covered_by_several_tracks_in_turn():
    from disconet_amd import tracking
    seq = C.generated_sequence(60, 2, 3, p_miss=0.3)
    host = tracking.HostIdentity(1, scale=C.SCALE)
    for tracks, gt in seq:
        host.update(tracks, gt)
    images = host.compute()["per_image"]
    for image, expected in enumerate(((82, 53, 278, 6, 22), (100, 56, 260, 6, 20))):
        got = tuple(images[image][key] for key in ("IDTP", "IDFP", "IDFN", "GT_IDs", "IDs"))
        want = _identity_restated(seq, image, C.SCALE)
        print("image %d: host %s, the kit's form %s, the issue's figures %s" % (image, got, want, expected))
        assert got == want == expected
        assert got[4] > 2 * got[3]                                 # a condition of the test: several tracks per identity


# ---- 4. a real assignment, at sizes past the kernel's lane count ------------------------------------------------------
@pytest.mark.parametrize("large", [False, True])
def test_seeded_matrices_need_a_real_assignment(large):
    from disconet_amd import tracking
    shapes, matrices, frames, params = I.matrix_cases(large)
    host = tracking.HostIdentity(1, **params)
    for tracks, gt in frames:
        host.update(tracks, gt)
    assert host.status_words().tolist() == [0, 0]
    I.check_matrix_run(host, shapes, matrices)
    assert [s[0] > s[1] for s in shapes] == [True, False]          # both orientations: more identities, more track ids


# ---- 5. the levels ---------------------------------------------------------------------------------------------------
def test_agents_sum_their_images_in_order():
    from disconet_amd import tracking
    seq = C.generated_sequence(16, 3, 1)
    host = tracking.HostIdentity(2, scale=C.SCALE)             # images 0, 1 -> agent 0; image 2 -> agent 1
    for tracks, gt in seq:
        host.update(tracks, gt)
    out = host.compute()
    assert len(out["per_agent"]) == 2 and len(out["per_image"]) == 3
    for key in ("IDTP", "IDFP", "IDFN", "Dets", "GT_Dets", "IDs", "GT_IDs", "frames"):
        assert out["per_agent"][0][key] == out["per_image"][0][key] + out["per_image"][1][key]
        assert out["per_agent"][1][key] == out["per_image"][2][key]
        assert out["overall"][key] == sum(c[key] for c in out["per_image"])
    o = out["overall"]
    assert o["IDF1"] == 2 * o["IDTP"] / (2 * o["IDTP"] + o["IDFP"] + o["IDFN"])
    assert o["IDP"] == o["IDTP"] / o["Dets"] and o["IDR"] == o["IDTP"] / o["GT_Dets"]
    line = tracking.idf_line("overall", o)
    assert line == "overall: IDF1 %.4f IDP %.4f IDR %.4f IDTP %d IDFP %d IDFN %d Dets %d GT_Dets %d IDs %d GT_IDs %d" % (
        o["IDF1"], o["IDP"], o["IDR"], o["IDTP"], o["IDFP"], o["IDFN"], o["Dets"], o["GT_Dets"], o["IDs"], o["GT_IDs"])
    assert tuple(tracking.IDF_FIGURES) == ("IDF1", "IDP", "IDR", "IDTP", "IDFP", "IDFN", "Dets", "GT_Dets", "IDs", "GT_IDs")
    empty = tracking.idf_figures(np.zeros((2, 8), dtype=np.int64), 1)["overall"]
    assert empty["IDF1"] == 0.0 and empty["IDP"] == 0.0 and empty["IDR"] == 0.0
