"""The tracker without a GPU: the host reference (tracking.HostSort) -- its Hungarian step against scipy, the SORT
lifecycle by hand, the shortcut and the assignment where they differ, the sequence generator -- and the C ABI of
dn_track_step: declared, bound, every refusal before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import track_cases as C
from tests.conftest import ROOT

NAMES = ("dn_track_state_bytes", "dn_track_reset", "dn_track_step")


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------
def test_header_declares_track_entry_points_and_bindings_exist():
    from disconet_amd import _lib, tracking
    raw = open(os.path.join(ROOT, "include", "disconet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.load(), name) is not None
    lib = _lib.load()
    assert lib.dn_version() >= 142
    from disconet_amd.csrc import build
    assert "track.hip" in build.SOURCES
    assert lib.dn_track_state_bytes(20, 128) == tracking.state_bytes(20, 128) == 20 * (64 + 480 * 128)
    assert lib.dn_track_state_bytes(1, 0) == 0 and lib.dn_track_state_bytes(1, 129) == 0 and lib.dn_track_state_bytes(0, 4) == 0


def _step(k=8, max_tracks=128, max_age=1, min_hits=3, thr=0.3, scale=4.0, n=3, null=None):
    """dn_track_step with fake (never dereferenced) device pointers: every refusal happens before a launch."""
    from disconet_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    names = ("boxes", "scores", "count", "state", "rect", "id", "det", "score", "out_count", "det_track")
    p = {name: (None if name == null else fake) for name in names}
    rc = lib.dn_track_step(p["boxes"], p["scores"], p["count"], n, k, max_tracks, max_age, min_hits, thr, scale, p["state"],
                           p["rect"], p["id"], p["det"], p["score"], p["out_count"], p["det_track"], None)
    return rc, lib.dn_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(k=0), "K = 0"), (dict(k=1025), "K = 1025"), (dict(max_tracks=0), "max_tracks = 0"),
    (dict(max_tracks=129), "max_tracks = 129"), (dict(scale=0.0), "scale"), (dict(scale=-4.0), "scale"),
    (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"), (dict(thr=float("nan")), "iou_threshold"),
    (dict(thr=float("inf")), "iou_threshold"), (dict(thr=-0.1), "iou_threshold"), (dict(n=0), "images"),
    (dict(max_age=-1), "max_age"), (dict(min_hits=-1), "min_hits"), (dict(null="state"), "null"),
    (dict(null="det_track"), "null")])
def test_track_step_refuses_bad_arguments(kw, word):
    rc, msg = _step(**kw)
    assert rc == -1, (kw, rc, msg)            # DN_ERR_ARG
    assert msg.startswith("track_step:") and word in msg, msg


def test_track_reset_refuses_bad_arguments():
    from disconet_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    assert lib.dn_track_reset(None, 3, 8, None) == -1
    assert lib.dn_track_reset(fake, 0, 8, None) == -1
    assert lib.dn_track_reset(fake, 3, 0, None) == -1 and lib.dn_track_reset(fake, 3, 129, None) == -1


def test_python_parameters_are_checked():
    from disconet_amd import tracking
    for cls in (tracking.Sort, tracking.HostSort):
        for kw in (dict(scale=0.0), dict(iou_threshold=float("nan")), dict(max_tracks=0), dict(max_tracks=129),
                   dict(max_age=-1), dict(min_hits=-1)):
            with pytest.raises(ValueError):
                cls(**kw)


# ---- 2. the Hungarian step against scipy ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (7, 3), (70, 67), (128, 128)])
def test_hungarian_total_equals_scipy(shape):
    so = pytest.importorskip("scipy.optimize")
    from disconet_amd import tracking
    rng = np.random.RandomState(17 + shape[0] * 131 + shape[1])
    for trial in range(3):
        iou = rng.uniform(0.0, 1.0, shape)
        if trial == 2:
            iou[rng.uniform(size=shape) < 0.6] = 0.0          # the sparse matrices a tracker sees; many equal entries
        pairs = tracking.hungarian_max(iou)
        assert len(pairs) == min(shape)
        assert len({t for t, _ in pairs}) == len(pairs) and len({d for _, d in pairs}) == len(pairs)
        r, c = so.linear_sum_assignment(-iou)
        got, want = sum(iou[t, d] for t, d in pairs), iou[r, c].sum()
        print("shape %s trial %d: total %.15g, scipy %.15g" % (shape, trial, got, want))
        assert abs(got - want) <= 1e-12


# ---- 3. the shortcut and the assignment disagree where they should ---------------------------------------------------
def test_shortcut_and_assignment_disagree_where_they_should():
    from disconet_amd import tracking
    # one pair at 0.35 against two crossing pairs at 0.29 each: a single entry above 0.3, the shortcut keeps it
    small = np.array([[0.35, 0.29], [0.29, 0.0]])
    match, path = tracking.associate(small, 0.3)
    assert path == "shortcut" and match.tolist() == [0, -1]
    # a second entry above the threshold beside another pair's (tracks 2, 3 / detections 2, 3): no shortcut; the
    # assignment takes the crossing pairs (0.58 > 0.35) and the threshold then drops both of them
    big = np.zeros((4, 4))
    big[:2, :2] = small
    big[2, 2], big[2, 3] = 0.5, 0.4
    match, path = tracking.associate(big, 0.3)
    assert path == "hungarian" and match.tolist() == [-1, -1, 2, -1]
    pairs = dict(tracking.hungarian_max(big))
    assert pairs[0] == 1 and pairs[1] == 0 and pairs[2] == 2
    # nothing above the threshold at all: the shortcut with no match; empty sides: nothing to do
    assert tracking.associate(np.full((2, 3), 0.1), 0.3)[1] == "shortcut"
    assert tracking.associate(np.zeros((0, 3)), 0.3)[1] == "none" and tracking.associate(np.zeros((3, 0)), 0.3)[1] == "none"
    # a pair exactly at the threshold is not above it (no shortcut entry) and not below it (kept by the assignment)
    at = np.array([[0.3, 0.5], [0.0, 0.6]])
    match, path = tracking.associate(at, 0.3)
    assert path == "hungarian" and match.tolist() == [0, 1]


# ---- 4. the lifecycle by hand ----------------------------------------------------------------------------------------
def _ids(host, img=0):
    return [t["id"] for t in host.images[img]["tracks"]]


def test_lifecycle_by_hand():
    from disconet_amd import tracking
    a, none = [C.aligned(10.0, 10.0)], []
    host = tracking.HostSort(max_age=1, min_hits=3, iou_threshold=0.3, scale=C.SCALE)
    seen = [a, a, a, a, none, a, a, a, none, none, a]
    # frames 1-3 always; later only with hit_streak >= 3 (frame 11's newborn has none and frame_count > min_hits)
    want_reported = [1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0]
    want_tracks = [1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1]             # dies after max_age + 1 = 2 missed frames
    for f, rows in enumerate(seen):
        out = host.update(C.pad([rows], k=2))
        assert int(out["count"][0]) == want_reported[f], "frame %d" % (f + 1)
        assert len(host.images[0]["tracks"]) == want_tracks[f], "frame %d" % (f + 1)
        assert (out["id"][0, int(out["count"][0]):] == -1).all() and not out["rect"][0, int(out["count"][0]):].any()
    assert _ids(host) == [2]                                    # ids never repeat
    trk = host.images[0]["tracks"][0]
    assert (trk["age"], trk["hits"], trk["streak"], trk["tsu"]) == (0, 0, 0, 0)
    host.status()
    # the reported rectangle of a track fed the same box every frame is that box's, in scaled units
    host.reset()
    for _ in range(3):
        out = host.update(C.pad([a], k=2))
    np.testing.assert_allclose(out["rect"][0, 0], [4 * 8.0, 4 * 9.0, 4 * 12.0, 4 * 11.0], atol=1e-9)
    assert out["id"][0, 0] == 1 and out["det"][0, 0] == 0 and out["det_track"][0].tolist() == [1, -1]
    assert out["score"][0, 0] == np.float32(0.9)


def test_list_stays_in_ascending_id_after_deletions():
    from disconet_amd import tracking
    a, b, c, d = (C.aligned(x, 0.0) for x in (0.0, 20.0, 40.0, 60.0))
    host = tracking.HostSort(scale=C.SCALE)
    host.update(C.pad([[a, b, c]], k=4))
    assert _ids(host) == [1, 2, 3]
    host.update(C.pad([[a, c]], k=4))
    assert _ids(host) == [1, 2, 3]
    out = host.update(C.pad([[c, a, d]], k=4))                  # b missed twice: deleted; d is born behind the survivors
    assert _ids(host) == [1, 3, 4]
    assert out["id"][0, :3].tolist() == [1, 3, 4] and out["det"][0, :3].tolist() == [1, 0, 2]
    assert out["det_track"][0].tolist() == [3, 1, 4, -1]
    buf = host.state_bytes()
    assert buf[:16].view(np.int32).tolist() == [3, 5, 3, 0]
    assert not buf[64 + 3 * 480:].any()                         # slots past the list are zero


def test_capacity_and_invalid_rows_set_sticky_bits():
    from disconet_amd import _lib, tracking
    host = tracking.HostSort(scale=C.SCALE, max_tracks=4)
    out = host.update(C.pad([C.grid_rows(6)], k=6))
    assert host.status_words().tolist() == [1] and out["det_track"][0].tolist() == [1, 2, 3, 4, -1, -1]
    host.update(C.pad([C.grid_rows(2)], k=6))
    assert host.status_words().tolist() == [1]
    with pytest.raises(_lib.DnError, match="max_tracks"):
        host.status()
    host.reset()
    assert host.status() == 0
    wide = tracking.HostSort(scale=C.SCALE)
    out = wide.update(C.pad([C.grid_rows(130)], k=136))
    assert wide.status_words().tolist() == [4] and (out["det_track"][0, :128] > 0).all() and (out["det_track"][0, 128:] == -1).all()
    seq, invalid = C.mixed_sequence()
    host = tracking.HostSort(scale=C.SCALE)
    for f, det in enumerate(seq):
        out = host.update(det)
        assert host.status_words().tolist() == [0, 0, 2 if f >= 3 else 0]
        for img, frame, row in invalid:
            if frame == f:
                assert out["det_track"][img, row] == -1


# ---- 5. the generator ------------------------------------------------------------------------------------------------
def test_clean_sequence_keeps_one_id_per_identity():
    from disconet_amd import tracking
    from disconet_amd.synthetic import make_track_sequence
    seq = make_track_sequence(12, 4, seed=5, noise=0.0, p_miss=0.0, false_positives=0)
    again = make_track_sequence(12, 4, seed=5, noise=0.0, p_miss=0.0, false_positives=0)
    host = tracking.HostSort(scale=C.SCALE)
    first = {}
    for f, (det, ident) in enumerate(seq):
        assert all(np.array_equal(det[key], again[f][0][key]) for key in det) and np.array_equal(ident, again[f][1])
        assert det["boxes"].dtype == np.float32 and det["count"].dtype == np.int32 and ident.dtype == np.int32
        out = host.update(det)
        for img in range(4):
            assert int(det["count"][img]) == 6 and sorted(ident[img, :6].tolist()) == list(range(6))
            for row in range(6):
                key = (img, int(ident[img, row]))
                first.setdefault(key, int(out["det_track"][img, row]))
                assert first[key] == int(out["det_track"][img, row]) > 0, (f, key)
    assert len(first) == 24 and host.status() == 0
    noisy = make_track_sequence(6, 2, seed=5)
    assert any((ident == -1).any() for _, ident in noisy) and any(int(det["count"].min()) < 7 for det, _ in noisy)


def test_mot_rows_format():
    from disconet_amd import tracking
    host = tracking.HostSort(scale=C.SCALE)
    out = host.update(C.pad([[C.aligned(10.0, 10.0)], []], k=2))
    lines = tracking.mot_rows(out, 7)
    assert lines[1] == [] and len(lines[0]) == 1
    fields = lines[0][0].split(",")
    assert fields[:2] == ["7", "1"] and fields[7:] == ["-1", "-1", "-1"] and len(fields) == 10
    np.testing.assert_allclose([float(v) for v in fields[2:7]], [32.0, 36.0, 16.0, 8.0, 0.9], atol=1e-4)
