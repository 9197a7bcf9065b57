"""Shared case builders of the tracker tests (tests/test_track_host_cpu.py, tests/test_gpu_track.py): detection
sequences as lists of postprocess.pad_detections-style dicts (numpy), and the frame-by-frame comparison of tracking.Sort
against tracking.HostSort."""
import numpy as np

SCALE = 4.0                       # 1 / voxel_size[0]: what the tools pass
OUT_KEYS = ("rect", "id", "det", "score", "count", "det_track")


def pad(rows, scores=None, k=None):
    """per image [n_i, 6] boxes (x, y, w, h, sin, cos) and scores -> one frame's dict"""
    from disconet_amd.postprocess import pad_detections
    rows = [np.asarray(r, dtype=np.float64).reshape(-1, 6) for r in rows]
    if scores is None:
        scores = [np.linspace(0.9, 0.6, len(r)) for r in rows]
    return pad_detections(rows, scores, k)


def aligned(x, y, w=4.0, h=2.0):
    """an axis-aligned box row"""
    return [x, y, w, h, 0.0, 1.0]


def mixed_sequence(frames=12):
    """n = 3 images, K = 8: image 0 has count 0 on frames 4, 5 and 9, image 1 carries a full K rows on every frame, image 2
    an invalid row on two frames (zero width, axis-aligned, on frame 3; a NaN score on frame 6).  Returns (list of dicts, (image, frame,
    row) of the invalid rows)."""
    from disconet_amd.synthetic import make_track_sequence
    base = make_track_sequence(frames, 3, seed=3, objects=5, false_positives=1, width=8)
    full = make_track_sequence(frames, 1, seed=4, objects=7, false_positives=1, p_miss=0.0, width=8)
    seq = []
    for f in range(frames):
        det = {key: base[f][0][key].copy() for key in ("boxes", "scores", "count")}
        for key in ("boxes", "scores", "count"):
            det[key][1] = full[f][0][key][0]
        assert int(det["count"][1]) == 8
        if f in (4, 5, 9):
            det["count"][0] = 0
        seq.append(det)
    assert int(seq[3]["count"][2]) >= 2 and int(seq[6]["count"][2]) >= 1
    seq[3]["boxes"][2, 1, 2:6] = (0.0, 4.0, 0.0, 1.0)      # axis-aligned, so that its rectangle has no width either
    seq[6]["scores"][2, 0] = np.nan
    return seq, ((2, 3, 1), (2, 6, 0))


def chain_sequence(n=70, k=72, w=4.0, h=2.0):
    """One image: n boxes of width w in a row at pitch w / 2 (each overlaps its neighbours at IoU 1/3), every frame
    shifted by a further 0.1 w (own IoU 0.82, next neighbour 0.43: two entries above 0.3 in every row, no shortcut).
    Frames 3, 4, 5 carry 67, 65 and all 70 of them: T > D twice, then T < D once the unseen tracks have died."""
    drops = [(), (), (9, 30, 51), (9, 30, 51, 3, 64), ()]
    seq = []
    for f, drop in enumerate(drops):
        rows = [aligned(i * w / 2.0 + 0.1 * w * f, 0.0, w, h) for i in range(n) if i not in drop]
        seq.append(pad([rows], k=k))
    return seq


def grid_rows(count, pitch=8.0, per_row=16):
    return [aligned((i % per_row) * pitch, (i // per_row) * pitch) for i in range(count)]


def tie_sequence():
    """One image, K = 4.  Frame 1: one box.  Frame 2: two identical detections over it (equal IoU: the lower row wins, the
    other starts a track).  Frame 3: detections far from every track (every IoU 0).  Frame 4: two identical detections over
    the two coincident tracks (a 2 x 2 matrix of equal entries)."""
    a = aligned(10.0, 10.0)
    far = [aligned(100.0, 50.0), aligned(-80.0, 20.0), aligned(0.0, -90.0)]
    return [pad([[a]], k=4), pad([[a, a]], k=4), pad([far], k=4), pad([[a, a]], k=4), pad([[a, a]], k=4)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def assert_same_bits(got, want, what):
    for key in OUT_KEYS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(bits(g), bits(w)):
            bad = np.argwhere(np.asarray(g != w) | (np.isnan(g.astype(np.float64)) != np.isnan(w.astype(np.float64))))
            raise AssertionError("%s: %s differs at %s: got %r, want %r" % (
                what, key, bad[:4].tolist(), g[tuple(bad[0])] if len(bad) else None, w[tuple(bad[0])] if len(bad) else None))


def to_device(det):
    import torch
    return {key: torch.from_numpy(np.ascontiguousarray(det[key])).cuda() for key in ("boxes", "scores", "count")}


def to_host(out):
    return {key: out[key].cpu().numpy() for key in OUT_KEYS}


def run_both(seq, check_state=True, **params):
    """Every frame of `seq` through Sort (the state stays on the device) and HostSort; after every frame all outputs, the
    status words and (check_state) the state bytes are compared as bits.  Returns (sort, host, host outputs per frame, host
    association paths per frame)."""
    from disconet_amd import tracking
    sort, host = tracking.Sort(**params), tracking.HostSort(**params)
    outs, paths = [], []
    for f, det in enumerate(seq):
        got = to_host(sort.update(to_device(det)))
        want = host.update(det)
        assert_same_bits(got, want, "frame %d" % (f + 1))
        assert sort.status_words().tolist() == host.status_words().tolist(), "frame %d status" % (f + 1)
        if check_state:
            assert np.array_equal(sort.state_bytes(), host.state_bytes()), "frame %d state bytes" % (f + 1)
        outs.append(want)
        paths.append(list(host.last_path))
    return sort, host, outs, paths
