"""Shared case builders of the tracking-evaluation tests (tests/test_mot_host_cpu.py, tests/test_gpu_mot.py): frames as
pairs (tracks, gt) of numpy dicts -- tracks in the form tracking.Sort.update() reports, gt = {"boxes", "ids", "count"} --
and the frame-by-frame comparison of tracking.ClearMot against tracking.HostClearMot."""
import numpy as np

from tests import track_cases as T

SCALE = T.SCALE
OUT_KEYS = ("match", "iou", "flags")


def tracks_frame(images, m=4):
    """per image a list of (id, (x1, y1, x2, y2)) -> the tracker's report {"rect" [N, m, 4], "id" [N, m], "count" [N]}"""
    n = len(images)
    out = {"rect": np.zeros((n, m, 4), dtype=np.float64), "id": np.full((n, m), -1, dtype=np.int32),
           "count": np.zeros(n, dtype=np.int32)}
    for i, rows in enumerate(images):
        for r, (ident, rect) in enumerate(rows):
            out["rect"][i, r] = rect
            out["id"][i, r] = ident
        out["count"][i] = len(rows)
    return out


def gt_frame(images, g=4):
    """per image a list of (id, box row (x, y, w, h, sin, cos)) -> {"boxes" [N, g, 6] float32, "ids" [N, g], "count" [N]}"""
    n = len(images)
    out = {"boxes": np.zeros((n, g, 6), dtype=np.float32), "ids": np.zeros((n, g), dtype=np.int32),
           "count": np.zeros(n, dtype=np.int32)}
    for i, rows in enumerate(images):
        for r, (ident, box) in enumerate(rows):
            out["boxes"][i, r] = box
            out["ids"][i, r] = ident
        out["count"][i] = len(rows)
    return out


def rect_box(x1, y1, x2, y2):
    """the axis-aligned box row of a rectangle"""
    return T.aligned((x1 + x2) / 2.0, (y1 + y2) / 2.0, x2 - x1, y2 - y1)


def scripted_sequence():
    """One image, scale 1, threshold 0.5, three identities: A (id 0) the unit square, B (id 1) a 2 x 2 square, C (id 2) far
    away and never tracked.  Returns (frames, expected integers).
      frame 1  track 1 = [0,2]x[0,1] over A: IoU exactly 0.5, matched; track 2 on B
      frame 2  track 1 = [0,1.5]x[0,1] (IoU 2/3) and a new track 3 exactly on A (IoU 1): the continuity term keeps track 1,
               track 3 is a false positive, no switch
      frame 3  track 1 is gone, track 3 takes A: one id switch (and no new segment: A was matched the frame before)
      frames 4, 5  track 2 is missing: B unmatched twice
      frame 6  track 2 is back on B: its second segment (Frag 1), the same id, no switch"""
    a, b, c = (0.0, 0.0, 1.0, 1.0), (10.0, 0.0, 12.0, 2.0), (100.0, 100.0, 101.0, 101.0)
    gt = gt_frame([[(0, rect_box(*a)), (1, rect_box(*b)), (2, rect_box(*c))]])
    reports = [[(1, (0.0, 0.0, 2.0, 1.0)), (2, b)],
               [(1, (0.0, 0.0, 1.5, 1.0)), (2, b), (3, a)],
               [(2, b), (3, a)],
               [(3, a)],
               [(3, a)],
               [(2, b), (3, a)]]
    frames = [(tracks_frame([rows]), gt) for rows in reports]
    motp = 0.0
    for iou in (0.5, 1.0, 1.0 / 1.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0):      # frame by frame, ascending ground-truth row
        motp = motp + iou
    want = {"TP": 10, "FP": 1, "FN": 8, "IDSW": 1, "Frag": 1, "MT": 1, "PT": 1, "ML": 1, "frames": 6, "motp_sum": motp,
            "match": [[1, 2, -1], [1, 2, -1], [3, 2, -1], [3, -1, -1], [3, -1, -1], [3, 2, -1]],
            "flags": [[5, 5, 0], [1, 1, 0], [3, 1, 0], [1, 0, 0], [1, 0, 0], [1, 5, 0]]}
    return frames, want


def check_scripted(outs, figures, want):
    """the per-frame outputs (numpy) and compute()'s dict of a run over scripted_sequence() against its expected figures"""
    for f, out in enumerate(outs):
        assert out["match"][0, :3].tolist() == want["match"][f], "frame %d" % (f + 1)
        assert out["flags"][0, :3].tolist() == want["flags"][f], "frame %d" % (f + 1)
        assert out["match"][0, 3] == -1 and out["flags"][0, 3] == 0 and out["iou"][0, 3] == 0.0
    assert outs[0]["iou"][0, 0] == 0.5 and outs[1]["iou"][0, 0] == 1.0 / 1.5
    for level in (figures["overall"], figures["per_agent"][0], figures["per_image"][0]):
        for key in ("TP", "FP", "FN", "IDSW", "Frag", "MT", "PT", "ML", "frames"):
            assert level[key] == want[key], (key, level[key], want[key])
        assert level["MOTA"] == (10 - 1 - 1) / 18.0 and level["MOTP"] == want["motp_sum"] / 10.0
        assert level["Recall"] == 10 / 18.0 and level["Precision"] == 10 / 11.0


_GENERATED = {}


def generated_sequence(frames, n_images, seed, **kw):
    """make_track_sequence(truth=True) through HostSort(scale=4): [(tracks, gt)] per frame (numpy), computed once per
    argument set and shared -- callers must not write into it."""
    from disconet_amd import tracking
    from disconet_amd.synthetic import make_track_sequence
    key = (frames, n_images, seed, tuple(sorted(kw.items())))
    if key not in _GENERATED:
        sort = tracking.HostSort(scale=SCALE)
        seq = []
        for det, _, gt in make_track_sequence(frames, n_images, seed=seed, truth=True, **kw):
            out = sort.update(det)
            seq.append(({name: out[name] for name in ("rect", "id", "count")}, gt))
        _GENERATED[key] = seq
    return _GENERATED[key]


def mixed_sequence(frames=12):
    """Three images x `frames` frames from the generator at p_miss = 0.3.  Image 0's ground-truth count is 0 on frames 4, 5
    and 9; image 2 is fed no tracks at all."""
    seq = []
    for f, (tracks, gt) in enumerate(generated_sequence(frames, 3, 2, p_miss=0.3)):
        tracks = {key: tracks[key].copy() for key in tracks}
        gt = {key: gt[key].copy() for key in gt}
        if f in (4, 5, 9):
            gt["count"][0] = 0
        tracks["count"][2] = 0
        seq.append((tracks, gt))
    return seq


def chain_frames():
    """One image on tests/track_cases.chain_sequence's chain (boxes at pitch w / 2, every frame shifted by 0.1 w: a box
    overlaps its own earlier position at IoU 0.82 and the next one's at 0.43), evaluated at threshold 0.3 so that every
    row of the score matrix holds two entries: 70 ground truths x 65 tracks, then 65 x 70.  Ground truth = the chain of
    one frame, tracks = the rectangles of the next frame's boxes, ids = chain position + 1."""
    from disconet_amd import tracking
    chain = T.chain_sequence()

    def rects(det):
        c = int(det["count"][0])
        rows, rect, _, status = tracking._measure(det["boxes"][0], det["scores"][0], c, SCALE)
        assert status == 0 and rows == list(range(c))
        return rect

    def frame(gt_det, gt_ids, track_det, track_ids):
        c = int(gt_det["count"][0])
        gt = {"boxes": gt_det["boxes"][:, :c].copy(), "ids": np.asarray([gt_ids], dtype=np.int32),
              "count": np.asarray([c], dtype=np.int32)}
        r = rects(track_det)[track_ids]
        return tracks_frame([[(i + 1, r[j]) for j, i in enumerate(track_ids)]], m=72), gt

    keep65 = [i for i in range(70) if i not in (9, 30, 51, 3, 64)]
    first = frame(chain[0], list(range(70)), chain[1], keep65)               # 70 ground truths x 65 tracks
    second = frame(chain[3], keep65, chain[4], list(range(70)))              # 65 x 70
    return [first, second]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def assert_same_bits(got, want, what):
    for key in OUT_KEYS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(bits(g), bits(w)):
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %s: got %r, want %r" % (
                what, key, bad[:4].tolist(), g[tuple(bad[0])] if len(bad) else None, w[tuple(bad[0])] if len(bad) else None))


def to_device(d):
    import torch
    return {key: torch.from_numpy(np.ascontiguousarray(d[key])).cuda() for key in d}


def to_host(out):
    return {key: out[key].cpu().numpy() for key in OUT_KEYS}


def run_both(seq, batch_size=1, **params):
    """Every frame of `seq` through ClearMot (the state stays on the device) and HostClearMot; after every frame the three
    outputs, the status words and the whole state are compared as bits.  Returns (device, host, host outputs per frame)."""
    from disconet_amd import tracking
    dev, host = tracking.ClearMot(batch_size, **params), tracking.HostClearMot(batch_size, **params)
    outs = []
    for f, (tracks, gt) in enumerate(seq):
        got = to_host(dev.update(to_device(tracks), to_device(gt)))
        want = host.update(tracks, gt)
        assert_same_bits(got, want, "frame %d" % (f + 1))
        assert dev.status_words().tolist() == host.status_words().tolist(), "frame %d status" % (f + 1)
        assert np.array_equal(dev.state_bytes(), host.state_bytes()), "frame %d state bytes" % (f + 1)
        outs.append(want)
    return dev, host, outs
