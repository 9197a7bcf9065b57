"""Shared case builders of the identity-metric tests (tests/test_idf_host_cpu.py, tests/test_gpu_idf.py): frames as pairs
(tracks, gt) of numpy dicts as in tests/mot_cases.py, the by-hand sequences with their figures, the seeded assignment
matrices driven through update(), and the frame-by-frame comparison of tracking.Identity against tracking.HostIdentity."""
import numpy as np

from tests import mot_cases as C
from tests import track_cases as T

SCALE = T.SCALE
A = (0.0, 0.0, 1.0, 1.0)                # identity 0 of the by-hand sequences, the unit square
B = (10.0, 0.0, 12.0, 2.0)              # identity 1

# what a run over mot_cases.scripted_sequence() must give (scale 1, threshold 0.5): in frame 2 tracks 1 and 3 both overlap
# A, and frame 1's pair at IoU exactly 0.5 counts
SCRIPTED = {"pairs": [[2, 0, 5], [0, 4, 0], [0, 0, 0]], "gt_count": [6, 6, 6], "track_count": [2, 4, 5],
            "overlaps": [[1, 1, 0], [2, 1, 0], [1, 1, 0], [1, 0, 0], [1, 0, 0], [1, 1, 0]],
            "figures": {"GT_Dets": 18, "Dets": 11, "IDTP": 9, "IDFP": 2, "IDFN": 9, "GT_IDs": 3, "IDs": 3, "frames": 6},
            "match": [3, 2, 0], "assignment": [(0, 3, 5), (1, 2, 4)]}
# the matrices of matrix_cases(): r identities x c track ids, seed -> (IDTP = scipy's maximum, the row-by-row greedy total)
MATRIX_TABLE = {(70, 65, 0): (425, 359), (65, 70, 1): (410, 377), (300, 260, 2): (1656, 1373), (260, 300, 3): (1628, 1449)}


def check_scripted(outs, dev):
    """the per-frame outputs (numpy) and the evaluation (Identity or HostIdentity) after mot_cases.scripted_sequence()"""
    from disconet_amd import tracking
    for f, out in enumerate(outs):
        assert out["overlaps"][0].tolist() == SCRIPTED["overlaps"][f] + [0], "frame %d" % (f + 1)
    g, t = dev.max_gt_ids, dev.max_track_ids
    pairs = dev.counts_matrix(0)
    assert pairs.shape == (g, t) and pairs[:3, :3].tolist() == SCRIPTED["pairs"] and int(pairs.sum()) == 11
    buf = dev.state_bytes()
    assert len(buf) == tracking.idf_state_bytes(1, g, t)
    assert buf[:24].view(np.int64).tolist() == [6, 18, 11] and not buf[24:64].any()
    gt_count = buf[64:64 + 4 * g].view(np.int32)
    track_count = buf[64 + 4 * g:64 + 4 * (g + t)].view(np.int32)
    assert gt_count[:3].tolist() == SCRIPTED["gt_count"] and not gt_count[3:].any()
    assert track_count[:3].tolist() == SCRIPTED["track_count"] and not track_count[3:].any()
    assert np.array_equal(buf[64 + 4 * (g + t):].view(np.int32).reshape(g, t), pairs)
    figures = dev.compute()
    for level in (figures["overall"], figures["per_agent"][0], figures["per_image"][0]):
        for key, want in SCRIPTED["figures"].items():
            assert level[key] == want, (key, level[key], want)
        assert level["IDF1"] == 18 / 29 and level["IDP"] == 9 / 11 and level["IDR"] == 9 / 18
    fin = dev.finish()
    counts, match = _np(fin["counts"]), _np(fin["match"])
    assert counts.dtype == np.int64 and counts.tolist() == [[6, 18, 11, 9, 3, 3, 0, 0]]
    assert match.dtype == np.int32 and match[0, :3].tolist() == SCRIPTED["match"] and not match[0, 3:].any()
    assert dev.assignment() == [SCRIPTED["assignment"]]


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def swap_sequence():
    """One image, scale 1, two identities A and B over nine frames: track 1 sits exactly on A in frames 1..5 and exactly on
    B in frames 6..9; track 2 = [0, 1.5] x [0, 1] covers A at IoU 2/3 in frames 1..4.  pairs = [[5, 4], [4, 0]]: the best
    mapping gives A track 2 and B track 1 (IDTP 8), a row-by-row pick gives A track 1 and B nothing (5)."""
    gt = C.gt_frame([[(0, C.rect_box(*A)), (1, C.rect_box(*B))]])
    frames = []
    for f in range(1, 10):
        rows = [(1, A if f <= 5 else B)]
        if f <= 4:
            rows.append((2, (0.0, 0.0, 1.5, 1.0)))
        frames.append((C.tracks_frame([rows]), gt))
    want = {"pairs": [[5, 4], [4, 0]], "counts": [9, 18, 13, 8, 2, 2, 0, 0], "match": [2, 1],
            "assignment": [(0, 2, 4), (1, 1, 4)]}
    return frames, want


def check_swap(dev, want):
    assert dev.counts_matrix(0)[:2, :2].tolist() == want["pairs"]
    fin = dev.finish()
    assert _np(fin["counts"]).tolist() == [want["counts"]] and _np(fin["match"])[0, :2].tolist() == want["match"]
    assert dev.assignment() == [want["assignment"]]
    level = dev.compute()["overall"]
    assert (level["IDTP"], level["IDFP"], level["IDFN"]) == (8, 5, 10) and level["IDF1"] == 16 / 31


def twice_frame():
    """One frame in which the track id 7 is reported on two rows, both over identity 0."""
    return C.tracks_frame([[(7, A), (7, (0.0, 0.0, 1.5, 1.0))]]), C.gt_frame([[(0, C.rect_box(*A))]])


def check_twice(out, dev):
    assert _np(out["overlaps"])[0].tolist() == [2, 0, 0, 0]
    pairs = dev.counts_matrix(0)
    assert pairs[0, 6] == 2 and int(pairs.sum()) == 2
    g = dev.max_gt_ids
    track_count = dev.state_bytes()[64 + 4 * g:64 + 4 * (g + dev.max_track_ids)].view(np.int32)
    assert track_count[6] == 2 and int(track_count.sum()) == 2
    assert _np(dev.finish()["counts"]).tolist() == [[1, 1, 2, 2, 1, 1, 0, 0]]     # Dets 2, IDTP 2: more than GT_Dets


def status_cases(max_track_ids=1024):
    """(bit, a word of its message, tracks, gt) for one image at scale 1: the four ground-truth bits on the cases of
    tests/test_gpu_mot.py, bit 16 on the track ids 0, -1 and max_track_ids + 1."""
    from tests.test_gpu_mot import _status_cases
    on_box = (0.0, 0.0, 4.0, 2.0)
    cases = [(bit, word, C.tracks_frame([[(1, on_box)]]), gt) for bit, word, gt in _status_cases()]
    for bad in (0, -1, max_track_ids + 1):
        cases.append((16, "max_track_ids", C.tracks_frame([[(bad, on_box), (1, on_box)]]),
                      C.gt_frame([[(0, C.rect_box(*on_box))]])))
    return cases


def clean_frame(g=4):
    on_box = (0.0, 0.0, 4.0, 2.0)
    return C.tracks_frame([[(1, on_box)]]), C.gt_frame([[(0, C.rect_box(*on_box))]], g=g)


# ---- seeded assignment matrices, driven through update() ---------------------------------------------------------------
def seeded_matrix(r, c, seed):
    """W [r, c]: three cells of 1..9 in every row"""
    rng = np.random.default_rng(seed)
    w = np.zeros((r, c), dtype=np.int64)
    for i in range(r):
        cols = rng.choice(c, 3, replace=False)
        w[i, cols] = rng.integers(1, 10, size=3)
    return w


def greedy_total(w):
    """the row-by-row pick: every row in order takes its largest cell among the columns still free"""
    free, total = np.ones(w.shape[1], dtype=bool), 0
    for row in w:
        cand = np.where(free, row, -1)
        j = int(np.argmax(cand))
        if cand[j] > 0:
            free[j] = False
            total += int(cand[j])
    return total


def matrix_rows(w, group=40):
    """W [identities, track ids] -> per frame (track rows, ground-truth rows) of ONE image whose pairs matrix is W: identity
    i is the rectangle [8 i, 8 i + 4] x [0, 2] at scale 1; the identities come `group` at a time (three cells per row: at
    most 120 track rows), and frame f of a group holds a track row exactly on identity i with id t + 1 for every cell W[i,
    t] > f."""
    assert w.max() <= 9 and ((w > 0).sum(1) <= 3).all()
    frames = []
    for lo in range(0, w.shape[0], group):
        idents = range(lo, min(lo + group, w.shape[0]))
        for f in range(9):
            rect = lambda i: (8.0 * i, 0.0, 8.0 * i + 4.0, 2.0)
            tracks = [(int(t) + 1, rect(i)) for i in idents for t in np.nonzero(w[i] > f)[0]]
            frames.append((tracks, [(i, C.rect_box(*rect(i))) for i in idents]))
    return frames


def matrix_frames(matrices, group=40):
    """One image per matrix -> [(tracks, gt)]; an image with fewer frames is padded with empty frames (both counts 0)."""
    rows = [matrix_rows(w, group) for w in matrices]
    frames = []
    for f in range(max(len(r) for r in rows)):
        now = [r[f] if f < len(r) else ([], []) for r in rows]
        frames.append((C.tracks_frame([tracks for tracks, _ in now], m=3 * group),
                       C.gt_frame([gt for _, gt in now], g=group)))
    return frames


_MATRIX = {}


def matrix_cases(large):
    """The two runs of two images each: (70 x 65, seed 0) with (65 x 70, seed 1), or (300 x 260, seed 2) with (260 x 300,
    seed 3).  Returns (shapes, matrices, frames, params); computed once and shared -- callers must not write into it."""
    if large not in _MATRIX:
        shapes = [(300, 260, 2), (260, 300, 3)] if large else [(70, 65, 0), (65, 70, 1)]
        matrices = [seeded_matrix(*s) for s in shapes]
        params = dict(scale=1.0, max_gt_ids=512, max_track_ids=512) if large else dict(scale=1.0)
        _MATRIX[large] = (shapes, matrices, matrix_frames(matrices), params)
    return _MATRIX[large]


def check_matrix_run(dev, shapes, matrices):
    """after the frames of matrix_cases(): the pairs blocks are the matrices and IDTP is the table's (= scipy's maximum)"""
    from scipy.optimize import linear_sum_assignment
    fin = dev.finish()
    counts, match = _np(fin["counts"]), _np(fin["match"])
    for img, (shape, w) in enumerate(zip(shapes, matrices)):
        r, c, _ = shape
        pairs = dev.counts_matrix(img)
        assert np.array_equal(pairs[:r, :c], w) and int(pairs.sum()) == int(w.sum()), shape
        rows, cols = linear_sum_assignment(w, maximize=True)
        best, greedy = int(w[rows, cols].sum()), greedy_total(w)
        print("%d x %d seed %d: IDTP %d, scipy %d, greedy %d, the issue's table %s" % (
            shape + (int(counts[img, 3]), best, greedy, MATRIX_TABLE[shape])))
        assert (best, greedy) == MATRIX_TABLE[shape]
        assert int(counts[img, 3]) == best and best > greedy               # a real assignment: greedy falls short
        assert counts[img, 1] == 9 * r and counts[img, 2] == int(w.sum()) and counts[img, 4] == r
        assert counts[img, 5] == int((w.sum(0) > 0).sum()) and counts[img, 6] == 0
        took = np.nonzero(match[img])[0]                                    # a matching: no track id twice, weights add up
        assert len(set(match[img, took].tolist())) == len(took)
        assert sum(int(w[i, match[img, i] - 1]) for i in took) == best


# ---- device against host ---------------------------------------------------------------------------------------------
def assert_same_bits(got, want, what, keys=("overlaps",)):
    for key in keys:
        g, w = _np(got[key]), _np(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(C.bits(g), C.bits(w)):
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %s: got %r, want %r" % (
                what, key, bad[:4].tolist(), g[tuple(bad[0])] if len(bad) else None, w[tuple(bad[0])] if len(bad) else None))


def assert_same_end(dev, host, raises=False):
    """finish()'s two tensors as bits; compute() and assignment() for equality (compute() of both raises on a status bit)"""
    assert_same_bits(dev.finish(), host.finish(), "finish", keys=("counts", "match"))
    assert dev.assignment() == host.assignment()
    if not raises:
        assert dev.compute() == host.compute()


def run_both(seq, batch_size=1, **params):
    """Every frame of `seq` through Identity (the state stays on the device) and HostIdentity; after every frame `overlaps`,
    the status words and the whole state are compared as bits, after the last frame finish(), compute() and assignment().
    Returns (device, host, host outputs per frame)."""
    from disconet_amd import tracking
    dev, host = tracking.Identity(batch_size, **params), tracking.HostIdentity(batch_size, **params)
    outs = []
    for f, (tracks, gt) in enumerate(seq):
        got = dev.update(C.to_device(tracks), C.to_device(gt))
        want = host.update(tracks, gt)
        assert_same_bits(got, want, "frame %d" % (f + 1))
        assert dev.status_words().tolist() == host.status_words().tolist(), "frame %d status" % (f + 1)
        assert np.array_equal(dev.state_bytes(), host.state_bytes()), "frame %d state bytes" % (f + 1)
        outs.append(want)
    assert_same_end(dev, host, raises=bool(host.status_words().any()))
    return dev, host, outs
