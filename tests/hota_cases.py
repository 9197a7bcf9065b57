"""Shared case builders of the HOTA tests (tests/test_hota_host_cpu.py, tests/test_gpu_hota.py): frames as pairs (tracks,
gt) of numpy dicts as in tests/mot_cases.py and tests/idf_cases.py, the by-hand sequences with their figures, and the
frame-by-frame comparison of tracking.Hota against tracking.HostHota."""
import numpy as np

from tests import idf_cases as I
from tests import mot_cases as C

SCALE = C.SCALE
SIZES = dict(max_gt_ids=64, max_track_ids=256, max_frames=16)     # what the GPU tests pass unless a case says otherwise
FIN_KEYS = ("counts", "alpha_counts", "alpha_sums", "match")
UNIT = I.A                                                         # the unit square


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def alpha_counts(ev, image=0):
    """finish()'s (TP, FN, FP) of one image as three lists of 19"""
    ac = _np(ev.finish()["alpha_counts"])[image]
    assert ac.dtype == np.int64 and ac.shape == (19, 4) and not ac[:, 3].any()
    return ac[:, 0].tolist(), ac[:, 1].tolist(), ac[:, 2].tolist()


# ---- by hand -----------------------------------------------------------------------------------------------------------
def check_swap(ev):
    """after idf_cases.swap_sequence() at scale 1 (track 1 exactly on A in frames 1..5 and on B in 6..9, track 2 over A at
    IoU 2/3 in frames 1..4): every frame's best pair is the exact hit, whatever the alignment score"""
    tp, fn, fp = alpha_counts(ev)
    assert tp == [9] * 19 and fn == [9] * 19 and fp == [4] * 19
    fin = ev.finish()
    sums = _np(fin["alpha_sums"])[0]
    assert sums.dtype == np.float64 and sums[:, 0].tolist() == [9.0] * 19
    for k in range(19):                      # cells (A, 1) = 5 of 9 + 9, (B, 1) = 4 of 9 + 9
        assert sums[k, 1] == 5.0 * (5.0 / 13.0) + 4.0 * (4.0 / 14.0) == 25 / 13 + 16 / 14
        assert sums[k, 2] == sums[k, 3] == 5.0 * (5.0 / 9.0) + 4.0 * (4.0 / 9.0) == 25 / 9 + 16 / 9
    assert _np(fin["counts"]).tolist() == [[9, 9, 18, 13, 2, 2, 0, 0]]
    pot = ev.potential_matrix(0)
    both, alone = 0.0, 0.0                   # frames 1..4: A's row sums to 1 + 2/3; then track 1 alone
    s2 = 1.0 / 1.5
    for _ in range(4):
        both = both + 1.0 / (((1.0 + s2) + 1.0) - 1.0)
        alone = alone + s2 / (((1.0 + s2) + s2) - s2)
    assert pot[0, 0] == both + 1.0 and pot[0, 1] == alone and pot[1, 0] == 4.0 and pot[1, 1] == 0.0
    assert abs(pot[0, 0] - (4 * 0.6 + 1)) < 1e-15 and abs(pot[0, 1] - 4 * 0.4) < 1e-15 and int((pot != 0).sum()) == 3
    match = ev.matches(0)
    assert match.shape == (9, 128) and match[:, 0].tolist() == [1] * 5 + [0] * 4 and match[:, 1].tolist() == [0] * 5 + [1] * 4
    assert not match[:, 2:].any()
    level = ev.compute()["overall"]
    assert level["TP"] == [9] * 19 and level["GT_IDs"] == 2 and level["IDs"] == 2 and level["LocA"] == 1.0
    assert level["DetA"] == 9 / 22 and level["HOTA(0)"] == float(np.sqrt((9 / 22) * ((25 / 13 + 16 / 14) / 9)))


def alpha_edge_frame():
    """One frame, three images at scale 1: [0, 20] x [0, 1] under a track [0, 3] x [0, 1] (IoU 3/20: counts at exactly 3
    alphas, and only with the epsilon -- 0.05 * 3 is 0.15000000000000002); the unit square under [0, 2] x [0, 1] (IoU 0.5: 10
    alphas); an exact hit (19)."""
    tracks = C.tracks_frame([[(1, (0.0, 0.0, 3.0, 1.0))], [(1, (0.0, 0.0, 2.0, 1.0))], [(1, UNIT)]])
    gt = C.gt_frame([[(0, C.rect_box(0.0, 0.0, 20.0, 1.0))], [(0, C.rect_box(*UNIT))], [(0, C.rect_box(*UNIT))]])
    return tracks, gt


def check_alpha_edges(ev):
    assert 0.05 * 3 > 3.0 / 20.0 and 3.0 / 20.0 == 0.15                # what the epsilon is for
    for image, (reach, iou) in enumerate(((3, 3.0 / 20.0), (10, 0.5), (19, 1.0))):
        tp, fn, fp = alpha_counts(ev, image)
        assert tp == [1] * reach + [0] * (19 - reach), (image, tp)
        assert fn == fp == [0] * reach + [1] * (19 - reach), (image, fn, fp)
        sums = _np(ev.finish()["alpha_sums"])[image]
        assert sums[:, 0].tolist() == [iou] * reach + [0.0] * (19 - reach)
        assert sums[:, 1].tolist() == sums[:, 2].tolist() == sums[:, 3].tolist() == [1.0] * reach + [0.0] * (19 - reach)
    assert _np(ev.finish()["counts"])[:, :6].tolist() == [[1, 1, 1, 1, 1, 1]] * 3


def alignment_sequence():
    """One image, scale 1, identity A the unit square over 10 frames: track 1 = [0, 1.5] x [0, 1] (IoU 2/3) in every frame,
    track 2 = [0, 1] x [0, 0.92] (IoU 0.92) in frame 5 only.  Track 1 is A's track over the sequence, so frame 5 keeps (A,
    track 1) although track 2 overlaps better there; a matcher that ranks frame 5 by IoU gives TP = 1 at alphas 13..17."""
    gt = C.gt_frame([[(0, C.rect_box(*UNIT))]])
    frames = []
    for f in range(1, 11):
        rows = [(1, (0.0, 0.0, 1.5, 1.0))]
        if f == 5:
            rows.append((2, (0.0, 0.0, 1.0, 0.92)))
        frames.append((C.tracks_frame([rows]), gt))
    return frames


def check_alignment(ev):
    tp, fn, fp = alpha_counts(ev)
    assert tp == [10] * 13 + [0] * 6, tp
    assert fp == [1] * 13 + [11] * 6 and fn == [0] * 13 + [10] * 6
    match = ev.matches(0)
    assert match.shape == (10, 128) and match[:, 0].tolist() == [1] * 10 and not match[:, 1:].any()
    pot = ev.potential_matrix(0)
    assert pot[0, 0] > 9.0 and 0.0 < pot[0, 1] < 1.0                      # the alignment: track 1 far ahead of track 2
    assert _np(ev.finish()["counts"]).tolist() == [[10, 10, 10, 11, 1, 2, 0, 0]]


def twice_frame():
    """One frame in which the track id 7 is reported on two rows, both over identity 0: the lower row is the column."""
    return I.twice_frame()


def check_twice(out, ev):
    assert ev.status_words().tolist() == [64]
    assert _np(ev.finish()["counts"]).tolist() == [[1, 1, 1, 1, 1, 1, 64, 0]]    # Dets 1: the second row is counted nowhere
    g, t, f = ev.max_gt_ids, ev.max_track_ids, ev.max_frames
    buf = ev.state_bytes()
    tail = buf[64 + 8 * g * t + 9232 * f:]
    assert tail[:4 * (g + t)].view(np.int32).sum() == 2                           # gt_count[0] = track_count[6] = 1
    slot = buf[64 + 8 * g * t:64 + 8 * g * t + 9232]
    assert slot[:8].view(np.int32).tolist() == [1, 1] and slot[528:532].view(np.int32).tolist() == [7]
    assert slot[5136:5168].view(np.float64).tolist() == [0.0, 0.0, 1.0, 1.0] and not slot[5168:].any()
    pot = ev.potential_matrix(0)
    assert pot[0, 6] == 1.0 and int((pot != 0).sum()) == 1 and _np(out["potential"])[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert alpha_counts(ev)[0] == [1] * 19


def status_cases(max_track_ids=256):
    """(bit, a word of its message, frames, params) for one image at scale 1: idf_cases.status_cases() (bits 4, 8, 2, 1 and
    three times 16), the full log (bit 32: max_frames = 1 and a second frame) and the duplicate track id (bit 64).  Every
    case ends with a clean frame.  max_gt_ids is 256 here: the cases of bit 1 carry the ids 0 .. 129."""
    params = dict(max_gt_ids=256, max_track_ids=max_track_ids, max_frames=4)
    cases = []
    for bit, word, tracks, gt in I.status_cases(max_track_ids):
        cases.append((bit, word, [(tracks, gt), I.clean_frame(g=gt["ids"].shape[1])], params))
    cases.append((32, "log was full", [I.clean_frame(), I.clean_frame()], dict(params, max_frames=1)))
    cases.append((64, "track id came twice", [twice_frame(), I.clean_frame()], params))
    return cases


def dense_frames():
    """Two frames of one image with 128 kept ground truths and 128 tracks, the largest matrix a launch holds: the
    ground truths [2 i, 2 i + 4] x [0, 2 + i / 64] overlap their neighbours, track j sits 0.4 (frame 1) or 1.2 (frame 2) to
    the right of ground truth j, so every row and column holds four or five overlaps and the frames disagree on the best
    neighbour; the ids of the second frame are shifted by one so that the alignment score matters."""
    gt = C.gt_frame([[(i, C.rect_box(2.0 * i, 0.0, 2.0 * i + 4.0, 2.0 + i / 64.0)) for i in range(128)]], g=128)
    frames = []
    for shift, first in ((0.4, 1), (1.2, 2)):
        rows = [(first + j, (2.0 * j + shift, 0.0, 2.0 * j + 4.0 + shift, 2.0 + j / 64.0)) for j in range(128)]
        frames.append((C.tracks_frame([rows], m=128), gt))
    return frames


def ragged_sequence():
    """Three images of different lengths from the generator at p_miss = 0.3, padded with empty frames: image 1 ends after 8
    of the 12 frames (both counts 0 from then on), image 2 has no ground truth on frames 3 and 4 (V = 0, C > 0) and is fed
    no tracks on frames 6 and 7 (C = 0, V > 0)."""
    seq = []
    for f, (tracks, gt) in enumerate(C.generated_sequence(12, 3, 2, p_miss=0.3)):
        tracks = {key: tracks[key].copy() for key in tracks}
        gt = {key: gt[key].copy() for key in gt}
        if f >= 8:
            tracks["count"][1] = 0
            gt["count"][1] = 0
        if f in (2, 3):
            gt["count"][2] = 0
        if f in (5, 6):
            tracks["count"][2] = 0
        seq.append((tracks, gt))
    return seq


# ---- device against host ---------------------------------------------------------------------------------------------
def assert_same_bits(got, want, what, keys=("potential",)):
    I.assert_same_bits(got, want, what, keys=keys)


def assert_same_end(dev, host, raises=False):
    """finish()'s four tensors as bits; compute() for equality (compute() of both raises on a status bit)"""
    assert_same_bits(dev.finish(), host.finish(), "finish", keys=FIN_KEYS)
    if not raises:
        assert dev.compute() == host.compute()


def run_both(seq, batch_size=1, **params):
    """Every frame of `seq` through Hota (the state stays on the device) and HostHota; after every frame `potential`, the
    status words and the whole state are compared as bits, after the last frame finish()'s four tensors as bits and
    compute() for equality.  Returns (device, host, host outputs per frame)."""
    from disconet_amd import tracking
    dev, host = tracking.Hota(batch_size, **params), tracking.HostHota(batch_size, **params)
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
