"""Cases for the stratified-AP tests (tests/test_strata_host_cpu.py, tests/test_gpu_strata.py) and a plain, sequential
restatement of the matching and of the metric to hold the library's host functions against.  TEST infrastructure.

Every box is axis-aligned with dyadic coordinates (2 x 4 boxes on a pitch-8 grid, detections shifted by 0, 1/4, 1/2 or 1
in x), so intersection and union are exact in float64 whatever the formulation and the IoU -- 1, 7/9, 3/5 or 1/3 -- is
one correctly rounded division: host and device agree in every bit, and the restatement below can use the rectangle
formula instead of a polygon clip."""
import math

import numpy as np

THRS2 = (0.5, 0.7)
THRS8 = (0.25, 1.0 / 3.0, 0.5, 0.6, 0.7, 7.0 / 9.0, 0.9, 1.0)     # three of them are attained exactly
SHIFTS = (0.0, 0.25, 0.5, 1.0)
PITCH = 8.0


def _gt_row(cell):
    return [PITCH * (cell % 16) - 60.0, PITCH * (cell // 16) - 60.0, 2.0, 4.0, 0.0, 1.0]


def make(seed, n_img, k, g, n_strata, dont_care=0.2, fill=0.6):
    """Padded arrays ({"boxes", "scores", "count"}, gt_boxes, gt_count, gt_stratum): per image up to g boxes on distinct
    grid cells (the second a copy of the first, in another stratum when there is one: the lowest column wins), strata
    drawn from [-1, n_strata) with `dont_care` of them -1, about `fill` * k detections: 70 % shifted copies of a box (so
    duplicates on one box and matches in every stratum occur), 30 % far from everything; scores quantised to 1/16 (ties).
    Rows beyond the counts hold garbage."""
    r = np.random.default_rng(seed)
    boxes = r.uniform(-50, 50, (n_img, k, 6)).astype(np.float32)
    scores = r.uniform(2, 3, (n_img, k)).astype(np.float32)
    gb = r.uniform(-50, 50, (n_img, g, 6)).astype(np.float32)
    st = r.integers(-5, 12, (n_img, g)).astype(np.int32)
    count, gc = np.zeros(n_img, np.int32), np.zeros(n_img, np.int32)
    for i in range(n_img):
        gc[i] = g if i == 0 else r.integers(max(1, g // 2), g + 1)
        cells = r.permutation(256)[:gc[i]]
        gb[i, :gc[i]] = [_gt_row(c) for c in cells]
        st[i, :gc[i]] = np.where(r.random(gc[i]) < dont_care, -1, r.integers(0, n_strata, gc[i]))
        if gc[i] >= 2:
            gb[i, 1] = gb[i, 0]
            st[i, 1] = (st[i, 0] + 1) % n_strata if st[i, 0] >= 0 else 0
        count[i] = k if i == 0 else max(1, int(fill * k) - int(r.integers(0, 5)))
        for d in range(count[i]):
            if r.random() < 0.7:
                boxes[i, d] = gb[i, r.integers(0, gc[i])]
                boxes[i, d, 0] += SHIFTS[r.integers(0, 4)] * (1 if r.random() < 0.5 else -1)
            else:
                boxes[i, d] = [1000.0 + PITCH * d, 500.0, 2.0, 4.0, 0.0, 1.0]
        scores[i, :count[i]] = r.integers(1, 16, count[i]).astype(np.float32) / 16
    return {"boxes": boxes, "scores": scores, "count": count}, gb, gc, st


def named(name):
    """-> dict(det, gb, gc, st, S, thrs, batch, status): `status` is the accumulator's status word after one update with
    room for every record"""
    if name == "k65_g17_s2":           # two 64-row blocks of the IoU launch, two 16-column pieces, an image without ground truth
        det, gb, gc, st = make(1, 3, 65, 17, 2)
        gc[2] = 0
        return dict(det=det, gb=gb, gc=gc, st=st, S=2, thrs=THRS2, batch=1, status=0)
    if name == "k257_g17_s8_t8":       # two 256-row blocks of the claim / tp launches, batch 2, counts outside [0, K] and [0, G]
        det, gb, gc, st = make(2, 4, 257, 17, 8, fill=0.3)
        det["count"][0] = 257 + 9
        det["count"][1] = -3
        gc[0] = 17 + 4
        return dict(det=det, gb=gb, gc=gc, st=st, S=8, thrs=THRS8, batch=2, status=0)
    if name == "s1":                   # one stratum, no don't-care box: MeanAP's figures
        det, gb, gc, st = make(3, 3, 65, 17, 1, dont_care=0.0)
        return dict(det=det, gb=gb, gc=gc, st=st, S=1, thrs=THRS2, batch=1, status=0)
    if name == "bad_strata":           # a stratum of S and one of -2 below gt_count: status bit 2, both count as -1
        det, gb, gc, st = make(4, 3, 65, 17, 2)
        st[0, 0], st[1, 2] = 2, -2
        return dict(det=det, gb=gb, gc=gc, st=st, S=2, thrs=THRS2, batch=1, status=4)
    if name == "nonfinite":            # an image whose scores are all non-finite: status bit 1, no record from it
        det, gb, gc, st = make(5, 3, 65, 17, 2)
        det["scores"][1, 0::3], det["scores"][1, 1::3], det["scores"][1, 2::3] = np.nan, np.inf, -np.inf
        return dict(det=det, gb=gb, gc=gc, st=st, S=2, thrs=THRS2, batch=1, status=2)
    if name == "no_dont_care":         # the partition identity
        det, gb, gc, st = make(6, 4, 65, 17, 3, dont_care=0.0)
        return dict(det=det, gb=gb, gc=gc, st=st, S=3, thrs=THRS2, batch=2, status=0)
    raise KeyError(name)


NAMES = ("k65_g17_s2", "k257_g17_s8_t8", "s1", "bad_strata", "nonfinite", "no_dont_care")


def hand():
    """The issue's hand case: one image, ground truth A (stratum 0), B (stratum 1), C (don't care); d1 0.90 = B, d3 0.85
    far from everything, d2 0.80 = A, d4 0.60 = C, d5 0.50 = A again; one threshold 0.5."""
    a, b, c = _gt_row(0), _gt_row(5), _gt_row(40)
    rows = [(b, 0.90), ([1000.0, 500.0, 2.0, 4.0, 0.0, 1.0], 0.85), (a, 0.80), (c, 0.60), (a, 0.50)]
    det = {"boxes": np.asarray([[r[0] for r in rows]], np.float32), "scores": np.asarray([[r[1] for r in rows]], np.float32),
           "count": np.asarray([5], np.int32)}
    return dict(det=det, gb=np.asarray([[a, b, c]], np.float32), gc=np.asarray([3], np.int32),
                st=np.asarray([[0, 1, -1]], np.int32), S=2, thrs=(0.5,), batch=1, status=0)


# ---- the plain restatement ------------------------------------------------------------------------------------------------
def _iou(d, t):
    """axis-aligned rectangles (x, y, w, h): exact for the cases of this file"""
    ix = min(d[0] + d[2] / 2, t[0] + t[2] / 2) - max(d[0] - d[2] / 2, t[0] - t[2] / 2)
    iy = min(d[1] + d[3] / 2, t[1] + t[3] / 2) - max(d[1] - d[3] / 2, t[1] - t[3] / 2)
    if ix <= 0 or iy <= 0:
        return 0.0
    inter = ix * iy
    return inter / (d[2] * d[3] + t[2] * t[3] - inter)


def brute_match(case):
    """One image after another, one row after another: the dict host_match_strata returns, and the records as a list of
    (score, agent, tp bits, stratum, reach bits, best_gt) in accumulation order."""
    det, gb, gc, st, S, thrs, batch = (case[q] for q in ("det", "gb", "gc", "st", "S", "thrs", "batch"))
    n, k = det["scores"].shape
    g = gb.shape[1]
    out = {"best_iou": np.zeros((n, k)), "best_gt": np.full((n, k), -1, np.int32), "rank": np.full((n, k), -1, np.int32),
           "tp": np.zeros((len(thrs), n, k), np.uint8), "gt_claim": np.full((len(thrs), n, g), -1, np.int32),
           "stratum": np.full((n, k), -1, np.int32), "reach": np.zeros((n, k), np.uint8),
           "counts": np.zeros((n, S + 1), np.int64), "status": 0}
    records = []
    for img in range(n):
        c, cg = min(max(int(det["count"][img]), 0), k), min(max(int(gc[img]), 0), g)
        strata = []
        for j in range(cg):
            s = int(st[img, j])
            if s < -1 or s >= S:
                out["status"] |= 4
                s = -1
            strata.append(s)
            out["counts"][img, S if s < 0 else s] += 1
        rows = [i for i in range(c) if math.isfinite(float(det["scores"][img, i]))]
        out["status"] |= 2 if len(rows) < c else 0
        rows.sort(key=lambda i: (-float(det["scores"][img, i]), i))
        taken = [set() for _ in thrs]
        for r, i in enumerate(rows):
            out["rank"][img, i] = r
            best, best_j = 0.0, -1
            for j in range(cg):
                v = _iou([float(x) for x in det["boxes"][img, i, :4]], [float(x) for x in gb[img, j, :4]])
                if v > best:
                    best, best_j = v, j
            out["best_iou"][img, i], out["best_gt"][img, i] = best, best_j
            tp_bits = reach = 0
            for t, thr in enumerate(thrs):
                if best_j >= 0 and best >= thr:
                    reach |= 1 << t
                    if best_j not in taken[t]:
                        taken[t].add(best_j)
                        tp_bits |= 1 << t
                        out["tp"][t, img, i] = 1
                        out["gt_claim"][t, img, best_j] = r
            s = strata[best_j] if best_j >= 0 else -1
            out["stratum"][img, i], out["reach"][img, i] = s, reach
            records.append((float(det["scores"][img, i]), img // batch, tp_bits, s, reach, best_j))
    return out, records


def record_words(records):
    """brute_match's records as the [R, 4] uint32 words of the C ABI"""
    out = np.zeros((len(records), 4), np.uint32)
    for q, (score, agent, tp_bits, s, reach, best_j) in enumerate(records):
        out[q] = (np.float32(score).view(np.uint32), (agent << 8) | tp_bits, ((s + 1) << 8) | reach,
                  np.int32(best_j).view(np.uint32))
    return out


def brute_ap(scores, hits, n_gt):
    """area under the interpolated precision / recall curve, one record after another"""
    if n_gt == 0:
        return 0.0
    order = sorted(range(len(scores)), key=lambda q: (-scores[q], q))
    tp = fp = 0
    rec, pre = [0.0], [0.0]
    for q in order:
        tp, fp = tp + (1 if hits[q] else 0), fp + (0 if hits[q] else 1)
        rec.append(tp / n_gt)
        pre.append(tp / max(tp + fp, 1))
    rec.append(1.0)
    pre.append(0.0)
    for q in range(len(pre) - 2, -1, -1):
        pre[q] = max(pre[q], pre[q + 1])
    steps = [(rec[q + 1] - rec[q]) * pre[q + 1] for q in range(len(rec) - 1) if rec[q + 1] != rec[q]]
    return float(np.sum(np.asarray(steps, np.float64)))         # numpy's summation order, as the library's function has it


def brute_row(records, counts, thrs, stratum, agent=None):
    """one row of the table from brute_match's records; stratum None = "all"; counts [n_agents][S + 1]"""
    S = len(counts[0]) - 1
    rows = [a for a in range(len(counts)) if agent is None or a == agent]
    n_gt = sum(int(counts[a][s]) for a in rows for s in range(S) if stratum is None or s == stratum)
    recs = [r for r in records if agent is None or r[1] == agent]
    out = {"n_gt": n_gt, "n_det": len(recs), "n_counted": [], "n_left_out": [], "n_tp": []}
    for t, thr in enumerate(thrs):
        kept = []
        for r in recs:
            reaches = (r[4] >> t) & 1
            if reaches and (r[3] == -1 if stratum is None else r[3] != stratum):
                continue
            kept.append(r)
        hits = [(r[2] >> t) & 1 for r in kept]
        out["AP@%g" % thr] = brute_ap([r[0] for r in kept], hits, n_gt)
        out["recall@%g" % thr] = sum(hits) / n_gt if n_gt else float("nan")
        out["n_counted"].append(len(kept))
        out["n_left_out"].append(len(recs) - len(kept))
        out["n_tp"].append(sum(hits))
    return out


def agent_counts(counts, batch):
    """per-image counts [N, S + 1] -> per-agent"""
    counts = np.asarray(counts)
    out = np.zeros((-(-len(counts) // batch), counts.shape[1]), np.int64)
    for i, row in enumerate(counts):
        out[i // batch] += row
    return out


def same_row(got, want):
    """two rows of the table: integers equal, floats equal as float64 bits (NaN included)"""
    keys = set(want)
    assert keys <= set(got), (keys, set(got))
    for key in keys:
        if isinstance(want[key], float):
            assert np.float64(got[key]).view(np.uint64) == np.float64(want[key]).view(np.uint64), (key, got[key], want[key])
        else:
            assert got[key] == want[key], (key, got[key], want[key])
