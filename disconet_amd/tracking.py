"""Multi-object tracking behind the detection tail: the last stage of the reference's det pipeline (train -> test ->
track; its tools dump each agent's detections with --tracking and hand them to a SORT tracker, `make sort`).

What the reference's tracker computes is RECALLED, NOT PINNED: the reference checkout holds no source.  The
contract is this project's own -- SORT (Bewley et al., "Simple online and realtime tracking") with filterpy's
constant-velocity Kalman filter as recalled -- and HostSort below is its normative statement: numpy / float64, every
sum written out in a fixed order, only + - * / and sqrt (the hypot of postprocess._corners is written sqrt(s s + c c) here), so that the GPU
kernel (dn_track_step, csrc/track.hip, built without contraction) reproduces it bit for bit.  Sort runs the same
contract on the GPU, one workgroup per image, graph-capturable behind detect(); the full text of the contract is in
include/disconet_hip.h.

Every image of the agent-major batch (image = agent * B + b) is its own sequence with its own tracker.

The stage behind it (`make eval`) is here too: the CLEAR MOT figures of the tracks against ground-truth boxes with
identities -- HostClearMot states that contract in the same way, ClearMot runs it on the GPU (dn_mot_step,
csrc/mot_eval.hip), graph-capturable behind Sort.update().  Beside them the identity figures (IDF1, IDP, IDR and the
counts) of the same kit, again recalled, not pinned: HostIdentity states that contract, Identity runs it on the GPU --
per frame dn_idf_step counts the overlapping (identity, track id) pairs into a matrix that stays on the device, at the
end dn_idf_finish solves the one global assignment over it there (csrc/idf_eval.hip).  And the third family, HOTA with
its detection, association and localisation parts: HostHota states that contract, Hota runs it on the GPU -- per frame
dn_hota_step adds to the potential-match matrix and logs the frame on the device, at the end dn_hota_finish matches every
logged frame of every image at once under the global alignment score (csrc/hota_eval.hip).
"""
import numpy as np
import torch

from . import _lib
from .postprocess import MAX_TOP_K, _host

MAX_TRACKS = 128          # track slots per image (M)
MAX_DETS = 128            # valid detection rows considered per image and frame
HEADER_BYTES = 64         # per image: int32 frame_count, next_id, n_tracks, status, 12 spare words (zero)
RECORD_BYTES = 480        # per slot: float64 x[7], P[7][7]; int32 id, age, hits, hit_streak, time_since_update, 3 spare
STATUS_BITS = ((1, "a birth found all max_tracks slots taken and was dropped"),
               (2, "a detection row below its count was invalid (non-finite score or rectangle, or no positive width / "
                   "height) and was ignored"),
               (4, "more than %d valid detection rows in one image; the rows past the first %d were ignored"
                   % (MAX_DETS, MAX_DETS)))

_R = (1.0, 1.0, 10.0, 10.0)
_Q = (1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001)
_P0 = (10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4)


def _check_params(max_age, min_hits, iou_threshold, scale, max_tracks):
    max_age, min_hits, max_tracks = int(max_age), int(min_hits), int(max_tracks)
    iou_threshold, scale = float(iou_threshold), float(scale)
    if max_age < 0 or min_hits < 0:
        raise ValueError("max_age = %d, min_hits = %d: both must be >= 0" % (max_age, min_hits))
    if not (np.isfinite(iou_threshold) and iou_threshold >= 0):
        raise ValueError("iou_threshold = %r: must be finite and >= 0" % iou_threshold)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("scale = %r: must be finite and > 0" % scale)
    if not 1 <= max_tracks <= MAX_TRACKS:
        raise ValueError("max_tracks = %d: 1..%d are supported" % (max_tracks, MAX_TRACKS))
    return max_age, min_hits, iou_threshold, scale, max_tracks


def state_bytes(n_images, max_tracks):
    """Bytes of the tracker state of n_images images (what dn_track_state_bytes returns)."""
    return int(n_images) * (HEADER_BYTES + RECORD_BYTES * int(max_tracks))


def _status_text(words):
    out = []
    for img, w in enumerate(words):
        for bit, text in STATUS_BITS:
            if int(w) & bit:
                out.append("image %d: %s" % (img, text))
    return out


# ---------------------------------------------------------------------------
# the host reference: every operation in the order the kernel runs it
# ---------------------------------------------------------------------------
def _rect_of_state(x):
    """(u, v, s, r, ...) -> (x1, y1, x2, y2): w = sqrt(s r), h = s / w."""
    with np.errstate(all="ignore"):
        w = np.sqrt(x[2] * x[3])
        h = x[2] / w
        return np.array([x[0] - w / 2.0, x[1] - h / 2.0, x[0] + w / 2.0, x[1] + h / 2.0], dtype=np.float64)


def iou_rect(a, b):
    """Axis-aligned IoU of (x1, y1, x2, y2) rectangles: 0 when the intersection is empty or the union <= 0."""
    w = min(a[2], b[2]) - max(a[0], b[0])
    h = min(a[3], b[3]) - max(a[1], b[1])
    if not (w > 0 and h > 0):
        return 0.0
    inter = w * h
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return float(inter / union) if union > 0 else 0.0


def hungarian_max(iou):
    """The assignment that maximises the total of `iou` [T, D] (float64): shortest augmenting paths on cost = -iou.
    Rows are the smaller side (the tracks when T <= D), processed in ascending order; potentials start at 0; the next
    column is the unused one with the smallest reduced cost, the lowest index among equals; a row's search takes at
    most (columns + 1) steps, so everything ends after rows x (columns + 1) steps whatever the numbers are.  Returns
    the pairs [(t, d)] in column order."""
    iou = np.asarray(iou, dtype=np.float64)
    t_n, d_n = iou.shape
    if t_n == 0 or d_n == 0:
        return []
    transposed = t_n > d_n
    cost = -(iou.T if transposed else iou)
    n, m = cost.shape
    inf = np.inf
    u = np.zeros(n + 1)
    v = np.zeros(m + 1)
    p = np.zeros(m + 1, dtype=np.int64)          # p[j] = row (1-based) that holds column j; column 0 is virtual
    way = np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(m + 1, inf)
        used = np.zeros(m + 1, dtype=bool)
        found = False
        for _ in range(m + 1):
            used[j0] = True
            i0 = p[j0]
            free = ~used[1:]
            cur = (cost[i0 - 1] - u[i0]) - v[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], inf)
            j1 = int(np.argmin(cand)) + 1          # the first (lowest) column among equal minima
            delta = cand[j1 - 1]
            if not delta < inf:
                break                              # nothing to reach (only with non-finite input): the row stays free
            up = np.nonzero(used)[0]
            u[p[up]] = u[p[up]] + delta
            v[up] = v[up] - delta
            minv[~used] = minv[~used] - delta
            j0 = j1
            if p[j0] == 0:
                found = True
                break
        if not found:
            p[0] = 0
            continue
        for _ in range(m + 1):
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            if j0 == 0:
                break
    pairs = []
    for j in range(1, m + 1):
        if p[j] > 0:
            pairs.append((j - 1, int(p[j]) - 1) if transposed else (int(p[j]) - 1, j - 1))
    return pairs


def associate(iou, iou_threshold):
    """SORT's association on an IoU matrix [T, D] -> (track -> detection or -1 [T], path): "shortcut" when every row and
    column holds at most one entry above the threshold (those entries are the matches), "hungarian" otherwise; either
    way a pair with iou < iou_threshold is unmatched.  path is "none" when there is nothing to associate."""
    iou = np.asarray(iou, dtype=np.float64)
    t_n, d_n = iou.shape
    match = np.full(t_n, -1, dtype=np.int64)
    if t_n == 0 or d_n == 0:
        return match, "none"
    a = iou > iou_threshold
    if a.sum(1).max() <= 1 and a.sum(0).max() <= 1:
        for t, d in zip(*np.nonzero(a)):
            match[t] = d
        return match, "shortcut"
    for t, d in hungarian_max(iou):
        if not iou[t, d] < iou_threshold:
            match[t] = d
    return match, "hungarian"


def _predict(trk):
    x, P = trk["x"], trk["P"]
    if x[6] + x[2] <= 0:
        x[6] = 0.0
    for i in range(3):                       # x = F x, F = I + ones at (0,4), (1,5), (2,6), in its sparse form
        x[i] = x[i] + x[i + 4]
    A = P.copy()                             # A = F P
    A[0:3, :] = P[0:3, :] + P[4:7, :]
    B = A.copy()                             # B = A F^T
    B[:, 0:3] = A[:, 0:3] + A[:, 4:7]
    for i in range(7):                       # + Q
        B[i, i] = B[i, i] + _Q[i]
    trk["P"] = B
    trk["age"] += 1
    if trk["tsu"] > 0:
        trk["streak"] = 0
    trk["tsu"] += 1


def _update(trk, z):
    x, P = trk["x"], trk["P"]
    trk["tsu"] = 0
    trk["hits"] += 1
    trk["streak"] += 1
    with np.errstate(all="ignore"):
        y = [z[i] - x[i] for i in range(4)]
        # S = P[:4, :4] + R: its lower triangle, factored L L^T in place
        L = np.zeros((4, 4))
        for i in range(4):
            for j in range(i + 1):
                s = P[i, j] + _R[i] if i == j else P[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
        # K = P[:, :4] S^-1: per row r, L w = P[r, :4], then L^T k = w
        K = np.zeros((7, 4))
        for r in range(7):
            w = [0.0] * 4
            for i in range(4):
                s = P[r, i]
                for k in range(i):
                    s = s - L[i, k] * w[k]
                w[i] = s / L[i, i]
            for i in (3, 2, 1, 0):
                s = w[i]
                for k in range(i + 1, 4):
                    s = s - L[k, i] * K[r, k]
                K[r, i] = s / L[i, i]
        for r in range(7):
            s = K[r, 0] * y[0]
            for j in range(1, 4):
                s = s + K[r, j] * y[j]
            x[r] = x[r] + s
        A = np.eye(7)                        # I - K H
        A[:, 0:4] = A[:, 0:4] - K
        AP = A[:, 0:1] * P[0:1, :]           # (A P)[r][c] = sum over k, left to right
        for k in range(1, 7):
            AP = AP + A[:, k:k + 1] * P[k:k + 1, :]
        J = AP[:, 0:1] * A[:, 0][None, :]    # (AP A^T)[r][c] = sum over k of AP[r][k] A[c][k]
        for k in range(1, 7):
            J = J + AP[:, k:k + 1] * A[:, k][None, :]
        KR = K * np.asarray(_R)[None, :]
        G = KR[:, 0:1] * K[:, 0][None, :]    # (K R K^T)[r][c]
        for j in range(1, 4):
            G = G + KR[:, j:j + 1] * K[:, j][None, :]
        trk["P"] = J + G


def _corners(b):
    """[K, 6] rows (x, y, w, h, sin, cos), float64 -> [K, 4, 2] corners: postprocess._corners operation for operation,
    but for its hypot, written sqrt(s s + c c) -- a library hypot is not the same bits on every platform, sqrt is."""
    n = np.maximum(np.sqrt(b[:, 4] * b[:, 4] + b[:, 5] * b[:, 5]), 1e-12)
    s, c = b[:, 4] / n, b[:, 5] / n
    dx, dy = b[:, 2] / 2.0, b[:, 3] / 2.0
    lx, ly = np.stack([-dx, dx, dx, -dx], 1), np.stack([-dy, -dy, dy, dy], 1)
    x = lx * c[:, None] - ly * s[:, None] + b[:, None, 0]
    y = lx * s[:, None] + ly * c[:, None] + b[:, None, 1]
    return np.stack([x, y], -1)


def _measure(boxes, scores, count, scale):
    """One image's rows -> (rows [D] of the valid detections used, rect [D, 4], z [D, 4], status bits)."""
    k = boxes.shape[0]
    c = min(max(int(count), 0), k)
    status = 0
    rows, rects, zs = [], [], []
    if c:
        with np.errstate(all="ignore"):
            cr = _corners(np.asarray(boxes[:c], dtype=np.float64)) * scale       # [c, 4, 2]
            x1, y1 = cr[:, :, 0].min(1), cr[:, :, 1].min(1)
            x2, y2 = cr[:, :, 0].max(1), cr[:, :, 1].max(1)
            w, h = x2 - x1, y2 - y1
            ok = (np.isfinite(scores[:c]) & np.isfinite(x1) & np.isfinite(y1) & np.isfinite(x2) & np.isfinite(y2)
                  & (w > 0) & (h > 0))
            if not ok.all():
                status |= 2
            valid = np.nonzero(ok)[0]
            if len(valid) > MAX_DETS:
                status |= 4
                valid = valid[:MAX_DETS]
            for i in valid:
                rows.append(int(i))
                rects.append((x1[i], y1[i], x2[i], y2[i]))
                zs.append((x1[i] + w[i] / 2.0, y1[i] + h[i] / 2.0, w[i] * h[i], w[i] / h[i]))
    return rows, np.asarray(rects, dtype=np.float64).reshape(-1, 4), np.asarray(zs, dtype=np.float64).reshape(-1, 4), status


class HostSort:
    """The numpy / float64 reference of Sort: the same interface on host arrays, and the statement of the contract.

    update(det): det = {"boxes" [N, K, 6], "scores" [N, K], "count" [N]} (numpy or tensors) -> numpy
    {"rect" [N, M, 4] float64 (x1, y1, x2, y2 in scaled units), "id" [N, M] int32, "det" [N, M] int32 (the detection row
    the track took this frame), "score" [N, M] float32, "count" [N] int32, "det_track" [N, K] int32}; rows at or past
    count are 0 with id and det -1.  last_path[image] names the association path of the last frame ("none", "shortcut",
    "hungarian")."""

    def __init__(self, max_age=1, min_hits=3, iou_threshold=0.3, scale=1.0, max_tracks=MAX_TRACKS):
        (self.max_age, self.min_hits, self.iou_threshold, self.scale,
         self.max_tracks) = _check_params(max_age, min_hits, iou_threshold, scale, max_tracks)
        self.images = None
        self.last_path = []

    def reset(self):
        if self.images is not None:
            self.images = [self._fresh() for _ in self.images]

    @staticmethod
    def _fresh():
        return {"frame_count": 0, "next_id": 1, "status": 0, "tracks": []}

    def update(self, det):
        boxes = np.asarray(_host(det["boxes"]), dtype=np.float32)
        scores = np.asarray(_host(det["scores"]), dtype=np.float32)
        count = np.asarray(_host(det["count"])).reshape(-1)
        n, k = scores.shape
        if not 1 <= k <= MAX_TOP_K or tuple(boxes.shape) != (n, k, 6) or count.shape[0] != n:
            raise ValueError("shapes: boxes %s scores %s count %s" % (boxes.shape, scores.shape, count.shape))
        if self.images is None:
            self.images = [self._fresh() for _ in range(n)]
        if len(self.images) != n:
            raise ValueError("the tracker holds %d images, this call has %d (reset() keeps the count)" % (len(self.images), n))
        m = self.max_tracks
        out = {"rect": np.zeros((n, m, 4), dtype=np.float64), "id": np.full((n, m), -1, dtype=np.int32),
               "det": np.full((n, m), -1, dtype=np.int32), "score": np.zeros((n, m), dtype=np.float32),
               "count": np.zeros(n, dtype=np.int32), "det_track": np.full((n, k), -1, dtype=np.int32)}
        self.last_path = []
        for img in range(n):
            self.last_path.append(self._step(self.images[img], boxes[img], scores[img], count[img], img, out))
        return out

    def _step(self, st, boxes, scores, count, img, out):
        m = self.max_tracks
        st["frame_count"] += 1
        rows, rects, zs, status = _measure(boxes, scores, count, self.scale)
        st["status"] |= status
        # predict; a track whose rectangle is not finite is deleted here
        alive, trects = [], []
        for trk in st["tracks"]:
            _predict(trk)
            r = _rect_of_state(trk["x"])
            if np.isfinite(r).all():
                alive.append(trk)
                trects.append(r)
        iou = np.zeros((len(alive), len(rows)), dtype=np.float64)
        for t in range(len(alive)):
            for d in range(len(rows)):
                iou[t, d] = iou_rect(trects[t], rects[d])
        match, path = associate(iou, self.iou_threshold)
        taken = np.zeros(len(rows), dtype=bool)
        for t, trk in enumerate(alive):
            trk["det"] = -1
            if match[t] >= 0:
                d = int(match[t])
                taken[d] = True
                _update(trk, zs[d])
                trk["det"] = rows[d]
                out["det_track"][img, rows[d]] = trk["id"]
        # deletions are decided first, then the births fill what is free, then the report
        tracks = [trk for trk in alive if not trk["tsu"] > self.max_age]
        for d in range(len(rows)):
            if taken[d]:
                continue
            if len(tracks) >= m:
                st["status"] |= 1
                continue
            P = np.zeros((7, 7), dtype=np.float64)
            for i in range(7):
                P[i, i] = _P0[i]
            trk = {"x": np.array(list(zs[d]) + [0.0, 0.0, 0.0], dtype=np.float64), "P": P, "id": st["next_id"], "age": 0,
                   "hits": 0, "streak": 0, "tsu": 0, "det": rows[d]}
            st["next_id"] += 1
            tracks.append(trk)
            out["det_track"][img, rows[d]] = trk["id"]
        c = 0
        for trk in tracks:
            if trk["tsu"] < 1 and (trk["streak"] >= self.min_hits or st["frame_count"] <= self.min_hits):
                out["rect"][img, c] = _rect_of_state(trk["x"])
                out["id"][img, c] = trk["id"]
                out["det"][img, c] = trk["det"]
                out["score"][img, c] = scores[trk["det"]]
                c += 1
        out["count"][img] = c
        st["tracks"] = tracks
        return path

    def status_words(self):
        """The status word of every image (numpy int32), without raising."""
        return np.asarray([st["status"] for st in (self.images or [])], dtype=np.int32)

    def status(self):
        """Raise DnError naming the set status bits (a run is never silently truncated); returns 0 otherwise."""
        text = _status_text(self.status_words())
        if text:
            raise _lib.DnError("Sort: " + "; ".join(text))
        return 0

    def state_bytes(self):
        """The state in the device layout (numpy uint8), byte for byte what Sort.state_bytes() returns for the same run."""
        m = self.max_tracks
        imgs = self.images or []
        buf = np.zeros((len(imgs), HEADER_BYTES + RECORD_BYTES * m), dtype=np.uint8)
        for i, st in enumerate(imgs):
            buf[i, :16] = np.asarray([st["frame_count"], st["next_id"], len(st["tracks"]), st["status"]],
                                     dtype=np.int32).view(np.uint8)
            for s, trk in enumerate(st["tracks"]):
                o = HEADER_BYTES + RECORD_BYTES * s
                buf[i, o:o + 56] = np.asarray(trk["x"], dtype=np.float64).view(np.uint8)
                buf[i, o + 56:o + 448] = np.ascontiguousarray(trk["P"], dtype=np.float64).reshape(-1).view(np.uint8)
                buf[i, o + 448:o + 468] = np.asarray([trk["id"], trk["age"], trk["hits"], trk["streak"], trk["tsu"]],
                                                     dtype=np.int32).view(np.uint8)
        return buf.reshape(-1)


# ---------------------------------------------------------------------------
# the same contract on the GPU (dn_track_step): one workgroup per image, kernel launches only
# ---------------------------------------------------------------------------
class Sort:
    """SORT on the GPU behind detect(): update() after every frame enqueues dn_track_step on torch's current stream
    (the state -- per image a header and max_tracks track records -- lives on the device, is allocated on first use and
    is never read back), so forward + detect() + update() can be one captured graph (graph.GraphedStep).  HostSort is
    the reference it equals bit for bit.

    update(det) takes detect()'s dict (device tensors "boxes" [N, K, 6], "scores" [N, K], "count" [N]; K <= 1024, at
    most 128 valid rows per image are used) and returns device tensors {"rect" [N, M, 4] float64, "id", "det" [N, M]
    int32, "score" [N, M] float32, "count" [N] int32, "det_track" [N, K] int32} as HostSort does.  `scale` multiplies the
    corners before the rectangle is taken (the tools pass 1 / voxel_size[0] = 4 px/m).  status() makes one small copy
    and raises DnError naming the sticky status bits.

    GraphedStep runs its step three times to warm up before it captures and those runs advance the tracker: call
    reset() after constructing the GraphedStep, before the first replay that counts (as with MeanAP)."""

    def __init__(self, max_age=1, min_hits=3, iou_threshold=0.3, scale=1.0, max_tracks=MAX_TRACKS):
        (self.max_age, self.min_hits, self.iou_threshold, self.scale,
         self.max_tracks) = _check_params(max_age, min_hits, iou_threshold, scale, max_tracks)
        self.state = None            # uint8 [N * (HEADER_BYTES + RECORD_BYTES * M)] on the device
        self.n_images = 0

    def _inputs(self, det):
        from .ops import _need_gpu
        boxes, scores, count = det["boxes"], det["scores"], det["count"]
        for t in (boxes, scores, count):
            if not isinstance(t, torch.Tensor):
                raise _lib.DnError("Sort.update needs device tensors (got %s); HostSort is the numpy reference"
                                   % type(t).__name__)
        _need_gpu(boxes, scores, count)
        n, k = scores.shape
        if not 1 <= k <= MAX_TOP_K:
            raise ValueError("K = %d detection rows: 1..%d are supported" % (k, MAX_TOP_K))
        if tuple(boxes.shape) != (n, k, 6) or count.numel() != n:
            raise ValueError("shapes: boxes %s scores %s count %s" % (tuple(boxes.shape), tuple(scores.shape),
                                                                      tuple(count.shape)))
        return (boxes.to(torch.float32).contiguous(), scores.to(torch.float32).contiguous(),
                count.to(torch.int32).contiguous(), n, k)

    def reset(self):
        """Forget every track: frame_count 0, ids from 1 again, status 0 (one launch on the current stream)."""
        if self.state is not None:
            from .ops import _ptr, _stream
            _lib.check(_lib.load().dn_track_reset(_ptr(self.state), self.n_images, self.max_tracks, _stream()),
                       "dn_track_reset")

    def update(self, det):
        from .ops import _ptr, _stream
        boxes, scores, count, n, k = self._inputs(det)
        lib = _lib.load()
        dev = scores.device
        _hold_state(self, "tracker", "dn_track_state_bytes", state_bytes, (n, self.max_tracks), dev)
        m = self.max_tracks
        out = {"rect": torch.empty((n, m, 4), dtype=torch.float64, device=dev),
               "id": torch.empty((n, m), dtype=torch.int32, device=dev),
               "det": torch.empty((n, m), dtype=torch.int32, device=dev),
               "score": torch.empty((n, m), dtype=torch.float32, device=dev),
               "count": torch.empty((n,), dtype=torch.int32, device=dev),
               "det_track": torch.empty((n, k), dtype=torch.int32, device=dev)}
        _lib.check(lib.dn_track_step(_ptr(boxes), _ptr(scores), _ptr(count), n, k, m, self.max_age, self.min_hits,
                                     self.iou_threshold, self.scale, _ptr(self.state), _ptr(out["rect"]), _ptr(out["id"]),
                                     _ptr(out["det"]), _ptr(out["score"]), _ptr(out["count"]), _ptr(out["det_track"]),
                                     _stream()), "dn_track_step")
        return out

    def status_words(self):
        """The status word of every image (numpy int32): one small copy, waits for the device."""
        return _status_words(self.state, self.n_images, 12)

    def status(self):
        """Raise DnError naming the set status bits (a run is never silently truncated); returns 0 otherwise."""
        text = _status_text(self.status_words())
        if text:
            raise _lib.DnError("Sort: " + "; ".join(text))
        return 0

    def state_bytes(self):
        """A host copy of the whole state (numpy uint8); HostSort.state_bytes() is its reference."""
        return self.state.cpu().numpy().copy() if self.state is not None else np.zeros(0, dtype=np.uint8)


def mot_rows(out, frame):
    """update()'s dict (host or device) -> per image the list of MOT lines `frame,id,x1,y1,w,h,score,-1,-1,-1` of the
    reported tracks, in ascending id: the form the reference's tracking dump is recalled to have."""
    rect, ids, score, count = _host(out["rect"]), _host(out["id"]), _host(out["score"]), _host(out["count"])
    lines = []
    for img in range(rect.shape[0]):
        rows = []
        for r in range(int(count[img])):
            x1, y1, x2, y2 = (float(v) for v in rect[img, r])
            rows.append("%d,%d,%.4f,%.4f,%.4f,%.4f,%.6f,-1,-1,-1" % (int(frame), int(ids[img, r]), x1, y1, x2 - x1,
                                                                    y2 - y1, float(score[img, r])))
        lines.append(rows)
    return lines


# ---------------------------------------------------------------------------
# CLEAR MOT evaluation of the tracks (dn_mot_step, csrc/mot_eval.hip): the stage behind the tracker
# ---------------------------------------------------------------------------
MAX_GT_ROWS = 1024        # ground-truth rows per image (G)
MAX_GT_USED = 128         # valid ground-truth rows used per image and frame
MAX_GT_IDS = 1024         # upper limit of max_gt_ids
MOT_HEADER_BYTES = 64     # per image: int64 frames, TP, FP, FN, IDSW; float64 motp_sum; int32 status; 12 spare bytes (zero)
MOT_RECORD_BYTES = 32     # per identity: int32 last, pst, frames_present, frames_matched, segments, 3 spare (zero)
MOT_CONTINUITY = 1000.0   # added to the score of the pair an identity held in the previous frame
MOT_STATUS_BITS = ((1, "more than %d valid ground-truth rows in one image; the rows past the first %d were ignored"
                       % (MAX_GT_USED, MAX_GT_USED)),
                   (2, "a ground-truth row below its count was invalid (non-finite rectangle, or no positive width / "
                       "height) and was ignored"),
                   (4, "a ground-truth id was outside 0 .. max_gt_ids - 1 and its row was ignored"),
                   (8, "a ground-truth id came twice in one frame; the lower row was kept"))
MOT_FIGURES = ("MOTA", "MOTP", "TP", "FP", "FN", "IDSW", "Frag", "MT", "PT", "ML")


def _check_mot_params(batch_size, iou_threshold, scale, max_gt_ids):
    batch_size, max_gt_ids = int(batch_size), int(max_gt_ids)
    iou_threshold, scale = float(iou_threshold), float(scale)
    if batch_size < 1:
        raise ValueError("batch_size = %d: must be positive" % batch_size)
    if not (np.isfinite(iou_threshold) and 0.0 < iou_threshold <= 1.0):
        raise ValueError("iou_threshold = %r: must be in (0, 1]" % iou_threshold)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("scale = %r: must be finite and > 0" % scale)
    if not 1 <= max_gt_ids <= MAX_GT_IDS:
        raise ValueError("max_gt_ids = %d: 1..%d are supported" % (max_gt_ids, MAX_GT_IDS))
    return batch_size, iou_threshold, scale, max_gt_ids


def mot_state_bytes(n_images, max_gt_ids):
    """Bytes of the evaluation state of n_images images (what dn_mot_state_bytes returns)."""
    return int(n_images) * (MOT_HEADER_BYTES + MOT_RECORD_BYTES * int(max_gt_ids))


def _mot_status_text(words):
    out = []
    for img, w in enumerate(words):
        for bit, text in MOT_STATUS_BITS:
            if int(w) & bit:
                out.append("image %d: %s" % (img, text))
    return out


def _mot_figures(c):
    """Counters {"TP", "FP", "FN", "IDSW", "Frag", "MT", "PT", "ML", "motp_sum", "frames"} -> the CLEAR figures."""
    tp, fp, fn, idsw = c["TP"], c["FP"], c["FN"], c["IDSW"]
    out = {"MOTA": float(tp - fp - idsw) / float(max(1, tp + fn)), "MOTP": float(c["motp_sum"]) / float(max(1, tp)),
           "Recall": float(tp) / float(max(1, tp + fn)), "Precision": float(tp) / float(max(1, tp + fp))}
    out.update({key: int(c[key]) for key in ("TP", "FP", "FN", "IDSW", "Frag", "MT", "PT", "ML", "frames")})
    return out


def mot_figures_from_state(buf, n_images, max_gt_ids, batch_size, who="ClearMot"):
    """The state bytes (numpy uint8, device layout) -> {"overall": figures, "per_agent": [figures], "per_image":
    [figures]}; float64 on the host, sums over images taken in image order.  Raises DnError naming any status bit."""
    per = MOT_HEADER_BYTES + MOT_RECORD_BYTES * max_gt_ids
    buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(n_images, per)
    text = _mot_status_text(buf[:, 48:52].copy().view(np.int32).reshape(-1))
    if text:
        raise _lib.DnError("%s: %s" % (who, "; ".join(text)))
    images = []
    for i in range(n_images):
        ints = buf[i, :40].copy().view(np.int64)
        rec = buf[i, MOT_HEADER_BYTES:].copy().view(np.int32).reshape(max_gt_ids, 8)
        c = {"frames": int(ints[0]), "TP": int(ints[1]), "FP": int(ints[2]), "FN": int(ints[3]), "IDSW": int(ints[4]),
             "motp_sum": float(buf[i, 40:48].copy().view(np.float64)[0]), "Frag": 0, "MT": 0, "PT": 0, "ML": 0}
        for last, pst, present, matched, segments in rec[:, :5].tolist():
            c["Frag"] += max(segments - 1, 0)
            if present > 0:
                ratio = float(matched) / float(present)
                c["MT" if ratio > 0.8 else ("ML" if ratio < 0.2 else "PT")] += 1
        images.append(c)

    def total(group):
        s = {key: 0 for key in ("frames", "TP", "FP", "FN", "IDSW", "Frag", "MT", "PT", "ML")}
        s["motp_sum"] = 0.0
        for c in group:
            for key in s:
                s[key] = s[key] + c[key]
        return s

    agents = -(-n_images // batch_size)
    return {"overall": _mot_figures(total(images)),
            "per_agent": [_mot_figures(total(images[a * batch_size:(a + 1) * batch_size])) for a in range(agents)],
            "per_image": [_mot_figures(c) for c in images]}


def mot_line(name, figures):
    """One line of the evaluation tool: the CLEAR figures of `name`."""
    return "%s: MOTA %.4f MOTP %.4f TP %d FP %d FN %d IDSW %d Frag %d MT %d PT %d ML %d" % (
        (name,) + tuple(figures[key] for key in MOT_FIGURES))


def _gt_measure(boxes, ids, count, scale, max_gt_ids):
    """One image's ground truth -> (rows, rect [V, 4], ids) of the rows used, status bits.  In this order: the rectangle
    of the scaled corners (_measure's rule) must be finite with positive width and height (else bit 2); the id must be in
    0 .. max_gt_ids - 1 (else bit 4); the first 128 such rows are kept (a 129th sets bit 1); of the kept rows, one whose id
    a lower kept row carries is dropped (bit 8)."""
    g = boxes.shape[0]
    c = min(max(int(count), 0), g)
    status = 0
    rows, rects, idents = [], [], []
    if c:
        with np.errstate(all="ignore"):
            cr = _corners(np.asarray(boxes[:c], dtype=np.float64)) * scale
            x1, y1 = cr[:, :, 0].min(1), cr[:, :, 1].min(1)
            x2, y2 = cr[:, :, 0].max(1), cr[:, :, 1].max(1)
            ok = (np.isfinite(x1) & np.isfinite(y1) & np.isfinite(x2) & np.isfinite(y2) & (x2 - x1 > 0) & (y2 - y1 > 0))
        kept = 0
        for r in range(c):
            if not ok[r]:
                status |= 2
                continue
            ident = int(ids[r])
            if not 0 <= ident < max_gt_ids:
                status |= 4
                continue
            if kept >= MAX_GT_USED:
                status |= 1
                continue
            kept += 1
            if ident in idents:
                status |= 8
                continue
            rows.append(r)
            rects.append((x1[r], y1[r], x2[r], y2[r]))
            idents.append(ident)
    return rows, np.asarray(rects, dtype=np.float64).reshape(-1, 4), idents, status


def _mot_tracks(tracks):
    rect = np.asarray(_host(tracks["rect"]), dtype=np.float64)
    ids = np.asarray(_host(tracks["id"]), dtype=np.int32)
    count = np.asarray(_host(tracks["count"])).reshape(-1)
    return rect, ids, count


def _eval_inputs_host(tracks, gt):
    """ClearMot.update()'s inputs as host arrays, shapes checked -> (rect, tid, tcount, boxes, gids, gcount, n, m, g)."""
    rect, tid, tcount = _mot_tracks(tracks)
    boxes = np.asarray(_host(gt["boxes"]), dtype=np.float32)
    gids = np.asarray(_host(gt["ids"]), dtype=np.int32)
    gcount = np.asarray(_host(gt["count"])).reshape(-1)
    if tid.ndim != 2:
        raise ValueError("shapes: id %s" % (tid.shape,))
    n, m = tid.shape
    g = gids.shape[1] if gids.ndim == 2 else 0
    if (not 1 <= m <= MAX_TRACKS or not 1 <= g <= MAX_GT_ROWS or tuple(rect.shape) != (n, m, 4) or gids.shape[0] != n
            or tuple(boxes.shape) != (n, g, 6) or tcount.shape[0] != n or gcount.shape[0] != n):
        raise ValueError("shapes: rect %s id %s count %s, gt boxes %s ids %s count %s" % (
            rect.shape, tid.shape, tcount.shape, boxes.shape, gids.shape, gcount.shape))
    return rect, tid, tcount, boxes, gids, gcount, n, m, g


def _eval_inputs_device(who, host_name, tracks, gt):
    """ClearMot.update()'s inputs as contiguous device tensors of the library's types, shapes checked -> (rect, tid,
    tcount, boxes, gids, gcount, n, m, g).  `who` and `host_name` name the class and its numpy reference in the errors."""
    from .ops import _need_gpu
    named = (("rect", tracks["rect"]), ("id", tracks["id"]), ("count", tracks["count"]), ("gt boxes", gt["boxes"]),
             ("gt ids", gt["ids"]), ("gt count", gt["count"]))
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise _lib.DnError("%s.update needs device tensors (%s is %s); %s is the numpy reference"
                               % (who, name, type(t).__name__, host_name))
    rect, tid, tcount, boxes, gids, gcount = (t for _, t in named)
    _need_gpu(rect, tid, tcount, boxes, gids, gcount)
    if tid.dim() != 2 or gids.dim() != 2:
        raise ValueError("shapes: id %s, gt ids %s" % (tuple(tid.shape), tuple(gids.shape)))
    (n, m), g = tid.shape, gids.shape[1]
    if not 1 <= m <= MAX_TRACKS:
        raise ValueError("M = %d track rows: 1..%d are supported" % (m, MAX_TRACKS))
    if not 1 <= g <= MAX_GT_ROWS:
        raise ValueError("G = %d ground-truth rows: 1..%d are supported" % (g, MAX_GT_ROWS))
    if (tuple(rect.shape) != (n, m, 4) or tcount.numel() != n or tuple(boxes.shape) != (n, g, 6) or gids.shape[0] != n
            or gcount.numel() != n):
        raise ValueError("shapes: rect %s id %s count %s, gt boxes %s ids %s count %s" % tuple(
            tuple(t.shape) for t in (rect, tid, tcount, boxes, gids, gcount)))
    rect, boxes = rect.to(torch.float64).contiguous(), boxes.to(torch.float32).contiguous()
    tid, tcount, gids, gcount = (t.to(torch.int32).contiguous() for t in (tid, tcount, gids, gcount))
    return rect, tid, tcount, boxes, gids, gcount, n, m, g


def _hold_state(ev, what, lib_name, formula, sizes, device):
    """The head of a device class's update(): on first use allocate ev.state (uint8, 8-byte aligned: viewed from an int64
    allocation) after checking the library's byte count `lib_name`(*sizes) against the module's `formula`(*sizes), set
    ev.n_images = sizes[0] and reset(); afterwards hold every call to that many images."""
    n = sizes[0]
    if ev.state is None:
        nbytes = int(getattr(_lib.load(), lib_name)(*sizes))
        if nbytes != formula(*sizes):
            raise _lib.DnError("%s%r = %d" % (lib_name, tuple(sizes), nbytes))
        ev.state = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device).view(torch.uint8)[:nbytes]
        ev.n_images = n
        ev.reset()
    if n != ev.n_images:
        raise ValueError("the %s holds %d images, this call has %d" % (what, ev.n_images, n))


def _status_words(state, n_images, offset):
    """The int32 status word at byte `offset` of every image's state (numpy int32): one small copy, waits for the device."""
    if state is None:
        return np.zeros(0, dtype=np.int32)
    words = state.view(n_images, -1)[:, offset:offset + 4].contiguous().cpu().numpy()
    return words.view(np.int32).reshape(-1).copy()


class HostClearMot:
    """The numpy / float64 reference of ClearMot and the statement of its contract (the CLEAR MOT metrics as the MOT
    benchmark's evaluation kit computes them, recalled, not pinned; the full text is in include/disconet_hip.h).

    update(tracks, gt): tracks = Sort.update()'s dict (the first `count` rows of "rect" [N, M, 4] and "id" [N, M], M <=
    128), gt = {"boxes" [N, G, 6] float32 (MeanAP's ground-truth rows), "ids" [N, G] int32, "count" [N]}, G <= 1024 ->
    numpy {"match" [N, G] int32 (the track id a ground-truth row took, else -1), "iou" [N, G] float64 (that pair's IoU,
    else 0), "flags" [N, G] int32 (bit 0 matched, bit 1 id switch, bit 2 segment start)}.  Every image is its own
    sequence.  A reported track whose rectangle has a non-finite member overlaps nothing (IoU 0: a false positive)."""

    def __init__(self, batch_size, iou_threshold=0.5, scale=1.0, max_gt_ids=256):
        self.batch_size, self.iou_threshold, self.scale, self.max_gt_ids = _check_mot_params(batch_size, iou_threshold,
                                                                                             scale, max_gt_ids)
        self.images = None
        self.last_score = []         # per image the score matrix [valid ground truths, tracks] of the last frame

    def _fresh(self):
        return {"frames": 0, "TP": 0, "FP": 0, "FN": 0, "IDSW": 0, "motp_sum": 0.0, "status": 0,
                "rec": np.zeros((self.max_gt_ids, 8), dtype=np.int32)}

    def reset(self):
        if self.images is not None:
            self.images = [self._fresh() for _ in self.images]

    def update(self, tracks, gt):
        rect, tid, tcount, boxes, gids, gcount, n, m, g = _eval_inputs_host(tracks, gt)
        if self.images is None:
            self.images = [self._fresh() for _ in range(n)]
        if len(self.images) != n:
            raise ValueError("the evaluation holds %d images, this call has %d (reset() keeps the count)"
                             % (len(self.images), n))
        out = {"match": np.full((n, g), -1, dtype=np.int32), "iou": np.zeros((n, g), dtype=np.float64),
               "flags": np.zeros((n, g), dtype=np.int32)}
        self.last_score = []
        for img in range(n):
            self._step(self.images[img], rect[img], tid[img], tcount[img], boxes[img], gids[img], gcount[img], img, out)
        return out

    def _step(self, st, rect, tid, tcount, boxes, gids, gcount, img, out):
        m = tid.shape[0]
        k = min(max(int(tcount), 0), m)
        rec = st["rec"]
        st["frames"] += 1
        rows, rects, idents, status = _gt_measure(boxes, gids, gcount, self.scale, self.max_gt_ids)
        st["status"] |= status
        v = len(rows)
        finite = [bool(np.isfinite(rect[t]).all()) for t in range(k)]
        score = np.zeros((v, k), dtype=np.float64)
        for a in range(v):
            pst = int(rec[idents[a], 1])
            for t in range(k):
                iou = iou_rect(rects[a], rect[t]) if finite[t] else 0.0
                if iou < self.iou_threshold:
                    continue
                score[a, t] = iou + MOT_CONTINUITY if int(tid[t]) == pst else iou
        self.last_score.append(score)
        took = [-1] * v
        for a, t in hungarian_max(score):
            if score[a, t] > 0:
                took[a] = t
        was = rec[:, 1].copy()
        rec[:, 1] = 0                                   # pst: this frame's matches only
        matched = 0
        for a in range(v):                              # ascending ground-truth row: the order of motp_sum
            ident = idents[a]
            rec[ident, 2] += 1
            if took[a] < 0:
                continue
            t = took[a]
            track = int(tid[t])
            iou = iou_rect(rects[a], rect[t])
            flags = 1
            if rec[ident, 0] != 0 and rec[ident, 0] != track:
                flags |= 2
                st["IDSW"] += 1
            if was[ident] == 0:
                flags |= 4
                rec[ident, 4] += 1
            rec[ident, 0] = track
            rec[ident, 1] = track
            rec[ident, 3] += 1
            st["motp_sum"] = st["motp_sum"] + iou
            matched += 1
            out["match"][img, rows[a]] = track
            out["iou"][img, rows[a]] = iou
            out["flags"][img, rows[a]] = flags
        st["TP"] += matched
        st["FN"] += v - matched
        st["FP"] += k - matched

    def status_words(self):
        """The status word of every image (numpy int32), without raising."""
        return np.asarray([st["status"] for st in (self.images or [])], dtype=np.int32)

    def state_bytes(self):
        """The state in the device layout (numpy uint8), byte for byte what ClearMot.state_bytes() returns."""
        imgs = self.images or []
        buf = np.zeros((len(imgs), MOT_HEADER_BYTES + MOT_RECORD_BYTES * self.max_gt_ids), dtype=np.uint8)
        for i, st in enumerate(imgs):
            buf[i, :40] = np.asarray([st["frames"], st["TP"], st["FP"], st["FN"], st["IDSW"]], dtype=np.int64).view(np.uint8)
            buf[i, 40:48] = np.asarray([st["motp_sum"]], dtype=np.float64).view(np.uint8)
            buf[i, 48:52] = np.asarray([st["status"]], dtype=np.int32).view(np.uint8)
            buf[i, MOT_HEADER_BYTES:] = np.ascontiguousarray(st["rec"]).reshape(-1).view(np.uint8)
        return buf.reshape(-1)

    def compute(self):
        """{"overall", "per_agent", "per_image"}: per entry MOTA, MOTP, Recall, Precision, TP, FP, FN, IDSW, Frag, MT, PT,
        ML, frames.  Raises DnError naming any sticky status bit."""
        return mot_figures_from_state(self.state_bytes(), len(self.images or []), self.max_gt_ids, self.batch_size,
                                      "HostClearMot")


class ClearMot:
    """CLEAR MOT evaluation on the GPU behind Sort.update(): update() after every frame enqueues dn_mot_step on torch's
    current stream (the state -- per image a header of counters and max_gt_ids identity records -- lives on the device,
    is allocated on first use and is never read back before compute()), so forward + detect() + Sort.update() +
    ClearMot.update() can be one captured graph (graph.GraphedStep).  HostClearMot is the reference it equals bit for
    bit, and states the contract.

    update(tracks, gt) takes Sort.update()'s dict and gt = {"boxes" [N, G, 6], "ids" [N, G], "count" [N]} (device
    tensors; G <= 1024, at most 128 valid rows per image are used, ids in 0 .. max_gt_ids - 1) and returns device
    tensors {"match" [N, G] int32, "iou" [N, G] float64, "flags" [N, G] int32} as HostClearMot does.  `scale` multiplies
    the ground truth's corners as Sort's does the detections' (pass the tracker's).  Images are agent-major,
    `batch_size` per agent, as in MeanAP.  compute() makes one copy of the state and raises DnError naming the sticky
    status bits -- never a silently truncated metric.

    GraphedStep runs its step three times to warm up before it captures and those runs are counted: call reset() after
    constructing the GraphedStep, before the first replay that counts (as with Sort and MeanAP)."""

    def __init__(self, batch_size, iou_threshold=0.5, scale=1.0, max_gt_ids=256):
        self.batch_size, self.iou_threshold, self.scale, self.max_gt_ids = _check_mot_params(batch_size, iou_threshold,
                                                                                             scale, max_gt_ids)
        self.state = None            # uint8 [N * (MOT_HEADER_BYTES + MOT_RECORD_BYTES * max_gt_ids)] on the device
        self.n_images = 0

    def reset(self):
        """Zero every counter, identity record and status word (one launch on the current stream)."""
        if self.state is not None:
            from .ops import _ptr, _stream
            _lib.check(_lib.load().dn_mot_reset(_ptr(self.state), self.n_images, self.max_gt_ids, _stream()),
                       "dn_mot_reset")

    def update(self, tracks, gt):
        from .ops import _ptr, _stream
        rect, tid, tcount, boxes, gids, gcount, n, m, g = _eval_inputs_device("ClearMot", "HostClearMot", tracks, gt)
        lib = _lib.load()
        dev = rect.device
        _hold_state(self, "evaluation", "dn_mot_state_bytes", mot_state_bytes, (n, self.max_gt_ids), dev)
        out = {"match": torch.empty((n, g), dtype=torch.int32, device=dev),
               "iou": torch.empty((n, g), dtype=torch.float64, device=dev),
               "flags": torch.empty((n, g), dtype=torch.int32, device=dev)}
        _lib.check(lib.dn_mot_step(_ptr(rect), _ptr(tid), _ptr(tcount), n, m, _ptr(boxes), _ptr(gids), _ptr(gcount), g,
                                   self.scale, self.iou_threshold, self.max_gt_ids, _ptr(self.state), _ptr(out["match"]),
                                   _ptr(out["iou"]), _ptr(out["flags"]), _stream()), "dn_mot_step")
        return out

    def status_words(self):
        """The status word of every image (numpy int32): one small copy, waits for the device."""
        return _status_words(self.state, self.n_images, 48)

    def state_bytes(self):
        """A host copy of the whole state (numpy uint8); HostClearMot.state_bytes() is its reference."""
        return self.state.cpu().numpy().copy() if self.state is not None else np.zeros(0, dtype=np.uint8)

    def compute(self):
        """One copy of the state, then HostClearMot.compute()'s dict in float64 on the host.  Raises DnError naming any
        sticky status bit."""
        return mot_figures_from_state(self.state_bytes(), self.n_images, self.max_gt_ids, self.batch_size, "ClearMot")


# ---------------------------------------------------------------------------
# Identity metrics of the tracks (dn_idf_step / dn_idf_finish, csrc/idf_eval.hip): IDF1 beside CLEAR
# ---------------------------------------------------------------------------
MAX_TRACK_IDS = 2048      # upper limit of max_track_ids
IDF_HEADER_BYTES = 64     # per image: int64 frames, gt_dets, dets; int32 status; 36 spare bytes (zero)
IDF_STATUS_BITS = MOT_STATUS_BITS + ((16, "a reported track id was outside 1 .. max_track_ids and its row was ignored"),)
IDF_FIGURES = ("IDF1", "IDP", "IDR", "IDTP", "IDFP", "IDFN", "Dets", "GT_Dets", "IDs", "GT_IDs")


def _check_idf_params(batch_size, iou_threshold, scale, max_gt_ids, max_track_ids):
    batch_size, iou_threshold, scale, max_gt_ids = _check_mot_params(batch_size, iou_threshold, scale, max_gt_ids)
    max_track_ids = int(max_track_ids)
    if not 1 <= max_track_ids <= MAX_TRACK_IDS:
        raise ValueError("max_track_ids = %d: 1..%d are supported" % (max_track_ids, MAX_TRACK_IDS))
    return batch_size, iou_threshold, scale, max_gt_ids, max_track_ids


def idf_state_bytes(n_images, max_gt_ids, max_track_ids):
    """Bytes of the identity state of n_images images (what dn_idf_state_bytes returns)."""
    g, t = int(max_gt_ids), int(max_track_ids)
    return int(n_images) * (IDF_HEADER_BYTES + 4 * (g + t + g * t))


def _idf_status_text(words):
    out = []
    for img, w in enumerate(words):
        for bit, text in IDF_STATUS_BITS:
            if int(w) & bit:
                out.append("image %d: %s" % (img, text))
    return out


def _idf_level(group):
    """Rows of `counts` (lists of ints), summed in the order given -> the identity figures of that level."""
    s = [0] * 6
    for row in group:
        for k in range(6):
            s[k] = s[k] + int(row[k])
    frames, gt_dets, dets, idtp, gt_ids, ids = s
    idfn, idfp = gt_dets - idtp, dets - idtp
    return {"IDF1": float(2 * idtp) / float(max(1, 2 * idtp + idfp + idfn)),
            "IDP": float(idtp) / float(max(1, idtp + idfp)), "IDR": float(idtp) / float(max(1, idtp + idfn)),
            "IDTP": idtp, "IDFP": idfp, "IDFN": idfn, "Dets": dets, "GT_Dets": gt_dets, "IDs": ids, "GT_IDs": gt_ids,
            "frames": frames}


def idf_figures(counts, batch_size, who="Identity"):
    """finish()'s `counts` [N, 8] int64 (frames, GT_Dets, Dets, IDTP, GT_IDs, IDs, status, 0) -> {"overall": figures,
    "per_agent": [figures], "per_image": [figures]}, each with IDF1, IDP, IDR, IDTP, IDFP, IDFN, Dets, GT_Dets, IDs, GT_IDs
    and frames; sums over images are taken in image order.  Raises DnError naming any status bit."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 8)
    text = _idf_status_text(counts[:, 6])
    if text:
        raise _lib.DnError("%s: %s" % (who, "; ".join(text)))
    rows = counts.tolist()
    n_images, batch_size = len(rows), int(batch_size)
    agents = -(-n_images // batch_size)
    return {"overall": _idf_level(rows),
            "per_agent": [_idf_level(rows[a * batch_size:(a + 1) * batch_size]) for a in range(agents)],
            "per_image": [_idf_level([row]) for row in rows]}


def idf_line(name, figures):
    """One line of the evaluation tool: the identity figures of `name`."""
    return "%s: IDF1 %.4f IDP %.4f IDR %.4f IDTP %d IDFP %d IDFN %d Dets %d GT_Dets %d IDs %d GT_IDs %d" % (
        (name,) + tuple(figures[key] for key in IDF_FIGURES))


def _idf_assignment(match, weight_of):
    """finish()'s `match` [N, max_gt_ids] -> per image [(identity, track id, frames)], ascending identity."""
    out = []
    for img in range(match.shape[0]):
        out.append([(int(i), int(match[img, i]), int(weight_of(img, int(i), int(match[img, i]))))
                    for i in np.nonzero(match[img])[0]])
    return out


class HostIdentity:
    """The numpy reference of Identity and the statement of its contract: the identity metrics (IDF1, IDP, IDR; Ristani
    et al., "Performance measures and a data set for multi-target, multi-camera tracking") as the MOT benchmark's
    evaluation kit computes them, recalled, not pinned; the full text is in include/disconet_hip.h.

    update(tracks, gt) takes exactly ClearMot.update()'s inputs -- tracks = Sort.update()'s dict (the first `count` rows
    of "rect" [N, M, 4] and "id" [N, M], M <= 128), gt = {"boxes" [N, G, 6] float32, "ids" [N, G] int32, "count" [N]}, G
    <= 1024 -- and returns numpy {"overlaps" [N, G] int32}: per ground-truth row the number of reported rows that overlap
    it at the threshold (`not iou < iou_threshold`), 0 for a row that was not kept.  Every such pair adds 1 to
    pairs[identity][track id - 1]; a reported row whose id is outside 1 .. max_track_ids sets status bit 16 and is counted
    nowhere; one with a non-finite rectangle is counted as reported and overlaps nothing.  Every image is its own
    sequence.  finish() reads the state and leaves it: over the identities and track ids seen so far, hungarian_max on
    the pairs matrix as float64 picks the identity-to-track mapping with the most matched frames (IDTP)."""

    def __init__(self, batch_size, iou_threshold=0.5, scale=1.0, max_gt_ids=256, max_track_ids=1024):
        (self.batch_size, self.iou_threshold, self.scale, self.max_gt_ids,
         self.max_track_ids) = _check_idf_params(batch_size, iou_threshold, scale, max_gt_ids, max_track_ids)
        self.images = None

    def _fresh(self):
        return {"frames": 0, "gt_dets": 0, "dets": 0, "status": 0,
                "gt_count": np.zeros(self.max_gt_ids, dtype=np.int32),
                "track_count": np.zeros(self.max_track_ids, dtype=np.int32),
                "pairs": np.zeros((self.max_gt_ids, self.max_track_ids), dtype=np.int32)}

    def reset(self):
        if self.images is not None:
            self.images = [self._fresh() for _ in self.images]

    def update(self, tracks, gt):
        rect, tid, tcount, boxes, gids, gcount, n, m, g = _eval_inputs_host(tracks, gt)
        if self.images is None:
            self.images = [self._fresh() for _ in range(n)]
        if len(self.images) != n:
            raise ValueError("the evaluation holds %d images, this call has %d (reset() keeps the count)"
                             % (len(self.images), n))
        out = {"overlaps": np.zeros((n, g), dtype=np.int32)}
        for img in range(n):
            self._step(self.images[img], rect[img], tid[img], tcount[img], boxes[img], gids[img], gcount[img], img, out)
        return out

    def _step(self, st, rect, tid, tcount, boxes, gids, gcount, img, out):
        m = tid.shape[0]
        k = min(max(int(tcount), 0), m)
        st["frames"] += 1
        rows, rects, idents, status = _gt_measure(boxes, gids, gcount, self.scale, self.max_gt_ids)
        reported = []                                   # (row, column) of the reported rows that are counted
        for t in range(k):
            track = int(tid[t])
            if not 1 <= track <= self.max_track_ids:
                status |= 16
                continue
            st["track_count"][track - 1] += 1
            st["dets"] += 1
            if bool(np.isfinite(rect[t]).all()):
                reported.append((t, track - 1))
        st["status"] |= status
        for a, ident in enumerate(idents):
            st["gt_count"][ident] += 1
            st["gt_dets"] += 1
            hits = 0
            for t, col in reported:
                if not iou_rect(rects[a], rect[t]) < self.iou_threshold:
                    st["pairs"][ident, col] += 1
                    hits += 1
            out["overlaps"][img, rows[a]] = hits

    def status_words(self):
        """The status word of every image (numpy int32), without raising."""
        return np.asarray([st["status"] for st in (self.images or [])], dtype=np.int32)

    def state_bytes(self):
        """The state in the device layout (numpy uint8), byte for byte what Identity.state_bytes() returns."""
        imgs = self.images or []
        g, t = self.max_gt_ids, self.max_track_ids
        buf = np.zeros((len(imgs), IDF_HEADER_BYTES + 4 * (g + t + g * t)), dtype=np.uint8)
        for i, st in enumerate(imgs):
            buf[i, :24] = np.asarray([st["frames"], st["gt_dets"], st["dets"]], dtype=np.int64).view(np.uint8)
            buf[i, 24:28] = np.asarray([st["status"]], dtype=np.int32).view(np.uint8)
            o = IDF_HEADER_BYTES
            buf[i, o:o + 4 * g] = st["gt_count"].view(np.uint8)
            buf[i, o + 4 * g:o + 4 * (g + t)] = st["track_count"].view(np.uint8)
            buf[i, o + 4 * (g + t):] = np.ascontiguousarray(st["pairs"]).reshape(-1).view(np.uint8)
        return buf.reshape(-1)

    def counts_matrix(self, image):
        """The pairs block of one image, [max_gt_ids, max_track_ids] int32 (a copy)."""
        return self.images[image]["pairs"].copy()

    def finish(self):
        """{"counts" [N, 8] int64: frames, GT_Dets, Dets, IDTP, GT_IDs, IDs, status, 0; "match" [N, max_gt_ids] int32: the
        track id an identity was given, else 0}.  Reads the state only: the sequence may go on."""
        imgs = self.images or []
        counts = np.zeros((len(imgs), 8), dtype=np.int64)
        match = np.zeros((len(imgs), self.max_gt_ids), dtype=np.int32)
        for i, st in enumerate(imgs):
            rows, cols = np.nonzero(st["gt_count"] > 0)[0], np.nonzero(st["track_count"] > 0)[0]
            weight = st["pairs"][np.ix_(rows, cols)].astype(np.float64)
            idtp = 0
            for a, t in hungarian_max(weight):
                if weight[a, t] > 0:
                    idtp += int(st["pairs"][rows[a], cols[t]])
                    match[i, rows[a]] = cols[t] + 1
            counts[i] = (st["frames"], st["gt_dets"], st["dets"], idtp, len(rows), len(cols), st["status"], 0)
        return {"counts": counts, "match": match}

    def compute(self):
        """{"overall", "per_agent", "per_image"}: idf_figures() of finish()'s counts.  Raises DnError naming any sticky
        status bit."""
        return idf_figures(self.finish()["counts"], self.batch_size, "HostIdentity")

    def assignment(self):
        """Per image the list of (identity, track id, frames) of the kept pairs, in ascending identity."""
        return _idf_assignment(self.finish()["match"], lambda img, i, t: self.images[img]["pairs"][i, t - 1])


class Identity:
    """The identity metrics on the GPU beside ClearMot: update() after every frame enqueues dn_idf_step on torch's
    current stream (the state -- per image a header, the two per-id counts and the max_gt_ids x max_track_ids pairs
    matrix -- lives on the device, is allocated on first use and is never read back), so forward + detect() +
    Sort.update() + ClearMot.update() + Identity.update() can be one captured graph (graph.GraphedStep).  finish()
    enqueues dn_idf_finish -- the global assignment over the pairs matrix, on the device -- and returns device tensors, so
    it may be captured too; it reads the state only and the sequence may go on.  HostIdentity is the reference both equal
    bit for bit, and states the contract.

    update(tracks, gt) takes ClearMot.update()'s inputs (device tensors) and returns {"overlaps" [N, G] int32}.  compute()
    is finish() plus the copy of `counts` (8 words per image) and raises DnError naming the sticky status bits -- never a
    silently truncated metric; assignment() also copies `match`.

    GraphedStep runs its step three times to warm up before it captures and those runs are counted: call reset() after
    constructing the GraphedStep, before the first replay that counts (as with ClearMot, Sort and MeanAP)."""

    def __init__(self, batch_size, iou_threshold=0.5, scale=1.0, max_gt_ids=256, max_track_ids=1024):
        (self.batch_size, self.iou_threshold, self.scale, self.max_gt_ids,
         self.max_track_ids) = _check_idf_params(batch_size, iou_threshold, scale, max_gt_ids, max_track_ids)
        self.state = None            # uint8 [idf_state_bytes(N, max_gt_ids, max_track_ids)] on the device
        self.n_images = 0

    def reset(self):
        """Zero every count, the pairs matrix and the status words (one launch on the current stream)."""
        if self.state is not None:
            from .ops import _ptr, _stream
            _lib.check(_lib.load().dn_idf_reset(_ptr(self.state), self.n_images, self.max_gt_ids, self.max_track_ids,
                                                _stream()), "dn_idf_reset")

    def update(self, tracks, gt):
        from .ops import _ptr, _stream
        rect, tid, tcount, boxes, gids, gcount, n, m, g = _eval_inputs_device("Identity", "HostIdentity", tracks, gt)
        lib = _lib.load()
        dev = rect.device
        _hold_state(self, "evaluation", "dn_idf_state_bytes", idf_state_bytes,
                    (n, self.max_gt_ids, self.max_track_ids), dev)
        out = {"overlaps": torch.empty((n, g), dtype=torch.int32, device=dev)}
        _lib.check(lib.dn_idf_step(_ptr(rect), _ptr(tid), _ptr(tcount), n, m, _ptr(boxes), _ptr(gids), _ptr(gcount), g,
                                   self.scale, self.iou_threshold, self.max_gt_ids, self.max_track_ids, _ptr(self.state),
                                   _ptr(out["overlaps"]), _stream()), "dn_idf_step")
        return out

    def finish(self):
        """Enqueue dn_idf_finish on the current stream -> device tensors {"counts" [N, 8] int64, "match" [N, max_gt_ids]
        int32} as HostIdentity.finish() returns them.  Reads the state only."""
        from .ops import _ptr, _stream
        if self.state is None:
            raise _lib.DnError("Identity.finish: no frame was evaluated yet")
        dev = self.state.device
        out = {"counts": torch.empty((self.n_images, 8), dtype=torch.int64, device=dev),
               "match": torch.empty((self.n_images, self.max_gt_ids), dtype=torch.int32, device=dev)}
        _lib.check(_lib.load().dn_idf_finish(_ptr(self.state), self.n_images, self.max_gt_ids, self.max_track_ids,
                                             _ptr(out["counts"]), _ptr(out["match"]), _stream()), "dn_idf_finish")
        return out

    def status_words(self):
        """The status word of every image (numpy int32): one small copy, waits for the device."""
        return _status_words(self.state, self.n_images, 24)

    def state_bytes(self):
        """A host copy of the whole state (numpy uint8); HostIdentity.state_bytes() is its reference."""
        return self.state.cpu().numpy().copy() if self.state is not None else np.zeros(0, dtype=np.uint8)

    def counts_matrix(self, image):
        """A host copy of the pairs block of one image, [max_gt_ids, max_track_ids] int32."""
        g, t = self.max_gt_ids, self.max_track_ids
        block = self.state.view(self.n_images, -1)[image, IDF_HEADER_BYTES + 4 * (g + t):].contiguous().cpu().numpy()
        return block.view(np.int32).reshape(g, t).copy()

    def compute(self):
        """finish() and the copy of its counts, then HostIdentity.compute()'s dict on the host.  Raises DnError naming
        any sticky status bit."""
        return idf_figures(self.finish()["counts"].cpu().numpy(), self.batch_size, "Identity")

    def assignment(self):
        """finish(), the copy of `match` and of the matched pairs' words -> HostIdentity.assignment()'s lists."""
        match = self.finish()["match"]
        g, t = self.max_gt_ids, self.max_track_ids
        pairs = self.state.view(self.n_images, -1)[:, IDF_HEADER_BYTES + 4 * (g + t):].view(torch.int32)
        pairs = pairs.view(self.n_images, g, t)
        frames = torch.gather(pairs, 2, (match.to(torch.int64) - 1).clamp_(min=0).unsqueeze(2)).squeeze(2).cpu().numpy()
        return _idf_assignment(match.cpu().numpy(), lambda img, i, _t: frames[img, i])


# ---------------------------------------------------------------------------
# HOTA of the tracks (dn_hota_step / dn_hota_finish, csrc/hota_eval.hip): detection, association and localisation
# ---------------------------------------------------------------------------
MAX_HOTA_FRAMES = 4096    # upper limit of max_frames
HOTA_HEADER_BYTES = 64    # per image: int64 frames, logged, gt_dets, dets; int32 status; 28 spare bytes (zero)
HOTA_SLOT_BYTES = 9232    # per logged frame: int32 V, C, 8 bytes 0; int32 gid[128], tid[128]; fp64 gt_rect[128][4], track_rect[128][4]
HOTA_ALPHAS = 19          # alpha_k = 0.05 (k + 1)
HOTA_BINS = 20            # a kept pair counts at K = 0 .. 19 alphas
HOTA_EPS = 2.0 ** -52     # the kit's epsilon: a pair counts at alpha when not (iou < alpha - HOTA_EPS)
HOTA_STATUS_BITS = IDF_STATUS_BITS + (
    (32, "the frame log was full (max_frames frames); the frames past it were counted in `frames` and left out of every figure"),
    (64, "a reported track id came twice in one frame; the lower row was kept"))
HOTA_FIGURES = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA", "HOTA(0)", "LocA(0)", "HOTALocA(0)")
HOTA_COUNTS = ("Dets", "GT_Dets", "IDs", "GT_IDs")


def hota_alphas():
    """The 19 alphas as the contract writes them: 0.05 * (k + 1), an fp64 product."""
    return [0.05 * (k + 1) for k in range(HOTA_ALPHAS)]


def _check_hota_params(batch_size, scale, max_gt_ids, max_track_ids, max_frames):
    batch_size, _, scale, max_gt_ids, max_track_ids = _check_idf_params(batch_size, 0.5, scale, max_gt_ids, max_track_ids)
    max_frames = int(max_frames)
    if not 1 <= max_frames <= MAX_HOTA_FRAMES:
        raise ValueError("max_frames = %d: 1..%d are supported" % (max_frames, MAX_HOTA_FRAMES))
    return batch_size, scale, max_gt_ids, max_track_ids, max_frames


def _hota_image_bytes(max_gt_ids, max_track_ids, max_frames):
    g, t, f = int(max_gt_ids), int(max_track_ids), int(max_frames)
    return (HOTA_HEADER_BYTES + 8 * g * t + HOTA_SLOT_BYTES * f + 4 * (g + t) + 7) // 8 * 8


def hota_state_bytes(n_images, max_gt_ids, max_track_ids, max_frames):
    """Bytes of the HOTA state of n_images images (what dn_hota_state_bytes returns)."""
    return int(n_images) * _hota_image_bytes(max_gt_ids, max_track_ids, max_frames)


def hota_work_bytes(n_images, max_gt_ids, max_track_ids, max_frames):
    """Bytes of dn_hota_finish's scratch (what dn_hota_work_bytes returns): per image the per-alpha TP words, the
    per-frame loc partials and 20 int32 bins per (identity, track id) cell."""
    g, t, f = int(max_gt_ids), int(max_track_ids), int(max_frames)
    return int(n_images) * (8 * HOTA_BINS * (1 + f) + 4 * HOTA_BINS * g * t)


def _hota_status_text(words):
    out = []
    for img, w in enumerate(words):
        for bit, text in HOTA_STATUS_BITS:
            if int(w) & bit:
                out.append("image %d: %s" % (img, text))
    return out


def _hota_level(counts, alpha_counts, alpha_sums):
    """Rows of one level (lists per image), added in the order given -> the HOTA figures of that level."""
    c = [0] * 6
    tp, fn, fp = [0] * HOTA_ALPHAS, [0] * HOTA_ALPHAS, [0] * HOTA_ALPHAS
    sums = [[0.0] * 4 for _ in range(HOTA_ALPHAS)]
    for row, ac, asum in zip(counts, alpha_counts, alpha_sums):
        for k in range(6):
            c[k] = c[k] + int(row[k])
        for k in range(HOTA_ALPHAS):
            tp[k], fn[k], fp[k] = tp[k] + int(ac[k][0]), fn[k] + int(ac[k][1]), fp[k] + int(ac[k][2])
            for q in range(4):
                sums[k][q] = sums[k][q] + float(asum[k][q])
    per = {key: [] for key in ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")}
    for k in range(HOTA_ALPHAS):
        loc, assa, assre, asspr = sums[k]
        det_a = float(tp[k]) / float(max(1, tp[k] + fn[k] + fp[k]))
        ass_a = assa / float(max(1, tp[k]))
        per["DetA"].append(det_a)
        per["DetRe"].append(float(tp[k]) / float(max(1, tp[k] + fn[k])))
        per["DetPr"].append(float(tp[k]) / float(max(1, tp[k] + fp[k])))
        per["AssA"].append(ass_a)
        per["AssRe"].append(assre / float(max(1, tp[k])))
        per["AssPr"].append(asspr / float(max(1, tp[k])))
        per["LocA"].append(loc / float(tp[k]) if tp[k] > 0 else 1.0)
        per["HOTA"].append(float(np.sqrt(det_a * ass_a)))
    out = {}
    for key, values in per.items():
        x = 0.0
        for v in values:
            x = x + v
        out[key] = x / float(HOTA_ALPHAS)
    out["HOTA(0)"], out["LocA(0)"] = per["HOTA"][0], per["LocA"][0]
    out["HOTALocA(0)"] = per["HOTA"][0] * per["LocA"][0]
    out.update({"frames": c[0], "logged": c[1], "GT_Dets": c[2], "Dets": c[3], "GT_IDs": c[4], "IDs": c[5],
                "TP": tp, "FN": fn, "FP": fp, "loc": [s[0] for s in sums], "assa": [s[1] for s in sums],
                "assre": [s[2] for s in sums], "asspr": [s[3] for s in sums], "per_alpha": per})
    return out


def hota_figures(fin, batch_size, who="Hota"):
    """finish()'s dict on the host ("counts" [N, 8] int64: frames, logged, GT_Dets, Dets, GT_IDs, IDs, status, 0;
    "alpha_counts" [N, 19, 4] int64: TP, FN, FP, 0; "alpha_sums" [N, 19, 4] float64: loc, assa, assre, asspr) ->
    {"overall": figures, "per_agent": [figures], "per_image": [figures]}.  Counts and sums are added in image order (adding
    the numerators is the kit's TP-weighted combination).  Per alpha DetA = TP / max(1, TP + FN + FP), DetRe, DetPr, AssA =
    assa / max(1, TP), AssRe, AssPr, LocA = loc / TP (1.0 when TP = 0), HOTA = sqrt(DetA AssA); every figure is its mean
    over the 19 alphas, beside them HOTA(0), LocA(0), HOTALocA(0) at alpha 0.05, the counts, the per-alpha lists TP, FN,
    FP, loc, assa, assre, asspr and "per_alpha".  Raises DnError naming any status bit."""
    counts = np.asarray(fin["counts"], dtype=np.int64).reshape(-1, 8)
    text = _hota_status_text(counts[:, 6])
    if text:
        raise _lib.DnError("%s: %s" % (who, "; ".join(text)))
    n_images, batch_size = counts.shape[0], int(batch_size)
    rows = counts.tolist()
    ac = np.asarray(fin["alpha_counts"], dtype=np.int64).reshape(n_images, HOTA_ALPHAS, 4).tolist()
    asum = np.asarray(fin["alpha_sums"], dtype=np.float64).reshape(n_images, HOTA_ALPHAS, 4).tolist()
    agents = -(-n_images // batch_size)

    def level(lo, hi):
        return _hota_level(rows[lo:hi], ac[lo:hi], asum[lo:hi])

    return {"overall": level(0, n_images),
            "per_agent": [level(a * batch_size, (a + 1) * batch_size) for a in range(agents)],
            "per_image": [level(i, i + 1) for i in range(n_images)]}


def hota_line(name, figures):
    """One line of the evaluation tool: the HOTA figures of `name`."""
    return ("%s: HOTA %.4f DetA %.4f AssA %.4f DetRe %.4f DetPr %.4f AssRe %.4f AssPr %.4f LocA %.4f HOTA(0) %.4f LocA(0) %.4f "
            "HOTALocA(0) %.4f Dets %d GT_Dets %d IDs %d GT_IDs %d" % (
                (name,) + tuple(figures[key] for key in HOTA_FIGURES + HOTA_COUNTS)))


def _iou_matrix(grect, trect):
    """iou_rect of every (ground truth [V, 4], column [C, 4]) pair, element for element the same operations; a column with
    a non-finite member overlaps nothing.  The ground-truth rectangles are finite."""
    g, t = np.asarray(grect, dtype=np.float64).reshape(-1, 4), np.asarray(trect, dtype=np.float64).reshape(-1, 4)
    fin = np.isfinite(t).all(1)
    t = np.where(fin[:, None], t, 0.0)
    with np.errstate(all="ignore"):
        w = np.minimum(g[:, None, 2], t[None, :, 2]) - np.maximum(g[:, None, 0], t[None, :, 0])
        h = np.minimum(g[:, None, 3], t[None, :, 3]) - np.maximum(g[:, None, 1], t[None, :, 1])
        inter = w * h
        union = ((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]))[:, None] + ((t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1]))[None, :] - inter
        ok = (w > 0) & (h > 0) & (union > 0) & fin[None, :]
        return np.where(ok, inter / np.where(ok, union, 1.0), 0.0)


class HostHota:
    """The numpy / float64 reference of Hota and the statement of its contract: HOTA (Luiten et al., "HOTA: A Higher Order
    Metric for Evaluating Multi-Object Tracking") with DetA / AssA / LocA and their recall and precision parts, as the MOT
    benchmark's evaluation kit computes them, recalled, not pinned; the full text is in include/disconet_hip.h.

    update(tracks, gt) takes ClearMot.update()'s inputs (there is no IoU threshold: HOTA averages over 19 of them) and
    returns numpy {"potential" [N, G] float64}: per ground-truth row the sum of s / (rs + cs - s) over the columns it
    overlaps, which is what the frame added to that identity's row of the potential-match matrix.  The frame's measured
    rectangles and ids are logged (max_frames frames per image; a frame past that sets status bit 32 and is left out).
    finish() reads the state and leaves it: the global alignment score A = pot / (gt_count + track_count - pot) weights a
    second pass over the logged frames -- per frame hungarian_max on A * IoU -- from which the per-alpha TP / FN / FP, the
    localisation sums and the association sums come.  Every image is its own sequence."""

    def __init__(self, batch_size, scale=1.0, max_gt_ids=256, max_track_ids=1024, max_frames=256):
        (self.batch_size, self.scale, self.max_gt_ids, self.max_track_ids,
         self.max_frames) = _check_hota_params(batch_size, scale, max_gt_ids, max_track_ids, max_frames)
        self.images = None

    def _fresh(self):
        return {"frames": 0, "gt_dets": 0, "dets": 0, "status": 0, "log": [],
                "gt_count": np.zeros(self.max_gt_ids, dtype=np.int32),
                "track_count": np.zeros(self.max_track_ids, dtype=np.int32),
                "pot": np.zeros((self.max_gt_ids, self.max_track_ids), dtype=np.float64)}

    def reset(self):
        if self.images is not None:
            self.images = [self._fresh() for _ in self.images]

    def update(self, tracks, gt):
        rect, tid, tcount, boxes, gids, gcount, n, m, g = _eval_inputs_host(tracks, gt)
        if self.images is None:
            self.images = [self._fresh() for _ in range(n)]
        if len(self.images) != n:
            raise ValueError("the evaluation holds %d images, this call has %d (reset() keeps the count)"
                             % (len(self.images), n))
        out = {"potential": np.zeros((n, g), dtype=np.float64)}
        for img in range(n):
            self._step(self.images[img], rect[img], tid[img], tcount[img], boxes[img], gids[img], gcount[img], img, out)
        return out

    def _step(self, st, rect, tid, tcount, boxes, gids, gcount, img, out):
        st["frames"] += 1
        if len(st["log"]) == self.max_frames:
            st["status"] |= 32
            return
        k = min(max(int(tcount), 0), tid.shape[0])
        rows, rects, idents, status = _gt_measure(boxes, gids, gcount, self.scale, self.max_gt_ids)
        cols, tids = [], []
        for t in range(k):
            track = int(tid[t])
            if not 1 <= track <= self.max_track_ids:
                status |= 16
                continue
            if track in tids:
                status |= 64
                continue
            cols.append(t)
            tids.append(track)
        st["status"] |= status
        v, c = len(rows), len(cols)
        gid, col = np.asarray(idents, dtype=np.int64), np.asarray(tids, dtype=np.int64) - 1
        trects = np.asarray(rect[cols], dtype=np.float64).reshape(c, 4)
        st["gt_count"][gid] += 1
        st["gt_dets"] += v
        st["track_count"][col] += 1
        st["dets"] += c
        s = _iou_matrix(rects, trects)                                   # [v, c]
        rs, cs = np.zeros(v), np.zeros(c)
        for t in range(c):                                               # ascending, from 0.0
            rs = rs + s[:, t]
        for a in range(v):
            cs = cs + s[a, :]
        with np.errstate(all="ignore"):
            term = np.where(s > 0, s / np.where(s > 0, (rs[:, None] + cs[None, :]) - s, 1.0), 0.0)
        if v and c:
            st["pot"][np.ix_(gid, col)] += term                          # ids are unique: one add per cell; + 0.0 changes nothing
        total = np.zeros(v)
        for t in range(c):
            total = total + term[:, t]
        out["potential"][img, rows] = total
        st["log"].append({"gid": np.asarray(idents, dtype=np.int32), "tid": np.asarray(tids, dtype=np.int32),
                          "grect": np.asarray(rects, dtype=np.float64).reshape(v, 4), "trect": trects.copy()})

    def status_words(self):
        """The status word of every image (numpy int32), without raising."""
        return np.asarray([st["status"] for st in (self.images or [])], dtype=np.int32)

    def state_bytes(self):
        """The state in the device layout (numpy uint8), byte for byte what Hota.state_bytes() returns."""
        imgs = self.images or []
        g, t, f = self.max_gt_ids, self.max_track_ids, self.max_frames
        buf = np.zeros((len(imgs), _hota_image_bytes(g, t, f)), dtype=np.uint8)
        for i, st in enumerate(imgs):
            buf[i, :32] = np.asarray([st["frames"], len(st["log"]), st["gt_dets"], st["dets"]], dtype=np.int64).view(np.uint8)
            buf[i, 32:36] = np.asarray([st["status"]], dtype=np.int32).view(np.uint8)
            o = HOTA_HEADER_BYTES
            buf[i, o:o + 8 * g * t] = np.ascontiguousarray(st["pot"]).reshape(-1).view(np.uint8)
            o += 8 * g * t
            for slot in st["log"]:
                v, c = len(slot["gid"]), len(slot["tid"])
                buf[i, o:o + 8] = np.asarray([v, c], dtype=np.int32).view(np.uint8)
                buf[i, o + 16:o + 16 + 4 * v] = slot["gid"].view(np.uint8)
                buf[i, o + 528:o + 528 + 4 * c] = slot["tid"].view(np.uint8)
                buf[i, o + 1040:o + 1040 + 32 * v] = np.ascontiguousarray(slot["grect"]).reshape(-1).view(np.uint8)
                buf[i, o + 5136:o + 5136 + 32 * c] = np.ascontiguousarray(slot["trect"]).reshape(-1).view(np.uint8)
                o += HOTA_SLOT_BYTES
            o = HOTA_HEADER_BYTES + 8 * g * t + HOTA_SLOT_BYTES * f
            buf[i, o:o + 4 * g] = st["gt_count"].view(np.uint8)
            buf[i, o + 4 * g:o + 4 * (g + t)] = st["track_count"].view(np.uint8)
        return buf.reshape(-1)

    def potential_matrix(self, image):
        """The pot block of one image, [max_gt_ids, max_track_ids] float64 (a copy)."""
        return self.images[image]["pot"].copy()

    def finish(self):
        """{"counts" [N, 8] int64, "alpha_counts" [N, 19, 4] int64, "alpha_sums" [N, 19, 4] float64, "match" [N, max_frames,
        128] int32: per logged frame and kept ground-truth row the track id taken, else 0}.  Reads the state only: the
        sequence may go on."""
        imgs = self.images or []
        n = len(imgs)
        counts = np.zeros((n, 8), dtype=np.int64)
        alpha_counts = np.zeros((n, HOTA_ALPHAS, 4), dtype=np.int64)
        alpha_sums = np.zeros((n, HOTA_ALPHAS, 4), dtype=np.float64)
        match = np.zeros((n, self.max_frames, MAX_GT_USED), dtype=np.int32)
        thresholds = [alpha - HOTA_EPS for alpha in hota_alphas()]
        for i, st in enumerate(imgs):
            gc, tc, pot = st["gt_count"], st["track_count"], st["pot"]
            with np.errstate(all="ignore"):
                both = (gc[:, None].astype(np.int64) + tc[None, :].astype(np.int64)).astype(np.float64)
                align = np.where(pot > 0, pot / np.where(pot > 0, both - pot, 1.0), 0.0)
            tp = [0] * HOTA_ALPHAS
            loc = [0.0] * HOTA_ALPHAS
            hist = {}                                                    # (identity, column) -> 20 bins
            for f, slot in enumerate(st["log"]):
                gid, col = slot["gid"].astype(np.int64), slot["tid"].astype(np.int64) - 1
                s = _iou_matrix(slot["grect"], slot["trect"])
                score = align[np.ix_(gid, col)] * s if len(gid) and len(col) else np.zeros((len(gid), len(col)))
                took = [-1] * len(gid)
                for a, t in hungarian_max(score):
                    if score[a, t] > 0:
                        took[a] = t
                part = [0.0] * HOTA_ALPHAS
                for a, t in enumerate(took):                             # ascending ground-truth row
                    if t < 0:
                        continue
                    iou = float(s[a, t])
                    reach = sum(1 for thr in thresholds if not iou < thr)
                    hist.setdefault((int(gid[a]), int(col[t])), [0] * HOTA_BINS)[reach] += 1
                    for k in range(reach):
                        tp[k] += 1
                        part[k] = part[k] + iou
                    match[i, f, a] = col[t] + 1
                for k in range(HOTA_ALPHAS):
                    loc[k] = loc[k] + part[k]
            sums = np.zeros((HOTA_ALPHAS, 3))
            cells = {}
            for (ident, column), bins in hist.items():
                cells.setdefault(ident, []).append((column, bins))
            for ident in sorted(cells):                                  # identities ascending, each from 0.0
                row = np.zeros((HOTA_ALPHAS, 3))
                for column, bins in sorted(cells[ident]):                # track ids ascending
                    for k in range(HOTA_ALPHAS):
                        cnt = sum(bins[k + 1:])
                        if cnt == 0:
                            continue
                        cd = float(cnt)
                        row[k, 0] = row[k, 0] + cd * (cd / (float(int(gc[ident]) + int(tc[column])) - cd))
                        row[k, 1] = row[k, 1] + cd * (cd / float(gc[ident]))
                        row[k, 2] = row[k, 2] + cd * (cd / float(tc[column]))
                sums = sums + row
            counts[i] = (st["frames"], len(st["log"]), st["gt_dets"], st["dets"], int((gc > 0).sum()), int((tc > 0).sum()),
                         st["status"], 0)
            for k in range(HOTA_ALPHAS):
                alpha_counts[i, k] = (tp[k], st["gt_dets"] - tp[k], st["dets"] - tp[k], 0)
                alpha_sums[i, k] = (loc[k], sums[k, 0], sums[k, 1], sums[k, 2])
        return {"counts": counts, "alpha_counts": alpha_counts, "alpha_sums": alpha_sums, "match": match}

    def compute(self):
        """{"overall", "per_agent", "per_image"}: hota_figures() of finish().  Raises DnError naming any sticky status bit."""
        return hota_figures(self.finish(), self.batch_size, "HostHota")

    def matches(self, image):
        """finish()'s match rows of one image, [logged, 128] int32: per logged frame and kept ground-truth row (in kept
        order) the track id taken, else 0."""
        return self.finish()["match"][image, :len(self.images[image]["log"])].copy()


class Hota:
    """HOTA on the GPU beside ClearMot and Identity: update() after every frame enqueues dn_hota_step on torch's current
    stream (the state -- per image a header, the fp64 potential-match matrix, max_frames log slots of 9232 bytes and the two
    per-id counts -- lives on the device, is allocated on first use and is never read back), so forward + detect() +
    Sort.update() + ClearMot.update() + Identity.update() + Hota.update() can be one captured graph (graph.GraphedStep).
    finish() enqueues dn_hota_finish -- every logged frame of every image matched at once, one wave per frame, then one
    fold per image -- and returns device tensors, so it may be captured too; it reads the state only and the sequence may
    go on.  HostHota is the reference both equal bit for bit, and states the contract.

    What it costs: the state is 8 max_gt_ids max_track_ids + 9232 max_frames bytes per image (4.5 MB at the defaults), and
    Hota owns the scratch of finish(), allocated at the first finish(): 80 bytes per (identity, track id) cell, about 20 MB
    per image at the defaults (256 x 1024), zeroed by every finish().  The tools pass smaller ids where they know the
    sequence (tools/hota_probe.py: 64 x 512 -- a sequence has tens of identities and a few hundred track ids;
    tools/track/eval_sort.py: its --max_gt_ids / --max_track_ids) and max_frames = the frames they run.

    update(tracks, gt) takes ClearMot.update()'s inputs (device tensors) and returns {"potential" [N, G] float64}.
    compute() is finish() plus the copy of three small tensors and raises DnError naming the sticky status bits -- never a
    silently truncated metric.

    GraphedStep runs its step three times to warm up before it captures and those runs are counted and logged: call
    reset() after constructing the GraphedStep, before the first replay that counts (as with Identity and ClearMot)."""

    def __init__(self, batch_size, scale=1.0, max_gt_ids=256, max_track_ids=1024, max_frames=256):
        (self.batch_size, self.scale, self.max_gt_ids, self.max_track_ids,
         self.max_frames) = _check_hota_params(batch_size, scale, max_gt_ids, max_track_ids, max_frames)
        self.state = None            # uint8 [hota_state_bytes(N, ...)] on the device, viewed from an int64 allocation
        self.work = None             # finish()'s scratch, allocated by the first finish()
        self.n_images = 0

    def _sizes(self):
        return self.n_images, self.max_gt_ids, self.max_track_ids, self.max_frames

    def reset(self):
        """Zero every count, the potential matrix, the log and the status words (one launch on the current stream)."""
        if self.state is not None:
            from .ops import _ptr, _stream
            _lib.check(_lib.load().dn_hota_reset(_ptr(self.state), *self._sizes(), _stream()), "dn_hota_reset")

    def update(self, tracks, gt):
        from .ops import _ptr, _stream
        rect, tid, tcount, boxes, gids, gcount, n, m, g = _eval_inputs_device("Hota", "HostHota", tracks, gt)
        lib = _lib.load()
        dev = rect.device
        _hold_state(self, "evaluation", "dn_hota_state_bytes", hota_state_bytes,
                    (n, self.max_gt_ids, self.max_track_ids, self.max_frames), dev)
        out = {"potential": torch.empty((n, g), dtype=torch.float64, device=dev)}
        _lib.check(lib.dn_hota_step(_ptr(rect), _ptr(tid), _ptr(tcount), n, m, _ptr(boxes), _ptr(gids), _ptr(gcount), g,
                                    self.scale, self.max_gt_ids, self.max_track_ids, self.max_frames, _ptr(self.state),
                                    _ptr(out["potential"]), _stream()), "dn_hota_step")
        return out

    def finish(self):
        """Enqueue dn_hota_finish on the current stream (three launches) -> device tensors {"counts" [N, 8] int64,
        "alpha_counts" [N, 19, 4] int64, "alpha_sums" [N, 19, 4] float64, "match" [N, max_frames, 128] int32} as
        HostHota.finish() returns them.  Reads the state only."""
        from .ops import _ptr, _stream
        if self.state is None:
            raise _lib.DnError("Hota.finish: no frame was evaluated yet")
        lib = _lib.load()
        dev = self.state.device
        if self.work is None:
            nbytes = int(lib.dn_hota_work_bytes(*self._sizes()))
            if nbytes != hota_work_bytes(*self._sizes()) or nbytes % 8:
                raise _lib.DnError("dn_hota_work_bytes%r = %d" % (self._sizes(), nbytes))
            self.work = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        n = self.n_images
        out = {"counts": torch.empty((n, 8), dtype=torch.int64, device=dev),
               "alpha_counts": torch.empty((n, HOTA_ALPHAS, 4), dtype=torch.int64, device=dev),
               "alpha_sums": torch.empty((n, HOTA_ALPHAS, 4), dtype=torch.float64, device=dev),
               "match": torch.empty((n, self.max_frames, MAX_GT_USED), dtype=torch.int32, device=dev)}
        _lib.check(lib.dn_hota_finish(_ptr(self.state), *self._sizes(), _ptr(self.work), _ptr(out["counts"]),
                                      _ptr(out["alpha_counts"]), _ptr(out["alpha_sums"]), _ptr(out["match"]), _stream()),
                   "dn_hota_finish")
        return out

    def status_words(self):
        """The status word of every image (numpy int32): one small copy, waits for the device."""
        return _status_words(self.state, self.n_images, 32)

    def state_bytes(self):
        """A host copy of the whole state (numpy uint8); HostHota.state_bytes() is its reference."""
        return self.state.cpu().numpy().copy() if self.state is not None else np.zeros(0, dtype=np.uint8)

    def potential_matrix(self, image):
        """A host copy of the pot block of one image, [max_gt_ids, max_track_ids] float64."""
        g, t = self.max_gt_ids, self.max_track_ids
        block = self.state.view(self.n_images, -1)[image, HOTA_HEADER_BYTES:HOTA_HEADER_BYTES + 8 * g * t]
        return block.contiguous().cpu().numpy().view(np.float64).reshape(g, t).copy()

    def compute(self):
        """finish() and the copy of its three small tensors, then HostHota.compute()'s dict on the host.  Raises DnError
        naming any sticky status bit."""
        fin = self.finish()
        return hota_figures({key: fin[key].cpu().numpy() for key in ("counts", "alpha_counts", "alpha_sums")},
                            self.batch_size, "Hota")

    def matches(self, image):
        """finish() and the copy of one image's match rows, [logged, 128] int32, as HostHota.matches()."""
        fin = self.finish()
        logged = int(fin["counts"][image, 1])
        return fin["match"][image, :logged].cpu().numpy().copy()
