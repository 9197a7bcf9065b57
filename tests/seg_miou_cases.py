"""What the mean-IoU tests share (tests/test_seg_miou_host_cpu.py, tests/test_gpu_seg_miou.py): the planted logit rows
for the prediction rule and the plain restatement of the confusion counts."""
import numpy as np

INF, NAN = float("inf"), float("nan")
# ties, NaN first / later / several, +inf beside NaN, all -inf, signed zeros
PLANTED_ROWS = [
    [1.0, 3.0, 3.0, 2.0, 3.0, 0.0, -1.0, 3.0],              # tie: the first maximum
    [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0],               # all equal
    [NAN, 9.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0],               # NaN first
    [1.0, 9.0, 1.0, NAN, 3.0, 4.0, 5.0, 6.0],               # NaN later, behind the maximum
    [1.0, 2.0, NAN, 9.0, NAN, 4.0, NAN, 6.0],               # several NaN: the first one
    [1.0, INF, 2.0, 3.0, NAN, 4.0, 5.0, 6.0],               # +inf before a NaN: the NaN wins
    [1.0, 2.0, NAN, 3.0, INF, 4.0, 5.0, 6.0],               # +inf behind a NaN
    [-INF, -INF, -INF, -INF, -INF, -INF, -INF, -INF],       # all -inf -> 0
    [-INF, -INF, -INF, -1e30, -INF, -INF, -INF, -INF],
    [1.0, INF, 2.0, INF, 3.0, 4.0, 5.0, 6.0],               # two +inf: the first
    [-0.0, 0.0, -1.0, -2.0, -3.0, -4.0, -5.0, -6.0],        # -0.0 == +0.0: the first of them
    [0.0, -0.0, 0.0, -2.0, -3.0, -4.0, -5.0, -6.0],
    [-1.0, -0.0, 0.0, -2.0, -3.0, -4.0, -5.0, 0.0],
    [-7.0, -6.0, -5.0, -4.0, -3.0, -2.0, -1.0, -0.5],       # the last column
    [NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN],
]


def planted_rows():
    return np.asarray(PLANTED_ROWS, dtype=np.float32)


def plain_confusion(pred, labels, classes, live=None):
    """the plain restatement: np.bincount over y * classes + p on the live pixels -> ([n, classes^2] counts, [n] ignored)"""
    n = labels.shape[0]
    counts, ignored = np.zeros((n, classes * classes), dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in range(n):
        y, p = labels[i].ravel().astype(np.int64), pred[i].ravel().astype(np.int64)
        keep = (y >= 0) & (y < classes)
        if live is not None and not live[i]:
            keep[:] = False
        counts[i] = np.bincount(y[keep] * classes + p[keep], minlength=classes * classes)
        ignored[i] = (~keep).sum()
    return counts, ignored
