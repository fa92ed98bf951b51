"""sklearn.metrics.roc_auc_score for binary labels and float32 scores, restated step by step in the order numpy computes it: the
contract NASREC_OP_ROC_AUC implements (DESIGN.md "ROC AUC on the device").  tests/test_roc_auc_cpu.py pins it to sklearn bit for bit."""
import numpy as np

CHUNK = 8192  # numpy's reduction buffer (elements)
LEAF = 128    # numpy's pairwise-sum block (PW_BLOCKSIZE)


def pairwise_sum(a):
    """numpy's pairwise_sum of float64 a (a list of Python floats: every addition one IEEE double addition)"""
    n = len(a)
    if n < 8:
        res = 0.0
        for v in a:
            res = res + v
        return res
    if n <= LEAF:
        r = list(a[:8])
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = r[j] + a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[i:]:
            res = res + v
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def curve_points(y_true, y_score):
    """(fps, tps) of the kept points of the curve, int64, without the prepended (0, 0)"""
    y = np.asarray(y_true, np.float32).ravel() == 1
    s = np.asarray(y_score, np.float32).ravel()
    order = np.argsort(-s.astype(np.float64), kind="stable")  # descending; +0 and -0 compare equal
    s, y = s[order], y[order]
    ends = np.r_[np.nonzero(s[1:] != s[:-1])[0], len(s) - 1]
    tps = np.cumsum(y, dtype=np.int64)[ends]
    fps = ends + 1 - tps
    if len(fps) > 2:  # drop_intermediate
        keep = np.r_[True, (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0), True]
        fps, tps = fps[keep], tps[keep]
    return fps, tps


def roc_auc_restated(y_true, y_score):
    fps, tps = curve_points(y_true, y_score)
    fps = np.r_[0, fps].astype(np.float64)
    tps = np.r_[0, tps].astype(np.float64)
    fpr, tpr = fps / fps[-1], tps / tps[-1]
    terms = ((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) / 2.0).tolist()
    total = 0.0
    for c in range(0, len(terms), CHUNK):
        total = total + pairwise_sum(terms[c:c + CHUNK])
    return total


def inputs_with_kept_points(k, seed):
    """labels and scores whose curve keeps exactly k points: k distinct scores whose labels alternate along the descending order,
    so that every step differs from the next one"""
    rng = np.random.default_rng(seed)
    y = (np.arange(k) % 2 == 0).astype(np.float32)
    s = np.sort(rng.choice(np.arange(1, 1 << 23), size=k, replace=False)).astype(np.float32)[::-1] / np.float32(1 << 23)
    perm = rng.permutation(k)
    return y[perm].copy(), np.ascontiguousarray(s[perm])
