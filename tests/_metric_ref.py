"""The two evaluation metrics of mindrec_amd/csrc/mrec_metric.hip restated in numpy with int64 arithmetic (include/mrec.h
'evaluation metrics' holds the definitions).  Written from the definitions, not from the kernels: levels by np.unique instead of a radix
sort, one display at a time instead of atomics."""
import numpy as np


def auc_counts(pred, label):
    """(twoU, P, N, n_nan) as Python ints.  A row is positive iff label > 0.5; NaN predictions are counted and left out;
    twoU = sum over positives i of (2 #{negatives j: pred_j < pred_i} + #{negatives j: pred_j == pred_i}), IEEE comparison."""
    pred = np.asarray(pred, np.float32).ravel()
    pos = np.asarray(label, np.float32).ravel() > np.float32(0.5)
    ok = ~np.isnan(pred)
    n_nan = int((~ok).sum())
    pred, pos = pred[ok], pos[ok]
    P, N = int(pos.sum()), int((~pos).sum())
    if pred.size == 0:
        return 0, 0, 0, n_nan
    levels, lv = np.unique(pred, return_inverse=True)                   # ascending; -0.0 == +0.0 is one level
    negs = np.bincount(lv[~pos], minlength=levels.size).astype(np.int64)
    poss = np.bincount(lv[pos], minlength=levels.size).astype(np.int64)
    below = np.cumsum(negs) - negs                                      # negatives strictly below each level
    return int((poss * (2 * below + negs)).sum()), P, N, n_nan


def auc(twoU, P, N):
    return twoU / (2 * P * N)                                           # (Python ints: one correctly rounded division)


def group_rank_hist(pred, label, group, topk=12, pad_to=30):
    """(hist int64 [topk], G).  Per distinct group value, rows in feed order: the clicked row c is the first holding the maximal label
    (np.argmax); rank = #{rows of the group with pred > pred[c]}, plus pad_to - m when the group has m < pad_to rows and pred[c] < 0;
    rank < topk adds one to hist[rank]."""
    pred = np.asarray(pred, np.float32).ravel()
    label = np.asarray(label, np.float32).ravel()
    group = np.asarray(group).ravel()
    order = np.argsort(group, kind="stable")
    starts = np.flatnonzero(np.r_[True, group[order][1:] != group[order][:-1]])
    hist = np.zeros(topk, np.int64)
    for rows in np.split(order, starts[1:]):
        c = rows[np.argmax(label[rows])]
        rank = int((pred[rows] > pred[c]).sum())
        if rows.size < pad_to and pred[c] < 0:
            rank += pad_to - rows.size
        if rank < topk:
            hist[rank] += 1
    return hist, int(starts.size)


def mean_ap(hist, G):
    """MAP@topk from the counts, float64, in ascending rank."""
    s = 0.0
    for r, h in enumerate(hist):
        s += int(h) / (r + 1)
    return s / int(G)
