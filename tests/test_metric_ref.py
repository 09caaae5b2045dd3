"""The numpy restatement of the two evaluation metrics (tests/_metric_ref.py) against what it restates: sklearn's roc_auc_score, and the
reference's own MAP@12 (tests/golden/ref_multitable_map.npz, written by tests/golden/make_ref_metric_fixture.py from
models/wide_and_deep_multitable/src/metrics.py as it is).  The GPU tests then hold the kernels to the restatement exactly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _metric_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_multitable_map.npz")


@pytest.mark.parametrize("quantised", [False, True], ids=["continuous", "16-level"])
@pytest.mark.parametrize("n", [7, 4097])
def test_restated_auc_is_sklearns(n, quantised):
    """twoU / (2 P N) is the trapezoidal ROC area.  Bound: roc_auc_score sums at most n + 1 float64 trapezoids, each of value <= 1, so its
    rounding error is at most (n + 1) 2^-52 (plus the one division here): (n + 2) 2^-52."""
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(100 + n + quantised)
    pred = rng.random(n).astype(np.float32)
    if quantised:
        pred = (np.floor(pred * 16) / 16).astype(np.float32)
    label = (rng.random(n) < 0.4).astype(np.float32)
    label[:2] = (0.0, 1.0)
    twoU, P, N, n_nan = R.auc_counts(pred, label)
    assert n_nan == 0 and P + N == n and P == int(label.sum())
    want = roc_auc_score(label, pred)
    got = R.auc(twoU, P, N)
    print(f"n={n} quantised={quantised}: |restated - sklearn| = {abs(got - want):.3e}")
    assert abs(got - want) <= (n + 2) * 2.0 ** -52


def test_restated_auc_definitions():
    # all equal: every (positive, negative) pair is a tie -> twoU = P N, AUC 0.5
    assert R.auc_counts(np.full(10, 0.25), np.r_[np.ones(4), np.zeros(6)]) == (24, 4, 6, 0)
    # -0.0 == +0.0; NaN rows leave every other count
    assert R.auc_counts(np.array([-0.0, 0.0, np.nan, 1.0], np.float32), np.array([1, 0, 1, 0], np.float32)) == (1, 1, 2, 1)
    # perfectly separated
    assert R.auc_counts(np.array([0.1, 0.2, 0.8, 0.9]), np.array([0, 0, 1, 1])) == (8, 2, 2, 0)


def test_restated_map_is_the_references():
    z = np.load(GOLDEN)
    assert z["pred"].shape == (5000,) and z["pred"].dtype == np.float32 and z["display_id"].dtype == np.int64
    hist, G = R.group_rank_hist(z["pred"], z["label"], z["display_id"], topk=12, pad_to=30)
    assert G == int(z["G"]) == 700
    assert hist.tolist() == z["hist"].tolist()
    got = R.mean_ap(hist, G)
    print(f"|restated MAP - reference MAP| = {abs(got - float(z['ref_map'])):.3e}")
    assert abs(got - float(z["ref_map"])) <= 1e-15


def test_restated_map_definitions():
    # a display with no positive takes its first row; with two positives the first; a negative clicked prediction in a display of 5
    # ranks behind 25 pads (rank 25 >= 12: counted in G only)
    pred = np.array([0.3, 0.9, 0.5,   0.2, 0.7, 0.6,   -0.1, -0.2, -0.3, -0.4, -0.5], np.float32)
    label = np.array([0, 0, 0,        0, 1, 1,         1, 0, 0, 0, 0], np.float32)
    group = np.array([7, 7, 7,        3, 3, 3,         9, 9, 9, 9, 9])
    hist, G = R.group_rank_hist(pred, label, group)
    assert G == 3 and hist.tolist() == [1, 0, 1] + [0] * 9          # display 3: rank 0; display 7: first row, two above it
    hist, G = R.group_rank_hist(pred, label, group, topk=30, pad_to=30)
    assert hist[25] == 1 and hist.sum() == 3
