"""Generator of tests/golden/ref_multitable_map.npz: runs the REFERENCE's own MAP@12 -- models/wide_and_deep_multitable/src/metrics.py,
`new_compute_mAP` (:70-107), unmodified, imported by path from a mindspore-lab/mindrec checkout -- over `compat/mindspore` (the file
imports mindspore.nn.metrics.Metric), as make_ref_fixtures.py runs the reference's models, and records what it computes.

The input: 5000 rows in 700 displays, fed in shuffled order; exactly one positive per display; predictions distinct within a display
(and none equal to the pads' 0.0).  For such input the reference's result does not depend on how its unstable sorts (sort_values by
display, np.argsort of the predictions) order equal elements.  Displays of 1 to more than 30 rows, a fifth of the clicked predictions
negative (the pads rank above them), display ids scattered over 40 bits.

Stored: pred, label (float32), display_id (int64), ref_map (the float new_compute_mAP returned), hist (int64 [12]: displays per rank of
the clicked row, from the per-display scores 1 / (rank + 1) the reference's mean_AP_topk returned, seen through a look-only wrapper)
and G (displays).  Nothing of the reference travels: only the .npz written here is committed.

Usage:  MREC_REFERENCE=<checkout> python tests/golden/make_ref_metric_fixture.py
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["MREC_REFERENCE"]
TOPK = 12


def ref_metrics():
    for p in (ROOT, os.path.join(ROOT, "compat"), os.path.join(REF, "models", "wide_and_deep_multitable")):
        sys.path.insert(0, p)
    m = importlib.import_module("src.metrics")
    assert m.__file__.startswith(REF), m.__file__
    return m


def make_input(rng, n=5000, G=700):
    sizes = np.ones(G, np.int64)
    sizes[:6] = (31, 35, 44, 30, 29, 13)                               # around the reference's 30 pads and its top 12
    left = n - int(sizes.sum())
    sizes[6:] += np.bincount(rng.integers(6, G, size=left), minlength=G)[6:]
    assert sizes.sum() == n and sizes.min() >= 1
    ids = rng.choice(1 << 40, size=G, replace=False).astype(np.int64) - (1 << 39)
    display = np.repeat(ids, sizes)
    # distinct within a display, none 0.0: distinct float32 values drawn once for all rows
    vals = np.unique((rng.random(4 * n) * 1.25 - 0.25).astype(np.float32))
    vals = vals[vals != 0]
    pred = rng.permutation(vals)[:n]
    label = np.zeros(n, np.float32)
    start = np.cumsum(sizes) - sizes
    label[start + rng.integers(0, sizes)] = 1.0
    feed = rng.permutation(n)
    return pred[feed], label[feed], display[feed]


if __name__ == "__main__":
    import pandas as pd
    m = ref_metrics()
    pred, label, display = make_input(np.random.default_rng(20260))
    scores = []
    inner = m.mean_AP_topk

    def spying_mean_AP_topk(*a, **k):                                   # (looks, does not touch)
        out = inner(*a, **k)
        scores.extend(out)
        return out

    m.mean_AP_topk = spying_mean_AP_topk
    # the frame as the reference's AUCMetric.eval builds it (:143-147): Python lists of what update() collected
    df = pd.DataFrame({"display_ids": display.tolist(), "preds": pred.tolist(), "labels": label.tolist()})
    ref_map = float(m.new_compute_mAP(df, gb_key="display_ids", top_k=TOPK))
    G = len(scores)
    hist = np.zeros(TOPK, np.int64)
    for s in scores:
        if s:
            r = round(1.0 / s) - 1
            assert 0 <= r < TOPK and s == 1.0 / (r + 1)
            hist[r] += 1
    assert G == np.unique(display).size == 700
    path = os.path.join(HERE, "ref_multitable_map.npz")
    np.savez_compressed(path, pred=pred, label=label, display_id=display, ref_map=np.float64(ref_map), hist=hist, G=np.int64(G))
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KB; map {ref_map!r} hist {hist.tolist()} G {G}")
