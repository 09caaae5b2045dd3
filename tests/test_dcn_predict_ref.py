"""The references of the one-launch Deep&Cross evaluation forward (_dcn_predict_cases.py), checked without a device: the fp32
restatement of the logit meets its derived float64 bound on every case and differs, in at least one bit, from a restatement that
leaves out the last owned slot of either half; the cases are what test_dcn_predict_gpu.py says they are.  c is the float64 cross
stack rounded to fp32 here (on the device: ops.cross_layers' output)."""
import functools

import numpy as np
import pytest

import _dcn_predict_cases as T

CASES = T.all_cases()
IDS = [T.name(c) for c in CASES]


def test_case_tables_reach_every_path_and_edge():
    buckets = [64 * n for n in (1, 2, 4, 8, 12, 16, 20, 24, 32)]
    bucket = lambda X: next(b for b in buckets if X <= b)      # noqa: E731
    assert {c.X for c in T.WIDTH_CASES} == set(T.WIDTHS) and {c.L for c in T.WIDTH_CASES} == {1, 6, 8}
    assert {bucket(X) for X in T.WIDTHS} >= {64, 128, 256, 512, 1280, 2048}
    assert {T.four_columns(X) for X in T.WIDTHS} == {False, True} and not T.four_columns(128) and T.four_columns(129)
    # w / b from global memory: more than 8 layers on the four-column path
    assert all(c.L > 8 and T.four_columns(c.X) for c in T.GLOBAL_W_CASES) and {c.X for c in T.GLOBAL_W_CASES} == {130, 257}
    assert all(c.L == 0 for c in T.NO_LAYER_CASES)
    assert {(c.H - 4) // 256 + 1 for c in T.DEEP_CASES} == {1, 2, 4} and {c.H for c in T.DEEP_CASES} == {4, 252, 256, 260, 1020, 1024}
    assert {c.B for c in T.ROW_CASES} == {1, 2, 31, 32, 33, 65} and {(c.H, c.X) for c in T.ROW_CASES} == {(64, 30), (1024, 1170)}
    c = T.SECOND_PAIR_CASE                                         # 256 workgroups x 16 waves x 2 rows a pass
    assert c.B > 2 * 256 * 16 * 2 and c.B - 2 * 256 * 16 * 2 == 33 and c.B * (c.X + c.H) * 4 < 5 << 20
    for c in T.all_cases():
        assert c.H % 4 == 0 and 0 < c.H <= T.HMAX and 0 < c.X <= T.XMAX


@functools.lru_cache(maxsize=None)
def _built(case):
    x = T.inputs(case)
    c = T.cross64(x["x0"], x["cw"], x["cb"]).astype(np.float32)
    return x, c


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_logit_restatement_meets_its_bound_and_tells_a_lost_slot(case):
    x, c = _built(case)
    d2, w3, b3 = x["d2"], x["w3"], x["b3"]
    z = T.logit32(d2, c, w3, b3)
    z64 = T.logit64(d2, c, w3, b3)
    bound = T.logit_bound(d2, c, w3, b3)
    assert z.dtype == np.float32 and z.shape == (case.B,) and np.isfinite(z).all()
    assert (np.abs(z.astype(np.float64) - z64) <= bound).all(), float((np.abs(z - z64) / bound).max())
    assert (d2 >= 0).all() and np.signbit(d2[d2 == 0]).any() and (d2 == 0).mean() > 0.3
    for drop in ("deep", "cross"):
        assert not np.array_equal(z.view(np.int32), T.logit32(d2, c, w3, b3, drop=drop).view(np.int32)), drop
    if case.kind == "values":
        for t in T.VALUE_LOGITS:
            near = np.abs(z - t) <= 0.02
            assert {float(v) for v in x["label"][near]} == {float(np.float32(v)) for v in T.VALUE_LABELS}, t
        loss, bnd = T.loss64(z, x["label"])
        assert np.isfinite(loss) and np.isfinite(bnd) and loss > 10
        assert np.isfinite(T.sigmoid64(z)).all()
