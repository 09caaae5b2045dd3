"""The references of the Deep&Cross head's edge tests (_dcn_head_cases.py), checked without a device: the fp32 restatement of the logit
meets its derived float64 bound on every case and differs from a restatement that leaves out the last slot of either half; the
cases are what test_dcn_head_edges_gpu.py says they are; and in every row-edge case a single row lost or doubled -- the last of a
wave, the only row of the last workgroup, any row -- moves a batch sum or the loss by more than its bound."""
import numpy as np
import pytest

import _dcn_head_cases as T

IDS = [T.name(c) for c in T.all_cases()]


def test_case_tables_reach_every_slot_and_row_edge():
    deep = {(c.H - 4) // 256 + 1 for c in T.SLOT_CASES}              # float4 slots q in use: the last owned column is H - 4
    assert deep == {1, 2, 4}
    for c in T.SLOT_CASES:                                           # ... and X = 2 q 64 +- 2 likewise
        assert c.H % 4 == 0 and c.X % 2 == 0 and c.H <= T.HMAX and c.X <= T.XMAX
    assert {c.H for c in T.SLOT_CASES} >= {4, 252, 256, 260, 1020, 1024} and {c.X for c in T.SLOT_CASES} >= {2, 126, 128, 130, 1170, 1278, 1280}
    # rows: a wave owns 8, a workgroup 32 -- B = 33 and 65 leave three waves of the last workgroup without a row, B = 9 two
    assert {B % 8 for B in T.ROW_B} == {0, 1, 7} and {B % 32 for B in T.ROW_B} >= {0, 1, 31}
    for (H, X) in T.REFUSED_SHAPES:
        assert H % 4 or X % 2 or H > T.HMAX or X > T.XMAX
    assert 2 * T.HMAX + T.XMAX + 2 == 3330                            # the widest partial row: 4 of them stay below 64 KiB of LDS


@pytest.mark.parametrize("case", T.all_cases(), ids=IDS)
def test_logit_restatement_meets_its_bound_and_tells_a_lost_slot(case):
    x = T.inputs(case)
    z = T.logit32(x["d2"], x["c"], x["w3"], x["b3"])
    z64 = T.logit64(x["d2"], x["c"], x["w3"], x["b3"])
    assert z.dtype == np.float32 and (np.abs(z.astype(np.float64) - z64) <= T.logit_bound(x["d2"], x["c"], x["w3"], x["b3"])).all()
    assert x["w3"][case.H] == 1.0 and np.signbit(x["d2"][x["d2"] == 0]).any() and (x["d2"] == 0).mean() > 0.3
    for drop in ("deep", "cross"):
        assert not np.array_equal(z.view(np.int32), T.logit32(x["d2"], x["c"], x["w3"], x["b3"], drop=drop).view(np.int32)), drop
    if case.kind == "moderate":
        assert np.abs(z).max() <= T.ZMAX and set(np.unique(x["label"])) <= {0.0, 1.0}
        assert np.abs(T.dlogit64(z, x["label"], 1.0)).min() >= 0.0179
    else:
        near = lambda t: np.abs(z - t) <= 0.02
        for t in T.VALUE_LOGITS:
            assert {float(v) for v in x["label"][near(t)]} == {float(np.float32(v)) for v in T.VALUE_LABELS}, t
        dl = T.dlogit64(z, x["label"], T.dscale(case))
        loss, bnd = T.loss64(z, x["label"])
        assert np.isfinite(dl).all() and np.isfinite(loss) and np.isfinite(bnd) and loss > 10


@pytest.mark.parametrize("case", T.ROW_CASES, ids=[T.name(c) for c in T.ROW_CASES])
def test_a_lost_or_doubled_row_moves_a_sum_past_its_bound(case):
    x = T.inputs(case)
    z = T.logit32(x["d2"], x["c"], x["w3"], x["b3"])
    dl = T.dlogit64(z, x["label"], T.dscale(case))
    dd2 = T.grads64(x, z, x["label"], T.dscale(case))[0]
    right, (loss, loss_bnd) = T.sums64(x, dl, dd2), T.loss64(z, x["label"])
    for r in range(case.B):
        for weight in (0.0, 2.0):
            rows = np.ones(case.B)
            rows[r] = weight
            wrong = T.sums64(x, dl, dd2, rows)
            moved = [k for k in right if (np.abs(wrong[k][0] - right[k][0]) > right[k][1]).any()]
            if abs(T.loss64(z, x["label"], rows)[0] - loss) > loss_bnd:
                moved.append("loss")
            assert moved, (r, weight)
            assert "db3" in moved and "dw3" in moved, (r, weight, moved)      # (more than asked: these two see every row)
