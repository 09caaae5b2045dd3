"""The two host references of the cross stack agree with each other before either judges a kernel (no GPU needed):
tests/_cross_ref.py's float32 closed form and the oracle's layer-by-layer backward against the float64 stack."""
import numpy as np
import pytest

import _cross_ref as R

U32 = 2.0 ** -24

# (B, D, L): an odd width under one 64-column pass, the Deep&Cross depth, the deepest stack the backward takes
SHAPES = [(9, 67, 3), (33, 300, 6), (5, 130, 8)]


def _bar(D, L):
    """Every quantity is built from L dots of D terms, each carried forward through up to L more layers.  A dot of D fp32
    products summed in any order is off by at most about sqrt(D) units in the last place of its terms' magnitude when the
    roundings do not conspire (D of them when they do); 8 (L + 1) sqrt(D) 2^-24 leaves that a factor 8 and is still 10^3
    times below what a wrong coefficient or a dropped term gives (1e-2 and up at these shapes)."""
    return 8 * (L + 1) * np.sqrt(D) * U32


@pytest.mark.parametrize("B,D,L", SHAPES)
def test_closed_form_and_oracle_agree_with_float64(oracle, B, D, L):
    x0, w, b, dy = R.inputs(B, D, L)
    y, dx0, dw, db = R.cross_f64(x0, w, b, dy)
    bar = _bar(D, L)
    cdx0, cdw, cdb = R.cross_bwd_closed_f32(x0, w, b, dy)
    odx0, odw, odb = oracle.cross_layers_bwd(x0, w, b, dy)
    errs = {"closed dx0": R.row_rel(cdx0, dx0), "closed dw": R.layer_rel(cdw, dw), "closed db": R.layer_rel(cdb, db),
            "oracle dx0": R.row_rel(odx0, dx0), "oracle dw": R.layer_rel(odw, dw), "oracle db": R.layer_rel(odb, db),
            "oracle y": R.row_rel(oracle.cross_layers(x0, w, b), y)}
    print((B, D, L), {k: f"{v:.2e}" for k, v in errs.items()}, f"bar {bar:.2e}")
    for k, v in errs.items():
        assert v <= bar, (k, v, bar)


def test_float64_gradient_is_the_gradient():
    """cross_f64's reverse mode against central differences of its own forward (float64: 1e-7 is h^2 with room)."""
    B, D, L = 3, 5, 4
    x0, w, b, dy = (a.astype(np.float64) for a in R.inputs(B, D, L))
    _, dx0, dw, db = R.cross_f64(x0, w, b, dy)
    loss = lambda x_, w_, b_: float((R.cross_f64(x_, w_, b_)[0] * dy).sum())
    h = 1e-5
    for k, (arr, grad) in enumerate(((x0, dx0), (w, dw), (b, db))):
        num = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            p = [x0.copy(), w.copy(), b.copy()]; m = [x0.copy(), w.copy(), b.copy()]
            p[k][i] += h; m[k][i] -= h
            num[i] = (loss(*p) - loss(*m)) / (2 * h)
        assert np.abs(num - grad).max() <= 1e-7 * max(1.0, np.abs(grad).max()), k


def test_metrics():
    r = np.array([[3.0, 4.0], [0.0, 1.0]])
    a = np.array([[3.0, 4.5], [0.0, 1.0]])
    assert R.row_rel(a, r) == pytest.approx(0.1) and R.row_rel(r, r) == 0.0
    assert R.layer_rel(np.zeros((0, 4)), np.zeros((0, 4))) == 0.0
