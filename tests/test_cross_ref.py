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


FWD_BAR = 1e-5      # the forward's bar (include/mrec.h; tests/test_cross_sweep_gpu.py), row_rel; the device's largest observed: 2.0e-6


def test_forward_restatement_is_a_forward_and_sees_its_wave_sum():
    """cross_fwd_bits, which the device is held to bit for bit, is itself within the forward's bar of the float64 stack at every
    pinned shape; and with the two wave sums exchanged it gives other bits at some shape of EACH layout -- the difference the
    pin exists to see is one it can see."""
    differs = {False: 0, True: 0}
    for B in R.BITS_B:
        for D, L in R.BITS_DL:
            x0, w, b, _ = R.inputs(B, D, L)
            y = R.cross_f64(x0, w, b)[0]
            got = R.cross_fwd_bits(x0, w, b)
            assert got.dtype == np.float32 and got.shape == (B, D)
            err = R.row_rel(got, y)
            print((B, D, L), f"err {err:.2e}")
            assert err <= FWD_BAR, (B, D, L, err)
            swapped = R.cross_fwd_bits(x0, w, b, swap_sums=True)
            assert R.row_rel(swapped, y) <= FWD_BAR
            differs[D > 128] += not np.array_equal(got.view(np.int32), swapped.view(np.int32))
    print("shapes at which the swapped wave sums change bits:", differs)
    assert differs[False] >= 1 and differs[True] >= 1


def test_wave_sums():
    """Both wave sums are sums (exact on small integers), and they are different orders: 2^24 in lane 0, 1 in lanes 1 and 33.
    The tree adds lanes 0 and 1 first and lane 33's 1 to 2^24 at the last level: both are lost to rounding.  The butterfly
    adds lanes 1 and 33 first (d = 32), and their 2 reaches 2^24 whole at d = 1."""
    t = np.arange(128, dtype=np.float32).reshape(2, 64)
    assert list(R.lane_tree(t)) == [2016.0, 6112.0] and list(R.lane_butterfly(t)) == [2016.0, 6112.0]
    t = np.zeros((1, 64), np.float32); t[0, 0] = 2.0 ** 24; t[0, 1] = 1; t[0, 33] = 1
    assert R.lane_tree(t)[0] == 2.0 ** 24 and R.lane_butterfly(t)[0] == 2.0 ** 24 + 2


def test_metrics():
    r = np.array([[3.0, 4.0], [0.0, 1.0]])
    a = np.array([[3.0, 4.5], [0.0, 1.0]])
    assert R.row_rel(a, r) == pytest.approx(0.1) and R.row_rel(r, r) == 0.0
    assert R.layer_rel(np.zeros((0, 4)), np.zeros((0, 4))) == 0.0
