"""The host restatements of the FM term's kernels (_fm_cases.py), checked without a device: on every case of test_fm_edges_gpu.py the
restatement meets the derived float64 bound, and every wrong variant of it -- the tree without its guard, the tree in place, the
remainder fields dropped, the last lane dropped -- differs from it in at least one bit wherever the variant applies.  So a device
result that equals the restatement bit for bit is within the bound of float64, and a kernel with one of these faults cannot equal it."""
import numpy as np
import pytest

import _fm_cases as T


def _widths():
    return [("vec", D) for D in T.VEC_D] + [("scalar", D) for D in T.SCALAR_D + T.MISALIGNED_D]


def _cases(path, D):
    cases = T.vec_cases(D) if path == "vec" else T.scalar_cases(D)
    return cases + [c for c in (T.Case("vec", *T.SECOND_TRIPS["fwd4"]), T.Case("scalar", *T.SECOND_TRIPS["fwd1"])) if (c.path, c.D) == (path, D)]


def test_case_tables_reach_every_lane_geometry():
    assert [T.lanes(D)[0] for D in T.VEC_D] == [1, 2, 3, 5, 16, 20, 21, 32, 33, 63, 64]
    assert {D for D in T.VEC_D if 64 % (D // 4)} == {12, 20, 80, 84, 132, 252}                    # spare lanes behind the last lane-group
    assert {D for D in T.VEC_D if T.lanes(D)[1] == 1} == {132, 252, 256}                          # one sample per wave, idle lanes but at 256
    assert all(D % 4 or D > 256 for D in T.SCALAR_D) and {-(-D // 64) for D in T.SCALAR_D} == {1, 2, 3, 4}
    assert {F % 4 for F in T.FS} == {0, 1, 3} and {F % 4 for F in T.COPY_F} == {0, 1, 3}
    assert 2 in {F % 4 for F in (c[1] for c in T.SECOND_TRIPS.values())}
    # the second trips: the forward's cap is 2048 workgroups of 4 waves, the backward's 4096 workgroups of 256 items
    B, F, D = T.SECOND_TRIPS["fwd4"]
    assert T.lanes(D)[1] == 1 and -(-B // 4) > 2048
    B, F, D = T.SECOND_TRIPS["fwd1"]
    assert D % 4 and -(-B // 4) > 2048
    for k in ("bwd4", "bwd4_mix"):
        B, F, D = T.SECOND_TRIPS[k]
        assert D % 4 == 0 and B * F * D // 4 > 4096 * 256
    B, F, D = T.SECOND_TRIPS["bwd1"]
    assert D % 4 and B * F * D > 4096 * 256


def test_inputs_are_what_the_cases_ask_for():
    x = T.inputs(65, 5, 80)
    vx, dout = x["vx"], x["dout"]
    assert not vx[1].any() and vx[0].all()
    scale = np.abs(vx).max(axis=(1, 2))
    assert scale[scale > 0].min() < 0.05 and scale.max() > 50
    zero_field = ~vx.any(axis=2)
    some = zero_field.any(axis=1) & ~zero_field.all(axis=1)
    assert 3 <= some.sum() <= 30                                                                  # about a fifth of 65
    assert (dout == 0).any() and (dout > 0).any() and (dout < 0).any()
    for plants, dt in ((T.BF16_PLANTS, "bf16"), (T.F16_PLANTS, "f16")):
        p = T.plant(np.zeros((2, 3, 20), np.float32), plants)
        assert np.isin(T.bits(plants), T.bits(p)).all(), dt
    f = T.F16_PLANTS.astype(np.float64)
    assert (np.abs(f) > 65504).any() and ((f != 0) & (np.abs(f) < 6e-8)).any()


@pytest.mark.parametrize("path,D", _widths())
def test_restatement_meets_the_float64_bound(path, D):
    worst = 0.0
    for case in _cases(path, D):
        x = T.inputs(case.B, case.F, D)
        for add in (None, x["add"]):
            fm, cs = T.restate(case)(x["vx"], add)
            assert fm.dtype == np.float32 and cs.dtype == np.float32
            err, bnd = np.abs(fm.astype(np.float64) - T.fm64(x["vx"], add)), T.bound(x["vx"], add)
            assert (err <= bnd).all(), (case, add is not None, float((err / np.maximum(bnd, 1e-300)).max()))
            worst = max(worst, float((err[bnd > 0] / bnd[bnd > 0]).max()))
            if case.F == 1:                      # s s - q = x x - x x: exactly +0, in every lane and after every tree
                want = np.zeros(case.B, np.float32) if add is None else add
                assert np.array_equal(T.bits(fm), T.bits(want)), case
        # the two restatements are different orders of one sum: each within the bound, so within twice the bound of one another
        if path == "vec":
            other = T.fm1(x["vx"], None)[0].astype(np.float64)
            assert (np.abs(other - T.fm4(x["vx"], None)[0]) <= 2 * T.bound(x["vx"])).all(), case
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("path,D", _widths())
def test_every_wrong_variant_is_told_apart(path, D):
    seen = set()
    for case in _cases(path, D):
        x = T.inputs(case.B, case.F, D)
        right = T.restate(case)(x["vx"], x["add"])
        for v in T.variants(case):
            wrong = T.restate(case)(x["vx"], x["add"], variant=v)
            same = np.array_equal(T.bits(right[0]), T.bits(wrong[0])) and np.array_equal(T.bits(right[1]), T.bits(wrong[1]))
            assert not same, (case, v)
            seen.add(v)
    if path == "vec":
        lpr, G = T.lanes(D)
        assert seen == {"nolast", "norem"} | ({"noguard"} if G >= 2 else set()) | ({"inplace"} if lpr >= 3 else set())
    else:
        assert seen == {"nolast"} | ({"first64"} if D > 64 else set())


def test_variants_that_do_not_apply_change_no_bit():
    """why variants() leaves them out: the unguarded tree in a wave of one sample, the in-place tree below three lanes, any tree at F = 1"""
    for D, B, F, v in ((256, 5, 5, "noguard"), (132, 5, 5, "noguard"), (80, 1, 5, "noguard"), (4, 9, 5, "inplace"), (8, 9, 5, "inplace"),
                       (80, 13, 1, "noguard"), (80, 13, 1, "inplace"), (80, 13, 1, "nolast")):
        x = T.inputs(B, F, D)
        assert np.array_equal(T.bits(T.fm4(x["vx"], x["add"])[0]), T.bits(T.fm4(x["vx"], x["add"], variant=v)[0])), (D, B, F, v)


def test_backward_restatement_against_float64():
    """g + dout (colsum - vx): three roundings, |err| <= u (|g| + 3 |dout| (|colsum| + |vx|)) to first order"""
    for (B, F, D) in ((5, 3, 20), (4, 5, 65), (9, 4, 256)):
        x = T.inputs(B, F, D)
        cs = T.col_sums(x["vx"])[0]
        got = T.backward(x["g"], x["vx"], cs, x["dout"]).astype(np.float64)
        g, vx, c, w = (a.astype(np.float64) for a in (x["g"], x["vx"], cs, x["dout"]))
        ref = g + w[:, None, None] * (c[:, None, :] - vx)
        bnd = T.U * (np.abs(g) + 3.001 * np.abs(w)[:, None, None] * (np.abs(c)[:, None, :] + np.abs(vx)))
        assert (np.abs(got - ref) <= bnd).all()
        assert np.array_equal(T.bits(got[x["dout"] == 0]), T.bits(x["g"][x["dout"] == 0]))      # dout = 0 leaves g's bits
