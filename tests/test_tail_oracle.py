"""The case table, the fragment-order restatement and the input families of test_tail_oracle_gpu.py, checked without a device:
the restatement of tail_pack_chunk's two formulas is a permutation; the table holds every batch, field count, stride and Dropout
variant the tests were written for; in every case the share of ReLU decisions that the accumulation bound leaves open stays under
the cap the GPU test applies (a condition on the inputs, asserted here with the oracle alone); the integer family is exact."""
import ctypes as C

import numpy as np
import pytest

import _tail_cases as T
from test_dense_gpu import EPS16, TINY


def test_pack_restatement_is_a_permutation():
    """every source element exactly once in its forward copy and once in its backward copy, the four copies in the stated order"""
    from mindrec_amd import _lib
    i2 = np.arange(T.K2 * T.N2, dtype=np.int64).reshape(T.K2, T.N2)
    i3 = np.arange(T.N2 * T.N3, dtype=np.int64).reshape(T.N2, T.N3) + i2.size
    for W in (i2, i3):
        for copy in (T.pack_fwd(W), T.pack_bwd(W)):
            assert copy.shape[2:] == (64, 8) and copy.size == W.size
            assert np.array_equal(np.sort(copy.ravel()), W.ravel())
    flat = T.pack_ref(i2, i3)
    n = C.c_int64(0)
    assert _lib.lib().mrec_tail_packed_elems(T.K2, T.N2, T.N3, C.byref(n)) == 0 and n.value == flat.size
    c2, c3 = i2.size, i3.size
    assert flat[:c2].max() < c2 and flat[c2:c2 + 2 * c3].min() >= c2 and flat[c2 + 2 * c3:].max() < c2
    # the two orders differ, and neither is the identity
    assert not np.array_equal(T.pack_fwd(i2).ravel(), T.pack_bwd(i2).ravel()) and not np.array_equal(T.pack_bwd(i2).ravel(), i2.ravel())
    # spot values of the formulas: lane 17 (row group 1, column 1), element 3
    assert T.pack_fwd(i2)[2, 5, 17, 3] == (2 * 32 + 8 + 3) * T.N2 + 5 * 16 + 1
    assert T.pack_bwd(i2)[2, 5, 17, 3] == (5 * 16 + 1) * T.N2 + 2 * 32 + 8 + 3
    # the patterns the GPU test packs tell every element of a matrix from its neighbours in a fragment
    p = T.index_patterns(T.K2, T.N2).view(np.uint16)
    assert p[0, 0] == 0 and p[1, 0] == T.N2 and p.ravel()[65521] == 0 and len(np.unique(p)) == 65521


def test_case_table_holds_what_it_was_written_for():
    from mindrec_amd import ops
    blocks = {c.B // T.R for c in T.CASES}
    assert {1, 2, 7, 8, 9, 63, 65, 512} <= blocks and all(c.B % T.R == 0 for c in T.CASES)
    assert {(n + 7) // 8 for n in (1, 2, 7, 8)} == {1} and (9 + 7) // 8 == 2          # finish_column's chunk changes between 8 and 9
    assert {0, 1, 15, 16, 17, 32, 33, 48, 49, 63, 64} <= {c.F for c in T.CASES}
    assert {c.pad for c in T.CASES} == {0, 8, 24}
    drops = [c.drop for c in T.CASES if c.drop]
    assert {d[0] for d in drops} == {0.5, 0.8} and {d[1] for d in drops} == {0, 128, 2 ** 33 + 64} and {d[2] for d in drops} == {2, 13}
    assert any(c.drop is None for c in T.CASES) and {c.family for c in T.CASES} == {"rand", "int"}
    assert {c.drop is None for c in T.CASES if c.family == "int"} == {True, False}
    assert all(c.drop[0] == 0.5 for c in T.CASES if c.family == "int" and c.drop)
    assert len(T.BY_NAME) == len(T.CASES)
    for c in T.CASES:
        assert ops.tail_supported(c.B, T.K2, T.N2, T.N3)
    assert not ops.tail_supported(64 * 513, T.K2, T.N2, T.N3) and not ops.tail_supported(0, T.K2, T.N2, T.N3)
    assert T.tiles(576) == [slice(0, 576)] and T.tiles(4032) == [slice(0, 64), slice(3968, 4032)]
    for r, c in T.TRANSPOSE_SHAPES:
        assert r % 8 == 0 and c % 8 == 0
    assert sum(1 for r, c in T.TRANSPOSE_SHAPES if r % 64 or c % 64) >= 3


def _forward(oracle, case, dt, sl):
    """both stages for the rows sl with the ORACLE's y2 standing in for the kernel's"""
    inp = T.inputs(oracle, case, dt)
    s2 = T.stage(oracle, inp["x"][sl], inp["w2"], inp["b2"], dt, T.masks(oracle, case, sl, 1), EPS16[dt], TINY[dt])
    s3 = T.stage(oracle, s2["ref"], inp["w3"], inp["b3"], dt, T.masks(oracle, case, sl, 2), EPS16[dt], TINY[dt])
    return inp, s2, s3


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_undecidable_share_is_under_the_cap(oracle, name, dt):
    case = T.BY_NAME[name]
    for sl in T.tiles(case.B):
        inp, s2, s3 = _forward(oracle, case, dt, sl)
        share = float(T.undecidable(s3).mean())
        # (the integer family leaves nothing open: its sums are exact, a pre-activation of 0 IS 0 -- test_integer_family_is_exact)
        assert share <= T.UNDECIDABLE_CAP or case.family == "int", (name, dt, sl, share)
        x = inp["x"][sl]
        if case.family == "rand":
            assert (x < 0).any() and (np.signbit(x) & (x == 0)).any() and (x > 0).mean() > 0.1
            assert (s2["ref"] > 0).mean() > 0.1 and (s3["ref"] > 0).mean() > 0.1         # the masks leave something to check
        if case.F:
            assert not inp["wide"][:, :, 1].any()
            mag = np.abs(inp["wide"][:, :, 0])
            assert mag.max() > 100 * np.median(mag) or case.F < 3 or case.family == "int"      # the order of the adds shows
        assert np.array_equal(oracle.round16(x, dt), x)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", [c.name for c in T.CASES if c.family == "int"])
def test_integer_family_is_exact(oracle, name, dt):
    """every 16-bit value an integer of magnitude <= 256, every sum of |terms| far under 2^24, the logit a dyadic number that fp32 holds"""
    case = T.BY_NAME[name]
    sl = slice(0, case.B)
    inp, s2, s3 = _forward(oracle, case, dt, sl)
    x, w2, w3 = inp["x"], inp["w2"], inp["w3"]
    assert set(np.unique(x)) <= {0.0, 1.0, 2.0, 4.0} and 0.4 < (x == 0).mean() < (0.8 if case.drop else 0.6)
    assert set(np.unique(w2)) == {-1.0, 0.0, 1.0} == set(np.unique(w3))
    for v in (inp["b2"], inp["b3"], s2["pre"], s3["pre"], s2["ref"], s3["ref"]):
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 256
    assert np.array_equal(s2["ref"], oracle.round16(s2["ref"], dt)) and s2["ref"].max() > 16 and s3["ref"].max() > 16
    assert (np.abs(x).astype(np.float64) @ np.abs(w2)).max() < 2.0 ** 20 and (np.abs(s2["ref"]).astype(np.float64) @ np.abs(w3)).max() < 2.0 ** 20
    assert (s3["pre"] == 0).any()                     # the ReLU's corner is met exactly
    assert not T.undecidable(s3).any() or (np.abs(s3["pre"])[T.undecidable(s3)] == 0).all()
    # the head: y3 . w5 in 2048ths, the wide terms in 128ths
    w5 = inp["w5"].astype(np.float64)
    assert np.array_equal(w5 * 2048, np.rint(w5 * 2048)) and np.array_equal(inp["wide"] * 128, np.rint(inp["wide"] * 128))
    tot = (s3["ref"].astype(np.float64) * np.abs(w5)).sum(1) + np.abs(inp["wide"][:, :, 0]).sum(1) + 1
    assert tot.max() * 2048 < 2.0 ** 24
    z = s3["ref"].astype(np.float64) @ w5 + float(inp["b5"][0]) + T.wide_sum_f32(inp["wide"], inp["wb"]).astype(np.float64)
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    assert np.array_equal(T.wide_sum_f32(inp["wide"], inp["wb"]).astype(np.float64), inp["wide"][:, :, 0].astype(np.float64).sum(1) + float(inp["wb"]))
