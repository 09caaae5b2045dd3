"""mrec_x3_tile_rows (the read-only query for the three-part fp32 GEMM's tile configuration) and the case tables of
test_x3_edges_gpu.py, checked without a device: the rule's 256 is literal, so its answers are the same everywhere."""
import ctypes as C

import numpy as np
import pytest

import _x3_edge_cases as T


def test_tile_rows_argument_errors():
    from mindrec_amd import _lib, ops
    l = _lib.lib()
    out = C.c_int32(-7)
    bad = [(-1, 64, 64, 64, 1), (3, 64, 64, 64, 1), (0, 0, 64, 64, 1), (1, -5, 64, 64, 1), (2, 64, 0, 64, 1), (0, 64, 64, 0, 1), (0, 64, -8, 64, 1),
           (0, 64, 64, 64, 0), (2, 64, 64, 64, -1), (0, 64, 64, 64, 2), (1, 64, 64, 64, 3),         # forms 0 and 1 take S = 1 only
           (2, 64, 64, 64, 4), (2, 64, 64, 64, 7), (2, 129, 64, 64, 17)]                           # form 2: a slab would stay empty
    for args in bad:
        assert l.mrec_x3_tile_rows(*args, C.byref(out)) == -1, args             # MREC_EINVAL
        assert out.value == -7                                                  # ... and nothing written
    assert l.mrec_x3_tile_rows(0, 64, 64, 64, 1, None) == -1
    with pytest.raises(_lib.MrecError) as e:
        ops.x3_tile_rows(0, 0, 8, 8)
    assert e.value.code == -1
    with pytest.raises(_lib.MrecError):
        ops.x3_tile_rows(2, 64, 8, 8, S=4)
    assert ops.x3_tile_rows(0, 64, 8, 8) == ops.x3_tile_rows(2, 64, 8, 8, S=6) == 128


def test_tile_rows_follow_the_rule_on_both_sides_of_its_threshold():
    """one round of 256-row tiles (t8 <= 256): 256-row tiles from t4 = 257 workgroups of 128 rows on; the reduction length plays no
    part.  Two rounds (256 < t8 <= 512): 128-row tiles up to t4 = 768."""
    from mindrec_amd import ops
    for red in (2, 64, 4096):
        # forms 0 and 1: one tile column; p = 128 * 256 rows are 256 tiles of 128 rows
        for form in (0, 1):
            at = lambda p: ops.x3_tile_rows(form, *T.mkn(form, p, red, 256))
            assert at(128 * 256) == 128 and at(128 * 256 + 1) == 256
            assert at(256 * 256 + 1) == 128                                     # t8 = 257, t4 = 513: 3 * 0.55 < 2
            assert at(128 * 768) == 128 and at(128 * 768 + 1) == 256            # t4 = 769: 4 * 0.55 > 2
    # form 2: tiles x slabs; 16 x 4 tiles x 4 slabs = 256, 17 x 4 x 4 = 272
    for M in (128, 1000):
        assert ops.x3_tile_rows(2, M, 2048, 1024, 4) == 128 and ops.x3_tile_rows(2, M, 2049, 1024, 4) == 256
        assert ops.x3_tile_rows(2, M, 2049, 1024, 3) == 128                     # ... the slabs count: 17 x 4 x 3 = 204
    # the restatement the tables are sized with says the same everywhere it is asked
    rng = np.random.default_rng(0)
    for _ in range(2000):
        form = int(rng.integers(0, 3))
        M, K, N = (int(v) for v in rng.integers(1, 70000, 3) // rng.choice([1, 16, 256], 3) + 1)
        S = 1 if form != 2 else int(rng.choice(T.slab_counts(6 * (T.up64(M) // 64))[0][:12]))
        assert ops.x3_tile_rows(form, M, K, N, S) == T.rule_rows(form, M, K, N, S), (form, M, K, N, S)


def test_case_table_reaches_the_configurations_it_was_written_for():
    from mindrec_amd import _lib, ops
    table = T.expected_configs()
    assert {rows for *_, rows in table} == {128, 256}
    for what, form, (M, K, N), S, rows in table:
        T.require_rows(ops, form, M, K, N, rows, S)
    for form in (0, 1, 2):
        assert {f for _, f, _, _, rows in table if rows == 256} == {0, 1, 2}
    # the sweeps: reduction lengths give 1, 1, 1, 2, 2, 3, 3 K-tiles per segment, widths all four (W % 4, ld % 4) classes
    assert [-(-r // 64) for r in T.SWEEP_RED] == [1, 1, 1, 2, 2, 3, 3] and {r % 64 == 0 for r in T.SWEEP_RED} == {True, False}
    assert T.classes(T.SWEEP_Q) == {(0, 0), (0, 2), (2, 0), (2, 2)}
    assert all(v % 2 == 0 for v in T.SWEEP_Q + T.POST_C)
    # the split input gradient: taken / not taken, and S, through the workspace query
    for (M, K, N), S, rem in T.SPLIT_TAKEN:
        assert T.split_plan(M, K, N)[0::2] == (S, rem)
        T.require_split(_lib, M, K, N, S, rem)
    M, K, N = T.SPLIT_NOT_TAKEN
    assert T.split_plan(M, K, N)[0] == 0 and K - 256 * (-(-K // 256) - 1) == 224
    T.require_split(_lib, M, K, N, 0, 0)
    assert {K % 4 for (M, K, N), _, _ in T.SPLIT_TAKEN} == {2}                   # ld = K: rows only 8-byte aligned


def test_slab_counts_valid_and_refused():
    """the S form 2 takes for each T = 6 ceil(M / 64) the slab tests use: ops.x3_slabs and the library's own check agree"""
    from mindrec_amd import _lib, ops
    assert [6 * (T.up64(M) // 64) for M in T.SLAB_M] == [6, 6, 12, 18, 18]
    assert T.slab_counts(6) == ([1, 2, 3, 6], [4, 5])
    assert T.slab_counts(12) == ([1, 2, 3, 4, 6, 12], [5, 7, 8, 9, 10, 11])
    assert T.slab_counts(18) == ([1, 2, 3, 4, 5, 6, 9, 18], [7, 8, 10, 11, 12, 13, 14, 15, 16, 17])
    for M in T.SLAB_M:
        Tt = 6 * (T.up64(M) // 64)
        ok, refused = T.slab_counts(Tt)
        assert sorted({ops.x3_slabs(M, s) for s in range(1, Tt + 1)}) == ok
        assert all(ops.x3_slabs(M, s) <= s for s in range(1, Tt + 1)) and ops.x3_slabs(M, Tt + 5) == Tt
        for K, N in T.SLAB_KN:
            for S in ok:
                assert ops.x3_slabs(M, S) == S and ops.x3_tile_rows(2, M, K, N, S) == 128
            for S in refused + [Tt + 1]:
                assert ops.x3_slabs(M, S) < S
                with pytest.raises(_lib.MrecError) as e:
                    ops.x3_tile_rows(2, M, K, N, S)
                assert e.value.code == -1
    # the first valid S > 1 and the first refused S at each T
    assert [(T.slab_counts(t)[0][1], T.slab_counts(t)[1][0]) for t in (6, 12, 18)] == [(2, 4), (2, 5), (2, 7)]


def _exact_cases():
    """every (family, form, p, red, q) the GPU tests run exact inputs at"""
    out = [(f, *T.SIMPLEST) for f in T.FAMILIES]
    out += [(f, form, *c) for f in T.FAMILIES for form in (0, 1, 2) for c in T.sweep_cases()]
    out += [(f, 2, K, M, N) for f in T.FAMILIES for M in T.SLAB_M for K, N in T.SLAB_KN]
    for name, form, (M, K, N), S in T.MR8_GEMM:
        p, red, q = {0: (M, K, N), 1: (M, N, K), 2: (K, M, N)}[form]
        out += [(f, form, p, red, q) for f in T.FAMILIES]
    (M, K, N), _, _ = T.SPLIT_TAKEN[0]
    out.append(("p", 1, M, N, K))
    return sorted(set(out))


def test_exact_families_are_exact_and_have_the_parts_they_claim():
    """sum_k |a_k| |b_k| < 2^24 for every output -- and the stronger sum over the PARTS' magnitudes, which bounds every partial sum of
    part products in any order; parts nonzero where claimed, adding back exactly, integer valued; a nonzero in every K-tile"""
    nparts = {"p": (3, 1), "q": (1, 3), "m": (2, 2)}
    for family, form, p, red, q in _exact_cases():
        what = (family, form, p, red, q)
        A, B = T.exact_inputs(family, form, p, red, q)
        assert A.shape == (p, red) and B.shape == (red, q) and A.dtype == B.dtype == np.float32
        assert float((np.abs(A).astype(np.float64) @ np.abs(B)).max()) < 2.0 ** 24, what
        assert T.exact_margin(A, B) < 1.0, what
        for X, n in ((A, nparts[family][0]), (B.T, nparts[family][1])):
            parts = T.split3(X).double().numpy()
            nz = X != 0
            assert np.array_equal(parts.sum(0), X.astype(np.float64)), what            # add back exactly
            assert np.array_equal(parts, np.rint(parts)), what                          # integers
            assert all((parts[i][nz] != 0).all() for i in range(n)) and all((parts[i] == 0).all() for i in range(n, 3)), what
            tiles = [nz[:, t:t + 64].sum(1) for t in range(0, red, 64)]                 # per dot product and K-tile
            assert all((c >= 1).all() and (c == c[0]).all() for c in tiles), what
    # the figures the families were proposed with: two 19-bit nonzeros per K-tile at 19 K-tiles is over the budget, 13 are not
    A, B = T.exact_inputs("p", 2, 1000, 777, 1016)
    assert (A != 0).sum(1).max() == 26 and 0.15 < T.exact_margin(A, B) < 0.85


def test_parts_image_is_the_header_layout():
    x = np.float32([[1.0, 3.14159274, -1e-8], [257.0, 0.0, 2.0 ** -20]])
    img = T.parts_image(x)
    assert tuple(img.shape) == (3, 64, 64) and float(img[:, 2:, :].abs().max()) == 0 and float(img[:, :, 3:].abs().max()) == 0
    assert np.array_equal(img[:, :2, :3].double().sum(0).numpy(), x.astype(np.float64))
    assert img[1, 1, 0] == 1.0 and img[2, 1, 0] == 0.0 and img[0, 1, 0] == 256.0
