"""The fp32-MFMA DenseLayer's host layer (csrc/mrec_gemm_f32.hip: mrec_dense32_fwd, mrec_dense32_bwd_input,
mrec_dense32_bwd_weight, mrec_dense32_bwd_weight_slabs, mrec_dense32_load_widths) and the case tables of
test_dense32_edges_gpu.py, without a device: every refusal below returns before any launch, so the fake non-null addresses are
never dereferenced."""
import ctypes as C

import numpy as np
import pytest

import _dense32_edge_cases as T

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
A = 0x10000                       # a 16-byte aligned address nobody reads


def fwd(l, x=A, ldx=64, w=A, ldw=64, bias=None, M=8, K=64, N=64, relu=1, y=A, ldy=64):
    return l.mrec_dense32_fwd(x, ldx, w, ldw, bias, M, K, N, relu, y, ldy, None)


def dgrad(l, dy=A, lddy=64, w=A, ldw=64, h=None, ldh=0, M=8, K=64, N=64, dx=A, lddx=64, colsum=None):
    return l.mrec_dense32_bwd_input(dy, lddy, w, ldw, h, ldh, M, K, N, dx, lddx, colsum, None)


def wgrad(l, x=A, ldx=64, dy=A, lddy=64, M=64, K=64, N=64, S=1, dw=A):
    return l.mrec_dense32_bwd_weight(x, ldx, dy, lddy, M, K, N, S, dw, None)


# entry -> {rule: (arguments changed against a valid call, code)}
ROWS = {
    fwd: {
        "M < 0": (dict(M=-1), EINVAL), "K = 0": (dict(K=0), EINVAL), "K < 0": (dict(K=-64), EINVAL), "N = 0": (dict(N=0), EINVAL),
        "N < 0": (dict(N=-1), EINVAL),
        "ldx < K": (dict(ldx=63), EINVAL), "ldw < N": (dict(ldw=63), EINVAL), "ldy < N": (dict(ldy=63), EINVAL),
        "null x": (dict(x=None), EINVAL), "null w": (dict(w=None), EINVAL), "null y": (dict(y=None), EINVAL),
        "M = 0": (dict(M=0, x=None, w=None, y=None), OK),
        "M = 0, ldy < N": (dict(M=0, ldy=1), EINVAL),
        "M > 2^30": (dict(M=2 ** 30 + 1), EUNSUPPORTED),
        "M ldx 4 = 2^31": (dict(M=2 ** 23), EUNSUPPORTED),
        "K ldw 4 = 2^31": (dict(K=2 ** 15, ldx=2 ** 15, ldw=2 ** 14), EUNSUPPORTED),
    },
    dgrad: {
        "M < 0": (dict(M=-1), EINVAL), "K = 0": (dict(K=0), EINVAL), "K < 0": (dict(K=-1), EINVAL), "N = 0": (dict(N=0), EINVAL),
        "N < 0": (dict(N=-64), EINVAL),
        "lddy < N": (dict(lddy=63), EINVAL), "ldw < N": (dict(ldw=63), EINVAL), "lddx < K": (dict(lddx=63), EINVAL),
        "ldh < K": (dict(h=A, ldh=63), EINVAL),
        "null dy": (dict(dy=None), EINVAL), "null w": (dict(w=None), EINVAL), "null dx": (dict(dx=None), EINVAL),
        "M = 0": (dict(M=0, dy=None, w=None, dx=None), OK),
        "M = 0, ldh < K": (dict(M=0, h=A, ldh=1), EINVAL),
        "M > 2^30": (dict(M=2 ** 30 + 1), EUNSUPPORTED),
        "M lddy 4 = 2^31": (dict(M=2 ** 23), EUNSUPPORTED),
        "K ldw 4 = 2^31": (dict(K=2 ** 15, lddx=2 ** 15, ldw=2 ** 14), EUNSUPPORTED),
    },
    wgrad: {
        "M < 0": (dict(M=-1), EINVAL), "K = 0": (dict(K=0), EINVAL), "K < 0": (dict(K=-1), EINVAL), "N = 0": (dict(N=0), EINVAL),
        "N < 0": (dict(N=-1), EINVAL),
        "ldx < K": (dict(ldx=63), EINVAL), "lddy < N": (dict(lddy=63), EINVAL),
        "S = 0": (dict(S=0), EINVAL), "S < 0": (dict(S=-2), EINVAL),
        "null dw_slabs": (dict(dw=None), EINVAL), "null dw_slabs, M = 0": (dict(dw=None, M=0), EINVAL),
        "null x": (dict(x=None), EINVAL), "null dy": (dict(dy=None), EINVAL),
        "empty slab: 64 rows in 3": (dict(S=3), EINVAL),            # 32 rows per slab: the third holds none
        "empty slab: 257 rows in 4": (dict(M=257, S=4), EINVAL),    # 96 rows per slab
        "empty slab: 1 row in 2": (dict(M=1, S=2), EINVAL),
        "M > 2^30": (dict(M=2 ** 30 + 1), EUNSUPPORTED),
        "M ldx 4 = 2^31": (dict(M=2 ** 23), EUNSUPPORTED),
        "M lddy 4 = 2^31": (dict(M=2 ** 14, lddy=2 ** 15), EUNSUPPORTED),
    },
}


@pytest.mark.parametrize("entry,rule", [(e, r) for e in ROWS for r in ROWS[e]], ids=[f"{e.__name__}: {r}" for e in ROWS for r in ROWS[e]])
def test_argument_refusals(entry, rule):
    from mindrec_amd import _lib
    args, code = ROWS[entry][rule]
    assert entry(_lib.lib(), **args) == code


def test_slab_proposal_argument_errors():
    from mindrec_amd import _lib, ops
    l = _lib.lib()
    out = C.c_int32(-7)
    for args in [(-1, 64, 64), (64, 0, 64), (64, -1, 64), (64, 64, 0), (64, 64, -5)]:
        assert l.mrec_dense32_bwd_weight_slabs(*args, C.byref(out)) == EINVAL, args
        assert out.value == -7                                                  # ... and nothing written
    assert l.mrec_dense32_bwd_weight_slabs(64, 64, 64, None) == EINVAL
    with pytest.raises(_lib.MrecError) as e:
        ops.dense32_bwd_weight_slabs(64, 0, 8)
    assert e.value.code == EINVAL
    assert ops.dense32_bwd_weight_slabs(0, 8, 8) == 1 and ops.dense32_bwd_weight_slabs(511, 8, 8) == 1       # 256 rows per slab at least


def test_slab_proposal_follows_its_cost_rule_and_is_never_refused():
    from mindrec_amd import _lib, ops
    l = _lib.lib()
    assert T.proposed_slabs(16384, 1170, 1024) == ops.dense32_bwd_weight_slabs(16384, 1170, 1024) > 1
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(2000):
        M = int(rng.integers(0, 70000) // rng.choice([1, 16, 256]))
        K, N = (int(v) for v in rng.integers(1, 5000, 2) // rng.choice([1, 16], 2) + 1)
        S = ops.dense32_bwd_weight_slabs(M, K, N)
        assert S == T.proposed_slabs(M, K, N), (M, K, N)
        assert M == 0 or T.slab_valid(M, S), (M, K, N, S)
        seen.add(S)
        # the restated validity is the library's: what it calls empty is refused (before any launch)
        bad = next((s for s in range(S + 1, 70) if not T.slab_valid(M, s)), None) if M > 0 else None
        if bad is not None and M * max(K, N) * 4 < 2 ** 31:
            assert wgrad(l, M=M, K=K, N=N, ldx=K, lddy=N, S=bad) == EINVAL, (M, K, N, bad)
    assert len(seen) > 8 and 1 in seen and max(seen) > 32


def test_slab_counts_valid_and_refused():
    assert T.slab_counts(1) == ([1], []) and T.slab_counts(32) == ([1], []) and T.slab_counts(33) == ([1, 2], [])
    assert T.slab_counts(64) == ([1, 2], []) and T.slab_counts(65) == ([1, 2, 3], [])
    assert T.slab_counts(100) == ([1, 2, 4], [3])
    assert T.slab_counts(257) == ([1, 2, 3, 5, 9], [4, 6, 7, 8])
    assert [T.rows_per_slab(257, S) for S in (1, 2, 3, 5, 9)] == [288, 160, 96, 64, 32]           # S = 5, 9: the last slab holds one row
    assert {T.proposed_slabs(M, K, N) for M in T.SLAB_M for K, N in T.SLAB_KN} == {1}              # below 512 rows: one slab


def test_sweeps_reach_every_k_tile_count_and_tail():
    tiles = [T.k_tiles(r) for r in T.SWEEP_RED]
    assert {t for t, _ in tiles} == {1, 2, 3, 4} and {1, 2, 31, 32} <= {k for _, k in tiles}
    assert {k for t, k in tiles if t == 1} >= {1, 2, 31, 32}                    # one K-tile: the prologue's tile is the last one
    assert T.k_tiles(T.BASE[1]) == (3, 2) and T.k_tiles(T.SIMPLEST[1]) == (1, 32)
    assert {p % 32 for p in T.SWEEP_P} >= {0, 1, 31} and {T.cdiv(p, 32) for p in T.SWEEP_P if p <= 128} == {1, 2, 3, 4}
    assert {T.cdiv(q, 32) for q in T.SWEEP_Q if q <= 128} == {1, 2, 3, 4} and max(T.SWEEP_Q) > 256 and max(T.SWEEP_P) > 256
    cases = T.sweep_cases()
    assert len(cases) == len(T.SWEEP_RED) + len(T.SWEEP_P) + len(T.SWEEP_Q)
    assert all(max(T.mkn(f, *c)) <= 258 for f in (0, 1, 2) for c in cases)


def load_widths(l, form, a, lda, b, ldb, K, N):
    va, vb = C.c_int32(-7), C.c_int32(-7)
    return l.mrec_dense32_load_widths(form, a, lda, b, ldb, K, N, C.byref(va), C.byref(vb)), (va.value, vb.value)


def test_load_width_query_is_the_restated_rule():
    """mrec_dense32_load_widths answers from the function the launches dispatch on: 4 floats per load where address, stride and
    contiguous extent are all multiples of 16 bytes, 2 where of 8, else 1; form 1's operands both have extent N"""
    from mindrec_amd import _lib
    l = _lib.lib()
    assert l.mrec_version() >= 106
    bad = [dict(form=-1), dict(form=3), dict(K=0), dict(K=-4), dict(N=0), dict(N=-1), dict(ldb=63), dict(form=0, lda=63), dict(form=2, lda=63),
           dict(form=1, K=32, lda=63)]
    for args in bad:
        assert load_widths(l, **{**dict(form=0, a=A, lda=64, b=A, ldb=64, K=64, N=64), **args}) == (EINVAL, (-7, -7)), args       # nothing written
    assert l.mrec_dense32_load_widths(0, A, 64, A, 64, 64, 64, None, None) == EINVAL
    assert load_widths(l, 1, A, 64, A, 64, 128, 64) == (OK, (4, 4))                     # form 1: K is no operand's extent
    for form in (0, 1, 2):
        for oa in range(5):
            for ob in range(5):
                for K in (60, 61, 62, 64):
                    for N in (64, 65, 66, 68):
                        for lda in (68, 69, 70, 72):
                            for ldb in (68, 69, 70):
                                ea = N if form == 1 else K
                                want = T.vec_of(4 * oa % 16, lda, ea), T.vec_of(4 * ob % 16, ldb, N)
                                assert load_widths(l, form, A + 4 * oa, lda, A + 4 * ob, ldb, K, N) == (OK, want), (form, oa, ob, K, N, lda, ldb)
    # the table's rows, their buffers' bases 16-byte aligned
    for form, shape, la, lb, want in T.width_cases():
        M, K, N = T.mkn(form, *shape)
        (ra, ea), (rb, eb) = T.operand_shapes(form, *shape)
        addr = lambda ext, off, pad: A + 4 * (T.FRONT * (off + ext + pad) + off)
        assert load_widths(l, form, addr(ea, *la), T.ld_of(ra, ea, *la), addr(eb, *lb), T.ld_of(rb, eb, *lb), K, N) == (OK, want), (form, shape, la, lb)


def test_width_table_reaches_all_nine_pairs_per_form():
    """with the buffers' bases 16-byte aligned (the device test asks again with the real pointers)"""
    table = T.width_cases()
    assert len(table) == 27
    for form in (0, 1, 2):
        assert {v for f, *_, v in table if f == form} == {(a, b) for a in (4, 2, 1) for b in (4, 2, 1)}
        assert T.GENERAL_WIDTHS[form][0] != T.GENERAL_WIDTHS[form][1]
    ways = {4: set(), 2: set(), 1: set()}
    for form, shape, la, lb, (va, vb) in table:
        assert T.case_widths(form, shape, la, lb) == (va, vb), (form, shape, la, lb)
        assert max(T.mkn(form, *shape)) <= 258 and la[1] >= 1 and lb[1] >= 1            # poisoned columns right of every window
        for (rows, ext), (off, pad), v in zip(T.operand_shapes(form, *shape), (la, lb), (va, vb)):
            ways[v].add((ext % 4, off, (off + ext + pad) % 4))
    # a strided operand loaded 2 and 4 wide, and each way of losing a width: the extent, the pointer, the stride
    assert ways[4] == {(0, 0, 0)} and ways[2] >= {(2, 0, 0), (0, 2, 0), (0, 0, 2)} and ways[1] >= {(1, 0, 0), (0, 1, 0), (0, 0, 1)}
    # the sweeps' windows
    for form in (0, 1, 2):
        for c in T.sweep_cases():
            assert T.case_widths(form, c, *T.SWEEP_LAYOUT) in {(a, b) for a in (4, 2, 1) for b in (4, 2, 1)}
    # the restatement itself
    assert [T.vec_of(*a) for a in [(0, 8, 8), (8, 8, 8), (0, 6, 8), (0, 8, 6), (4, 8, 8), (0, 7, 8), (0, 8, 7), (8, 6, 6)]] == [4, 2, 2, 2, 1, 1, 1, 2]


def _exact_cases():
    out = [(f, *T.SIMPLEST) for f in (0, 1, 2)] + [(f, *T.BASE) for f in (0, 1, 2)]
    out += [(f, *c) for f in (0, 1, 2) for c in T.sweep_cases()]
    out += [(f, *shape) for f, shape, *_ in T.width_cases()]
    out += [(1, M, 66, 130) for M in T.COLSUM_M]
    out += [(2, K, M, N) for M in T.SLAB_M for K, N in T.SLAB_KN]
    return sorted(set(out))


def test_exact_family_stays_below_2_to_24():
    worst = 0.0
    for form, p, red, q in _exact_cases():
        d = T.exact_inputs(form, p, red, q)
        for name, a in d.items():
            assert a.dtype == np.float32 and np.abs(a).max() <= 8, (form, p, red, q, name)
            if name != "h":                                                     # (h only gates: the sign of each element matters)
                assert np.array_equal(a, np.rint(a)) and (a != 0).all(), (form, p, red, q, name)      # a dropped term always changes a sum
        worst = max(worst, T.exact_margin(form, d))
    assert worst < 1.0
    h = T.exact_inputs(1, *T.BASE)["h"]
    assert (h < 0).any() and (h > 0).any() and ((h == 0) & np.signbit(h)).any() and ((h == 0) & ~np.signbit(h)).any()


def test_general_forward_cases_stay_clear_of_the_relu_corner():
    """the share of outputs within the bound of the ReLU's corner, where either side is right, from the float64 reference alone"""
    cases = T.general_forward_cases()
    assert T.BASE in cases and len(cases) >= 2
    for p, red, q in cases:
        pre, tol, near0 = T.forward_reference(T.general_inputs(0, p, red, q))
        assert near0.mean() <= T.NEAR0_CAP, (p, red, q, float(near0.mean()))


def test_colsum_restatement_orders_rows_as_the_epilogue():
    """on integers (any order is exact) it is the plain block sum; on rows of 2^24 and ones it is not, in the way the order says"""
    rng = np.random.default_rng(3)
    for M in T.COLSUM_M:
        dx = rng.integers(-50, 50, (M, 5)).astype(np.float32)
        want = np.stack([dx[r:r + 64].astype(np.float64).sum(0) for r in range(0, M, 64)])
        assert np.array_equal(T.colsum_restated(dx), want)
    dx = np.ones((64, 1), np.float32)
    dx[0] = 2.0 ** 24               # row 0 is the first of S(0, 0): its 15 ones are absorbed one at a time; the other three sums hold 16
    assert T.colsum_restated(dx)[0, 0] == 2.0 ** 24 + 48
    dx[0], dx[36] = 1.0, 2.0 ** 24  # row 36 = 32 + 4: the first of S(1, 1)
    assert T.colsum_restated(dx)[0, 0] == 2.0 ** 24 + 48
    dx[36], dx[63] = 1.0, 2.0 ** 24  # row 63 = 32 + 3 + 24 + 4: the last of S(1, 1), added to 15
    assert T.colsum_restated(dx)[0, 0] == 2.0 ** 24 + 64            # 2^24 + 15 rounds to even
