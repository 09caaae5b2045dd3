"""ops.multitable_optim_ / mrec_mt_optim (csrc/mrec_mt_optim.hip) on the GPU: bit for bit (torch.equal) the composition it replaces, on
clones -- per table ops.dense_adam_rows_l2_ for p, m, v and, for its wide vector, ops.scatter_unique_rows_ into a zero [V] gradient,
ops.dense_ftrl_ and a clearing scatter; ops.dense_ftrl_ for the plain vectors.  Everything starts from non-zero m, v, accum and linear,
so rows without a gradient move too.  The rows of sums / wsums past a plan's device count hold NaN: reading one poisons a table.

The reference's [V] gradient buffer is a slice of V + 1 words: ops.scatter_rows_ takes no V, so the hand-made plan's row V -- which both
sides must ignore in the tables -- lands in the spare word there instead of outside the buffer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ADAM = dict(lr=0.003, beta1=0.9, beta2=0.999, eps=1e-6, beta1_power=float(np.float32(0.9) ** 3), beta2_power=float(np.float32(0.999) ** 3),
            grad_scale=0.5)
FTRL = dict(lr=0.1, l1=5e-4, l2=5e-4, lr_power=-0.5, grad_scale=2.0)
L2 = 0.25


def _rand(rng, *shape, s=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * s).astype(np.float32)).cuda()


def _real_plan(rng, V, n, every_row=False):
    from mindrec_amd import ops
    ids = rng.integers(0, V, (n,)).astype(np.int32)
    if every_row:
        ids[:V] = rng.permutation(V).astype(np.int32)
    return ops.sparse_plan(torch.from_numpy(ids).cuda().view(-1, 1) if n else torch.empty((0, 2), dtype=torch.int32, device="cuda"))


def _hand_plan(uniq, n_dev):
    from mindrec_amd import ops
    return ops.Dedup(torch.empty(0, dtype=torch.int32, device="cuda"), torch.tensor(uniq, dtype=torch.int32, device="cuda"), None,
                     torch.tensor([n_dev], dtype=torch.int64, device="cuda"))


def _table(rng, V, D, plan, U, wide=True):
    """a table record's tensors: [p, m, v, plan, sums, w, accum, linear, wsums]; rows of sums / wsums at index >= U are NaN"""
    n = plan.uniq_buf.numel()
    sums, wsums = _rand(rng, n, D), _rand(rng, n)
    sums[U:], wsums[U:] = float("nan"), float("nan")
    rec = [_rand(rng, V, D, s=0.5), _rand(rng, V, D, s=0.01), _rand(rng, V, D, s=0.01).abs(), plan, sums]
    return rec + ([_rand(rng, V, s=0.3), _rand(rng, V, s=0.2).abs() + 0.1, _rand(rng, V, s=0.05), wsums] if wide else [None] * 4)


def _vector(rng, n):
    return [_rand(rng, n, s=0.1), _rand(rng, n, s=0.2).abs() + 0.1, _rand(rng, n, s=0.05), _rand(rng, n)]


def _clone(rec):
    return [t.clone() if isinstance(t, torch.Tensor) else t for t in rec]


def _composition(tables, vectors, adam, ftrl, l2):
    """the launches the fused chain replaces, on the given tensors"""
    from mindrec_amd import ops
    for p, m, v, plan, sums, w, acc, lin, wsums in tables:
        ops.dense_adam_rows_l2_(p, m, v, plan, sums, l2, **adam)
        if w is None:
            continue
        V, n = w.numel(), plan.uniq_buf.numel()
        gb = torch.zeros(V + 1, dtype=torch.float32, device="cuda")[:V]
        ops.scatter_unique_rows_(gb.view(-1, 1), plan, wsums.view(-1, 1))
        ops.dense_ftrl_(w, acc, lin, gb, **ftrl)
        ops.scatter_unique_rows_(gb.view(-1, 1), plan, torch.zeros((n, 1), dtype=torch.float32, device="cuda"))
        assert not gb.any()
    for w, acc, lin, g in vectors:
        ops.dense_ftrl_(w, acc, lin, g, **ftrl)


def _fused(tables, vectors, adam, ftrl, l2, step_state=None):
    from mindrec_amd import ops
    ops.multitable_optim_([ops.MtOptTable(*t) for t in tables], [ops.MtOptVector(*q) for q in vectors], adam=dict(adam, l2_scaled=l2),
                          ftrl=ftrl, step_state=step_state)


def _same(got, want, what):
    """every tensor the optimizers write -- a table's p, m, v, w, accum, linear; a vector's w, accum, linear -- equal bit for bit, and finite:
    nothing past a plan's count was read"""
    for i, (a, b) in enumerate(zip(got, want)):
        for j in (0, 1, 2, 5, 6, 7) if len(a) == 9 else (0, 1, 2):
            if a[j] is not None:
                assert torch.equal(a[j], b[j]) and torch.isfinite(a[j]).all(), (what, i, j)


def _maximum(rng):
    """8 tables + 4 plain vectors: every case of the table in the module docstring's terms"""
    tabs = []
    pl = _real_plan(rng, 1, 3)
    tabs.append(_table(rng, 1, 64, pl, pl.U))                                            # V = 1: the smallest table
    pl = _real_plan(rng, 16, 40, every_row=True)
    assert pl.U == 16
    tabs.append(_table(rng, 16, 64, pl, 16))                                             # every row touched: U = V
    pl = _real_plan(rng, 40, 0)
    assert pl.U == 0
    tabs.append(_table(rng, 40, 128, pl, 0))                                             # a plan over an empty id tensor: U = 0
    pl = _real_plan(rng, 33, 20)
    tabs.append(_table(rng, 33, 6, pl, pl.U))                                            # D = 6: the scalar path; 198 elements
    pl = _real_plan(rng, 64, 30)
    tabs.append(_table(rng, 64, 64, pl, pl.U, wide=False))                               # 4096 elements = 4 x (256 x 4): ends on a workgroup; no wide vector
    pl = _hand_plan([3, -1, 7, 50, 0, 49, 5, 5], 6)                                      # rows -1 and V = 50; entries 6, 7 lie past the device count
    tabs.append(_table(rng, 50, 128, pl, 6))
    pl = _real_plan(rng, 300, 500)
    tabs.append(_table(rng, 300, 64, pl, pl.U))                                          # 19 workgroups of float4s, 2 of wide entries
    pl = _real_plan(rng, 7, 4)
    tabs.append(_table(rng, 7, 6, pl, pl.U))
    return tabs, [_vector(rng, n) for n in (32, 1, 300, 5)]


def test_maximum_8_tables_4_vectors_against_the_composition():
    tabs, vecs = _maximum(np.random.default_rng(7))
    want_t, want_v = [_clone(t) for t in tabs], [_clone(q) for q in vecs]
    _composition(want_t, want_v, ADAM, FTRL, L2)
    got_t, got_v = [_clone(t) for t in tabs], [_clone(q) for q in vecs]
    _fused(got_t, got_v, ADAM, FTRL, L2)
    _same(got_t, want_t, "tables")
    _same(got_v, want_v, "vectors")
    # every row moved: those without a gradient on their momentum / from linear and accum
    for t0, t1 in zip(tabs, got_t):
        assert (t0[0] != t1[0]).any(1).all()
        assert t0[5] is None or (t0[5] != t1[5]).any()
    # a second run from the same start: identical bits
    again_t, again_v = [_clone(t) for t in tabs], [_clone(q) for q in vecs]
    _fused(again_t, again_v, ADAM, FTRL, L2)
    _same(again_t, got_t, "second run")
    _same(again_v, got_v, "second run, vectors")


@pytest.mark.parametrize("D", [128, 64, 6])
def test_minimum_1_table_0_vectors(D):
    rng = np.random.default_rng(D)
    pl = _real_plan(rng, 40, 25)
    tab = _table(rng, 40, D, pl, pl.U)
    want, got = _clone(tab), _clone(tab)
    _composition([want], [], ADAM, FTRL, 0.0)
    _fused([got], [], ADAM, FTRL, 0.0)
    _same([got], [want], f"D = {D}")


def test_vectors_alone_and_nothing_at_all():
    rng = np.random.default_rng(3)
    vecs = [_vector(rng, 32), _vector(rng, 1)]
    want, got = [_clone(q) for q in vecs], [_clone(q) for q in vecs]
    _composition([], want, ADAM, FTRL, 0.0)
    _fused([], got, ADAM, FTRL, 0.0)
    _same(got, want, "vectors alone")
    _fused([], [], ADAM, FTRL, 0.0)


def test_step_state_gives_the_step_size_of_the_host_powers():
    from mindrec_amd import ops
    rng = np.random.default_rng(11)
    b1, b2 = np.float32(0.9), np.float32(0.999)
    b1p, b2p = np.float32(b1 * b1), np.float32(b2 * b2)              # two steps done
    pl, pl2 = _real_plan(rng, 40, 25), _real_plan(rng, 33, 9)
    tabs = [_table(rng, 40, 128, pl, pl.U), _table(rng, 33, 6, pl2, pl2.U)]
    vecs = [_vector(rng, 32)]
    st = ops.StepState(torch.device("cuda"), float(b1p), float(b2p), 2)
    st.advance(ADAM["lr"], float(b1), float(b2))                      # the third step's powers, on the device
    host = dict(ADAM, beta1=float(b1), beta2=float(b2), beta1_power=float(np.float32(b1p * b1)), beta2_power=float(np.float32(b2p * b2)))
    want_t, want_v = [_clone(t) for t in tabs], [_clone(q) for q in vecs]
    _composition(want_t, want_v, host, FTRL, L2)
    got_t, got_v = [_clone(t) for t in tabs], [_clone(q) for q in vecs]
    _fused(got_t, got_v, dict(ADAM, beta1=float(b1), beta2=float(b2), beta1_power=0.0, beta2_power=0.0), FTRL, L2, step_state=st)
    _same(got_t, want_t, "step_state")
    _same(got_v, want_v, "step_state, vectors")
    # and the composition's own step_state form agrees (the same device word)
    alt = _clone(tabs[0])
    ops.dense_adam_rows_l2_(*alt[:5], L2, **dict(ADAM, beta1=float(b1), beta2=float(b2), beta1_power=0.0, beta2_power=0.0), step_state=st)
    assert torch.equal(alt[0], got_t[0][0])


def test_dense_adam_step_state():
    """ops.dense_adam_(step_state=...) -- the fp32 net's optimizer in a captured step -- against host powers of the same step, at a
    size with a float4 body and a scalar tail"""
    from mindrec_amd import ops
    rng = np.random.default_rng(13)
    n = 4 * 300 + 3
    p, m, v, g = _rand(rng, n), _rand(rng, n, s=0.01), _rand(rng, n, s=0.01).abs(), _rand(rng, n)
    b1, b2 = np.float32(0.9), np.float32(0.999)
    st = ops.StepState(torch.device("cuda"), 1.0, 1.0, 0)
    st.advance(0.003, float(b1), float(b2))
    want, got = [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)]
    kw = dict(lr=0.003, beta1=float(b1), beta2=float(b2), eps=1e-6, grad_scale=0.001)
    ops.dense_adam_(*want, g, beta1_power=float(b1), beta2_power=float(b2), **kw)
    ops.dense_adam_(*got, g, beta1_power=0.0, beta2_power=0.0, step_state=st, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
