"""The deep and the wide side of multi-hot fields from one plan, on the GPU: MultiHotEmbedding.apply_(plan=) against apply_ building
its own plan; MultiHotWideDeep against the two MultiHotEmbedding objects it replaces, eager and captured; its single-hot case against
ops.gather_rows and the host restatement of the slot sum (tests/_pool_ref.py).  Every comparison is on raw bits, over all rows."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pool_ref as P  # noqa: E402

V = 1500


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().float().cpu().numpy().view(np.uint32)


def _same(got, ref, what):
    got = got.view(np.uint32) if got.dtype != np.uint32 else got
    ref = np.ascontiguousarray(ref, np.float32).view(np.uint32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = (got != ref).reshape(got.shape[0], -1).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, e.g. rows {np.nonzero(bad)[0][:6].tolist()}"


def _ids(rng, B, Ls, V, idt):
    """ids mostly in the table, some a little outside [0, V) on both sides"""
    ids = rng.integers(0, V, size=(B, Ls))
    out = rng.random((B, Ls)) < 0.05
    ids[out] = rng.choice(np.array([-7, -2, -1, V, V + 1, V + 5]), size=int(out.sum()))
    return ids.astype(idt)


# ---- single-hot ------------------------------------------------------------------------------------------------------------------
def test_pair_single_hot_is_gather_rows_flattened_and_the_slot_sum(dev):
    """bag = (1,) * 5 without a mask: Gather + Flatten on the deep side, the five-slot sum on the wide side, one of them written into
    column 2 of a [B, 5] matrix whose other columns keep their bits; a sample whose every id is out of range: +0.0, sign bit included"""
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotWideDeep
    rng = np.random.default_rng(5)
    n, D, Bs = 5, 128, 257
    ids = _ids(rng, Bs, n, V, np.int64)
    ids[7] = V + 1
    pair = MultiHotWideDeep(V, D, (1,) * n, mode="mean", device=dev, seed=3, wide_seed=4)
    pair.wide.table.copy_(-pair.wide.table.abs() - 1.0)             # all weights negative: a +0.0 is the out-of-range rule's
    tid = T(ids, dev)
    m0 = rng.standard_normal((Bs, 5)).astype(np.float32)
    tm5 = T(m0, dev)
    x, w = pair.lookup(tid, wide_out=tm5[:, 2])
    assert w.data_ptr() == tm5[:, 2].data_ptr() and tuple(x.shape) == (Bs, n * D)
    rows = ops.gather_rows(pair.deep.table, tid.reshape(-1)).reshape(Bs, n * D)
    assert np.array_equal(_bits(x), _bits(rows))
    m0[:, 2:3] = P.gather_pool(pair.wide.table.cpu().numpy(), ids, None, "sum")
    _same(_bits(tm5), m0, "the five-slot sum in column 2 of 5")
    assert _bits(w)[7] == 0 and (_bits(x)[7] == 0).all()
    x1, w1 = pair.lookup(tid[5:6])                                   # B = 1
    assert np.array_equal(_bits(x1)[0], _bits(x)[5]) and _bits(w1)[0] == _bits(w)[5]


# ---- 4. apply_(plan=) ----------------------------------------------------------------------------------------------------------------
LENS, D64, V300, B200, STEPS = (3, 5, 4, 3, 4, 2), 64, 300, 200, 3


def _steps(rng, idt, dev):
    """ids that repeat across fields and steps (a small Zipf-like range), a 0/1 mask, dy and dwide per step"""
    shape = (B200, sum(LENS))
    out = []
    for _ in range(STEPS):
        ids = np.minimum(rng.zipf(1.3, size=shape) - 1 + rng.integers(0, 30, size=shape), V300 + 1).astype(idt)
        mask = (rng.random(shape) < 0.7).astype(np.float32)
        dy = (rng.standard_normal((B200, len(LENS) * D64)) * 0.01).astype(np.float32)
        dw = (rng.standard_normal(B200) * 0.01).astype(np.float32)
        out.append(tuple(T(a, dev) for a in (ids, mask, dy, dw)))
    return out


def _equal_state(a, b, what):
    for name, x, y in zip(("table", "state 1", "state 2"), (a.table,) + tuple(a.state), (b.table,) + tuple(b.state)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: {name} differs"


@pytest.mark.parametrize("opt", ["lazy_adam", "ftrl", "adam"])
def test_apply_with_a_plan_built_outside_is_apply(dev, opt):
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotEmbedding
    steps = _steps(np.random.default_rng(len(opt)), np.int32, dev)
    a = MultiHotEmbedding(V300, D64, LENS, mode="mean", optimizer=opt, device=dev, seed=21)
    b = MultiHotEmbedding(V300, D64, LENS, mode="mean", optimizer=opt, device=dev, seed=21)
    start = a.table.clone()
    for t, (ids, mask, dy, _) in enumerate(steps):
        xa, xb = a.lookup(ids, mask), b.lookup(ids, mask)
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))
        a.apply_(dy)
        plan = ops.sparse_plan(ids)
        assert b.apply_(dy, plan=plan) is plan
        _equal_state(a, b, f"{opt} step {t}")
    assert a.step_count == b.step_count == STEPS and a.beta1_power == b.beta1_power and a.beta2_power == b.beta2_power
    assert not torch.equal(a.table, start)
    with pytest.raises(ValueError):
        b.apply_(steps[0][2], plan=ops.sparse_plan(steps[0][0][:, :5].contiguous()))      # a plan of another number of ids


# ---- 5. the pair against the two objects it replaces ---------------------------------------------------------------------------------
def _pair_and_halves(dev, opt):
    from mindrec_amd.multi_hot import MultiHotEmbedding, MultiHotWideDeep
    kw = dict(lr=1e-3, beta1=0.8, eps=1e-7)
    wkw = dict(lr=0.1, l1=1e-6, l2=1e-5, initial_accum=0.5)
    pair = MultiHotWideDeep(V300, D64, LENS, mode="mean", optimizer=opt, wide_optimizer="ftrl", device=dev, seed=31, wide_seed=32,
                            wide_lr=0.1, l1=1e-6, l2=1e-5, initial_accum=0.5, **kw)
    deep = MultiHotEmbedding(V300, D64, LENS, mode="mean", optimizer=opt, device=dev, seed=31, l1=1e-6, l2=1e-5, initial_accum=0.5, **kw)
    wide = MultiHotEmbedding(V300, 1, sum(LENS), mode="sum", optimizer="ftrl", device=dev, seed=32, beta1=0.8, eps=1e-7, **wkw)
    return pair, deep, wide


@pytest.mark.parametrize("opt,idt", [("lazy_adam", np.int64), ("adam", np.int32)])
def test_pair_is_the_two_embeddings_it_replaces(dev, opt, idt):
    pair, deep, wide = _pair_and_halves(dev, opt)
    assert pair.deep.fields == LENS and pair.wide.fields == (sum(LENS),) and pair.wide.dim == 1 and pair.wide.mode == "sum"
    assert pair.deep.optimizer == opt and pair.wide.optimizer == "ftrl"
    _equal_state(pair.deep, deep, "start, deep")
    _equal_state(pair.wide, wide, "start, wide")
    start_d, start_w = deep.table.clone(), wide.table.clone()
    for t, (ids, mask, dy, dw) in enumerate(_steps(np.random.default_rng(7), idt, dev)):
        x, w = pair.lookup(ids, mask)
        xd, ww = deep.lookup(ids, mask), wide.lookup(ids, mask)
        assert tuple(x.shape) == (B200, len(LENS) * D64) and tuple(w.shape) == (B200,) and tuple(ww.shape) == (B200, 1)
        assert torch.equal(x.view(torch.int32), xd.view(torch.int32)), f"step {t}: x"
        assert torch.equal(w.view(torch.int32), ww.view(torch.int32).view(-1)), f"step {t}: w"
        pair.apply_(dy, dw, grad_scale=0.5)
        deep.apply_(dy, grad_scale=0.5)
        wide.apply_(dw.view(B200, 1), grad_scale=0.5)
        _equal_state(pair.deep, deep, f"step {t}, deep")
        _equal_state(pair.wide, wide, f"step {t}, wide")
    assert pair.deep.step_count == pair.wide.step_count == STEPS
    assert pair.deep.beta1_power == deep.beta1_power and pair.wide.beta2_power == wide.beta2_power
    assert not torch.equal(deep.table, start_d) and not torch.equal(wide.table, start_w)


def test_pair_apply_refuses_a_bad_dwide_before_either_half_steps(dev):
    pair = _pair_and_halves(dev, "lazy_adam")[0]
    ids, mask, dy, dw = _steps(np.random.default_rng(3), np.int32, dev)[0]
    pair.lookup(ids, mask)
    before = [t.clone() for t in (pair.deep.table,) + tuple(pair.deep.state) + (pair.wide.table,) + tuple(pair.wide.state)]
    for bad in (dw.double(), dw.cpu(), dw[:-1], torch.stack([dw, dw], 1)[:, 0]):
        with pytest.raises(TypeError):
            pair.apply_(dy, bad)
    torch.cuda.synchronize()
    after = (pair.deep.table,) + tuple(pair.deep.state) + (pair.wide.table,) + tuple(pair.wide.state)
    assert all(torch.equal(x, y) for x, y in zip(before, after)) and pair.deep.step_count == pair.wide.step_count == 0
    assert pair.deep.beta1_power == np.float32(1.0)


# ---- 6. captured ---------------------------------------------------------------------------------------------------------------------
def test_pair_captured_equals_eager(dev):
    """three steps of lookup -> apply_ of the pair captured into ONE HIP graph on one stream and replayed once: the eager pair's bits"""
    steps = _steps(np.random.default_rng(9), np.int32, dev)

    def run(pair, x, w):
        for ids, mask, dy, dw in steps:
            pair.lookup(ids, mask, out=x, wide_out=w)
            pair.apply_(dy, dw)

    def bufs():
        return torch.zeros((B200, len(LENS) * D64), dtype=torch.float32, device=dev), torch.zeros(B200, dtype=torch.float32, device=dev)

    eager = _pair_and_halves(dev, "lazy_adam")[0]
    xe, we = bufs()
    run(eager, xe, we)
    torch.cuda.synchronize()
    cap = _pair_and_halves(dev, "lazy_adam")[0]
    start = cap.deep.table.clone()
    xc, wc = bufs()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(cap, xc, wc)
    torch.cuda.synchronize()
    assert torch.equal(cap.deep.table, start) and not wc.any()          # (capture ran nothing)
    graph.replay()
    torch.cuda.synchronize()
    _equal_state(eager.deep, cap.deep, "captured, deep")
    _equal_state(eager.wide, cap.wide, "captured, wide")
    assert torch.equal(xe.view(torch.int32), xc.view(torch.int32)) and torch.equal(we.view(torch.int32), wc.view(torch.int32))
    assert not torch.equal(cap.deep.table, start) and wc.any()
