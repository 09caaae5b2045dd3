"""Every (key width, gradient type) pair the sparse-apply entries dispatch on, through the public ops wrappers against the CPU oracle: the
six LazyAdam pairs, FTRL's two key widths, the segment sum's three gradient types.  One small case each -- 9 positions with duplicates
over a 16-row table of width 8, the last run crossing the first window of 8 -- held to what tests/test_gpu_parity.py holds the same
updater to: rows summed in the oracle's order bit for bit, the run that crosses a window within the updater's bound there."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_parity import RTOL, T, check_rows, crossing  # noqa: E402

V, D = 16, 8
IDS = [3, 7, 3, 0, 15, 3, 7, 15, 3]           # first occurrences 3, 7, 0, 15: runs of 4, 2, 1 and 2 entries, the last over positions 7-8
KEYS = [np.int32, np.int64]
GRADS = [torch.float32, torch.bfloat16, torch.float16]


def _inputs(dev, kdt, gdt):
    rng = np.random.default_rng(7)
    ids = np.array(IDS, kdt)
    g = torch.from_numpy((rng.standard_normal((len(IDS), D)) * 1024).astype(np.float32)).to(gdt)      # (a 16-bit g: rounded here, once)
    sc = rng.random(len(IDS)).astype(np.float32)
    state = (rng.standard_normal((V, D)) * 0.01).astype(np.float32)
    return ids, g.to(dev), g.float().numpy(), sc, state


@pytest.mark.parametrize("gdt", GRADS, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kdt", KEYS, ids=["i32", "i64"])
def test_lazy_adam_key_and_gradient_types(dev, oracle, kdt, gdt):
    from mindrec_amd import ops
    ids, tg, g, sc, p = _inputs(dev, kdt, gdt)
    m = np.zeros_like(p); v = np.zeros_like(p)
    tp, tm, tv = T(p, dev), T(m, dev), T(v, dev)
    plan = ops.sparse_plan(T(ids, dev))
    assert plan.uniq_buf.dtype == (torch.int32 if kdt == np.int32 else torch.int64) and tg.dtype == gdt
    ops.sparse_lazy_adam_(tp, tm, tv, plan, tg, T(sc, dev), grad_scale=1.0 / 1024)
    oracle.sparse_lazy_adam(p, m, v, ids, g, sc, grad_scale=1.0 / 1024)
    cross = plan.uniq.cpu().numpy()[crossing(plan, D)].astype(np.int64)
    assert cross.tolist() == [15]
    check_rows((tp.cpu().numpy(), tm.cpu().numpy(), tv.cpu().numpy()), (p, m, v), rows_exact=[0], rows_close=cross, tol=RTOL)
    assert (v[[0, 3, 7, 15]] > 0).all() and not v[[1, 2, 14]].any()            # (the four ids' rows moved, and only they)


@pytest.mark.parametrize("kdt", KEYS, ids=["i32", "i64"])
def test_ftrl_key_types(dev, oracle, kdt):
    from mindrec_amd import ops
    ids, tg, g, sc, var = _inputs(dev, kdt, torch.float32)
    acc = np.ones_like(var); lin = np.zeros_like(var)
    tv, ta, tl = T(var, dev), T(acc, dev), T(lin, dev)
    plan = ops.sparse_plan(T(ids, dev))
    ops.sparse_ftrl_(tv, ta, tl, plan, tg, T(sc, dev), grad_scale=1.0 / 1024)
    oracle.sparse_ftrl(var, acc, lin, ids, g, sc, grad_scale=1.0 / 1024)
    cross = plan.uniq.cpu().numpy()[crossing(plan, D)].astype(np.int64)
    check_rows((tv.cpu().numpy(), ta.cpu().numpy(), tl.cpu().numpy()), (var, acc, lin), rows_exact=[0], rows_close=cross, tol=5e-5)
    assert (acc[[0, 3, 7, 15]] != 1).all()


@pytest.mark.parametrize("gdt", GRADS, ids=["f32", "bf16", "f16"])
def test_segment_sum_gradient_types(dev, oracle, gdt):
    from mindrec_amd import ops
    ids, tg, g, _, _ = _inputs(dev, np.int32, gdt)
    u_ref, inv_ref = oracle.unique(ids)
    ref = oracle.segment_sum(g, inv_ref, u_ref.size)
    plan = ops.sparse_plan(T(ids, dev))
    out = ops.segment_sum(plan, tg)[: plan.U].cpu().numpy()
    cr = crossing(plan, D)
    assert cr.tolist() == [False, False, False, True]
    assert np.array_equal(out[~cr].view(np.uint32), ref[~cr].view(np.uint32))     # oracle order: bit-exact
    # the run that crosses: any-order fp32 summation bound against the exact (float64) sum, |err| <= (count - 1) * eps * sum|x|
    exact = np.zeros((u_ref.size, D)); absum = np.zeros((u_ref.size, D))
    np.add.at(exact, inv_ref, g.astype(np.float64)); np.add.at(absum, inv_ref, np.abs(g).astype(np.float64))
    cnt = np.bincount(inv_ref, minlength=u_ref.size)[:, None]
    assert (np.abs(out - exact) <= np.maximum(cnt - 1, 1) * 2.0 ** -23 * absum).all()
