"""The step's plan at its structural seams, in both forms -- mrec_sparse_plan_* (fused) and mrec_dedup_* + mrec_group_by_inverse
(two calls) -- against the host restatement of tests/_plan_cases.py; every output is an integer and compared exactly.
  * every (passes, digit bits) layout of radix_plan: one pass of 1..11 bits, two of 6..11, three of 8 (n = 2^22 + 1) -- the
    ping-pong of plan_impl and of group_impl at every pass count, 11-bit digits (the full cnt[w][RNB] tables) on many tiles;
  * the duplicate count, known on the device only, on either side of kSmallDups = 1024 and of a 2048 tile edge of the duplicate
    list, with one to three live radix tiles among up to 35 whose hist rows an earlier call left behind;
  * padding counted with the duplicates (MREC_PLAN_SKIP_NEGATIVE) at the same limits;
  * one primed workspace taken through the radix path, the small path, no duplicates and padding in turn.
tests/test_plan_cases.py holds the inputs to the counts claimed here; n at the 2048 tile edges and the look-back scan past 64 tiles
are tests/test_map_plan_dispatch_gpu.py's."""
import numpy as np
import pytest
import torch

import _plan_cases as P
from _plan_cases import T, check_plan, plan_ref

pytestmark = pytest.mark.gpu

DTYPES = [np.int32, np.int64]


def sfx_of(dtype):
    return "i32" if dtype == np.int32 else "i64"


def primed(ops, n, dtype):
    return [k for k in ops._PLAN_PRIMED if k[1:] == (n, sfx_of(dtype))]


def unprime(ops, n, dtype):
    for k in primed(ops, n, dtype):
        del ops._PLAN_PRIMED[k]


def same_plan(p, n, ref, U=None, n_valid=None):
    """the buffers of plan p against ref = plan_ref(...); U / n_valid: as read by the caller (default: p.U, p.n_valid_dev)"""
    uniq, inv, spos, sseg, offs, nv = ref
    assert (p.U if U is None else U) == uniq.size
    U = uniq.size
    assert np.array_equal(p.uniq_buf[:U].cpu().numpy(), uniq)
    assert np.array_equal(p.inv.cpu().numpy(), inv)
    assert np.array_equal(p.sorted_pos[:n].cpu().numpy(), spos)
    assert np.array_equal(p.sorted_seg[:n].cpu().numpy(), sseg)
    assert np.array_equal(p.seg_offsets[:offs.size].cpu().numpy(), offs)
    if p.n_valid_dev is not None:
        assert (int(p.n_valid_dev.item()) if n_valid is None else n_valid) == nv
        if nv < n:
            assert int(p.uniq_buf[U].item()) == -1 and offs.size == U + 2 and int(p.seg_offsets[U + 1].item()) == n


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_by_inverse_every_pass_layout(dev, dtype):
    """ascending, then descending: the shared "dedup" and "group" workspaces are reused by a larger and by a smaller n, so a pass
    finds hist rows, tk / tv and look-back words of another size in them"""
    from mindrec_amd import ops
    cases = {n: P.sweep_case_ids(n, dtype) for n in P.PASS_SWEEP}
    refs = {n: plan_ref(ids) for n, ids in cases.items()}
    for n in P.PASS_SWEEP + P.PASS_SWEEP[::-1]:
        p = ops.group_by_inverse(ops.unique(T(cases[n], dev)))
        torch.cuda.synchronize()
        same_plan(p, n, refs[n])


@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_every_pass_layout(dev, dtype):
    """the fused form over the same sweep.  From n = 2048 on more inputs make its radix passes run at that bit layout whatever the
    first one's duplicate count: half the positions (three quarters below 4096) duplicates of 7 keys, and at n = 2^k -- where the
    padding's key n - 1 has every bit of the layout set -- the first input's non-negative twin with half its positions padding."""
    from mindrec_amd import ops
    for n in P.PASS_SWEEP:
        inputs = [(P.sweep_case_ids(n, dtype), False)]
        if n >= 2048:
            nD = n // 2 if n >= 4096 else 3 * n // 4
            inputs.append((P.ids_with_dups(n, nD, "few_groups", dtype, P.case_rng(6, n, nD)), False))
            if n & (n - 1) == 0:
                inputs.append((P.with_padding(P.sweep_case_ids(n, dtype, nonneg=True), n // 2, P.case_rng(7, n))[0], True))
            assert all(P.n_dups(ids, skip) > P.SMALL_DUPS for ids, skip in inputs[1:])
        for ids, skip in inputs:
            ref = plan_ref(ids, skip)
            same_plan(check_plan(ops, dev, ids, skip, ref), n, ref)
            assert len(primed(ops, n, dtype)) == 1
            same_plan(check_plan(ops, dev, ids, skip, ref), n, ref)              # primed


@pytest.mark.parametrize("n", P.BIG)
def test_big_n(dev, n):
    """two passes of 11 bits on 1025 tiles; the last two-pass n; three passes of 8 bits.  Both forms, int32; at 2^22 + 1 the fused
    form over int64 keys too (the same ids: the same plan).
    Measured on an MI355X, host reference (np.unique and two stable argsorts of ~4 M ids) included: 0.39 s, 0.90 s, 0.95 s."""
    from mindrec_amd import ops
    ids = P.big_case_ids(n)
    ref = plan_ref(ids)
    assert ref[0].size > 1 << 21 if n > 1 << 22 else ref[0].size > 1 << 20
    t = T(ids, dev)
    p = ops.sparse_plan(t)
    torch.cuda.synchronize()
    same_plan(p, n, ref)
    del p
    p = ops.group_by_inverse(ops.unique(t))
    torch.cuda.synchronize()
    same_plan(p, n, ref)
    del p
    if n == P.BIG[-1]:
        p = ops.sparse_plan(t.to(torch.int64))
        torch.cuda.synchronize()
        same_plan(p, n, ref)


_DIRTY = {}


def dirty_workspace(ops, dev, n, dtype):
    """a plan over n ids of which half are duplicates: it leaves a hist row in every radix tile of the first half, and tk / tv /
    dup_pos full of its own entries, in the workspace the next plan of this (n, dtype) gets"""
    key = (n, sfx_of(dtype))
    if key not in _DIRTY:
        ids = P.ids_with_dups(n, n // 2, "few_groups", dtype, P.case_rng(8, n), skip_negative=True)
        pad = P.with_padding(ids, 7, P.case_rng(9, n))[0]
        _DIRTY[key] = (ids, plan_ref(ids), pad, plan_ref(pad, True))
    ids, ref, pad, pref = _DIRTY[key]
    check_plan(ops, dev, ids, False, ref)
    check_plan(ops, dev, pad, True, pref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", P.DUP_SEAMS, ids=P.case_id)
def test_duplicate_count_seams(dev, dtype, c):
    from mindrec_amd import ops
    ids = P.dup_case_ids(c, dtype)
    assert P.side_of(P.n_dups(ids)) == (c.path, c.live_tiles)
    ref = plan_ref(ids)
    dirty_workspace(ops, dev, c.n, dtype)
    unprime(ops, c.n, dtype)
    same_plan(check_plan(ops, dev, ids, False, ref), c.n, ref)                   # unprimed, over what the plans before left
    assert len(primed(ops, c.n, dtype)) == 1
    dirty_workspace(ops, dev, c.n, dtype)
    same_plan(check_plan(ops, dev, ids, False, ref), c.n, ref)                   # primed


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", P.PAD_SEAMS, ids=P.case_id)
def test_padding_counts_toward_the_small_path_limit(dev, dtype, c):
    from mindrec_amd import ops
    ids = P.pad_case_ids(c, dtype)
    assert P.side_of(P.n_dups(ids, True)) == (c.path, c.live_tiles) and int((ids < 0).sum()) == c.k
    ref = plan_ref(ids, True)
    dirty_workspace(ops, dev, c.n, dtype)
    unprime(ops, c.n, dtype)
    for _ in range(2):                                                           # unprimed, then primed
        p = check_plan(ops, dev, ids, True, ref)
        same_plan(p, c.n, ref)
        U = ref[0].size
        assert int(p.n_valid_dev.item()) == c.n - c.k == ref[5]
        if c.k:
            assert int(p.uniq_buf[U].item()) == -1 and int(p.seg_offsets[U + 1].item()) == c.n
        assert int(p.seg_offsets[U].item()) == c.n - c.k
    assert len(primed(ops, c.n, dtype)) == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_primed_workspace_across_changing_paths(dev, dtype):
    """each step finds what the one before left: tk / tv of a longer duplicate list, hist rows of tiles now dead, dup_pos entries
    past its own count"""
    from mindrec_amd import ops
    steps = P.path_inputs(dtype)
    unprime(ops, P.PATH_N, dtype)
    for what, (ids, skip) in zip(P.PATH_STEPS, steps):
        ref = plan_ref(ids, skip)
        same_plan(check_plan(ops, dev, ids, skip, ref), P.PATH_N, ref)
        assert len(primed(ops, P.PATH_N, dtype)) == 1, what
    ids, skip = steps[1]
    check_plan(ops, dev, ids, skip)                                              # and the small path behind the radix path once more
