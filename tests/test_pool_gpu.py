"""Multi-hot fields on the GPU: the pooled lookup (ops.gather_pool, which runs mrec_gather_pool_fields with one field, and the C entry
mrec_gather_pool itself) bit for bit against its host restatement (tests/_pool_ref.py), the pooled sparse apply (mrec_apply_opts_t.pool) bit for bit against the restatement of the apply's order of additions (tests/
_apply_order.py) AND against the plain apply on the explicitly expanded gradient, the arming rules, and MultiHotEmbedding's training
loop, eager and captured.  Every comparison is on raw bits, over all rows (touched and untouched)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _apply_order as A  # noqa: E402
import _pool_ref as P  # noqa: E402
from oracle import oracle as O  # noqa: E402

DS = (1, 3, 16, 64, 80, 252)
LS = (1, 2, 7, 8, 33)
_KIND = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
_NP = {torch.int32: np.int32, torch.int64: np.int64}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    """a device tensor's values as fp32 bits (16-bit types widen exactly)"""
    return t.detach().float().cpu().numpy().view(np.uint32)


def _same(got, ref, what):
    got = got.view(np.uint32) if got.dtype != np.uint32 else got
    ref = np.ascontiguousarray(ref, np.float32).view(np.uint32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = (got != ref).reshape(got.shape[0], -1).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, e.g. rows {np.nonzero(bad)[0][:6].tolist()}"


def _bag_ids(rng, B, L, V, idt):
    """ids mostly in the table, some a little outside [0, V) on both sides"""
    ids = rng.integers(0, V, size=(B, L))
    out = rng.random((B, L)) < 0.05
    ids[out] = rng.choice(np.array([-7, -2, -1, V, V + 1, V + 5]), size=int(out.sum()))
    return ids.astype(idt)


def _masks(rng, B, L):
    """0/1 masks: all-zero bags, all-one bags, random ones"""
    m = (rng.random((B, L)) < 0.6).astype(np.float32)
    m[: B // 8] = 0.0
    m[B // 8: B // 4] = 1.0
    return m


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("D", DS)
def test_gather_pool_bitwise(dev, D, L):
    from mindrec_amd import ops
    rng = np.random.default_rng(D * 100 + L)
    V, B = 1500, 1237
    table = rng.standard_normal((V, D)).astype(np.float32)
    tt = T(table, dev)
    mask = _masks(rng, B, L)
    for idt in (torch.int32, torch.int64):
        ids = _bag_ids(rng, B, L, V, _NP[idt])
        tid, tm = T(ids, dev), T(mask, dev)
        for odt in (torch.float32, torch.bfloat16, torch.float16):
            for mode in ("sum", "mean"):
                got = ops.gather_pool(tt, tid, tm, mode=mode, out_dtype=odt)
                assert got.dtype == odt and tuple(got.shape) == (B, D)
                _same(_bits(got), P.gather_pool(table, ids, mask, mode, _KIND[odt]), f"D={D} L={L} {idt} {odt} {mode}")


@pytest.mark.parametrize("D,L", [(64, 2), (64, 7), (3, 1), (3, 9)])
def test_mrec_gather_pool_entry_bitwise(dev, D, L):
    """the C entry itself (ops.gather_pool goes through mrec_gather_pool_fields): float4 and single-column lanes, two and eight slots
    in flight, int32 and int64 ids, mean into fp32 and sum into bf16, ldo = 0 (the default row stride)"""
    from mindrec_amd import _lib, ops
    rng = np.random.default_rng(D * 10 + L)
    V, B = 700, 517
    table = rng.standard_normal((V, D)).astype(np.float32)
    tt = T(table, dev)
    mask = _masks(rng, B, L)
    tm = T(mask, dev)
    for idt, mode, odt in ((np.int32, "mean", torch.float32), (np.int64, "sum", torch.bfloat16)):
        ids = _bag_ids(rng, B, L, V, idt)
        tid = T(ids, dev)
        out = torch.empty((B, D), dtype=odt, device=dev)
        _lib.call("mrec_gather_pool", ops._ptr(tt), V, D, D, ops._ptr(tid), ids.itemsize, B, L, ops._ptr(tm), 1 if mode == "mean" else 0,
                  ops._ptr(out), ops._KIND[odt], 0, ops._stream())
        _same(_bits(out), P.gather_pool(table, ids, mask, mode, _KIND[odt]), f"mrec_gather_pool D={D} L={L} {mode} {odt}")


@pytest.mark.parametrize("D,L", [(1, 7), (3, 2), (64, 8), (80, 33), (252, 1), (260, 7), (70, 8)])
def test_gather_pool_no_mask_and_weights(dev, D, L):
    """mask=None (all ones: no product at all), and a mask of real-valued weights (the product is a product, not a select);
    D = 260 walks two column blocks of float4 lanes, D = 70 two of single columns"""
    from mindrec_amd import ops
    rng = np.random.default_rng(D + L)
    V, B = 900, 515
    table = rng.standard_normal((V, D)).astype(np.float32)
    ids = _bag_ids(rng, B, L, V, np.int32)
    w = rng.standard_normal((B, L)).astype(np.float32)
    for mode in ("sum", "mean"):
        for odt in (torch.float32, torch.float16):
            _same(_bits(ops.gather_pool(T(table, dev), T(ids, dev), None, mode=mode, out_dtype=odt)),
                  P.gather_pool(table, ids, None, mode, _KIND[odt]), f"no mask {mode} {odt}")
            _same(_bits(ops.gather_pool(T(table, dev), T(ids, dev), T(w, dev), mode=mode, out_dtype=odt)),
                  P.gather_pool(table, ids, w, mode, _KIND[odt]), f"weights {mode} {odt}")


@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,W,c0", [(64, 200, 72), (64, 203, 71), (80, 512, 0), (3, 11, 5), (1, 4, 2)])
def test_gather_pool_into_a_column_block(dev, odt, D, W, c0):
    """out = columns [c0, c0 + D) of a wider matrix (ldo = W > D; W = 203 / c0 = 71 take the float4 lanes away): the other columns
    keep their bits"""
    from mindrec_amd import ops
    rng = np.random.default_rng(D + W + c0)
    V, B, L = 700, 333, 7
    table = rng.standard_normal((V, D)).astype(np.float32)
    ids = _bag_ids(rng, B, L, V, np.int64)
    mask = _masks(rng, B, L)
    wide0 = (rng.integers(-64, 65, size=(B, W)) / 8.0).astype(np.float32)               # (values every output type holds exactly)
    wide = T(wide0, dev).to(odt)
    ret = ops.gather_pool(T(table, dev), T(ids, dev), T(mask, dev), mode="mean", out=wide[:, c0:c0 + D])
    assert ret.data_ptr() == wide[:, c0:c0 + D].data_ptr()
    ref = wide0.copy()
    ref[:, c0:c0 + D] = P.gather_pool(table, ids, mask, "mean", _KIND[odt])
    _same(_bits(wide), ref, "column block and its neighbours")


@pytest.mark.parametrize("D", [64, 80, 16])
def test_gather_pool_misaligned_table_view(dev, D):
    """a table view that starts one float into wider rows: rows are not 16-byte aligned, every lane takes one column"""
    from mindrec_amd import ops
    rng = np.random.default_rng(D)
    V, B, L = 800, 411, 8
    big = rng.standard_normal((V, D + 4)).astype(np.float32)
    tbig = T(big, dev)
    view = tbig[:, 1:1 + D]
    assert view.data_ptr() % 16 != 0 and view.stride(0) == D + 4
    ids = _bag_ids(rng, B, L, V, np.int32)
    mask = _masks(rng, B, L)
    for mode in ("sum", "mean"):
        for odt in (torch.float32, torch.bfloat16):
            _same(_bits(ops.gather_pool(view, T(ids, dev), T(mask, dev), mode=mode, out_dtype=odt)),
                  P.gather_pool(big[:, 1:1 + D], ids, mask, mode, _KIND[odt]), f"misaligned {mode} {odt}")


@pytest.mark.parametrize("D", DS)
def test_gather_pool_of_one_slot_is_the_lookup(dev, D):
    """the meaning pinned without the restatement: L = 1, mode "sum" is ops.gather_rows(table, ids, mask), bit for bit"""
    from mindrec_amd import ops
    rng = np.random.default_rng(D + 5)
    V, B = 1200, 2049
    tt = T(rng.standard_normal((V, D)).astype(np.float32), dev)
    for idt in (np.int32, np.int64):
        ids = T(_bag_ids(rng, B, 1, V, idt), dev)
        mask = T(_masks(rng, B, 1) * rng.standard_normal((B, 1)).astype(np.float32), dev)
        for m in (mask, None):
            a = ops.gather_pool(tt, ids, m, mode="sum")
            b = ops.gather_rows(tt, ids.reshape(-1), m.reshape(-1) if m is not None else None)
            assert np.array_equal(_bits(a), _bits(b))


def test_mean_divides_by_the_bag_length(dev):
    """5. a bag with ONE unmasked slot returns row / L (ReduceMean counts every slot), not the row"""
    from mindrec_amd import ops
    rng = np.random.default_rng(5)
    V, D, B, L = 300, 64, 97, 8
    table = rng.standard_normal((V, D)).astype(np.float32)
    ids = rng.integers(0, V, size=(B, L)).astype(np.int32)
    mask = np.zeros((B, L), np.float32)
    slot = rng.integers(0, L, size=B)
    mask[np.arange(B), slot] = 1.0
    got = ops.gather_pool(T(table, dev), T(ids, dev), T(mask, dev), mode="mean").cpu().numpy()
    rows = table[ids[np.arange(B), slot]]
    # (the other slots add +-0.0 products: x + 0.0 == x for every x != 0, and the table has no zeros)
    assert np.array_equal(got, (rows / np.float32(L)).astype(np.float32)) and not np.array_equal(got, rows)


# ---- 2. backward --------------------------------------------------------------------------------------------------------------------
def _regime_ids(regime, rng, L, idt):
    """(flat ids [n], V).  'unique': ids mostly unique (the in-window path); 'zipf': the reference's regime -- V = 20 900 rows under
    >= 100 000 positions drawn Zipf-like (long runs: the tree of window partials and the finishing launch); 'ragged': n a multiple
    neither of the window nor of L (the last bag is short)"""
    if regime == "zipf":
        V = 20900
        n = -(-100000 // L) * L
        ids = np.minimum(rng.zipf(1.2, size=n) - 1, V - 1)
    elif regime == "unique":
        V = 50000
        n = 600 * L
        ids = rng.permutation(V)[:n]
        dup = rng.random(n) < 0.02
        ids[dup] = ids[rng.integers(0, n, size=int(dup.sum()))]
    else:
        V = 3000
        n = 457 * L + (L // 2 if L > 1 else 0)
        while n % 8 == 0 or (L > 1 and n % L == 0):
            n += 1
        ids = np.minimum(rng.zipf(1.5, size=n) - 1 + rng.integers(0, 40, size=n), V - 1)
    ids = ids.astype(np.int64)
    ids[:: 97] = V + 2                                   # a few rows outside the table
    return ids.astype(idt), V, int(n)


def _check_regime(regime, c, n, aw):
    if regime == "zipf":
        assert n >= 100000, n
        for b in c["blocks"]:                            # long runs through pass A, the tree (pass B) and windows wholly inside a run
            assert b["pass_a"] > 20 and b["pass_b"] >= 1, c
        assert c["crossing"] > 100 and c["inside"] > 1000 and c["U"] < n // 4, c
    elif regime == "unique":
        assert c["U"] > 0.9 * n, c
    else:
        assert n % aw != 0, (n, aw)


def _g_rows(rng, rows, D, gdt, dev):
    g = rng.standard_normal((rows, D)).astype(np.float32)
    if gdt != torch.float32:
        g = O.round16(g, _KIND[gdt])
    return g, T(g, dev).to(gdt)


def _state(rng, V, D, kind):
    a = (rng.standard_normal((V, D)) * 0.01).astype(np.float32)
    if kind == "adam":
        return [a, (rng.standard_normal((V, D)) * 1e-3).astype(np.float32), (rng.random((V, D)) * 1e-5).astype(np.float32)]
    return [a, (rng.random((V, D)) + 0.5).astype(np.float32), (rng.standard_normal((V, D)) * 1e-3).astype(np.float32)]


_BWD = [("segment_sum", 64, torch.float32), ("segment_sum", 30, torch.bfloat16), ("lazy_adam", 64, torch.float32),
        ("lazy_adam", 64, torch.bfloat16), ("lazy_adam", 80, torch.float16), ("ftrl", 1, torch.float32), ("ftrl", 64, torch.float32)]


@pytest.mark.parametrize("regime", ["unique", "zipf", "ragged"])
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("op,D,gdt", _BWD)
def test_pooled_apply_bitwise(dev, op, D, gdt, L, regime):
    """the pooled call against (i) the restatement: contributions(g[i // L], mask, grad_scale) -> sums, and (ii) the plain call on
    g.repeat_interleave(L, 0) with the same row_scale -- same contributions, same order"""
    from mindrec_amd import ops
    rng = np.random.default_rng(D * 1000 + L * 10 + len(regime) + len(op))
    idt = (np.int32, np.int64)[(L + D) % 2]
    ids, V, n = _regime_ids(regime, rng, L, idt)
    rows = -(-n // L)
    vec = A.lane_width(D, D, D, [0], 0, 2 if gdt != torch.float32 else 4)
    aw = ops.apply_window(D, vec == 4)
    idx = A.Index(ids)
    _check_regime(regime, A.census(idx, D, vec, aw, V=V), n, aw)
    g, tg = _g_rows(rng, rows, D, gdt, dev)
    rs = _masks(rng, n, 1).reshape(-1) * (rng.random(n) + 0.25).astype(np.float32)
    trs = T(rs, dev)
    gs = 0.37
    plan = ops.sparse_plan(T(ids, dev))
    tg_big = tg.repeat_interleave(L, 0)[:n].contiguous()
    G = P.sums(idx, P.pooled_contributions(g, L, n, rs, gs), D, vec, aw)
    if op == "segment_sum":
        got = ops.segment_sum(plan, tg, trs, grad_scale=gs, pool=L)[: idx.U].cpu().numpy()
        plain = ops.segment_sum(plan, tg_big, trs, grad_scale=gs)[: idx.U].cpu().numpy()
        _same(got, G, "pooled segment sum vs restatement")
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), "pooled segment sum vs the expanded gradient"
        return
    kind = "adam" if op == "lazy_adam" else "ftrl"
    st = _state(rng, V, D, kind)
    ta, tb = [T(a, dev) for a in st], [T(a, dev) for a in st]
    if op == "lazy_adam":
        kw = dict(beta1_power=0.81, beta2_power=0.998001, grad_scale=gs, use_nesterov=bool(L % 2))
        ops.sparse_lazy_adam_(*ta, plan, tg, trs, pool=L, **kw)
        ops.sparse_lazy_adam_(*tb, plan, tg_big, trs, **kw)
        A.lazy_adam(*st, idx.uniq, G, b1_pow=0.81, b2_pow=0.998001, nesterov=bool(L % 2))
    else:
        ops.sparse_ftrl_(*ta, plan, tg, trs, grad_scale=gs, pool=L)
        ops.sparse_ftrl_(*tb, plan, tg_big, trs, grad_scale=gs)
        A.ftrl(*st, idx.uniq, G)
    for name, x, y, ref in zip("012", ta, tb, st):
        _same(x.cpu().numpy(), ref, f"{op} state {name} vs restatement")
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{op} state {name}: pooled vs the expanded gradient"


@pytest.mark.parametrize("L,n,D,binary_mask", [(5000, 5003, 4, False), (3, 30, 6, True)])
def test_pooled_apply_one_length_as_one_field(dev, L, n, D, binary_mask):
    """pool=L runs the fields form's windows with one field, and two cases are its own.  L = 5000: above the fields form's cap of 4096
    bag slots and above the 16-bit range of a field offset, n = 5003: the last bag is partial (three positions) -- 2 gradient rows.
    L = 3, grad_scale = 0.37 under a 0/1 mask, D = 6 (8-byte lanes): the contribution's second factor is the armed call's own
    grad_scale.  int32 ids drawn from 8 rows (long runs), segment sum and LazyAdam, against the host restatement alone."""
    from mindrec_amd import ops
    rng = np.random.default_rng(L + n)
    V, gs = 8, 0.37
    ids = rng.integers(0, V, size=n).astype(np.int32)
    rows = -(-n // L)
    vec = A.lane_width(D, D, D, [0], 0, 4)
    aw = ops.apply_window(D, vec == 4)
    idx = A.Index(ids)
    g, tg = _g_rows(rng, rows, D, torch.float32, dev)
    rs = (rng.random(n) < 0.6).astype(np.float32) if binary_mask else (rng.random(n) + 0.25).astype(np.float32)
    trs = T(rs, dev)
    plan = ops.sparse_plan(T(ids, dev))
    G = P.sums(idx, P.pooled_contributions(g, L, n, rs, gs), D, vec, aw)
    _same(ops.segment_sum(plan, tg, trs, grad_scale=gs, pool=L)[: idx.U].cpu().numpy(), G, "pooled segment sum")
    st = _state(rng, V, D, "adam")
    ts = [T(a, dev) for a in st]
    ops.sparse_lazy_adam_(*ts, plan, tg, trs, pool=L, beta1_power=0.81, beta2_power=0.998001, grad_scale=gs)
    A.lazy_adam(*st, idx.uniq, G, b1_pow=0.81, b2_pow=0.998001)
    for name, x, ref in zip("pmv", ts, st):
        _same(x.cpu().numpy(), ref, f"pooled LazyAdam {name}")


# ---- 3. arming ----------------------------------------------------------------------------------------------------------------------
def _arming_case(dev, D=64, L=8, B=700):
    rng = np.random.default_rng(33)
    V, n = 4000, B * L
    ids = np.minimum(rng.zipf(1.3, size=n) - 1, V - 1).astype(np.int32)
    st = _state(rng, V, D, "adam")
    g_small = rng.standard_normal((B, D)).astype(np.float32)
    g_big = rng.standard_normal((n, D)).astype(np.float32)
    rs = (rng.random(n) + 0.25).astype(np.float32)
    return V, n, ids, st, T(g_small, dev), T(g_big, dev), T(rs, dev)


def test_a_pooled_call_arms_one_call_only(dev):
    from mindrec_amd import ops
    D, L = 64, 8
    V, n, ids, st, tgs, tgb, trs = _arming_case(dev, D, L)
    plan = ops.sparse_plan(T(ids, dev))
    kw = dict(beta1_power=0.9, beta2_power=0.999, grad_scale=0.5)
    never = [T(a, dev) for a in st]
    ops.sparse_lazy_adam_(*never, plan, tgb, trs, **kw)                       # never armed
    seg_never = ops.segment_sum(plan, tgb, trs)
    scratch, after = [T(a, dev) for a in st], [T(a, dev) for a in st]
    ops.sparse_lazy_adam_(*scratch, plan, tgs, trs, pool=L, **kw)             # armed, ran
    ops.sparse_lazy_adam_(*after, plan, tgb, trs, **kw)                       # the same arguments as `never`: plain
    for x, y in zip(never, after):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    ops.segment_sum(plan, tgs, trs, pool=L)
    U = plan.U                                                                # (rows >= U of a segment sum's buffer are unspecified)
    assert torch.equal(ops.segment_sum(plan, tgb, trs)[:U].view(torch.int32), seg_never[:U].view(torch.int32))
    assert not torch.equal(scratch[0], never[0])


def test_refused_combinations_launch_nothing_and_disarm(dev, monkeypatch):
    """pool with max_norm, with constant columns, and on the folded wide apply: MREC_EUNSUPPORTED, tables untouched, and the next
    plain call is the plain call.  ops has no keyword for the last two: the call is handed their record (mrec_apply_opts_t) here."""
    import ctypes
    from mindrec_amd import _lib, ops

    def with_record(rec, fn, *args, **kwargs):
        with monkeypatch.context() as mp:
            mp.setattr(ops, "_opts_ptr", lambda _: ctypes.byref(rec))
            return fn(*args, **kwargs)
    D, L, F = 64, 8, 8
    V, n, ids, st, tgs, tgb, trs = _arming_case(dev, D, L)
    tid = T(ids, dev)
    plan = ops.sparse_plan(tid)
    kw = dict(beta1_power=0.9, beta2_power=0.999, grad_scale=0.5)
    never = [T(a, dev) for a in st]
    ops.sparse_lazy_adam_(*never, plan, tgb, trs, **kw)

    def untouched(ts, ref):
        torch.cuda.synchronize()
        for t, a in zip(ts, ref):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))

    def plain_is_plain(ts):
        ops.sparse_lazy_adam_(*ts, plan, tgb, trs, **kw)
        for x, y in zip(never, ts):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))

    # max_norm
    ts = [T(a, dev) for a in st]
    with pytest.raises(_lib.MrecError) as e:
        ops.sparse_lazy_adam_(*ts, plan, tgs, trs, max_norm=0.05, pool=L, **kw)
    assert e.value.code == -3
    untouched(ts, st)
    plain_is_plain(ts)
    # constant columns in the same record
    ts = [T(a, dev) for a in st]
    ids2 = tid.reshape(-1, F).contiguous()
    state = ops.const_cols_detect(ids2, V)
    rec = ops.ApplyOpts(pool=L, const_state=ops._ptr(state), const_ids=ops._ptr(ids2), const_id_bytes=4, const_B=ids2.shape[0])
    with pytest.raises(_lib.MrecError) as e:
        with_record(rec, ops.sparse_lazy_adam_, *ts, plan, tgs, trs, pool=L, **kw)
    assert e.value.code == -3
    untouched(ts, st)
    plain_is_plain(ts)
    # the folded wide apply (fused rows [p | w accum linear pad | m | v | pad]), launched and deferred
    rng = np.random.default_rng(7)
    ld = -(-(3 * D + 4) // 32) * 32
    buf = (rng.standard_normal((V, ld)) * 0.01).astype(np.float32)
    buf[:, D + 1] = 1.0 + rng.random(V).astype(np.float32)
    buf[:, 2 * D + 4:3 * D + 4] = np.abs(buf[:, 2 * D + 4:3 * D + 4]) * 1e-3
    gw = T(rng.standard_normal(n // F).astype(np.float32), dev)

    def wide(tb, **extra):
        return ops.sparse_lazy_adam_wide_(tb[:, :D], tb[:, D + 4:2 * D + 4], tb[:, 2 * D + 4:3 * D + 4], plan, tgb, trs, gw, F, D, **kw, **extra)

    wnever = T(buf, dev)
    wide(wnever)
    for defer in (False, True):
        tb = T(buf, dev)
        with pytest.raises(_lib.MrecError) as e:
            with_record(ops.ApplyOpts(pool=L), wide, tb, defer=defer)
        assert e.value.code == -3
        untouched([tb], [buf])
        wide(tb)                                                              # plain again
        assert torch.equal(tb.view(torch.int32), wnever.view(torch.int32))


def test_pool_checks_the_gradient_rows(dev):
    from mindrec_amd import ops
    V, n, ids, st, tgs, tgb, trs = _arming_case(dev)
    plan = ops.sparse_plan(T(ids, dev))
    with pytest.raises(TypeError):
        ops.segment_sum(plan, tgb, trs, pool=8)                               # n rows where ceil(n / L) are wanted
    with pytest.raises(ValueError):
        ops.segment_sum(plan, tgs, trs, pool=0)
    seg = ops.segment_sum(plan, tgb, trs)                                     # nothing was left armed by the refusals
    assert torch.equal(seg[: plan.U].view(torch.int32), ops.segment_sum(plan, tgb, trs, pool=1)[: plan.U].view(torch.int32))


# ---- 4. MultiHotEmbedding -----------------------------------------------------------------------------------------------------------
_HYP = dict(lazy_adam=dict(lr=3.5e-4), adam=dict(lr=3.5e-4), ftrl=dict(lr=5e-2))


def _mh_reference(opt, mode, V, D, L, seed, ids, masks, targets, steps, gs0=1.0):
    """the same loop on the host: _pool_ref forward, dy = pooled - target, _apply_order sums, the oracle's update formulas; returns the
    table and the two state arrays after every step"""
    table = O.fill_normal(seed, V, D, 0.01)
    s1 = np.ones_like(table) if opt == "ftrl" else np.zeros_like(table)
    s2 = np.zeros_like(table)
    b1, b2 = np.float32(0.9), np.float32(0.999)
    b1p, b2p = np.float32(1.0), np.float32(1.0)
    vec = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    from mindrec_amd import ops
    aw = ops.apply_window(D, vec == 4)
    out = []
    for t in range(steps):
        flat = ids[t].reshape(-1, L)
        m = masks[t].reshape(-1, L) if masks[t] is not None else None
        pooled = P.gather_pool(table, flat, m, mode)
        dy = (pooled.reshape(targets[t].shape) - targets[t]).astype(np.float32)
        idx = A.Index(flat)
        n = flat.size
        x = P.pooled_contributions(dy.reshape(-1, D), L, n, m.reshape(-1) if m is not None else None, P.mean_scale(gs0, L, mode))
        G = P.sums(idx, x, D, vec, aw)
        b1p, b2p = np.float32(b1p * b1), np.float32(b2p * b2)
        if opt == "lazy_adam":
            A.lazy_adam(table, s1, s2, idx.uniq, G, b1_pow=float(b1p), b2_pow=float(b2p), lr=3.5e-4)
        elif opt == "ftrl":
            A.ftrl(table, s1, s2, idx.uniq, G, lr=5e-2)
        else:                     # dense Adam: zeros, the sums scattered to their rows, g + fl(0 * p), the oracle's Adam over the whole table
            gd = np.zeros_like(table)
            rows = idx.uniq.astype(np.int64)
            ok = (rows >= 0) & (rows < V)
            gd[rows[ok]] = G[ok]
            gd = (gd + (table * np.float32(0.0)).astype(np.float32)).astype(np.float32)
            O.dense_adam(table, s1, s2, gd, lr=3.5e-4, b1_pow=float(b1p), b2_pow=float(b2p), grad_scale=1.0)
        out.append((table.copy(), s1.copy(), s2.copy(), pooled.reshape(targets[t].shape).copy()))
    return out


def _mh_inputs(rng, V, B, F, L, D, steps, idt, with_mask):
    shape = (B, L) if F == 1 else (B, F, L)
    ids = [np.minimum(rng.zipf(1.3, size=shape) - 1 + rng.integers(0, 30, size=shape), V + 1).astype(idt) for _ in range(steps)]
    masks = [(rng.random(shape) < 0.7).astype(np.float32) if with_mask else None for _ in range(steps)]
    targets = [(rng.standard_normal((B, F * D)) * 0.01).astype(np.float32) for _ in range(steps)]
    return ids, masks, targets


@pytest.mark.parametrize("opt,mode,D,F,idt,with_mask", [("lazy_adam", "mean", 64, 1, np.int32, True), ("lazy_adam", "mean", 64, 6, np.int64, True),
                                                         ("lazy_adam", "sum", 30, 1, np.int32, False), ("ftrl", "sum", 1, 1, np.int32, True),
                                                         ("ftrl", "sum", 1, 6, np.int64, True), ("adam", "mean", 64, 1, np.int32, True),
                                                         ("adam", "mean", 64, 6, np.int32, True)])
def test_multi_hot_embedding_five_steps(dev, opt, mode, D, F, idt, with_mask):
    from mindrec_amd.multi_hot import MultiHotEmbedding
    rng = np.random.default_rng(D + F + len(opt))
    V, B, L, steps, seed = 2090, 512, 8, 5, 1234
    ids, masks, targets = _mh_inputs(rng, V, B, F, L, D, steps, idt, with_mask)
    ref = _mh_reference(opt, mode, V, D, L, seed, ids, masks, targets, steps)
    emb = MultiHotEmbedding(V, D, L, mode=mode, optimizer=opt, device=dev, seed=seed, **_HYP[opt])
    dy = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    for t in range(steps):
        pooled = emb.lookup(T(ids[t], dev), T(masks[t], dev) if with_mask else None)
        assert tuple(pooled.shape) == (B, F * D)
        torch.sub(pooled, T(targets[t], dev), out=dy)                          # an exact fp32 subtraction on both sides
        emb.apply_(dy)
        _same(pooled.cpu().numpy(), ref[t][3], f"step {t}: pooled rows")
        for name, x, r in zip(("table", "state 1", "state 2"), (emb.table,) + tuple(emb.state), ref[t][:3]):
            _same(x.cpu().numpy(), r, f"step {t}: {name}")
    assert emb.step_count == steps


@pytest.mark.parametrize("opt,mode,D,F", [("lazy_adam", "mean", 64, 6), ("ftrl", "sum", 1, 1), ("adam", "mean", 64, 1)])
def test_multi_hot_embedding_captured_equals_eager(dev, opt, mode, D, F):
    """five steps of lookup -> dy -> apply_ captured into ONE HIP graph on one stream and replayed: the eager run's bits"""
    from mindrec_amd.multi_hot import MultiHotEmbedding
    rng = np.random.default_rng(D + F)
    V, B, L, steps, seed = 2090, 256, 8, 5, 99
    ids, masks, targets = _mh_inputs(rng, V, B, F, L, D, steps, np.int32, True)
    tids, tmasks, ttargets = [T(a, dev) for a in ids], [T(a, dev) for a in masks], [T(a, dev) for a in targets]

    def run(emb, dy):
        for t in range(steps):
            pooled = emb.lookup(tids[t], tmasks[t])
            torch.sub(pooled, ttargets[t], out=dy)
            emb.apply_(dy)

    eager = MultiHotEmbedding(V, D, L, mode=mode, optimizer=opt, device=dev, seed=seed, **_HYP[opt])
    run(eager, torch.empty((B, F * D), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    cap = MultiHotEmbedding(V, D, L, mode=mode, optimizer=opt, device=dev, seed=seed, **_HYP[opt])
    dyc = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(cap, dyc)
    torch.cuda.synchronize()
    # (capture ran nothing: the table still holds its initial values)
    assert np.array_equal(cap.table.cpu().numpy().view(np.uint32), O.fill_normal(seed, V, D, 0.01).view(np.uint32))
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip((eager.table,) + tuple(eager.state), (cap.table,) + tuple(cap.state)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not np.array_equal(cap.table.cpu().numpy(), O.fill_normal(seed, V, D, 0.01))
