"""Multi-hot fields of UNEQUAL bag length on the GPU: the fields lookup (mrec_gather_pool_fields) bit for bit against its host
restatement (tests/_pool_fields_ref.py) and against the one-length kernel field by field; the fields apply
(the fields form of mrec_apply_opts_t) bit for bit against the restated contributions pushed through the apply's order of additions
(tests/_pool_ref.sums), against pool=L where the lengths are equal, and -- independently of every restatement -- against the plain
apply on the explicitly expanded gradient where the field scales are powers of two; MultiHotEmbedding with a tuple `bag`, eager and
captured, and the one-update-per-step property the fields form exists for.  Every comparison is on raw bits, over all rows."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _apply_order as A  # noqa: E402
import _pool_fields_ref as FR  # noqa: E402
import _pool_ref as P  # noqa: E402
from oracle import oracle as O  # noqa: E402

FIELD_SETS = [(3, 5, 4, 3, 4, 2), (1, 9), (7,), (1, 1, 1)]
_KIND = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
_NP = {torch.int32: np.int32, torch.int64: np.int64}


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


def _masks(rng, B, Ls):
    """0/1 masks: all-zero samples, all-one samples, random ones"""
    m = (rng.random((B, Ls)) < 0.6).astype(np.float32)
    m[: B // 8] = 0.0
    m[B // 8: B // 4] = 1.0
    return m


# ---- 1. forward against the host restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", FIELD_SETS)
@pytest.mark.parametrize("D", [1, 3, 64, 80, 128, 260])
def test_gather_pool_fields_bitwise(dev, D, lens):
    """int32 ids: a table view inside wider rows (ld = D + 8) and the result written into a column block of a wider matrix
    (ldo = F * D + 8), whose other columns keep their bits -- at D = 80 both start five floats in, which takes the float4 lanes away
    and walks the 80 columns in two blocks of single-column lanes; int64 ids: the default strides.  B = 333 does not fill the last
    wave."""
    from mindrec_amd import ops
    rng = np.random.default_rng(D * 100 + sum(lens))
    V, B, F, Ls = 1500, 333, len(lens), sum(lens)
    big = rng.standard_normal((V, D + 8)).astype(np.float32)
    c0 = 5 if D == 80 else 4
    table = np.ascontiguousarray(big[:, c0:c0 + D])
    tbig, tt = T(big, dev), T(table, dev)
    mask = _masks(rng, B, Ls)
    for idt in (torch.int32, torch.int64):
        ids = _ids(rng, B, Ls, V, _NP[idt])
        tid = T(ids, dev)
        for m, tm in ((mask, T(mask, dev)), (None, None)):
            for mode in ("sum", "mean"):
                for odt in (torch.float32, torch.bfloat16, torch.float16):
                    ref = FR.gather_pool_fields(table, ids, lens, m, mode, _KIND[odt])
                    what = f"D={D} fields={lens} {idt} {odt} {mode} mask={m is not None}"
                    if idt == torch.int64:
                        got = ops.gather_pool_fields(tt, tid, lens, tm, mode=mode, out_dtype=odt)
                        assert got.dtype == odt and tuple(got.shape) == (B, F * D)
                        _same(_bits(got), ref, what)
                    else:
                        wide0 = (rng.integers(-64, 65, size=(B, F * D + 8)) / 8.0).astype(np.float32)      # (exact in every output type)
                        wide = T(wide0, dev).to(odt)
                        blk = wide[:, c0:c0 + F * D]
                        assert ops.gather_pool_fields(tbig[:, c0:c0 + D], tid, lens, tm, mode=mode, out=blk).data_ptr() == blk.data_ptr()
                        wide0[:, c0:c0 + F * D] = ref
                        _same(_bits(wide), wide0, what + " (column block)")


# ---- 2. forward against the existing kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", FIELD_SETS + [(4, 4, 4)])
@pytest.mark.parametrize("D", [3, 64])
def test_fields_lookup_is_the_one_length_lookup_field_by_field(dev, D, lens):
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotEmbedding
    rng = np.random.default_rng(D + len(lens))
    V, B, F, Ls = 900, 515, len(lens), sum(lens)
    tt = T(rng.standard_normal((V, D)).astype(np.float32), dev)
    tid, tm = T(_ids(rng, B, Ls, V, np.int32), dev), T(_masks(rng, B, Ls), dev)
    for mode in ("sum", "mean"):
        for odt in (torch.float32, torch.bfloat16):
            got = ops.gather_pool_fields(tt, tid, lens, tm, mode=mode, out_dtype=odt)
            for f, off in enumerate(FR.offsets(lens)):
                one = ops.gather_pool(tt, tid[:, off:off + lens[f]], tm[:, off:off + lens[f]], mode=mode, out_dtype=odt)
                assert np.array_equal(_bits(got[:, f * D:(f + 1) * D]), _bits(one)), (mode, odt, f)
    if len(set(lens)) == 1:                      # equal lengths: today's [B, F, L] lookup
        a = MultiHotEmbedding(V, D, lens, mode="mean", device=dev, seed=5)
        b = MultiHotEmbedding(V, D, lens[0], mode="mean", device=dev, seed=5)
        assert torch.equal(a.table, b.table)
        xa = a.lookup(tid, tm)
        xb = b.lookup(tid.view(B, F, lens[0]), tm.view(B, F, lens[0]))
        assert tuple(xa.shape) == tuple(xb.shape) == (B, F * D) and np.array_equal(_bits(xa), _bits(xb))


# ---- 3. apply against the host restatement ------------------------------------------------------------------------------------------
def _dup_ids(rng, B, Ls, V, idt):
    """ids from a small range, Zipf-like: most ids occur in several fields and many samples (runs that cross windows, the tree of
    partial sums); a few rows outside the table"""
    ids = np.minimum(rng.zipf(1.3, size=(B, Ls)) - 1 + rng.integers(0, 40, size=(B, Ls)), V - 1).astype(np.int64)
    ids.reshape(-1)[::97] = V + 2
    return ids.astype(idt)


def _row_scale(rng, ids, n_dead=5):
    """0/1 mask times a weight, with every position of a few ids masked (rows whose every contribution is a signed zero)"""
    flat = ids.reshape(-1)
    rs = ((rng.random(flat.size) < 0.7) * (rng.random(flat.size) + 0.25)).astype(np.float32)
    dead = np.unique(flat)[3:3 + n_dead]
    rs[np.isin(flat, dead)] = 0.0
    return rs, dead


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


def _geometry(D, gdt):
    from mindrec_amd import ops
    vec = A.lane_width(D, D, D, [0], 0, 2 if gdt != torch.float32 else 4)
    return vec, ops.apply_window(D, vec == 4)


_BWD = [("segment_sum", 64, torch.float32), ("segment_sum", 30, torch.bfloat16), ("lazy_adam", 64, torch.float32),
        ("lazy_adam", 64, torch.bfloat16), ("lazy_adam", 80, torch.float16), ("ftrl", 1, torch.float32), ("ftrl", 64, torch.float32)]


@pytest.mark.parametrize("lens", FIELD_SETS)
@pytest.mark.parametrize("op,D,gdt", _BWD)
def test_fields_apply_bitwise(dev, op, D, gdt, lens):
    from mindrec_amd import ops
    rng = np.random.default_rng(D * 1000 + sum(lens) * 10 + len(op))
    F, Ls = len(lens), sum(lens)
    V, B = 300, 1511
    n = B * Ls
    idt = (np.int32, np.int64)[(Ls + D) % 2]
    ids = _dup_ids(rng, B, Ls, V, idt)
    idx = A.Index(ids)
    per_id_fields = [len(set(FR.slot_field(lens)[np.nonzero(ids == u)[1]])) for u in idx.uniq[:50]]
    assert F == 1 or np.mean(np.array(per_id_fields) > 1) > 0.5, "most ids are to occur in several fields"
    vec, aw = _geometry(D, gdt)
    assert (np.diff(idx.offs) > 4 * aw).sum() > 10                      # runs that cross several windows
    g, tg = _g_rows(rng, B * F, D, gdt, dev)
    rs, dead = _row_scale(rng, ids)
    rs.reshape(B, Ls)[: B // 8] = 0.0                                   # samples whose every position is masked
    fs = tuple(float(np.float32(0.37) / np.float32(L)) for L in lens)
    G = P.sums(idx, FR.contributions(g, lens, n, rs, fs), D, vec, aw)
    assert all((G[idx.uniq == d] == 0).all() for d in dead)
    plan = ops.sparse_plan(T(ids, dev))
    trs = T(rs, dev)
    tg2 = tg.view(B, F * D)                                              # the gradient as the lookup's result has it
    if op == "segment_sum":
        got = ops.segment_sum(plan, tg2, trs, fields=lens, field_scale=fs)[: idx.U].cpu().numpy()
        _same(got, G, "fields segment sum vs restatement")
        return
    kind = "adam" if op == "lazy_adam" else "ftrl"
    st = _state(rng, V, D, kind)
    ts = [T(a, dev) for a in st]
    if op == "lazy_adam":
        ops.sparse_lazy_adam_(*ts, plan, tg2, trs, beta1_power=0.81, beta2_power=0.998001, use_nesterov=bool(Ls % 2), fields=lens, field_scale=fs)
        A.lazy_adam(*st, idx.uniq, G, b1_pow=0.81, b2_pow=0.998001, nesterov=bool(Ls % 2))
    else:
        ops.sparse_ftrl_(*ts, plan, tg, trs, fields=lens, field_scale=fs)
        A.ftrl(*st, idx.uniq, G)
    for name, x, ref in zip("012", ts, st):
        _same(x.cpu().numpy(), ref, f"{op} state {name} vs restatement")


# ---- 4. fields == pooled where the lengths are equal --------------------------------------------------------------------------------
@pytest.mark.parametrize("op,D,L,F", [("lazy_adam", 64, 8, 6), ("ftrl", 1, 3, 4), ("segment_sum", 30, 2, 3), ("lazy_adam", 80, 1, 5)])
def test_fields_of_equal_length_is_the_pooled_apply(dev, op, D, L, F):
    from mindrec_amd import ops
    rng = np.random.default_rng(D + L + F)
    V, B, gs = 400, 517, 0.37
    ids = _dup_ids(rng, B, F * L, V, np.int32)
    rs, _ = _row_scale(rng, ids)
    plan = ops.sparse_plan(T(ids, dev))
    tg, trs = T(rng.standard_normal((B * F, D)).astype(np.float32), dev), T(rs, dev)
    fkw, pkw = dict(fields=(L,) * F, field_scale=(gs,) * F), dict(pool=L, grad_scale=gs)
    if op == "segment_sum":
        a, b = ops.segment_sum(plan, tg, trs, **fkw)[: plan.U], ops.segment_sum(plan, tg, trs, **pkw)[: plan.U]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        c = ops.segment_sum(plan, tg, trs, fields=(L,) * F, grad_scale=gs)[: plan.U]          # without field_scale: grad_scale for every field
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
        return
    st = _state(rng, V, D, "adam" if op == "lazy_adam" else "ftrl")
    ta, tb = [T(x, dev) for x in st], [T(x, dev) for x in st]
    fn = ops.sparse_lazy_adam_ if op == "lazy_adam" else ops.sparse_ftrl_
    fn(*ta, plan, tg, trs, **fkw)
    fn(*tb, plan, tg, trs, **pkw)
    for x, y, z in zip(ta, tb, st):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert not np.array_equal(x.cpu().numpy(), z)


# ---- 5. an independent check against the plain, unpooled apply ----------------------------------------------------------------------
@pytest.mark.parametrize("op,D,gdt", [("segment_sum", 64, torch.float32), ("lazy_adam", 64, torch.bfloat16), ("lazy_adam", 3, torch.float32),
                                      ("ftrl", 64, torch.float32)])
def test_fields_apply_is_the_plain_apply_on_the_expanded_gradient(dev, op, D, gdt):
    """fields (1, 2, 4, 8), the mean with grad_scale 1: every gs_f = 1 / L_f is a power of two, so (g * mask) * gs_f -- the fields
    form's contribution -- and (g * (mask * gs_f)) * 1 -- the plain apply's on the expanded gradient with row_scale = mask * gs_f --
    are the same fp32 number as long as neither is subnormal.  No host restatement takes part."""
    from mindrec_amd import ops
    lens = (1, 2, 4, 8)
    rng = np.random.default_rng(D)
    F, Ls, V, B = len(lens), sum(lens), 300, 523
    n = B * Ls
    ids = _dup_ids(rng, B, Ls, V, np.int64)
    g, tg = _g_rows(rng, B * F, D, gdt, dev)
    mask = _masks(rng, B, Ls).reshape(-1)
    fs = FR.field_scales(1.0, lens, "mean")
    assert fs == (1.0, 0.5, 0.25, 0.125)
    # the premise, checked on the inputs: no product is subnormal (0/1 mask, so the products are 0 or g * gs_f)
    tiny = np.finfo(np.float32).tiny
    assert set(np.unique(mask)) <= {0.0, 1.0} and (np.abs(g[g != 0]) * np.float32(min(fs)) >= tiny).all()
    rows, f = FR.bag_rows(lens, n)
    rs_plain = (mask * np.asarray(fs, np.float32)[f]).astype(np.float32)
    tg_big = tg[T(rows, dev)].contiguous()
    plan = ops.sparse_plan(T(ids, dev))
    tm, trs = T(mask, dev), T(rs_plain, dev)
    if op == "segment_sum":
        a = ops.segment_sum(plan, tg, tm, fields=lens, field_scale=fs)[: plan.U]
        b = ops.segment_sum(plan, tg_big, trs)[: plan.U]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        return
    st = _state(rng, V, D, "adam" if op == "lazy_adam" else "ftrl")
    ta, tb = [T(x, dev) for x in st], [T(x, dev) for x in st]
    fn = ops.sparse_lazy_adam_ if op == "lazy_adam" else ops.sparse_ftrl_
    fn(*ta, plan, tg, tm, fields=lens, field_scale=fs)
    fn(*tb, plan, tg_big, trs)
    for x, y, z in zip(ta, tb, st):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert not np.array_equal(x.cpu().numpy(), z)


def test_fields_arm_one_call_only_and_refusals_disarm(dev):
    from mindrec_amd import _lib, ops
    lens, D = (3, 5, 4), 64
    rng = np.random.default_rng(3)
    V, B, F, Ls = 500, 300, len(lens), sum(lens)
    ids = _dup_ids(rng, B, Ls, V, np.int32)
    plan = ops.sparse_plan(T(ids, dev))
    tgs, tgb = T(rng.standard_normal((B * F, D)).astype(np.float32), dev), T(rng.standard_normal((B * Ls, D)).astype(np.float32), dev)
    st = _state(rng, V, D, "adam")
    never = [T(a, dev) for a in st]
    ops.sparse_lazy_adam_(*never, plan, tgb)
    scratch, after = [T(a, dev) for a in st], [T(a, dev) for a in st]
    ops.sparse_lazy_adam_(*scratch, plan, tgs, fields=lens)                    # armed, ran
    ops.sparse_lazy_adam_(*after, plan, tgb)                                   # plain again
    for x, y in zip(never, after):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    ts = [T(a, dev) for a in st]
    with pytest.raises(_lib.MrecError) as e:
        ops.sparse_lazy_adam_(*ts, plan, tgs, fields=lens, max_norm=0.05)      # refused before any launch
    assert e.value.code == -3
    torch.cuda.synchronize()
    for t, a in zip(ts, st):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))
    ops.sparse_lazy_adam_(*ts, plan, tgb)                                      # ... and disarmed
    for x, y in zip(never, ts):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    with pytest.raises(ValueError):
        ops.segment_sum(plan, tgs, fields=lens, pool=4)                        # one form or the other
    with pytest.raises(TypeError):
        ops.segment_sum(plan, tgb, fields=lens)                                # B * Ls rows where B * F are wanted
    with pytest.raises(ValueError):
        ops.segment_sum(plan, tgs, fields=lens, field_scale=(1.0, 1.0, 1.0), grad_scale=0.5)


# ---- 6. MultiHotEmbedding with a tuple bag ------------------------------------------------------------------------------------------
_HYP = dict(lazy_adam=dict(lr=3.5e-4), adam=dict(lr=3.5e-4), ftrl=dict(lr=5e-2))


def _mh_reference(opt, mode, V, D, lens, seed, ids, masks, targets, steps):
    """the loop on the host: the restated lookup, dy = pooled - target, the restated contributions and sums, the oracle's updates"""
    from mindrec_amd import ops
    table = O.fill_normal(seed, V, D, 0.01)
    s1 = np.ones_like(table) if opt == "ftrl" else np.zeros_like(table)
    s2 = np.zeros_like(table)
    b1, b2 = np.float32(0.9), np.float32(0.999)
    b1p, b2p = np.float32(1.0), np.float32(1.0)
    vec = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    aw = ops.apply_window(D, vec == 4)
    F = len(lens)
    out = []
    for t in range(steps):
        pooled = FR.gather_pool_fields(table, ids[t], lens, masks[t], mode)
        dy = (pooled - targets[t]).astype(np.float32)
        idx = A.Index(ids[t])
        x = FR.contributions(dy.reshape(-1, D), lens, ids[t].size, None if masks[t] is None else masks[t].reshape(-1),
                             FR.field_scales(1.0, lens, mode))
        G = P.sums(idx, x, D, vec, aw)
        b1p, b2p = np.float32(b1p * b1), np.float32(b2p * b2)
        if opt == "lazy_adam":
            A.lazy_adam(table, s1, s2, idx.uniq, G, b1_pow=float(b1p), b2_pow=float(b2p), lr=3.5e-4)
        elif opt == "ftrl":
            A.ftrl(table, s1, s2, idx.uniq, G, lr=5e-2)
        else:                     # dense Adam over the whole table: the sums scattered to their rows, zeros elsewhere
            gd = np.zeros_like(table)
            rows = idx.uniq.astype(np.int64)
            ok = (rows >= 0) & (rows < V)
            gd[rows[ok]] = G[ok]
            gd = (gd + (table * np.float32(0.0)).astype(np.float32)).astype(np.float32)
            O.dense_adam(table, s1, s2, gd, lr=3.5e-4, b1_pow=float(b1p), b2_pow=float(b2p), grad_scale=1.0)
        out.append((table.copy(), s1.copy(), s2.copy(), pooled.copy()))
    assert F * D == out[0][3].shape[1]
    return out


def _mh_inputs(rng, V, B, lens, D, steps, idt, with_mask):
    shape = (B, sum(lens))
    ids = [np.minimum(rng.zipf(1.3, size=shape) - 1 + rng.integers(0, 30, size=shape), V + 1).astype(idt) for _ in range(steps)]
    masks = [(rng.random(shape) < 0.7).astype(np.float32) if with_mask else None for _ in range(steps)]
    targets = [(rng.standard_normal((B, len(lens) * D)) * 0.01).astype(np.float32) for _ in range(steps)]
    return ids, masks, targets


@pytest.mark.parametrize("opt,mode,D,lens,idt,with_mask", [("lazy_adam", "mean", 64, (3, 5, 4, 3, 4, 2), np.int64, True),
                                                            ("lazy_adam", "sum", 30, (1, 9), np.int32, False),
                                                            ("ftrl", "sum", 1, (3, 5, 4, 3, 4, 2), np.int64, True),
                                                            ("adam", "mean", 64, (3, 5, 4, 3, 4, 2), np.int32, True),
                                                            ("adam", "mean", 64, (7,), np.int32, True)])
def test_multi_hot_embedding_fields_three_steps(dev, opt, mode, D, lens, idt, with_mask):
    from mindrec_amd.multi_hot import MultiHotEmbedding
    rng = np.random.default_rng(D + len(lens) + len(opt))
    V, B, steps, seed, F = 2090, 384, 3, 1234, len(lens)
    ids, masks, targets = _mh_inputs(rng, V, B, lens, D, steps, idt, with_mask)
    ref = _mh_reference(opt, mode, V, D, lens, seed, ids, masks, targets, steps)
    emb = MultiHotEmbedding(V, D, lens, mode=mode, optimizer=opt, device=dev, seed=seed, **_HYP[opt])
    assert emb.fields == tuple(lens) and emb.bag == sum(lens)
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


@pytest.mark.parametrize("opt", ["lazy_adam", "ftrl", "adam"])
def test_an_id_in_two_fields_gets_one_update_per_step(dev, opt):
    """What the fields form exists for.  Fields (2, 3) over one table; one step.  The fields form sums an id's gradients over both
    fields and updates its row once (checked against the restatement, which does exactly that); a lookup and an apply_ per length
    -- two embeddings sharing the table and the state -- update a row that occurs in both fields twice, and must come out different
    on those rows, while the forward pass is the same."""
    from mindrec_amd.multi_hot import MultiHotEmbedding
    rng = np.random.default_rng(len(opt))
    lens, V, D, B, seed = (2, 3), 400, 64, 256, 77
    ids = rng.integers(0, V, size=(B, 5)).astype(np.int32)
    target = (rng.standard_normal((B, 2 * D)) * 0.01).astype(np.float32)
    in0, in1 = np.unique(ids[:, :2]), np.unique(ids[:, 2:])
    both = np.intersect1d(in0, in1)
    assert both.size > 50
    tid, tt = T(ids, dev), T(target, dev)
    one = MultiHotEmbedding(V, D, lens, mode="mean", optimizer=opt, device=dev, seed=seed, **_HYP[opt])
    x1 = one.lookup(tid)
    dy = x1 - tt
    one.apply_(dy)
    ref = _mh_reference(opt, "mean", V, D, lens, seed, [ids], [None], [target], 1)[0]
    for x, r in zip((one.table,) + tuple(one.state), ref[:3]):
        _same(x.cpu().numpy(), r, "the fields form vs the restatement: one update of the summed gradient")
    a = MultiHotEmbedding(V, D, 2, mode="mean", optimizer=opt, device=dev, seed=seed, **_HYP[opt])
    b = MultiHotEmbedding(V, D, 3, mode="mean", optimizer=opt, device=dev, seed=seed, **_HYP[opt])
    b.table, b.state = a.table, a.state
    if opt == "ftrl":
        b.accum, b.linear = a.accum, a.linear
    else:
        b.m, b.v = a.m, a.v
    xa, xb = a.lookup(tid[:, :2].contiguous()), b.lookup(tid[:, 2:].contiguous())
    assert torch.equal(torch.cat([xa, xb], 1), x1)                       # the same forward pass, bit for bit
    a.apply_(dy[:, :D].contiguous())
    b.apply_(dy[:, D:].contiguous())
    two, got = a.table.cpu().numpy(), one.table.cpu().numpy()
    differs = (two != got).any(axis=1)
    assert differs[both].mean() > 0.9, "an id in both fields: two updates are not one update of the summed gradient"


@pytest.mark.parametrize("opt,mode,D,lens", [("lazy_adam", "mean", 64, (3, 5, 4, 3, 4, 2)), ("ftrl", "sum", 1, (1, 9)), ("adam", "mean", 64, (1, 2, 4, 8))])
def test_multi_hot_embedding_fields_captured_equals_eager(dev, opt, mode, D, lens):
    """three steps of lookup -> dy -> apply_ captured into ONE HIP graph on one stream and replayed: the eager run's bits"""
    from mindrec_amd.multi_hot import MultiHotEmbedding
    rng = np.random.default_rng(D + len(lens))
    V, B, steps, seed, F = 2090, 256, 3, 99, len(lens)
    ids, masks, targets = _mh_inputs(rng, V, B, lens, D, steps, np.int32, True)
    tids, tmasks, ttargets = [T(a, dev) for a in ids], [T(a, dev) for a in masks], [T(a, dev) for a in targets]

    def run(emb, dy):
        for t in range(steps):
            pooled = emb.lookup(tids[t], tmasks[t])
            torch.sub(pooled, ttargets[t], out=dy)
            emb.apply_(dy)

    eager = MultiHotEmbedding(V, D, lens, mode=mode, optimizer=opt, device=dev, seed=seed, **_HYP[opt])
    run(eager, torch.empty((B, F * D), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    cap = MultiHotEmbedding(V, D, lens, mode=mode, optimizer=opt, device=dev, seed=seed, **_HYP[opt])
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
