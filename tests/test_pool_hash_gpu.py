"""Multi-hot fields over a hash table on the GPU: the keyed pooled lookup (mrec_gather_pool_fields_keyed) and MultiHotHashEmbedding.
Every comparison is on raw bits -- the pooled arithmetic is restated on the host (tests/_pool_fields_ref.py), and the rows it is
applied to come from the existing MapTensorGet path, MapParameter.get(insert_default_value=False), on a twin of the map.

  lookup: probe + keyed pooled launch against the host pooling of the twin's [n, D] rows, over widths, fields, key types, masks,
    output types, default values and none / half / all of the keys missing; with every key resident also against
    ops.gather_pool_fields over the row numbers;
  full table: keys dropped by a full table contribute their default rows and are not updated;
  apply: map.values and both slot tables after lookup(train=True) + apply_ against the dense MultiHotEmbedding over clones of the
    tables and the admitted row numbers, two steps under permit_filter_value = 2, a key in several fields of one sample;
  eviction: a key that went stale and was evicted reads and trains as a new key;
  capture: lookup(train=False) captured and replayed.  (The training pair is NOT captured: MapParameter.lookup_rows(insert=True)
    advances the table's step on the host, and nothing in the project captures it.)"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pool_fields_ref as FR  # noqa: E402

_KIND = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
_NP = {torch.int32: np.int32, torch.int64: np.int64}
SIX = (3, 5, 4, 3, 4, 2)
_HYP = {"lazy_adam": dict(lr=0.05), "ftrl": dict(lr=0.1, l1=1e-3, l2=1e-3)}
_SLOTS = {"lazy_adam": ("moment1", "moment2"), "ftrl": ("accum", "linear")}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().float().cpu().numpy().view(np.uint32)


def _same(got, ref, what):
    ref = np.ascontiguousarray(ref, np.float32).view(np.uint32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = (got != ref).reshape(got.shape[0], -1).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, e.g. rows {np.nonzero(bad)[0][:6].tolist()}"


def _distinct_keys(rng, n, kdt):
    lo, hi = (-2 ** 30, 2 ** 30) if kdt == torch.int32 else (-2 ** 40, 2 ** 40)
    k = np.unique(rng.integers(lo, hi, size=4 * n))
    assert k.size >= n
    return rng.permutation(k)[:n].astype(_NP[kdt])


def _new_map(dev, kdt, D, default="normal", capacity=1024, **kw):
    from mindrec_amd.experimental import MapParameter
    return MapParameter(key_dtype=kdt, value_shape=D, default_value=default, capacity=capacity, device=dev, seed=11, **kw)


def _masks(rng, B, Ls):
    """None, a 0/1 mask (an all-zero and an all-one sample among them), arbitrary weights"""
    m01 = (rng.random((B, Ls)) < 0.6).astype(np.float32)
    m01[0], m01[1] = 0.0, 1.0
    return (None, m01, (rng.standard_normal((B, Ls)) * 1.5).astype(np.float32))


def _pool_rows(rows_nd, B, lens, mask, mode, kind="f32"):
    """the host pooling of [B * Ls, D] rows, one per key position"""
    n = rows_nd.shape[0]
    return FR.gather_pool_fields(np.ascontiguousarray(rows_nd, np.float32), np.arange(n).reshape(B, sum(lens)), lens, mask, mode, kind)


def _default_rows(dev, kdt, D, default, keys):
    """the default row of every key: MapTensorGet without insertion on an EMPTY map of the same seed"""
    return _new_map(dev, kdt, D, default, capacity=8).get(T(keys.reshape(-1), dev), insert_default_value=False).cpu().numpy()


# ---- 1. lookup -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1,), (9,), SIX])
@pytest.mark.parametrize("D", [1, 6, 64, 320])
def test_keyed_lookup_bitwise(dev, D, lens):
    """D = 1 and 6: one column per lane; 64: float4 lanes; 320: column blocks beyond one wave.  (9,): two batches of PB = 8 slots.
    B = 37 does not fill the last wave."""
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotHashEmbedding
    rng = np.random.default_rng(1000 * D + sum(lens))
    B, F, Ls, R = 37, len(lens), sum(lens), 300
    for kdt in (torch.int32, torch.int64):
        allk = _distinct_keys(rng, 2 * R, kdt)
        res, fresh = allk[:R], allk[R:]
        vals = rng.standard_normal((R, D)).astype(np.float32)             # resident rows that are NOT their keys' default rows
        for default in ("normal", "zeros", 0.5):
            m, twin = (_new_map(dev, kdt, D, default) for _ in range(2))
            for t in (m, twin):
                t.put(T(res, dev), T(vals, dev))
            embs = {mode: MultiHotHashEmbedding(m, bag=lens, mode=mode) for mode in ("sum", "mean")}
            for frac in (0.0, 0.5, 1.0):
                miss = rng.random((B, Ls)) < frac
                keys = np.where(miss, rng.choice(fresh, size=(B, Ls)), rng.choice(res, size=(B, Ls))).astype(_NP[kdt])
                tk = T(keys, dev)
                rows_e = twin.get(tk.reshape(-1), insert_default_value=False).cpu().numpy()      # [B * Ls, D]: the existing path
                rows = m.lookup_rows(tk.reshape(-1), insert=False)[2].view(B, Ls)
                assert bool((rows.cpu().numpy() < 0).reshape(B, Ls)[miss].all()) and int((rows < 0).sum()) == int(miss.sum())
                for mask in _masks(rng, B, Ls):
                    tm = T(mask, dev) if mask is not None else None
                    for mode in ("sum", "mean"):
                        for odt in (torch.float32, torch.bfloat16, torch.float16):
                            what = f"D={D} fields={lens} {kdt} default={default} missing={frac} {mode} {odt} mask={mask is not None}"
                            ref = _pool_rows(rows_e, B, lens, mask, mode, _KIND[odt])
                            out = torch.empty((B, F * D), dtype=odt, device=dev)
                            got = embs[mode].lookup(tk, tm, out=out, train=False)
                            assert got.data_ptr() == out.data_ptr()
                            _same(_bits(got), ref, what)
                            if frac == 0.0:
                                plain = ops.gather_pool_fields(m.values, rows, lens, tm, mode=mode, out_dtype=odt)
                                assert np.array_equal(_bits(got), _bits(plain)), what + " (against gather_pool_fields)"
            # probes change nothing: no key entered the table, no step was counted
            assert len(m) == R and m.step == 0 and embs["sum"].rows is None


def test_keyed_lookup_column_block_out_dtype_and_bags_per_sample(dev):
    """out as a column block of a wider matrix (its other columns keep their bits), out_dtype without out, and -- one field --
    keys [B, G, L]: G bags per sample."""
    from mindrec_amd.multi_hot import MultiHotHashEmbedding
    rng = np.random.default_rng(5)
    kdt, D, B, R = torch.int64, 8, 37, 200
    allk = _distinct_keys(rng, 2 * R, kdt)
    m, twin = (_new_map(dev, kdt, D) for _ in range(2))
    vals = rng.standard_normal((R, D)).astype(np.float32)
    for t in (m, twin):
        t.put(T(allk[:R], dev), T(vals, dev))
    lens, F, Ls = SIX, len(SIX), sum(SIX)
    keys = rng.choice(allk, size=(B, Ls))
    mask = _masks(rng, B, Ls)[1]
    rows_e = twin.get(T(keys.reshape(-1), dev), insert_default_value=False).cpu().numpy()
    emb = MultiHotHashEmbedding(m, bag=lens, mode="mean", out_dtype=torch.bfloat16)
    got = emb.lookup(T(keys, dev), T(mask, dev), train=False)
    assert got.dtype == torch.bfloat16
    _same(_bits(got), _pool_rows(rows_e, B, lens, mask, "mean", "bf16"), "out_dtype")
    wide0 = (rng.integers(-64, 65, size=(B, F * D + 8)) / 8.0).astype(np.float32)
    wide = T(wide0, dev)
    emb.lookup(T(keys, dev), T(mask, dev), out=wide[:, 4:4 + F * D], train=False)
    wide0[:, 4:4 + F * D] = _pool_rows(rows_e, B, lens, mask, "mean")
    _same(_bits(wide), wide0, "column block")
    G, L = 3, 7
    one = MultiHotHashEmbedding(m, bag=L, mode="sum")
    k3 = rng.choice(allk, size=(B, G, L))
    m3 = (rng.random((B, G, L)) < 0.7).astype(np.float32)
    r3 = twin.get(T(k3.reshape(-1), dev), insert_default_value=False).cpu().numpy()
    got = one.lookup(T(k3, dev), T(m3, dev), train=False)
    assert tuple(got.shape) == (B, G * D)
    _same(_bits(got), _pool_rows(r3, B * G, (L,), m3.reshape(B * G, L), "sum").reshape(B, G * D), "[B, G, L]")
    with pytest.raises(TypeError):
        emb.lookup(T(keys.astype(np.int32), dev), train=False)            # not the map's key dtype
    with pytest.raises(RuntimeError):
        emb.apply_(torch.zeros((B, F * D), device=dev))                   # no training lookup to apply


# ---- 2. the dense sibling as the apply's reference -----------------------------------------------------------------------------------
def _dense_twin(dev, m, emb, opt):
    """MultiHotEmbedding over CLONES of the map's value rows and slot tables (row number = id), with emb's hyper-parameters and powers"""
    from mindrec_amd.multi_hot import MultiHotEmbedding
    d = MultiHotEmbedding(m.capacity, emb.dim, emb.fields, mode=emb.mode, optimizer=opt, device=dev, **_HYP[opt])
    d.beta1_power, d.beta2_power = emb.beta1_power, emb.beta2_power
    return d


def _sync_dense(d, m, opt):
    d.table.copy_(m.values)
    for dst, name in zip(d.state, _SLOTS[opt]):
        dst.copy_(m.slots[name]["table"])


def _assert_tables(m, d, opt, what):
    assert np.array_equal(_bits(m.values), _bits(d.table)), what + ": values"
    for st, name in zip(d.state, _SLOTS[opt]):
        assert np.array_equal(_bits(m.slots[name]["table"]), _bits(st)), f"{what}: slot {name}"


def _step(emb, dense, m, opt, tk, tm, dy, what, after_lookup=None):
    """lookup(train=True) + apply_ on the hash side; the dense sibling from the tables as the lookup left them, by the admitted rows"""
    x = emb.lookup(tk, tm, train=True)
    if after_lookup is not None:
        after_lookup()
    _sync_dense(dense, m, opt)
    before = m.values.clone()
    dense.lookup(emb.rows, tm)
    emb.apply_(dy)
    dense.apply_(dy)
    assert (emb.beta1_power, emb.beta2_power) == (dense.beta1_power, dense.beta2_power)
    _assert_tables(m, dense, opt, what)
    return x, before


@pytest.mark.parametrize("opt,D,mode,lens", [("lazy_adam", 64, "mean", SIX), ("ftrl", 1, "sum", (21,)), ("lazy_adam", 6, "sum", (9,)),
                                             ("ftrl", 8, "mean", SIX)])
def test_apply_two_steps_under_the_permit_filter(dev, opt, D, mode, lens):
    """permit_filter_value = 2: in step 1 every key is seen for the first time -- it reads its default row and is left alone; in step 2
    the keys of step 1 are admitted and updated, the keys new in step 2 are not.  Slot 0 of the first two bags of every sample holds the
    same key (a key in several fields of one sample: one update from the summed gradient).  ("ftrl", 1, "sum", (21,)) is the wide side."""
    from mindrec_amd.multi_hot import MultiHotHashEmbedding
    rng = np.random.default_rng(D + len(lens))
    kdt, B, F, Ls = torch.int64, 37, len(lens), sum(lens)
    pool = _distinct_keys(rng, 120, kdt)
    m = _new_map(dev, kdt, D, permit_filter_value=2)
    emb = MultiHotHashEmbedding(m, bag=lens, mode=mode, optimizer=opt, **_HYP[opt])
    dense = _dense_twin(dev, m, emb, opt)
    keys1 = rng.choice(pool[:80], size=(B, Ls))
    keys1[:, min(lens[0], Ls - 1)] = keys1[:, 0]
    keys2 = np.where(rng.random((B, Ls)) < 0.25, rng.choice(pool[80:], size=(B, Ls)), keys1)
    mask = _masks(rng, B, Ls)[2]
    tm = T(mask, dev)
    dys = [T(rng.standard_normal((B, F * D)).astype(np.float32), dev) for _ in range(2)]
    # step 1
    x1, before = _step(emb, dense, m, opt, T(keys1, dev), tm, dys[0], "step 1")
    assert bool((emb.rows < 0).all()), "first-seen keys must not be admitted"
    assert torch.equal(m.values, before), "step 1 must leave every row alone"
    _same(_bits(x1), _pool_rows(_default_rows(dev, kdt, D, "normal", keys1), B, lens, mask, mode), "step 1 reads default rows")
    # step 2
    twin_rows = m.get(T(keys2.reshape(-1), dev), insert_default_value=False).cpu().numpy()      # (a probe: changes nothing)
    x2, before = _step(emb, dense, m, opt, T(keys2, dev), tm, dys[1], "step 2")
    _same(_bits(x2), _pool_rows(twin_rows, B, lens, mask, mode), "step 2 lookup")
    adm = emb.rows.cpu().numpy()
    new2 = ~np.isin(keys2, keys1)
    assert new2.any() and (adm[new2] < 0).all() and (adm[~new2] >= 0).all()
    changed = (m.values != before).any(dim=1).cpu().numpy()
    assert changed[np.unique(adm[adm >= 0])].any() and not changed[np.setdiff1d(np.arange(m.capacity), adm[adm >= 0])].any()
    assert m.step == 2 and emb.step_count == 2


@pytest.mark.parametrize("opt", ["lazy_adam", "ftrl"])
def test_full_table_drops_read_default_rows_and_are_not_updated(dev, opt):
    """capacity 256 and more distinct keys than that in one training lookup: the keys past the 256th (in order of first appearance)
    are dropped -- row -1 -- contribute their default rows to the sums and receive no update; the others match the dense sibling."""
    from mindrec_amd.multi_hot import MultiHotHashEmbedding
    rng = np.random.default_rng(77)
    kdt, D, lens, B = torch.int32, 8, (3, 5), 64
    F, Ls = len(lens), sum(lens)
    keys = rng.choice(_distinct_keys(rng, 420, kdt), size=(B, Ls))
    assert np.unique(keys).size > 256
    m = _new_map(dev, kdt, D, capacity=256)
    emb = MultiHotHashEmbedding(m, bag=lens, mode="mean", optimizer=opt, **_HYP[opt])
    dense = _dense_twin(dev, m, emb, opt)
    mask = _masks(rng, B, Ls)[1]
    dy = T(rng.standard_normal((B, F * D)).astype(np.float32), dev)
    x, before = _step(emb, dense, m, opt, T(keys, dev), T(mask, dev), dy, "full table")
    rows = emb.rows.cpu().numpy()
    # the first 256 distinct keys in order of first appearance hold rows 0 .. 255, every other key was dropped
    _, first = np.unique(keys.reshape(-1), return_index=True)
    kept = keys.reshape(-1)[np.sort(first)[:256]]
    assert np.array_equal(rows >= 0, np.isin(keys, kept)) and (rows < 0).any()
    hwm, live, dropped, _ = m.index.counters()
    assert (hwm, live) == (256, 256) and dropped == np.unique(keys).size - 256
    # every key, kept (a new row holds the default value) or dropped, read its default row
    _same(_bits(x), _pool_rows(_default_rows(dev, kdt, D, "normal", keys), B, lens, mask, "mean"), "dropped keys read default rows")
    assert bool((m.values != before).any())
    # ... and at evaluation the dropped keys still read their default rows, the kept ones their updated rows
    ref = m.get(T(keys.reshape(-1), dev), insert_default_value=False).cpu().numpy()
    _same(_bits(emb.lookup(T(keys, dev), T(mask, dev), train=False)), _pool_rows(ref, B, lens, mask, "mean"), "after the update")


def test_evicted_key_reads_and_trains_as_a_new_key(dev):
    from mindrec_amd.multi_hot import MultiHotHashEmbedding
    rng = np.random.default_rng(3)
    kdt, D, lens, B, opt = torch.int64, 8, (2, 3), 37, "lazy_adam"
    F, Ls = len(lens), sum(lens)
    pool = _distinct_keys(rng, 100, kdt)
    ka, kb = rng.choice(pool[:50], size=(B, Ls)), rng.choice(pool[50:], size=(B, Ls))
    m = _new_map(dev, kdt, D, evict_filter_value=1)
    emb = MultiHotHashEmbedding(m, bag=lens, mode="sum", optimizer=opt, **_HYP[opt])
    dense = _dense_twin(dev, m, emb, opt)
    dy = T(rng.standard_normal((B, F * D)).astype(np.float32), dev)
    dflt = _pool_rows(_default_rows(dev, kdt, D, "normal", ka), B, lens, None, "sum")
    x, _ = _step(emb, dense, m, opt, T(ka, dev), None, dy, "step 1")
    _same(_bits(x), dflt, "new keys")
    trained = emb.lookup(T(ka, dev), train=False)
    assert not np.array_equal(_bits(trained), dflt.view(np.uint32)), "step 1 must have moved the rows of A"
    for s in (2, 3):                                                     # A goes stale: two training steps without it
        _step(emb, dense, m, opt, T(kb, dev), None, dy, f"step {s}")
    nA = np.unique(ka).size
    assert m.evict() == nA and len(m) == np.unique(kb).size
    _same(_bits(emb.lookup(T(ka, dev), train=False)), dflt, "an evicted key reads its default row")

    def fresh_slots():                                                   # the rows A holds now were handed out again: zero moments
        rows = emb.rows.reshape(-1).long()
        assert bool((rows >= 0).all())
        assert not m.slots["moment1"]["table"][rows].any() and not m.slots["moment2"]["table"][rows].any()

    x, before = _step(emb, dense, m, opt, T(ka, dev), None, dy, "step 4", after_lookup=fresh_slots)      # ... and trains as a new key
    _same(_bits(x), dflt, "an evicted key seen again reads as a new key")
    assert len(m) == np.unique(kb).size + nA and bool((m.values != before).any())


def test_probe_lookup_captured(dev):
    """lookup(train=False) in a HIP graph: the replay equals the eager result, and follows the table (the graph holds no copy)"""
    from mindrec_amd.multi_hot import MultiHotHashEmbedding
    rng = np.random.default_rng(9)
    kdt, D, lens, B, R = torch.int64, 64, SIX, 37, 200
    F, Ls = len(lens), sum(lens)
    allk = _distinct_keys(rng, 2 * R, kdt)
    m = _new_map(dev, kdt, D)
    m.put(T(allk[:R], dev), T(rng.standard_normal((R, D)).astype(np.float32), dev))
    emb = MultiHotHashEmbedding(m, bag=lens, mode="mean")
    tk, tm = T(rng.choice(allk, size=(B, Ls)), dev), T(_masks(rng, B, Ls)[1], dev)
    eager = emb.lookup(tk, tm, train=False).clone()
    out = torch.zeros((B, F * D), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        emb.lookup(tk, tm, out=out, train=False)
    torch.cuda.synchronize()
    assert not out.any()                                                  # (capture ran nothing)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(eager))
    m.values.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(emb.lookup(tk, tm, train=False)))
