"""The key index and the step's plan through the pieces their host and device layers share: the tile scan of mrec_common.h past one
look-back round (65 x 2048 + 1 items: 66 tiles, one more than the 64 a round reads, the last one ragged) in each kernel that runs it --
the plan's rank kernel, the lookup chain's place kernel, evict -- and the entries that go through FindWs / rank_flags / launch_rebuild /
by_key.  References: numpy for the plan (first-occurrence Unique, stable argsort: plan_ref of tests/_plan_cases.py),
tests/_map_model.py for the index; everything is an integer and compared exactly.  Already held elsewhere and not repeated: the place kernel past the look-back window for BOTH key widths
at 69 tiles (tests/test_map_edges_gpu.py::test_many_tiles_past_the_lookback_window -- the int64 case below is the issue's size, with the
counters and the export on top); evict, reuse and rebuild at small capacities (::test_evict_then_reuse_and_rebuild); the refusals
(tests/test_map_plan_abi.py)."""
import numpy as np
import pytest
import torch

from _map_model import MapModel
from _plan_cases import T, check_plan

pytestmark = pytest.mark.gpu

N66 = 65 * 2048 + 1


def ids_with_firsts_in_every_tile(rng, n, dtype):
    ids = np.arange(n, dtype=np.int64) * 7 + 3
    dup = np.flatnonzero(rng.random(n) < 0.4)
    dup = dup[dup > 0]
    ids[dup] = ids[(rng.random(dup.size) * dup).astype(np.int64)]      # a copy of some earlier position (perhaps itself a copy)
    first = np.unique(ids, return_index=True)[1]
    assert np.unique(first // 2048).size == (n + 2047) // 2048
    return ids.astype(dtype)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_plan_past_one_lookback_round(dev, dtype):
    from mindrec_amd import ops
    rng = np.random.default_rng(66)
    ids = ids_with_firsts_in_every_tile(rng, N66, dtype)
    sfx = "i32" if dtype == np.int32 else "i64"
    primed = lambda: [k for k in ops._PLAN_PRIMED if k[1:] == (N66, sfx)]
    for k in primed():
        del ops._PLAN_PRIMED[k]                          # (whoever planned this n before: the first call below starts unprimed)
    check_plan(ops, dev, ids)
    assert len(primed()) == 1                            # ... and the second runs with MREC_PLAN_WS_PRIMED
    check_plan(ops, dev, ids[::-1].copy())
    pad = ids.copy()
    pad[[0, 5, 2047, N66 - 1, N66 - 700]] = -1           # padding in the first and in the last tile
    pad[rng.integers(0, N66, 1000)] = -1
    check_plan(ops, dev, pad, skip_negative=True)
    check_plan(ops, dev, ids)                            # and the workspace it left is still a primed one


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049])
def test_plan_at_tile_edges(dev, dtype, n):
    from mindrec_amd import ops
    rng = np.random.default_rng(n)
    ids = rng.integers(0, max(n // 2, 1), size=n).astype(dtype)
    check_plan(ops, dev, ids)
    check_plan(ops, dev, ids)                            # primed
    pad = ids.copy()
    pad[[0, n - 1]] = -1
    check_plan(ops, dev, pad, skip_negative=True)


def counters(ki):
    c = ki.counters_all()
    return c[:5] + (c[6],)


def test_lookup_past_one_lookback_round(dev):
    from mindrec_amd import ops
    rng = np.random.default_rng(67)
    keys = rng.permutation(np.arange(1, 4 * N66, dtype=np.int64))[:N66] * 1000003
    keys[rng.integers(0, N66, N66 // 8)] = keys[rng.integers(0, N66, N66 // 8)]
    ki, m = ops.KeyIndex(N66, dev), MapModel(N66)
    rows = ki.lookup(T(keys, dev), insert=True, train=True, step=3)
    torch.cuda.synchronize()
    ref, _ = m.lookup(keys, True, True, 3, 1)
    assert np.array_equal(rows.cpu().numpy(), ref)
    assert counters(ki)[:4] == m.counters()[:4] and m.live > 100000
    k, r = ki.export()
    mk, mr = m.export()
    assert np.array_equal(k.cpu().numpy(), mk) and np.array_equal(r.cpu().numpy(), mr)


def test_evict_past_one_lookback_round(dev):
    from mindrec_amd import ops
    C = N66
    keys = np.arange(C, dtype=np.int64) * 11 + 5
    ki, m = ops.KeyIndex(C, dev), MapModel(C)
    rows = ki.lookup(T(keys, dev), insert=True, train=True, step=1).cpu().numpy()
    assert np.array_equal(rows, m.lookup(keys, True, True, 1, 1)[0]) and np.array_equal(rows, np.arange(C))
    fresh = keys[(np.arange(C) % 3 != 0) & (np.arange(C) != C - 1)]          # every third row and the last row stay stale
    ki.lookup(T(fresh, dev), insert=False, train=True, step=10)
    m.lookup(fresh, False, True, 10, 1)
    ki.export_dirty(clear=True)
    m.export_dirty(True)
    n_ev = ki.evict(10, 5)
    torch.cuda.synchronize()
    assert int(n_ev.item()) == m.evict(10, 5) == (C + 2) // 3 + 1
    assert counters(ki) == m.counters()                  # 44375 tombstones of 262144 slots: no rebuild
    k, r, s = ki.export_dirty(clear=False)               # the erased-keys log, in row order behind the (no) modified rows
    mk, mr, ms = m.export_dirty(False)
    assert np.array_equal(k.cpu().numpy(), mk) and np.array_equal(r.cpu().numpy(), mr) and np.array_equal(s.cpu().numpy(), ms)
    assert mk.size == (C + 2) // 3 + 1 and int(mk[-1]) == int(keys[C - 1])
    # the free list's order: the table has no fresh row left, so new keys take it from its top
    new = np.arange(5000, dtype=np.int64) * 11 + 6
    got = ki.lookup(T(new, dev), insert=True, train=True, step=11).cpu().numpy()
    assert np.array_equal(got, m.lookup(new, True, True, 11, 1)[0]) and got[0] == C - 1 and got[1] == C - 1 - (C - 1) % 3
    assert counters(ki)[:4] == m.counters()[:4]


def test_find_erase_rebuild_export_on_one_index(dev):
    from mindrec_amd import ops
    ki, m = ops.KeyIndex(300, dev), MapModel(300)
    assert ki.n_slots == 1024
    keys = np.arange(300, dtype=np.int64) * 97 + 13
    rows, is_new = ki.find_or_insert(T(keys, dev))
    assert np.array_equal(rows.cpu().numpy(), m.lookup(keys, True, False, 0, 0)[0]) and bool(is_new.all())
    gone, stay = keys[40:245], np.concatenate([keys[:40], keys[245:]])
    ki.erase(T(gone[:204], dev))
    assert not m.erase(gone[:204]) and counters(ki) == m.counters() == (300, 96, 0, 204, 204, 0)      # 204 * 5 <= 1024
    ki.erase(T(np.concatenate([gone[204:], [7, 8]]), dev))                   # the 205th tombstone: 1025 > 1024 (two keys are not there)
    assert m.erase(gone[204:]) and counters(ki) == m.counters() == (300, 95, 0, 205, 0, 1)
    krow = ki.slots()[1].cpu().numpy()
    assert (krow == -2).sum() == 0 and (krow >= 0).sum() == 95               # the rebuild emptied every tombstone
    rows, is_new = ki.find_or_insert(T(keys, dev), insert=False)
    ref = m.lookup(keys, False, False, 0, 0)[0]
    assert np.array_equal(rows.cpu().numpy(), ref) and (ref[40:245] == -1).all() and (ref[:40] >= 0).all() and not bool(is_new.any())
    new = np.arange(50, dtype=np.int64) * 97 + 14
    both = np.concatenate([stay[:10], new])
    rows, is_new = ki.find_or_insert(T(both, dev))
    assert np.array_equal(rows.cpu().numpy(), m.lookup(both, True, False, 0, 0)[0])
    assert np.array_equal(is_new.cpu().numpy(), np.r_[np.zeros(10, np.uint8), np.ones(50, np.uint8)])
    assert counters(ki)[:4] == m.counters()[:4] == (300, 145, 0, 155)
    k, r = ki.export()
    mk, mr = m.export()
    assert np.array_equal(k.cpu().numpy(), mk) and np.array_equal(r.cpu().numpy(), mr)


def test_export_dirty_around_mark_dirty_and_erase(dev):
    from mindrec_amd import ops
    ki, m = ops.KeyIndex(300, dev), MapModel(300)
    keys = np.arange(100, dtype=np.int64) * 31 + 1
    ki.lookup(T(keys, dev), insert=True, train=True, step=1)
    m.lookup(keys, True, True, 1, 1)

    def same(clear):
        got, ref = ki.export_dirty(clear=clear), m.export_dirty(clear)
        for g, r in zip(got, ref):
            assert np.array_equal(g.cpu().numpy(), r)
        return ref[0].size

    assert same(True) == 100 and same(True) == 0
    ki.mark_dirty(T(np.array([3, 5, -1, 300, 77], np.int32), dev))           # rows outside the table are nobody's
    m.dirty[[3, 5, 77]] = 1
    ki.erase(T(keys[[5, 10, 11]], dev))
    m.erase(keys[[5, 10, 11]])
    assert same(False) == 5 and same(False) == 5                            # rows 3 and 77 modified; keys 5, 10, 11 erased
    assert same(True) == 5 and same(True) == 0
    ki.lookup(T(keys[[10]], dev), insert=True, train=False, step=2)          # erased, then back: modified only
    m.lookup(keys[[10]], True, False, 2, 1)
    assert same(True) == 1


def test_put_rows_last_and_fill_missing(dev):
    from mindrec_amd import ops
    table = torch.zeros((10, 4), device=dev)
    winner = torch.full((10,), -1, dtype=torch.int32, device=dev)
    rows = T(np.array([2, 5, 2, -1, 7, 2], np.int32), dev)
    vals = torch.arange(24, dtype=torch.float32, device=dev).reshape(6, 4) + 1
    ops.put_rows_last_(table, rows, vals, winner)
    ref = np.zeros((10, 4), np.float32)
    ref[5], ref[7], ref[2] = vals[1].cpu().numpy(), vals[4].cpu().numpy(), vals[5].cpu().numpy()      # the last of the three wins
    assert np.array_equal(table.cpu().numpy(), ref) and bool((winner == -1).all())
    ki = ops.KeyIndex(64, dev)
    kv = np.array([5, -7, 123456, 2 ** 31 - 1, -2 ** 31, 0, 99], np.int64)
    found = T(np.array([-1, -1, 3, -1, -1, -1, 0], np.int32), dev)
    outs = []
    for dt in (np.int32, np.int64):
        out = torch.full((7, 6), 9.0, device=dev)
        ki.fill_missing(T(kv.astype(dt), dev), found, out, 0.05, None, 11)
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and (outs[0][[2, 6]] == 9.0).all() and (outs[0][[0, 1, 3, 4, 5]] != 9.0).all()
