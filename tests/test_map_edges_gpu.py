"""The MapParameter key index (csrc/mrec_hash.hip) held to the sequential host model of tests/_map_model.py at its edges: the
three-launch lookup chain (probe -> place -> finish) on tables that fill up, reuse rows and hold tombstones, with n_dev, unique
keys, padding keys and lookup(out=...); eviction followed by reuse and a rebuild; the argument checks of the chain.

Every comparison is exact and is made after EVERY call (`Pair.check`): rows, admitted rows, counter words 0-4 and 6, the per-row
hits / last step / dirty arrays, the keys of live rows, the full export, the slot array (every live key in exactly one slot, as
many tombstones as word 4 says, the slots the model says are taken) and every row of every table (default rows of new keys from
the oracle's generator, all other rows untouched)."""
import numpy as np
import pytest
import torch

from _map_model import MapModel, fill_slots, home_slot

pytestmark = pytest.mark.gpu

SENT = 7.0            # what a table row holds before any key owns it
MODES = ["positions", "unique"]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Pair:
    """A KeyIndex with two tables (values: normal default rows, D = 4, the 16-byte store path; a slot table: constant fill, D = 3,
    the scalar path) and the model, driven together."""

    SEED, SIGMA, FILL = 11, 0.02, 0.5

    def __init__(self, cap, dev, oracle, key_dtype):
        from mindrec_amd import ops
        self.ops, self.dev, self.oracle, self.kd = ops, dev, oracle, key_dtype
        self.ki = ops.KeyIndex(cap, dev)
        self.m = MapModel(cap)
        assert self.ki.n_slots == self.m.S
        self.vals = torch.full((cap, 4), SENT, device=dev)
        self.slot = torch.full((cap, 3), SENT, device=dev)
        self.tables = [(self.vals, self.SIGMA, None, self.SEED), (self.slot, None, self.FILL, 0)]
        self.ref_vals = np.full((cap, 4), SENT, np.float32)
        self.ref_slot = np.full((cap, 3), SENT, np.float32)

    def slot_rows(self):
        return self.ki.slots()[1].cpu().numpy()

    def lookup(self, keys, insert=True, train=False, step=0, permit=1, n_valid=None, skip_pad=False, unique=False, dedup=False):
        """dedup: the keys go through ops.unique first and its output (buffer + device count) is what the index is given"""
        keys = np.asarray(keys, self.kd)
        if dedup:
            d = self.ops.unique(T(keys, self.dev))
            tk, n_dev, unique = d.uniq_buf, d.n_uniq_dev, True
            keys, n_valid = tk.cpu().numpy(), int(n_dev.item())
        else:
            tk = T(keys, self.dev)
            n_dev = None if n_valid is None else torch.tensor([n_valid], dtype=torch.int64, device=self.dev)
        before = self.slot_rows() if insert else None
        rows, adm = self.ki.lookup(tk, insert=insert, unique=unique, train=train, step=step, permit=permit, tables=self.tables if insert else (),
                                   n_dev=n_dev, want_admitted=True, skip_pad=skip_pad)
        mrows, madm = self.m.lookup(keys, insert, train, step, permit, n_valid=n_valid, skip_pad=skip_pad)
        taken = None
        if insert:
            nk = np.array(self.m.new_keys, np.int64)
            taken, reused = fill_slots(before, home_slot(nk, np.int64, self.m.S), rows=self.m.new_rows)
            self.m.tombstones_reused(reused)
            if nk.size:
                self.ref_vals[self.m.new_rows] = self.oracle.normal_rows(self.SEED, nk, 4, self.SIGMA)
                self.ref_slot[self.m.new_rows] = self.FILL
        rows, adm = rows.cpu().numpy(), adm.cpu().numpy()
        assert np.array_equal(rows, mrows), np.flatnonzero(rows != mrows)[:10]
        assert np.array_equal(adm, madm), np.flatnonzero(adm != madm)[:10]
        self.check(taken)
        return rows

    def erase(self, keys):
        self.ki.erase(T(np.asarray(keys, np.int64), self.dev))
        self.m.erase(keys)
        self.check()

    def evict(self, step, threshold):
        got = int(self.ki.evict(step, threshold).item())
        want = self.m.evict(step, threshold)
        assert got == want
        self.check()
        return got

    def export_dirty(self, clear=True):
        k, r, s = (x.cpu().numpy() for x in self.ki.export_dirty(clear=clear))
        mk, mr, ms = self.m.export_dirty(clear)
        assert np.array_equal(k, mk) and np.array_equal(r, mr) and np.array_equal(s, ms)
        self.check()
        return k, r, s

    def check(self, taken=None):
        m, ki = self.m, self.ki
        c = ki.counters_all()
        assert (c[0], c[1], c[2], c[3], c[4], c[6]) == m.counters(), (c, m.counters())
        hits, last, dirty = (x.cpu().numpy() for x in ki.tracking())
        assert np.array_equal(hits, m.hits) and np.array_equal(last, m.last_step) and np.array_equal(dirty, m.dirty)
        live = m.live_rows()
        assert np.array_equal(ki.row_keys().cpu().numpy()[live], m.row_key[live])
        k, r = ki.export()
        mk, mr = m.export()
        assert np.array_equal(k.cpu().numpy(), mk) and np.array_equal(r.cpu().numpy(), mr)
        sk, sr = (x.cpu().numpy() for x in ki.slots())
        held = np.flatnonzero(sr >= 0)
        o = np.argsort(sr[held])
        assert np.array_equal(sr[held][o], live) and np.array_equal(sk[held][o], m.row_key[live])        # every live key in one slot
        assert int((sr == -2).sum()) == m.tomb and int((sr < -2).sum()) == 0
        if taken is not None:
            assert np.array_equal(sr >= 0, taken >= 0) and np.array_equal(sr == -2, taken == -2)
        assert np.array_equal(self.vals.cpu().numpy(), self.ref_vals) and np.array_equal(self.slot.cpu().numpy(), self.ref_slot)


def _distinct(rng, n, key_dtype, lo=1000):
    """n distinct keys of the dtype's range, none of the special values the tests add by hand"""
    hi = 2 ** 31 - 1 if key_dtype == np.int32 else 2 ** 62
    k = np.unique(rng.integers(lo, hi, size=2 * n + 64))
    k = k[k != 0x7F7F7F7F]
    assert k.size >= n
    return rng.permutation(k)[:n].astype(key_dtype)


def _churned(p, rng, key_dtype):
    """capacity 3000: 2500 rows filled, 700 of them erased again (500 fresh rows + 700 on the free list)"""
    res = _distinct(rng, 2500, key_dtype)
    p.lookup(res, dedup=False)
    p.erase(res[100:2200:3])
    assert p.m.counters()[:4] == (2500, 1800, 0, 700)
    return np.delete(res, np.arange(100, 2200, 3))


def _straddle_keys(rng, resident, key_dtype, unique):
    """5000 positions = 3 tiles of 2048: ~1500 distinct new keys whose first occurrences lie in all three tiles, each with
    later copies, between resident keys (`unique`: 5000 distinct keys, every resident one and 3200 new ones)"""
    new = _distinct(rng, 5200 if unique else 1500, key_dtype, lo=2 ** 30)
    new = new[~np.isin(new, resident)]
    if unique:
        keys = rng.permutation(np.concatenate([new[:5000 - resident.size], resident]))
    else:
        keys = rng.choice(resident, size=5000)
        at = np.sort(rng.choice(5000, size=new.size, replace=False))            # first occurrences, spread over the tiles
        keys[at] = new
        rest = np.setdiff1d(np.arange(5000), at)
        dup = rng.choice(rest, size=1200, replace=False)                         # later copies, anywhere behind the first occurrence
        src = rng.integers(0, new.size, size=1200)
        ok = dup > at[src]
        keys[dup[ok]] = new[src[ok]]
        assert (at < 2048).any() and (at >= 4096).any() and np.unique(keys[dup[ok]]).size > 300
    assert keys.size == 5000
    return keys.astype(key_dtype)


def _scratch_is_clean(dev, n):
    """The lookup workspace of problem size n between two calls, as LookupWs of mrec_hash.hip lays it out: the position-valued
    scratch table first, every word 'empty'; the look-back words behind srank / sidx / newrow / newkey, all zero.  (A scratch
    slot left behind answers the next call of the same size consistently -- it names a position of that call's own keys -- so
    only exhaustion would show it: it is looked at directly.)"""
    from mindrec_amd import _lib, ops
    al = lambda b: (b + 255) // 256 * 256
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    ws = ops.workspace(f"maplookup:{n}", _lib.query_bytes("mrec_map_lookup_workspace_bytes", n), dev)
    off = 2 * al(4 * cap) + 2 * al(4 * n) + al(8 * n)
    status = ws[off: off + 4 * ((n + 2047) // 2048)].view(torch.int32)
    return bool((ws[: 4 * cap].view(torch.int32) == 0x7F7F7F7F).all()) and bool((status == 0).all())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key_dtype", [np.int32, np.int64])
def test_straddle_and_drop_across_tiles(dev, oracle, key_dtype, mode):
    """One lookup whose new keys use up the 500 fresh rows, pop all 700 free rows and are dropped from there on, their ranks
    crossing two tile boundaries; the same call again on the now primed workspace (scratch table and look-back words handed
    back clean after a call that dropped keys) must answer the same."""
    rng = np.random.default_rng(31)
    p = Pair(3000, dev, oracle, key_dtype)
    resident = _churned(p, rng, key_dtype)
    keys = _straddle_keys(rng, resident, key_dtype, unique=False)
    dd = mode == "unique"
    rows = p.lookup(keys, train=True, step=1, permit=2, dedup=dd)
    hwm, live, dropped, free = p.m.counters()[:4]
    assert (hwm, live, free) == (3000, 3000, 0) and dropped > 100 and (rows == -1).sum() >= dropped
    new = np.array(p.m.new_rows)
    assert np.array_equal(new[:500], np.arange(2500, 3000)) and np.unique(new[500:]).size == 700        # fresh first, then the free rows
    assert _scratch_is_clean(dev, 5000)
    again = p.lookup(keys, train=True, step=1, permit=2, dedup=dd)
    assert _scratch_is_clean(dev, 5000)
    assert np.array_equal(again, rows) and p.m.counters()[:4] == (3000, 3000, 2 * dropped, 0)
    p.lookup(keys, insert=False, train=True, step=2, permit=2, dedup=dd)            # second hit: the kept keys are admitted now


@pytest.mark.parametrize("key_dtype", [np.int32, np.int64])
def test_straddle_find_or_insert_path(dev, oracle, key_dtype):
    """the older five-launch path on the same shape (unique keys; it keeps no per-row tracking, so rows, counters, slots and the
    export are what is compared)"""
    from mindrec_amd import ops
    rng = np.random.default_rng(32)
    ki, m = ops.KeyIndex(3000, dev), MapModel(3000)

    def step(keys, insert=True):
        before = ki.slots()[1].cpu().numpy()
        rows, is_new = ki.find_or_insert(T(keys.astype(np.int64), dev), insert=insert)
        mrows, _ = m.lookup(keys, insert, False, 0, 1)
        taken, reused = fill_slots(before, home_slot(m.new_keys, np.int64, m.S), rows=m.new_rows)
        m.tombstones_reused(reused)
        assert np.array_equal(rows.cpu().numpy(), mrows)
        isn = np.zeros(keys.size, bool)
        isn[np.isin(keys, np.array(m.new_keys, np.int64))] = True
        assert np.array_equal(is_new.cpu().numpy().astype(bool), isn)
        c = ki.counters_all()
        assert (c[0], c[1], c[2], c[3], c[4], c[6]) == m.counters()
        k, r = ki.export()
        assert np.array_equal(k.cpu().numpy(), m.export()[0]) and np.array_equal(r.cpu().numpy(), m.export()[1])
        sr = ki.slots()[1].cpu().numpy()
        assert np.array_equal(sr >= 0, taken >= 0) and int((sr == -2).sum()) == m.tomb

    res = _distinct(rng, 2500, key_dtype)
    step(res)
    gone = res[100:2200:3]
    ki.erase(T(gone.astype(np.int64), dev)); m.erase(gone)
    step(_straddle_keys(rng, np.delete(res, np.arange(100, 2200, 3)), key_dtype, unique=True))
    assert m.counters()[:2] == (3000, 3000) and m.dropped > 100 and not m.free


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key_dtype", [np.int32, np.int64])
def test_n_dev_at_tile_boundaries(dev, oracle, key_dtype, mode):
    """Only the first n_dev positions count: the keys behind them are new and must stay out.  n_dev = 0, 1, one short of a tile,
    a tile, one more, all -- the last call straddles fresh rows, free rows and the full table."""
    rng = np.random.default_rng(33)
    p = Pair(3000, dev, oracle, key_dtype)
    resident = _churned(p, rng, key_dtype)
    keys = _straddle_keys(rng, resident, key_dtype, unique=(mode == "unique"))
    for nd in (0, 1, 2047, 2048, 2049, 5000):
        live0 = p.m.live
        rows = p.lookup(keys, train=True, step=nd + 1, permit=2, n_valid=nd, unique=(mode == "unique"))
        assert (rows[nd:] == -1).all() and p.m.live - live0 == len(p.m.new_keys)
    assert p.m.counters()[0] == 3000 and p.m.dropped > 100 and not p.m.free
    behind = _distinct(rng, 64, key_dtype, lo=2 ** 29)
    p.lookup(np.concatenate([resident[:10], behind]), n_valid=10, unique=True)                            # a full table changes nothing here
    assert (p.lookup(behind, insert=False) == -1).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key_dtype", [np.int32, np.int64])
def test_padding_key_and_ordinary_odd_keys(dev, oracle, key_dtype, mode):
    """skip_pad: key -1 is nobody's key wherever it sits (first, last, either side of both tile boundaries).  Without it -1 is
    a key like any other, as are 0, -2, the extremes of the dtype and the value the scratch table uses for 'empty'."""
    rng = np.random.default_rng(34)
    dd = mode == "unique"
    p = Pair(3000, dev, oracle, key_dtype)
    resident = _churned(p, rng, key_dtype)
    keys = _straddle_keys(rng, resident, key_dtype, unique=False)
    keys[[0, 2047, 2048, 4095, 4096, 4999]] = -1
    keys[rng.choice(5000, size=40, replace=False)] = -1
    rows = p.lookup(keys, train=True, step=1, skip_pad=True, dedup=dd)
    placed = list(p.m.new_keys)
    assert -1 not in p.m.row_of and p.m.counters()[:4] == (3000, 3000, p.m.dropped, 0) and p.m.dropped > 100
    if not dd:
        assert (rows[keys == -1] == -1).all()
    assert (p.lookup(np.array([-1], key_dtype), insert=False) == -1).all()
    # the table is full now: make room, then the odd keys are ordinary
    p.erase(np.array(placed[:50], np.int64))                     # (the first new keys got the fresh rows 2500, 2501, ...)
    info = np.iinfo(key_dtype)
    odd = np.array([-1, 0, -2, info.min, info.max, 0x7F7F7F7F], key_dtype)
    k2 = np.concatenate([odd, resident[:30].astype(key_dtype), odd[::-1]])
    rows = p.lookup(k2, train=True, step=2, dedup=dd)
    assert all(int(k) in p.m.row_of for k in odd) and p.m.new_rows == [2549, 2548, 2547, 2546, 2545, 2544]       # the stack's top
    p.lookup(odd, insert=False, skip_pad=True, dedup=dd)                                                   # -1 is in the table and still skipped
    p.erase(odd.astype(np.int64))
    assert (p.lookup(odd, insert=False) == -1).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key_dtype", [np.int32, np.int64])
def test_many_tiles_past_the_lookback_window(dev, oracle, key_dtype, mode):
    """69 tiles: more than the 64 tiles one look-back step of the place kernel's scan covers"""
    rng = np.random.default_rng(35)
    p = Pair(160000, dev, oracle, key_dtype)
    n = 140001
    keys = _distinct(rng, n, key_dtype)
    src = rng.integers(0, n, size=n // 8)
    keys[rng.integers(0, n, size=n // 8)] = keys[src]                            # ~12% repeats, anywhere
    p.lookup(keys, dedup=(mode == "unique"))
    assert p.m.live > 110000 and p.m.counters()[0] == p.m.live
    p.lookup(keys[::-1].copy(), insert=False, dedup=(mode == "unique"))


_CLUSTERS = {}


def _cluster_keys(S, key_dtype):
    """keys whose probes start in the last three slots (their cluster wraps to slot 0) and keys that all start at slot S / 2"""
    if S not in _CLUSTERS:
        cand = np.arange(1, 150000, dtype=np.int64)
        home = home_slot(cand, np.int64, S)                # the index hashes the widened key
        _CLUSTERS[S] = (cand[home >= S - 3], cand[home == S // 2])
    wrap, one = _CLUSTERS[S]
    assert wrap.size >= 50 and one.size >= 50
    return wrap.astype(key_dtype), one.astype(key_dtype)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key_dtype", [np.int32, np.int64])
def test_collision_cluster_with_wrap_around(dev, oracle, key_dtype, mode):
    dd = mode == "unique"
    p = Pair(400, dev, oracle, key_dtype)
    S = p.m.S
    assert S == 1024
    wrap, one = _cluster_keys(S, key_dtype)
    first = np.concatenate([wrap[:40], one[:40]])
    p.lookup(np.concatenate([first, first[::7]]) if not dd else first, dedup=dd)
    # where the keys sit: the host restatement of the hash, and the wrap
    sk, sr = (x.cpu().numpy() for x in p.ki.slots())
    at = {int(k): s for s, (k, r) in enumerate(zip(sk.tolist(), sr.tolist())) if r >= 0}
    home = dict(zip(first.tolist(), home_slot(first, np.int64, S).tolist()))
    dist = {int(k): (at[int(k)] - home[int(k)]) & (S - 1) for k in first}
    assert max(dist.values()) <= 40 + 3
    assert sorted(at[int(k)] for k in wrap[:40]) == list(range(37)) + [S - 3, S - 2, S - 1]            # the chain wraps
    assert sorted(at[int(k)] for k in one[:40]) == list(range(S // 2, S // 2 + 40))
    # the first 20 of each chain leave: the 20 behind the tombstones are still found
    chain_w = sorted((int(k) for k in wrap[:40]), key=lambda k: (at[k] - (S - 3)) & (S - 1))
    chain_o = sorted((int(k) for k in one[:40]), key=lambda k: at[k])
    p.erase(np.array(chain_w[:20] + chain_o[:20], np.int64))
    assert p.m.tomb == 40
    rows = p.lookup(np.array(chain_w[20:] + chain_o[20:] + chain_w[:20], key_dtype), insert=False, dedup=dd)
    assert (rows[:40] >= 0).all() and (rows[40:60] == -1).all()
    # ten new keys per chain with the same homes: each takes a tombstone back (fresh rows remain, so the free list is not touched)
    p.lookup(np.concatenate([wrap[40:50], one[40:50]]), dedup=dd)
    assert p.m.tomb == 20 and p.m.counters()[:4] == (100, 60, 0, 40)
    # a live key from deep in a chain, looked up by an INSERTING lookup: found behind the tombstones, not inserted twice
    sr = p.slot_rows()
    deep = chain_o[-1]
    assert at[deep] == S // 2 + 39 and (sr[S // 2: at[deep]] == -2).sum() == 10
    live0, row0 = p.m.live, p.m.row_of[deep]
    rows = p.lookup(np.array([deep, deep], key_dtype), dedup=dd)
    assert (rows[:1 if dd else 2] == row0).all() and p.m.live == live0 and not p.m.new_keys
    k, _ = p.ki.export()
    assert np.unique(k.cpu().numpy()).size == k.numel() == live0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key_dtype", [np.int32, np.int64])
def test_evict_then_reuse_and_rebuild(dev, oracle, key_dtype, mode):
    """capacity 5000 = 3 evict tiles, 16384 slots.  Four training steps, then an eviction of more than S / 5 rows (the slot array
    is rebuilt), reuse of the evicted rows from the highest down, the incremental export, and a small eviction that leaves
    tombstones."""
    rng = np.random.default_rng(36)
    dd = mode == "unique"
    p = Pair(5000, dev, oracle, key_dtype)
    K = _distinct(rng, 5600, key_dtype)

    def batch(lo, hi, extra=()):
        pool = np.concatenate([K[lo:hi], np.asarray(extra, key_dtype)])
        return np.concatenate([pool, rng.choice(pool, size=pool.size // 2)])[rng.permutation(pool.size + pool.size // 2)]

    p.lookup(batch(0, 3500), train=True, step=1, permit=2, dedup=dd)
    p.lookup(batch(3000, 4500), train=True, step=2, permit=2, dedup=dd)
    p.lookup(batch(4200, 4900), train=True, step=3, permit=2, dedup=dd)
    p.lookup(batch(4400, 5000, K[:100]), train=True, step=4, permit=2, dedup=dd)
    assert p.m.counters()[:4] == (5000, 5000, 0, 0)
    p.export_dirty(clear=True)
    c0 = p.m.counters()
    gone_rows = [r for r in range(5000) if 4 - p.m.last_step[r] > 1]
    gone_keys = [int(p.m.row_key[r]) for r in gone_rows]
    n_ev = p.evict(4, 1)
    assert n_ev == len(gone_rows) == 4100 and n_ev * 5 > p.m.S
    assert p.m.counters()[4:] == (0, c0[5] + 1) and p.m.free == gone_rows
    rows = p.lookup(K[:5000], insert=False, dedup=dd)                                  # survivors found, evicted keys miss
    if not dd:
        assert np.array_equal(rows >= 0, ~np.isin(K[:5000], np.array(gone_keys, key_dtype)))
    # the next inserts get the evicted rows, the highest first; their counters start afresh
    back = np.array(gone_keys[10:110], key_dtype)
    fresh = np.concatenate([K[5000:5200], back])
    p.lookup(np.concatenate([fresh, fresh[::3]]) if not dd else fresh, train=True, step=5, permit=2, dedup=dd)
    assert p.m.new_rows == gone_rows[::-1][:300]
    assert (p.m.hits[p.m.new_rows] == 1).all() and (p.m.last_step[p.m.new_rows] == 5).all()
    k, r, s = p.export_dirty(clear=True)
    assert k[s == 2].tolist() == [g for g in gone_keys if g not in set(back.tolist())]
    assert sorted(k[s == 1].tolist()) == sorted(int(x) for x in fresh)
    # a small eviction: tombstones stay, no rebuild
    p.lookup(K[4500:5000], insert=False, train=True, step=6, permit=2, dedup=dd)
    c1 = p.m.counters()
    n2 = p.evict(6, 0)
    assert 0 < n2 == c1[1] - 500 and n2 * 5 <= p.m.S and p.m.counters()[4:] == (n2, c1[5])
    assert (p.lookup(K[4500:5000], insert=False, dedup=dd) >= 0).all()


@pytest.mark.parametrize("D", [8, 6])
@pytest.mark.parametrize("key_dtype", [np.int32, np.int64])
def test_get_on_a_full_table_reads_default_rows(dev, oracle, key_dtype, D):
    """MapTensorGet over more keys than the table holds: every position reads its key's default row, kept (the new row holds it)
    or dropped (no row holds it: read, not stored -- as an un-admitted key).  D = 8 is the lookup(out=...) path, D = 6 the
    lookup + gather path."""
    from mindrec_amd.experimental import MapParameter
    rng = np.random.default_rng(37)
    tdt = torch.int32 if key_dtype == np.int32 else torch.int64
    mp = MapParameter(key_dtype=tdt, value_shape=(D,), capacity=64, device=dev, seed=5)
    m = MapModel(64)
    pool = _distinct(rng, 100, key_dtype)
    keys = np.concatenate([pool, rng.choice(pool, size=50)])[rng.permutation(150)]
    want = oracle.normal_rows(5, keys.astype(np.int64), D, 0.01)
    got = mp.get(T(keys, dev)).cpu().numpy()
    mrows, _ = m.lookup(keys, True, False, 0, 1)
    assert m.dropped == 36 and m.new_rows == list(range(64))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad[:10], mrows[bad[:10]])
    assert np.array_equal(mp.index.lookup(T(keys, dev), insert=False).cpu().numpy(), mrows)          # rows 0..63 by first appearance
    c = mp.index.counters_all()
    assert (c[0], c[1], c[2], c[3]) == (64, 64, 36, 0)
    assert np.array_equal(mp.values.cpu().numpy(), oracle.normal_rows(5, np.array(m.new_keys, np.int64), D, 0.01))
    assert np.array_equal(mp.get(T(keys, dev), insert_default_value=False).cpu().numpy(), want)
    assert np.array_equal(mp.get(T(keys, dev)).cpu().numpy(), want) and mp.index.counters_all()[2] == 72


@pytest.mark.parametrize("unique", [False, True])
@pytest.mark.parametrize("D,ldo", [(8, 12), (6, 8)])
@pytest.mark.parametrize("key_dtype", [np.int32, np.int64])
def test_lookup_out_on_a_full_table(dev, oracle, key_dtype, D, ldo, unique):
    """KeyIndex.lookup(out=...): out is written exactly where rows_gather is -1 -- the first position of a new key and EVERY
    position of a dropped one -- with the key's default row; rows_gather = rows elsewhere; the padding of out's rows and the
    rows the gather behind the call fills are not touched."""
    from mindrec_amd import ops
    rng = np.random.default_rng(38)
    ki, m = ops.KeyIndex(64, dev), MapModel(64)
    vals = torch.full((64, D), SENT, device=dev)
    tables = [(vals, 0.01, None, 5)]
    pool = _distinct(rng, 100, key_dtype)
    ki.lookup(T(pool[:20], dev), tables=tables)
    m.lookup(pool[:20], True, False, 0, 1)
    keys = rng.permutation(pool) if unique else np.concatenate([pool, rng.choice(pool, size=50)])[rng.permutation(150)]
    n = keys.size
    buf = torch.full((n, ldo), SENT, device=dev)
    rows, rows_g = ki.lookup(T(keys, dev), unique=unique, tables=tables, out=buf[:, :D])
    rows, rows_g, out = rows.cpu().numpy(), rows_g.cpu().numpy(), buf.cpu().numpy()
    mrows, _ = m.lookup(keys, True, False, 0, 1)
    assert np.array_equal(rows, mrows) and m.dropped == 36
    first_new = np.zeros(n, bool)
    first_new[[int(np.flatnonzero(keys == k)[0]) for k in m.new_keys]] = True
    written = first_new | (mrows < 0)
    assert np.array_equal(rows_g == -1, written) and np.array_equal(rows_g[~written], rows[~written])
    assert (out[:, D:] == SENT).all() and (out[~written] == SENT).all()
    assert np.array_equal(out[written, :D], oracle.normal_rows(5, keys[written].astype(np.int64), D, 0.01))
    ref = np.full((64, D), SENT, np.float32)
    for k, r in m.row_of.items():
        ref[r] = oracle.normal_rows(5, np.array([k], np.int64), D, 0.01)[0]
    assert np.array_equal(vals.cpu().numpy(), ref)                                   # no table row written for a dropped key
    c = ki.counters_all()
    assert (c[0], c[1], c[2], c[3]) == (64, 64, 36, 0)
    # the gather behind the call completes the output (its kernel takes rows of whole float4s)
    if D % 4 == 0:
        done = ops.gather_rows_skip_(vals, T(rows_g, dev), torch.from_numpy(out[:, :D].copy()).to(dev)).cpu().numpy()
        assert np.array_equal(done, oracle.normal_rows(5, keys.astype(np.int64), D, 0.01))


def test_argument_checks_of_the_chain(dev, oracle):
    """each refused with an error code before anything is launched: the index and its tables are as they were"""
    from mindrec_amd import _lib, ops
    p = Pair(5000, dev, oracle, np.int64)
    keys = np.arange(100, 164)
    p.lookup(keys, train=True, step=1)
    tk = T(keys + 1000, dev)
    t6 = torch.full((5000, 6), SENT, device=dev)

    def refused(code, fn):
        with pytest.raises(_lib.MrecError) as e:
            fn()
        assert e.value.code == code
        torch.cuda.synchronize()
        p.check()
        assert float(t6.min()) == SENT == float(t6.max())

    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
    refused(EUNSUPPORTED, lambda: p.ki.lookup(tk, tables=[(t6, 0.01, None, 1)], out=torch.empty((64, 6), device=dev)))      # ldo = 6
    refused(EINVAL, lambda: p.ki.lookup(tk, tables=p.tables, out=torch.empty((64, 4), device=dev), out_table=2))
    refused(EINVAL, lambda: p.ki.lookup(tk, tables=p.tables, out=torch.empty((64, 4), device=dev), out_table=-1))
    refused(EINVAL, lambda: p.ki.lookup(tk, tables=[p.tables[0]] * 9))
    refused(EINVAL, lambda: p.ki.lookup(tk, tables=p.tables, step=-1))
    refused(EINVAL, lambda: p.ki.evict(5, -1))
    n_ev = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.zeros(64, dtype=torch.uint8, device=dev)
    refused(EWORKSPACE, lambda: _lib.call("mrec_map_evict", p.ki._h, 5, 0, ops._ptr(n_ev), ops._ptr(ws), 11, ops._stream()))      # 3 tiles: 12 bytes
    assert int(n_ev.item()) == 0
    p.lookup(keys + 1000, train=True, step=2)                                        # and the chain still works behind the refusals
