"""The host model of the key index (tests/_map_model.py) against the oracle's map wherever that map defines the behaviour
(sequential find-or-insert with duplicates, a full table, erase while fresh rows remain: the oracle never reuses a row), and
hand-written cases for the rules that are the index's own (mrec.h "MapParameter key index")."""
import numpy as np
import pytest

from _map_model import MapModel, fill_slots, hash_key, home_slot, n_slots


def _same_as_oracle(m, om):
    ok, _ = om.export()
    mk, mr = m.export()
    assert m.live == om.size() and np.array_equal(mk, ok)
    return mr


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_append_only_sequences_match_oracle_map(oracle, seed):
    rng = np.random.default_rng(seed)
    cap = 450
    m, om = MapModel(cap), oracle.Map(4, cap, seed=1)
    pool = np.concatenate([rng.integers(-2 ** 62, 2 ** 62, size=900), [0, -1, -2, np.iinfo(np.int64).min, np.iinfo(np.int64).max]])
    for call in range(8):                                        # the last calls run into the full table: both drop
        n = [1, 5, 130, 257, 300, 64, 400, 200][call]
        keys = rng.choice(pool, size=n).astype(np.int64)         # duplicates inside the call and across calls
        insert = call != 3
        rows, _ = m.lookup(keys, insert, False, 0, 1)
        assert np.array_equal(rows, om.find_or_insert(keys, insert)), call
        _same_as_oracle(m, om)
    assert m.hwm == cap and m.dropped > 0 and not m.free


def test_erase_with_fresh_rows_left_matches_oracle_map(oracle):
    """fresh rows first: until they run out an erased row is not reused, which is all the oracle's map ever does"""
    rng = np.random.default_rng(5)
    m, om = MapModel(500), oracle.Map(4, 500, seed=1)
    keys = rng.integers(0, 10 ** 9, size=300).astype(np.int64)
    assert np.array_equal(m.lookup(keys, True, False, 0, 1)[0], om.find_or_insert(keys, True))
    gone = np.unique(keys)[::3]
    m.erase(gone); om.erase(gone)
    probe = np.concatenate([gone[:20], keys[:50]])
    assert np.array_equal(m.lookup(probe, False, False, 0, 1)[0], om.find_or_insert(probe, False))
    more = np.concatenate([gone[:30], rng.integers(10 ** 10, 10 ** 11, size=60)]).astype(np.int64)       # erased keys come back
    assert np.array_equal(m.lookup(more, True, False, 0, 1)[0], om.find_or_insert(more, True))
    _same_as_oracle(m, om)
    assert len(m.free) == gone.size and m.counters()[4] == gone.size


def test_free_rows_are_reused_last_erased_first():
    m = MapModel(6)
    assert m.lookup(np.arange(10, 16), True, False, 0, 1)[0].tolist() == [0, 1, 2, 3, 4, 5]
    m.erase(np.array([11, 13, 15]))
    assert m.free == [1, 3, 5] and m.log == [11, 13, 15]
    assert m.lookup(np.array([20, 21]), True, False, 0, 1)[0].tolist() == [5, 3]
    assert m.counters() == (6, 5, 0, 1, 3, 0)
    assert m.lookup(np.array([22, 23, 22]), True, False, 0, 1)[0].tolist() == [1, -1, 1] and m.dropped == 1


def test_one_call_straddles_fresh_rows_free_rows_and_the_full_table():
    m = MapModel(8)
    m.lookup(np.arange(6), True, False, 0, 1)
    m.erase(np.array([1, 4]))
    #            resident  new   new  dup  new  new   new: dropped, twice   resident
    keys = np.array([0, 100, 101, 100, 102, 103, 104, 104, 5])
    rows, _ = m.lookup(keys, True, False, 0, 1)
    assert rows.tolist() == [0, 6, 7, 6, 4, 1, -1, -1, 5]        # two fresh rows, then the stack [1, 4] from its top
    assert m.counters()[:4] == (8, 8, 1, 0) and m.new_keys == [100, 101, 102, 103] and m.new_rows == [6, 7, 4, 1]
    assert m.lookup(np.array([104]), False, False, 0, 1)[0].tolist() == [-1]        # a dropped key was not inserted


def test_n_valid_and_padding_keys():
    m = MapModel(8)
    rows, _ = m.lookup(np.array([7, -1, 8, -1, 9]), True, False, 0, 1, n_valid=4, skip_pad=True)
    assert rows.tolist() == [0, -1, 1, -1, -1] and m.live == 2 and 9 not in m.row_of and -1 not in m.row_of
    rows, _ = m.lookup(np.array([-1, 7]), True, False, 0, 1)                         # without skip_pad -1 is a key like any other
    assert rows.tolist() == [2, 0]
    assert m.lookup(np.array([5, 6]), True, False, 0, 1, n_valid=0)[0].tolist() == [-1, -1] and m.live == 3


def test_one_hit_per_key_and_step_and_admission():
    m = MapModel(16)
    rows, adm = m.lookup(np.array([3, 3, 4]), True, True, 1, 2)
    assert rows.tolist() == [0, 0, 1] and adm.tolist() == [-1, -1, -1]
    assert m.hits[:2].tolist() == [1, 1] and m.last_step[:2].tolist() == [1, 1]
    m.lookup(np.array([3]), True, True, 1, 2)                                        # the same step again: no second hit
    assert m.hits[0] == 1
    rows, adm = m.lookup(np.array([3, 3, 3, 5]), True, True, 2, 2)
    assert m.hits[:3].tolist() == [2, 1, 1] and adm.tolist() == [0, 0, 0, -1]
    m.lookup(np.array([4]), False, False, 3, 2)                                      # not a training lookup: nothing counted
    assert m.hits[1] == 1 and m.last_step[1] == 1
    rows, _ = m.lookup(np.array([6]), True, False, 3, 2)                             # inserted outside training: no hit yet
    assert m.hits[rows[0]] == 0 and m.last_step[rows[0]] == 3 and m.dirty[rows[0]] == 1


def test_evict_goes_in_row_order_and_export_skips_keys_that_came_back():
    m = MapModel(6)
    m.lookup(np.array([50, 40, 30, 20, 10, 60]), True, True, 1, 1)
    m.lookup(np.array([40, 10]), True, True, 4, 1)
    m.export_dirty(clear=True)
    assert m.evict(5, 2) == 4 and m.free == [0, 2, 3, 5] and m.log == [50, 30, 20, 60] and m.live == 2
    assert m.evict(5, 2) == 0
    rows, _ = m.lookup(np.array([70, 30]), True, True, 5, 1)
    assert rows.tolist() == [5, 3] and m.hits[[5, 3]].tolist() == [1, 1] and m.last_step[[5, 3]].tolist() == [5, 5]
    k, r, s = m.export_dirty(clear=True)
    assert k.tolist() == [30, 70, 50, 20, 60] and r.tolist() == [3, 5, -1, -1, -1] and s.tolist() == [1, 1, 2, 2, 2]
    assert m.export_dirty(clear=False)[0].size == 0


def test_erased_keys_log_is_capped_at_the_capacity():
    m = MapModel(4)
    for rnd in range(3):
        keys = np.arange(4) + 10 * rnd
        m.lookup(keys, True, False, 0, 1)
        m.erase(keys)
    assert m.log == [0, 1, 2, 3] and m.live == 0 and sorted(m.free) == [0, 1, 2, 3]
    k, r, s = m.export_dirty(clear=True)
    assert k.tolist() == [0, 1, 2, 3] and (s == 2).all() and m.log == []


def test_tombstone_count_and_rebuild_threshold():
    m = MapModel(400)                                                # 1024 slots: a rebuild once tombstones exceed 204
    m.lookup(np.arange(400), True, False, 0, 1)
    assert not m.erase(np.arange(204)) and m.counters()[4:] == (204, 0)
    assert m.erase(np.arange(204, 205)) and m.counters()[4:] == (0, 1)


def test_hash_restatement_and_slot_filling():
    assert n_slots(1) == 1024 and n_slots(512) == 1024 and n_slots(513) == 2048 and n_slots(3000) == 8192
    # mrec_mix64 is splitmix64's output function: its first outputs from state 0 are public test vectors
    from _map_model import _mix64
    assert _mix64(0) == 0xE220A8397B1DCDAF and _mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert hash_key(0, np.int32) == 0                                  # the xorshift-multiply hash fixes 0
    assert hash_key(-1, np.int64) == hash_key(np.int64(-1), np.int64) != hash_key(-1, np.int32)
    odd = np.array([0, -1, -2, 1, 2 ** 31 - 1, -2 ** 31, 0x7F7F7F7F, 123456789], np.int64)
    for dt, more in ((np.int32, []), (np.int64, [2 ** 63 - 1, -2 ** 63, 2 ** 40 + 7])):              # array-wise = key by key
        ks = np.concatenate([odd, np.array(more, np.int64)])
        assert home_slot(ks.astype(dt), dt, 1 << 20).tolist() == [hash_key(k, dt) & ((1 << 20) - 1) for k in ks.tolist()]
    h = home_slot(np.arange(5000), np.int64, 1024)
    assert h.min() >= 0 and h.max() < 1024 and np.unique(h).size > 900
    # three keys behind each other at the end of the array wrap to its start; a tombstone is taken back, an empty slot is not
    sr = np.full(8, -1)
    sr[7] = 3
    sr[0] = -2
    after, reused = fill_slots(sr, [7, 7, 6], rows=[10, 11, 12])
    assert after.tolist() == [10, 11, -1, -1, -1, -1, 12, 3] and reused == 1
    a2, r2 = fill_slots(sr, [6, 7, 7], rows=[12, 10, 11])              # another order of arrival: the same slots are taken
    assert (a2 >= 0).tolist() == (after >= 0).tolist() and r2 == reused
