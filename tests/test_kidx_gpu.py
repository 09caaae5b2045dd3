"""ops.FrozenKeyIndex (csrc/mrec_kidx.hip) against a Python dict and the host model of the slot array (tests/_map_model.py): every stored
key found, absent keys and key -1 not, the occupied slots those of fill_slots, max_probe at least a cluster's length."""
import numpy as np
import pytest
import torch

import _map_model as M

pytestmark = pytest.mark.gpu


def _keys(n, S, dt):
    """n distinct keys of dtype dt: 0, negatives, the extremes, ~40 keys of one home slot and a cluster at home S - 1 (fewer where n is)"""
    rng = np.random.default_rng(n)
    info = np.iinfo(dt)
    pool = np.unique(rng.integers(info.min, info.max, size=60 * S, dtype=np.int64, endpoint=True))
    pool = pool[(pool != -1) & (pool != 0)]
    home = M.home_slot(pool, np.int64, S)
    nc = min(40, n // 4)
    fixed = np.array([0, -2, info.min, info.max, -12345], np.int64)[: max(1, min(5, n - 2 * nc))]
    cl = np.concatenate([pool[home == 7][:nc], pool[home == S - 1][:nc]])
    rest = np.setdiff1d(pool, np.concatenate([fixed, cl]))
    keys = np.concatenate([fixed, cl, rng.permutation(rest[:-n])])[:n]
    assert cl.size == 2 * nc and keys.size == n and np.unique(keys).size == n
    return keys, nc, rest[-n:]                                           # (the pool's far end: as many keys that are not stored)


@pytest.mark.parametrize("explicit_rows", [False, True], ids=["rows-null", "rows"])
@pytest.mark.parametrize("dt", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("n", [1, 700, 5000])
def test_frozen_key_index(dev, n, dt, explicit_rows):
    from mindrec_amd import ops
    S = M.n_slots(n)
    keys, nc, absent = _keys(n, S, dt)
    given = np.concatenate([keys[: n // 2], [-1], keys[n // 2:]])        # key -1 among the inputs: skipped
    rows = np.random.default_rng(1).permutation(n + 1).astype(np.int32) if explicit_rows else np.arange(n + 1, dtype=np.int32)
    want = {int(k): int(r) for k, r in zip(given, rows) if k != -1}
    ki = ops.FrozenKeyIndex(torch.from_numpy(given.astype(dt)).to(dev), torch.from_numpy(rows).to(dev) if explicit_rows else None)
    assert (ki.n, ki.n_slots) == (n + 1, S) and S == {1: 1024, 700: 2048, 5000: 16384}[n]
    probe = np.concatenate([keys, absent[: max(n, 1)], [-1]]).astype(dt).reshape(1, -1)
    got = ki.find(torch.from_numpy(probe).to(dev))
    assert got.dtype == torch.int32 and got.shape == probe.shape
    assert got.cpu().numpy().ravel().tolist() == [want.get(int(k), -1) for k in probe.ravel()]
    skey, srow = (t.cpu().numpy() for t in ki.slots())
    model, _ = M.fill_slots(np.full(S, -1), M.home_slot(keys, np.int64, S))
    assert np.array_equal(srow >= 0, model >= 0), "occupied slots differ from fill_slots"
    assert {int(k): int(r) for k, r in zip(skey[srow >= 0], srow[srow >= 0])} == want
    assert max(nc, 1) <= ki.max_probe() <= S
