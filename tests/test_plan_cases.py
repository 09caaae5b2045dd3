"""tests/_plan_cases.py held to what it states, on any machine: every builder hits its counts, the host restatement of the plan
(plan_ref) agrees with the oracle's Unique and with a stable argsort of its inverse, and the case tables lie where their names say
-- every (passes, digit bits) layout of radix_plan up to n = 2^22 + 1, every duplicate count on its side of 1024 and of a 2048
tile edge.  The kernels run over the same cases in tests/test_plan_seams_gpu.py."""
import numpy as np
import pytest

import _plan_cases as P

DTYPES = [np.int32, np.int64]
N_MAX_ORACLE = 1 << 17


def radix_plan(n):
    """radix_plan of mrec_dedup.hip: (passes, digit bits per pass) for keys < n, 11-bit digits at most"""
    bits = max(1, (n - 1).bit_length())                          # = ceil(log2 n)
    passes = -(-bits // 11)
    return passes, -(-bits // passes)


def agree(oracle, ids, skip_negative):
    uniq, inv, spos, sseg, offs, n_valid = P.plan_ref(ids, skip_negative)
    u_o, inv_o = (oracle.unique_skip_negative if skip_negative else oracle.unique)(ids)
    assert np.array_equal(uniq, u_o) and np.array_equal(inv, inv_o)
    ok = np.flatnonzero(inv_o >= 0)
    order = ok[np.argsort(inv_o[ok], kind="stable")]
    assert n_valid == ok.size and np.array_equal(spos[:n_valid], order) and np.array_equal(sseg[:n_valid], inv_o[order])
    assert np.array_equal(spos[n_valid:], np.flatnonzero(inv_o < 0)) and (sseg[n_valid:] == uniq.size).all()
    assert np.array_equal(offs[:uniq.size + 1], np.searchsorted(inv_o[order], np.arange(uniq.size + 1)))
    assert offs.size == uniq.size + 1 + (n_valid < ids.size) and offs[-1] == ids.size


def test_radix_plan_restated():
    assert [radix_plan(n) for n in (1, 2, 3, 2048, 2049, 1 << 20, (1 << 20) + 1, 1 << 22, (1 << 22) + 1)] == \
        [(1, 1), (1, 1), (1, 2), (1, 11), (2, 6), (2, 10), (2, 11), (2, 11), (3, 8)]


def test_tables_hold_every_enumerated_case():
    assert P.PASS_SWEEP == sorted(set(P.PASS_SWEEP)) and len(P.PASS_SWEEP) == 40
    assert {2, 3, 5} <= set(P.PASS_SWEEP) and all((1 << k) + d in P.PASS_SWEEP for k in range(1, 21) for d in (0, 1))
    assert P.BIG == [2097153, 4194304, 4194305]
    assert sorted({c.nD for c in P.DUP_SEAMS}) == [0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
    assert len(P.DUP_SEAMS) == 2 * 10 * 3 == len(set(P.DUP_SEAMS))
    assert {(c.n, c.nD, c.shape) for c in P.DUP_SEAMS} == {(n, d, s) for n in (6000, 70001) for d in P.SEAM_SIDE for s in P.SHAPES}
    assert [(c.total, c.k) for c in P.PAD_SEAMS] == [(1024, 1024), (1024, 0), (1024, 512), (1025, 1025), (1025, 0), (1025, 512), (2049, 5)]
    assert all(c.n == 6000 for c in P.PAD_SEAMS)


def test_sweep_and_big_cover_every_pass_layout():
    every = {radix_plan(n) for n in range(1, 1 << 12)} | {radix_plan((1 << k) + 1) for k in range(11, 23)}      # a layout is a function
    assert every == {(1, b) for b in range(1, 12)} | {(2, b) for b in range(6, 12)} | {(3, 8)}                  # of ceil(log2 n) alone
    assert {radix_plan(n) for n in P.PASS_SWEEP} == {(1, b) for b in range(1, 12)} | {(2, b) for b in range(6, 12)}
    assert [radix_plan(n) for n in P.BIG] == [(2, 11), (2, 11), (3, 8)]
    assert {radix_plan(n) for n in P.PASS_SWEEP + P.BIG} == every


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_ids(oracle, dtype):
    for n in P.PASS_SWEEP:
        ids = P.sweep_case_ids(n, dtype)
        assert ids.dtype == dtype and ids.size == n
        U = np.unique(ids).size
        if n >= 64:
            assert 0.55 * n < U < 0.7 * n
        if n >= 256:                                             # (fewer ids: the few duplicates of the last groups may miss a bit)
            bits = (n - 1).bit_length()
            inv = P.plan_ref(ids)[1]
            dup = np.ones(n, bool)
            dup[np.unique(ids, return_index=True)[1]] = False
            for keys in (inv, inv[dup]):                         # the keys the group-by sorts, and those the plan sorts
                assert all(np.unique((keys >> b) & 1).size == 2 for b in range(bits - 1))
        if dtype == np.int64 and n >= 64:
            assert (ids < 0).any() and (ids > 1 << 32).any()
            assert (P.sweep_case_ids(n, dtype, nonneg=True) >= 0).all()
        if n <= N_MAX_ORACLE:
            agree(oracle, ids, False)


def test_big_ids():
    for n in P.BIG:
        ids = P.big_case_ids(n)
        U = np.unique(ids).size
        assert ids.dtype == np.int32 and ids.size == n and ids.min() >= 0 and ids.max() < n
        assert (1 << 20) < 0.6 * n < U < 0.66 * n                # group numbers well past 2^16: the third digit varies


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", P.DUP_SEAMS, ids=P.case_id)
def test_dup_seam_ids(oracle, dtype, c):
    ids = P.dup_case_ids(c, dtype)
    assert ids.dtype == dtype and ids.size == c.n
    u, first, cnt = np.unique(ids, return_index=True, return_counts=True)
    assert u.size == c.n - c.nD and P.n_dups(ids) == c.nD
    assert P.side_of(c.nD) == (c.path, c.live_tiles) == P.SEAM_SIDE[c.nD]
    assert (c.path == "small") == (c.nD <= 1024) and c.live_tiles == (0 if c.nD <= 1024 else -(-c.nD // 2048))
    tiles = -(-c.n // 2048)
    assert (tiles, c.live_tiles <= tiles) == (3, True) if c.n == 6000 else tiles == 35 and c.live_tiles <= 3       # one to three live tiles of 35
    assert first.min() == 0
    if dtype == np.int64:
        assert (ids < 0).any() and (ids > 1 << 32).any()
        assert (P.dup_case_ids(c, dtype, skip_negative=True) >= 0).all()
    if c.nD >= 2:
        runs = np.sort(cnt[cnt > 1])
        if c.shape == "one_group":
            assert runs.tolist() == [c.nD + 1]
        elif c.shape == "few_groups":
            assert 1 <= runs.size <= min(7, c.nD) and runs.sum() == c.nD + runs.size
            if c.nD >= 1023:                                     # each key's copies lie all over the range: runs interleave across tiles
                assert runs.size == 7
                for k in u[cnt > 1]:
                    where = np.flatnonzero(ids == k)
                    assert np.unique(where // 2048).size > -(-c.n // 2048) // 2
        elif c.nD <= 1025:
            assert runs.size > 0.9 * c.nD                        # spread: (nearly) every duplicate copies a key of its own
    agree(oracle, ids, False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", P.PAD_SEAMS, ids=P.case_id)
def test_pad_seam_ids(oracle, dtype, c):
    ids = P.pad_case_ids(c, dtype)
    assert ids.dtype == dtype and ids.size == c.n
    pad = ids < 0
    assert int(pad.sum()) == c.k and (ids[pad] == -1).all()
    U = np.unique(ids[~pad]).size
    assert c.n - U == c.total and (c.n - c.k) - U == c.total - c.k           # padding + real duplicates, and the real ones alone
    assert P.side_of(c.total) == (c.path, c.live_tiles)
    assert (c.path == "small") == (c.total <= 1024) and c.live_tiles == (0 if c.total <= 1024 else -(-c.total // 2048))
    if c.k >= 3:
        assert pad[0] and pad[c.n - 1] and pad[2047]
    agree(oracle, ids, True)


def test_with_padding_counts_again():
    ids = np.array([5, 5, 6, 7, 7, 7, 8], np.int64)              # 3 duplicates
    out, total = P.with_padding(ids, 2, P.case_rng(0))           # blanks position 0 (a first occurrence) and position 6 (a key of its own)
    assert out.tolist() == [-1, 5, 6, 7, 7, 7, -1] and total == 4 and P.n_dups(out, True) == 4
    assert P.with_padding(ids, 0, P.case_rng(0))[1] == 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_inputs(oracle, dtype):
    for nonneg in (False, True):
        steps = P.path_inputs(dtype, nonneg)
        assert len(steps) == len(P.PATH_STEPS) == 7
        sides = [P.side_of(P.n_dups(ids, skip)) for ids, skip in steps]
        assert sides == [("radix", 2), ("small", 0), ("small", 0), ("radix", 1), ("small", 0), ("radix", 3), ("radix", 2)]
        counts = [(P.n_dups(ids, skip), int((ids < 0).sum()) if skip else 0) for ids, skip in steps]
        assert counts == [(3000, 0), (5, 0), (0, 0), (2000, 2000), (3, 3), (5999, 0), (3000, 0)]
        assert np.array_equal(steps[0][0], steps[6][0])
        for ids, skip in steps:
            assert ids.dtype == dtype and ids.size == P.PATH_N
            if nonneg:
                assert (ids[ids != -1] >= 0).all()
                agree(oracle, ids, True)
            agree(oracle, ids, skip)
