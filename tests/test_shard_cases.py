"""tests/_shard_cases.py -- the host restatement that tests/test_shard_edges_gpu.py holds the shard exchange kernels to -- held
itself: against the oracle where the oracle says the same thing, against the header's constants, and the device's division by
F against the true quotient up to the bound include/mrec.h states (and not past it)."""
import os
import re

import numpy as np
import pytest

import _shard_cases as SC
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_radix_constants_are_the_headers():
    text = open(os.path.join(ROOT, "mindrec_amd", "csrc", "mrec_radix.h")).read()
    maxb = int(re.search(r"constexpr int RMAXB = (\d+);", text).group(1))
    assert re.search(r"constexpr int RNB = 1 << RMAXB;", text) and SC.RNB == 1 << maxb
    assert SC.RT == int(re.search(r"constexpr int RT = (\d+);", text).group(1))


def existing_inputs():
    """the inputs of tests/test_shard_gpu.py's two routing tests"""
    for idt in (np.int32, np.int64):
        for world, hashed, factor in [(1, False, 1.25), (2, False, 1.25), (8, False, 1.25), (5, True, 1.5), (4, False, 0.9)]:
            rng = np.random.default_rng(7)
            n = 5000
            ids = rng.integers(0, 1 << 40 if (hashed and idt == np.int64) else 100_000, size=n).astype(idt)
            ids[::7] = ids[0]
            if hashed:
                ids[5] = -123456
            yield ids, rng.random(n).astype(np.float32), world, O.shard_capacity(n, world, factor), hashed, 0
    for world, rank in [(1, 0), (2, 0), (2, 1), (5, 3), (8, 7)]:
        rng = np.random.default_rng(3 + world)
        n = 4000
        ids = rng.integers(0, 100_000, size=n).astype(np.int32)
        yield ids, rng.random(n).astype(np.float32), world, O.shard_capacity(n, world, 1.5), False, (rank + 1) % world


def same(a, b):
    assert len(a) == len(b) == 5
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
    assert a[4] == b[4]


def test_route_slots_ref_equals_the_oracle_and_a_full_length_changes_nothing():
    some_dropped = False
    for ids, wts, S, cap, hashed, rot in existing_inputs():
        want = O.shard_route_slots(ids, wts, S, cap, hashed, rot=rot)
        got = SC.route_slots_ref(ids, wts, S, cap, hashed, rot)
        same(got, want)
        same(SC.route_slots_ref(ids, wts, S, cap, hashed, rot, n_valid=ids.size), got)
        same(O.shard_route_slots(ids, wts, S, cap, hashed, rot=rot, n_valid=ids.size), want)
        same(SC.route_slots_ref(ids, None, S, cap, hashed, rot), O.shard_route_slots(ids, None, S, cap, hashed, rot=rot))
        some_dropped |= got[4] > 0
    assert some_dropped


@pytest.mark.parametrize("n_valid", [0, 1, 2999, 4999])
def test_a_device_length_is_the_list_cut_there(n_valid):
    """Routing with n_valid = routing the first n_valid entries, with -1 for the positions behind; the oracle's n_valid agrees."""
    for ids, wts, S, cap, hashed, rot in list(existing_inputs())[3:12:4]:
        ids = ids.copy()
        ids[n_valid:] = ids[0]                                  # were they counted, their owner's bucket would overflow
        got = SC.route_slots_ref(ids, wts, S, cap, hashed, rot, n_valid=n_valid)
        cut = SC.route_slots_ref(ids[:n_valid], wts[:n_valid], S, cap, hashed, rot)
        assert np.array_equal(got[2][:n_valid], cut[2]) and (got[2][n_valid:] == -1).all()
        for k in (0, 1, 3):
            assert np.array_equal(got[k], cut[k])
        assert got[4] == cut[4]
        same(O.shard_route_slots(ids, wts, S, cap, hashed, rot=rot, n_valid=n_valid), got)
        if n_valid == 0:
            assert (got[0] == -1).all() and not got[1].any() and (got[3] == -1).all() and got[4] == 0


def test_req_entries_layout():
    e = SC.req_entries(np.array([5, -1], np.int64), np.array([-0.0, 1.0], np.float32), np.int64)
    assert e.tolist() == [[5, 0x80000000], [-1, 0x3F800000]]                 # int64: the pad word behind the weight is 0
    e = SC.req_entries(np.array([5, -1], np.int64), np.array([-0.0, 1.0], np.float32), np.int32)
    assert e.tolist() == [[5, -(1 << 31)], [-1, 0x3F800000]]


def test_message_restatements_on_a_case_small_enough_to_read():
    back = np.arange(3 * 8, dtype=np.int32).reshape(3, 8) + 100            # Dw = 4, W = 8
    emb, pair = SC.unroute_ref(back, np.array([2, -1, 0], np.int32), 4)
    assert emb.tolist() == [[116, 117, 118, 119], [0, 0, 0, 0], [100, 101, 102, 103]] and pair.tolist() == [[120, 0], [0, 0], [104, 0]]
    g = np.arange(6 * 5, dtype=np.int32).reshape(6, 5)                      # ldg = 5 > Dw = 4
    dl = np.array([1.0, 2.0], np.float32)
    before = np.full((3, 12), 7, np.int32)                                  # W = 12 > Dw + 4
    msg, held = SC.route_grads_ref(g, dl, 3, np.array([4, -1, 2], np.int32), 4, 12, before)
    assert (before == 7).all()
    assert msg[0].tolist() == [20, 21, 22, 23, 0x40000000, 7, 7, 7, 7, 7, 7, 7] and held[0].tolist() == [True] * 5 + [False] * 3 + [True] * 4
    assert (msg[1] == 7).all() and held[1].all()
    assert msg[2].tolist()[:5] == [10, 11, 12, 13, 0x3F800000]


def test_lane_geometry_table():
    assert [SC.lane_geometry(Dw)[1] for Dw in SC.MSG_DW] == [32, 21, 16, 5, 4, 3, 2, 1, 1]
    assert [64 - SC.lane_geometry(Dw)[0] * SC.lane_geometry(Dw)[1] for Dw in SC.MSG_DW] == [0, 1, 0, 9, 0, 1, 0, 31, 0]
    assert SC.msg_counts(80) == (1, 47, 48, 49, 99)
    assert SC.route_n_valid(1) == [0, 1] and SC.route_n_valid(2048) == [0, 1, 2047, 2048]


@pytest.mark.parametrize("F", SC.MSG_F + SC.DIV_F)
def test_umulhi_div_is_the_quotient_up_to_the_bound(F):
    pmax = SC.div_bound(F)
    assert pmax * F < 1 << 32 <= (pmax + 1) * F
    for p in (0, F - 1, F, pmax - F, pmax):
        assert SC.umulhi_div(p, F) == p // F, (p, F)
    ps = np.random.default_rng(F).integers(0, pmax + 1, size=20000)
    assert all(SC.umulhi_div(int(p), F) == int(p) // F for p in ps)


def test_umulhi_div_first_fails_just_past_the_bound():
    """what include/mrec.h states at mrec_shard_route_grads: pos * F < 2^32, and no more than that"""
    assert SC.div_bound(4096) == 1_048_575
    assert SC.umulhi_div(1_052_671, 4096) != 1_052_671 // 4096
    assert all(SC.umulhi_div(p, 4096) == p // 4096 for p in range(1_048_575, 1_052_671))
    assert SC.umulhi_div(1_122_029, 4095) != 1_122_029 // 4095 and SC.umulhi_div(252_645_158, 39) != 252_645_158 // 39
    assert SC.umulhi_div(1_122_028, 4095) == 1_122_028 // 4095 and SC.umulhi_div(252_645_157, 39) == 252_645_157 // 39


def test_the_wrapper_refuses_positions_past_the_bound():
    from mindrec_amd import ops
    ops._route_grads_positions_ok(1_048_575, 4096)
    ops._route_grads_positions_ok((1 << 32) - 1, 1)
    for n, F in [(1_048_576, 4096), (1 << 32, 1), (257 * 4095, 4095)]:
        with pytest.raises(ValueError, match="2\\^32"):
            ops._route_grads_positions_ok(n, F)
