"""The step's plan (mrec_sparse_plan_*, mrec_dedup_* + mrec_group_by_inverse) on the host: its definition restated in numpy, and the
inputs that put it at its structural seams -- every (passes, digit bits) layout of radix_plan, the duplicate count around the
one-workgroup limit (kSmallDups = 1024) and around a tile edge of the duplicate list (2048), padding counted with the duplicates.
Nothing here needs a GPU: tests/test_plan_cases.py holds the builders to their stated counts on any machine,
tests/test_plan_seams_gpu.py runs the kernels over them."""
from collections import namedtuple

import numpy as np

SMALL_DUPS = 1024            # kSmallDups of mrec_dedup.hip: up to this many duplicates are sorted by one workgroup
RADIX_TILE = 2048            # RT of mrec_radix.h
SHAPES = ("spread", "one_group", "few_groups")


def T(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def plan_ref(ids, skip_negative=False):
    """(uniq, inv, sorted_pos, sorted_seg, seg_offsets, n_valid) as mrec.h defines them"""
    n = ids.size
    valid = ids >= 0 if skip_negative else np.ones(n, bool)
    vpos = np.flatnonzero(valid)
    u, first, inv_s = np.unique(ids[vpos], return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                     # groups in the order of first appearance
    rank = np.empty(u.size, np.int64)
    rank[order] = np.arange(u.size)
    inv = np.full(n, -1, np.int64)
    inv[vpos] = rank[inv_s]
    U = u.size
    pos_v = vpos[np.argsort(inv[vpos], kind="stable")]
    pad = np.flatnonzero(~valid)
    sorted_pos = np.concatenate([pos_v, pad])
    sorted_seg = np.concatenate([inv[pos_v], np.full(pad.size, U, np.int64)])
    offs = np.concatenate([[0], np.cumsum(np.bincount(inv[vpos], minlength=U))])
    if pad.size:
        offs = np.concatenate([offs, [n]])
    return u[order], inv, sorted_pos, sorted_seg, offs, vpos.size


def check_plan(ops, dev, ids, skip_negative=False, ref=None):
    """ref: plan_ref(ids, skip_negative), where the caller already has it"""
    import torch
    p = ops.sparse_plan(T(ids, dev), skip_negative=skip_negative)
    torch.cuda.synchronize()
    uniq, inv, spos, sseg, offs, n_valid = ref if ref is not None else plan_ref(ids, skip_negative)
    U = uniq.size
    assert p.U == U
    assert np.array_equal(p.uniq_buf[:U].cpu().numpy(), uniq) and np.array_equal(p.inv.cpu().numpy(), inv)
    assert np.array_equal(p.sorted_pos[:ids.size].cpu().numpy(), spos) and np.array_equal(p.sorted_seg[:ids.size].cpu().numpy(), sseg)
    assert np.array_equal(p.seg_offsets[:offs.size].cpu().numpy(), offs)
    if skip_negative:
        assert int(p.n_valid_dev.item()) == n_valid
        if n_valid < ids.size:
            assert int(p.uniq_buf[U].item()) == -1
    return p


def case_rng(*parts):
    """one generator per case, a function of the case alone: the CPU and the GPU tests build the same ids"""
    return np.random.default_rng([int(x) for x in parts])


def distinct_keys(n, dtype, rng, nonneg=False):
    """n distinct keys, not in sorted order; int64 (unless nonneg): a third of them negative, a third above 2^32"""
    k = rng.permutation(n).astype(np.int64) * 7 + 3
    if np.dtype(dtype) == np.int64 and not nonneg:
        third = np.arange(n) % 3
        k = np.where(third == 1, -k - 1, np.where(third == 2, k + (1 << 33), k))
    return k.astype(dtype)


def ids_with_dups(n, nD, shape, dtype, rng, skip_negative=False):
    """n ids with exactly nD duplicate positions (U = n - nD): n distinct keys, then nD positions other than position 0 each
    overwritten with the key of an earlier position that is not itself overwritten -- so the positions left alone are the first
    occurrences, and the group of the r-th of them is r."""
    assert 0 <= nD < max(n, 1) and shape in SHAPES
    ids = distinct_keys(n, dtype, rng, nonneg=skip_negative)
    if nD == 0:
        return ids
    # few_groups keeps a head of the range free of duplicates, so that 7 source positions precede every one of them
    lo = max(1, min(n // 4, n - nD)) if shape == "few_groups" else 1
    chosen = np.sort(rng.choice(np.arange(lo, n), size=nD, replace=False))
    free = np.setdiff1d(np.arange(n), chosen)                    # ascending; free[r] starts group r
    before = chosen - np.arange(nD)                              # number of free positions in front of each chosen one (>= lo)
    if shape == "spread":                                        # a different earlier key each, while the tries find one
        src = np.empty(nD, np.int64)
        used = set()
        tries = rng.random((nD, 8))
        for j in range(nD):
            for t in tries[j]:
                r = int(t * before[j])
                if r not in used:
                    break
            used.add(r)
            src[j] = r
    elif shape == "one_group":                                   # one run of nD + 1 entries, its group number not 0 where it can be
        src = np.full(nD, before[0] - 1)
    else:                                                        # 7 keys, each one's copies anywhere in [lo, n)
        heads = rng.choice(lo, size=min(7, lo), replace=False)
        src = heads[rng.integers(0, heads.size, size=nD)]
    assert (src < before).all()
    ids[chosen] = ids[free[src]]
    assert np.unique(ids).size == n - nD
    return ids


def n_dups(ids, skip_negative=False):
    """what the plan counts as duplicates: n - U, padding included"""
    return ids.size - np.unique(ids[ids >= 0] if skip_negative else ids).size


def with_padding(ids, k, rng):
    """(ids with k positions set to -1, the new count of real duplicates + padding).  Position 0, position n - 1 and one position
    at a 2048 boundary are among the k (as far as k reaches).  The count is taken again from the result: blanking a first
    occurrence makes a duplicate of its key the new first one."""
    n = ids.size
    out = ids.copy()
    must = [0, n - 1] + ([RADIX_TILE - 1] if n > RADIX_TILE else [])
    must = list(dict.fromkeys(must))[:k]
    rest = np.setdiff1d(np.arange(n), must)
    pos = np.concatenate([np.array(must, np.int64), rng.choice(rest, size=k - len(must), replace=False)])
    out[pos] = -1
    return out, n_dups(out, skip_negative=True)


def sweep_ids(n, dtype, rng, nonneg=False):
    """groups drawn with replacement from n distinct keys: U ~ 0.63 n, every digit of every pass varies"""
    return distinct_keys(n, dtype, rng, nonneg)[rng.integers(0, n, size=n)]


def big_ids(n, dtype, rng):
    return rng.integers(0, n, size=n).astype(dtype)


def pad_ids(n, total, k, dtype, rng):
    """n ids, k of them padding, with (real duplicates + padding) == total exactly.  A blanked position whose key lives on elsewhere
    adds nothing to the sum (one duplicate less, one padding more), so the shortfall is made up afterwards: as many keys that
    occur once are overwritten with a key that stays."""
    ids, t = with_padding(ids_with_dups(n, total - k, "spread", dtype, rng, skip_negative=True), k, rng)
    short = total - t
    assert 0 <= short <= k
    if short:
        u, first, cnt = np.unique(ids, return_index=True, return_counts=True)
        once = first[(cnt == 1) & (u >= 0)]
        gone = rng.choice(once[once > 0], size=short, replace=False)
        stay = np.setdiff1d(np.flatnonzero(ids >= 0), gone)
        ids[gone] = ids[stay[rng.integers(0, stay.size, size=short)]]
    assert n_dups(ids, True) == total and int((ids < 0).sum()) == k
    return ids


# ---- the case tables

# every (passes, digit bits) layout of radix_plan up to two passes of 10 bits
PASS_SWEEP = sorted({2, 3, 5} | {(1 << k) + d for k in range(1, 21) for d in (0, 1)})

# two passes of 11 bits; the last two-pass n; three passes of 8 bits
BIG = [(1 << 21) + 1, 1 << 22, (1 << 22) + 1]

# the side of the two limits a duplicate count lies on: which path sorts the duplicates, and how many radix tiles are live
SEAM_SIDE = {0: ("small", 0), 1: ("small", 0), 2: ("small", 0), 1023: ("small", 0), 1024: ("small", 0), 1025: ("radix", 1),
             2047: ("radix", 1), 2048: ("radix", 1), 2049: ("radix", 2), 4097: ("radix", 3)}

DupCase = namedtuple("DupCase", "n nD shape path live_tiles")
DUP_SEAMS = [DupCase(n, nD, shape, *SEAM_SIDE[nD]) for n in (6000, 70001) for nD in SEAM_SIDE for shape in SHAPES]

PadCase = namedtuple("PadCase", "n total k path live_tiles")
PAD_SEAMS = [PadCase(6000, total, k, path, tiles)
             for total, path, tiles, ks in ((1024, "small", 0, (1024, 0, 512)), (1025, "radix", 1, (1025, 0, 512)), (2049, "radix", 2, (5,)))
             for k in ks]


def side_of(count):
    """(path, live radix tiles) of a duplicate count, as plan_impl takes them"""
    if count <= SMALL_DUPS:
        return "small", 0
    return "radix", -(-count // RADIX_TILE)


def dup_case_ids(c, dtype, skip_negative=False):
    return ids_with_dups(c.n, c.nD, c.shape, dtype, case_rng(1, c.n, c.nD, SHAPES.index(c.shape), np.dtype(dtype).itemsize),
                         skip_negative=skip_negative)


def pad_case_ids(c, dtype):
    return pad_ids(c.n, c.total, c.k, dtype, case_rng(2, c.n, c.total, c.k, np.dtype(dtype).itemsize))


def sweep_case_ids(n, dtype, nonneg=False):
    return sweep_ids(n, dtype, case_rng(3, n, np.dtype(dtype).itemsize), nonneg)


def big_case_ids(n, dtype=np.int32):
    return big_ids(n, dtype, case_rng(4, n))


def case_id(c):
    return "-".join(str(x) for x in c)


# ---- one workspace, every path: the inputs of the primed-workspace and graph-replay tests, in the order they run
PATH_N = 6000
PATH_STEPS = ("radix 3000 dups", "small 5 dups", "no dups", "radix 2000 padding", "small 3 padding", "all equal", "radix 3000 dups again")


def path_inputs(dtype, nonneg=False):
    """[(ids, skip_negative)] at n = 6000: the radix path, the small path, no duplicates, padding on the radix path, padding on the
    small path, all ids equal, the first again.  nonneg: no negative keys, for a caller that plans them all with skip_negative."""
    sz = np.dtype(dtype).itemsize
    mk = lambda nD, shape, seed, neg: ids_with_dups(PATH_N, nD, shape, dtype, case_rng(5, seed, sz), skip_negative=neg or nonneg)
    first = mk(3000, "few_groups", 0, False)
    pad_many = with_padding(mk(0, "spread", 3, True), 2000, case_rng(5, 13, sz))[0]
    pad_few = with_padding(mk(0, "spread", 4, True), 3, case_rng(5, 14, sz))[0]
    same = np.full(PATH_N, first[PATH_N // 2], dtype)
    return [(first, False), (mk(5, "spread", 1, False), False), (mk(0, "spread", 2, False), False), (pad_many, True), (pad_few, True),
            (same, False), (first.copy(), False)]
