"""The host restatement of the sparse apply's order of additions (tests/_apply_order.py) checked without a GPU: where every run lies in
one window it IS the oracle's sequential sum, bit for bit; everywhere it obeys the any-order fp32 bound; its layout generator produces
exactly the run sequences asked for; and each standard layout makes the apply do what the GPU tests claim it exercises."""
import numpy as np
import pytest

import _apply_order as A
from oracle import oracle as O


def _within_windows(rng, aw, nruns):
    """run lengths 1 .. aw placed so that no run crosses a window boundary"""
    seq, cur = [], 0
    for _ in range(nruns):
        L = int(rng.integers(1, aw + 1))
        if cur // aw != (cur + L - 1) // aw:
            pad = aw - cur % aw
            seq += [1] * pad
            cur += pad
        seq.append(L)
        cur += L
    return seq


@pytest.mark.parametrize("D,vec,aw", [(80, 4, 8), (16, 4, 8), (1, 1, 8), (30, 2, 8), (7, 1, 8), (260, 4, 8), (512, 4, 16), (130, 2, 4)])
@pytest.mark.parametrize("use_rs", [True, False])
def test_within_one_window_equals_the_oracle(D, vec, aw, use_rs):
    rng = np.random.default_rng(D * 3 + aw + use_rs)
    seq = _within_windows(rng, aw, 300)
    V = len(seq) + 50
    keys = rng.permutation(V)[: len(seq)].astype(np.int32)
    keys[::17] = -1 - np.arange(keys[::17].size)                  # rows outside the table: skipped by both
    ids = A.layout_ids(seq, keys, rng)
    n = ids.size
    g = rng.standard_normal((n, D)).astype(np.float32)
    rs = rng.random(n).astype(np.float32) + 0.5 if use_rs else None
    gs = 1 / 1024
    idx = A.Index(ids)
    assert A.census(idx, D, vec, aw)["crossing"] == 0
    G = A.sums(idx, A.contributions(g, rs, gs), D, vec, aw)
    # segment sum
    ref = O.segment_sum(A.contributions(g, rs, gs), O.unique(ids)[1], idx.U)
    assert np.array_equal(G.view(np.uint32), ref.view(np.uint32))
    # LazyAdam and FTRL
    p0 = (rng.standard_normal((V, D)) * 0.01).astype(np.float32)
    s1, s2 = [p0.copy(), np.zeros_like(p0), np.zeros_like(p0)], [p0.copy(), np.zeros_like(p0), np.zeros_like(p0)]
    O.sparse_lazy_adam(*s1, ids, g, rs, grad_scale=gs, b1_pow=0.81, b2_pow=0.998)
    A.lazy_adam(*s2, idx.uniq, G, b1_pow=0.81, b2_pow=0.998)
    for a, b in zip(s1, s2):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    s1, s2 = [p0.copy(), np.ones_like(p0), np.zeros_like(p0)], [p0.copy(), np.ones_like(p0), np.zeros_like(p0)]
    O.sparse_ftrl(*s1, ids, g, rs, grad_scale=gs)
    A.ftrl(*s2, idx.uniq, G)
    for a, b in zip(s1, s2):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("layout", ["boundaries", "tree", "pairs"])
@pytest.mark.parametrize("D,vec,wide", [(80, 4, True), (16, 4, False), (1, 1, False), (260, 4, False)])
def test_sums_obey_the_any_order_bound(layout, D, vec, wide):
    rng = np.random.default_rng(D + len(layout))
    aw = 8
    ngs = [b[3] for b in A.col_blocks(D, vec, wide)]
    seq = {"boundaries": A.boundaries(aw), "tree": A.tree(aw, ngs, rng), "pairs": A.pairs(aw, "under")}[layout]
    if D > 64 and layout == "tree":
        seq = A.tree(aw, [min(ngs)], rng)                     # (the 16 NG runs of the narrow blocks: thousands of 260-wide rows)
    ids = A.layout_ids(seq, np.arange(len(seq)), rng)
    n = ids.size
    g = rng.standard_normal((n, D)).astype(np.float32)
    gw = rng.standard_normal(n).astype(np.float32) if wide else None
    idx = A.Index(ids)
    x = A.contributions(g, None, 1.0)
    G = A.sums(idx, x, D, vec, aw, xw=gw)
    xa = np.concatenate([x, gw[:, None]], axis=1) if wide else x
    inv = O.unique(ids)[1]
    exact = np.zeros((idx.U, xa.shape[1]))
    absum = np.zeros_like(exact)
    np.add.at(exact, inv, xa.astype(np.float64))
    np.add.at(absum, inv, np.abs(xa).astype(np.float64))
    cnt = np.bincount(inv, minlength=idx.U)[:, None]
    assert (np.abs(G - exact) <= np.maximum(cnt - 1, 1) * 2.0 ** -23 * absum).all()
    # and it is not the oracle's sequential order wherever a run is long (the restatement is not a copy of it)
    if layout == "tree":
        seqsum = O.segment_sum(xa, inv, idx.U)
        assert not np.array_equal(G, seqsum)


def test_tree_is_sequential_up_to_ng_partials():
    """For k + 1 <= NG every lane-group holds one partial: the tree is the partials added in order (pass A)."""
    rng = np.random.default_rng(1)
    P = rng.standard_normal((40, 5)).astype(np.float32)
    ps, npc = np.array([0, 3, 10, 22]), np.array([3, 7, 12, 18])
    out = A._combine(P, ps, npc, 12)
    for r in range(3):
        acc = P[ps[r]].copy()
        for t in range(1, npc[r]):
            acc = acc + P[ps[r] + t]
        assert np.array_equal(out[r], acc)
    # 18 partials over 12 lane-groups: groups 0 .. 5 hold two each
    S = [P[22 + j] + P[22 + j + 12] if j < 6 else P[22 + j] for j in range(12)]
    acc = S[0]
    for j in range(1, 12):
        acc = acc + S[j]
    assert np.array_equal(out[3], acc)


def test_hot_sum_order():
    """the hot columns' order: 64-sample chunks, per = ceil(nlg / NG) chunks per lane-group, group sums in order"""
    rng = np.random.default_rng(2)
    B, NG = 64 * 30 + 5, 12
    b = np.sort(rng.choice(B, size=900, replace=False))
    b = b[(b // 64) != 7]                                      # an empty chunk
    xh = rng.standard_normal((b.size, 3)).astype(np.float32)
    nlg = (B + 63) // 64
    per = (nlg + NG - 1) // NG
    chunks = [np.zeros(3, np.float32) for _ in range(nlg)]
    seen = [False] * nlg
    for i, s in enumerate(b):
        c = s // 64
        chunks[c] = xh[i].copy() if not seen[c] else chunks[c] + xh[i]
        seen[c] = True
    groups = []
    for j in range(NG):
        if j * per >= nlg:
            break
        acc = chunks[j * per].copy()
        for c in range(j * per + 1, min((j + 1) * per, nlg)):
            acc = acc + chunks[c]
        groups.append(acc)
    acc = groups[0]
    for s in groups[1:]:
        acc = acc + s
    assert np.array_equal(A._hot_sum(xh, b, nlg, NG), acc)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_generator_makes_the_requested_runs(seed):
    rng = np.random.default_rng(seed)
    seq = list(rng.integers(1, 40, size=200))
    keys = rng.permutation(10_000)[:200].astype(np.int64) - 5000
    ids = A.layout_ids(seq, keys, rng)
    assert np.array_equal(A.run_lengths(ids), seq)
    idx = A.Index(ids)
    assert np.array_equal(idx.uniq, keys[:200])                     # groups in the order asked for
    for aw in (4, 8, 16):
        for name, s in (("boundaries", A.boundaries(aw)), ("pairs", A.pairs(aw, "at")), ("tree", A.tree(aw, [12], rng))):
            assert np.array_equal(A.run_lengths(A.layout_ids(s, np.arange(len(s)), rng)), s), name


@pytest.mark.parametrize("aw", [8, 16])
def test_standard_layouts_hit_their_targets(aw):
    rng = np.random.default_rng(aw)

    def cen(seq, D, vec, wide=False, **kw):
        return A.census(A.Index(A.layout_ids(seq, np.arange(len(seq)), rng)), D, vec, aw, wide, **kw)

    c = cen(A.boundaries(aw), 80, 4, True)
    assert not c["pairs_on"] and c["pairs"] > 0 and c["inside"] > 0 and c["blocks"][0]["pass_a"] == c["crossing"] > 100
    for rate, on in (("under", True), ("at", True), ("over", False)):
        s = A.pairs(aw, rate)
        c = cen(s, 16, 4)
        n, U = c["n"], c["U"]
        assert c["pairs_on"] == on and c["pairs"] >= 12, rate
        assert abs((n - U) * 16 - n) <= aw + 1, rate                  # just under / at / just over the threshold
        assert (rate == "at") == ((n - U) * 16 == n)
        if rate != "at":
            assert s[-1] == 2 and n % aw == 1                       # a pair ends the index; the final window holds one entry
    for D, vec, wide in ((80, 4, True), (16, 4, False), (1, 1, False), (128, 4, False)):
        ngs = [b[3] for b in A.col_blocks(D, vec, wide)]
        c = cen(A.tree(aw, ngs, rng), D, vec, wide)
        for b in c["blocks"]:
            assert b["at_ng"] >= 2 and b["at_ng1"] >= 2 and b["over_long"] >= 2 and b["pass_a"] > 0 and b["pass_b"] > 0
    for D, vec, wide, G in ((128, 4, False, 2), (80, 4, True, 3)):
        n_cap = A.MREC_APPLY_MAXB * 4 * G * aw
        s = A.grow(A.boundaries(aw), n_cap + 1)
        c = cen(s, D, vec, wide)
        assert c["n"] > n_cap and c["blocks"][0]["capped"] and c["crossing"] > 1000
    # out-of-range rows in crossing runs
    s = A.boundaries(aw)
    keys = np.arange(len(s), dtype=np.int64)
    keys[1::3] = -keys[1::3] - 1
    keys[2::3] += 2 ** 31 + 10
    c = A.census(A.Index(A.layout_ids(s, keys, rng)), 16, 4, aw, V=len(s))
    assert c["oob_crossing"] > 50


# the widths the wide-folded path is swept over (tests/test_wide_widths_gpu.py): D -> (lpr, G, NG, floats of the engine's fused row)
_WIDE_WIDTHS = {4: (2, 32, 128, 32), 12: (4, 16, 64, 64), 60: (16, 4, 16, 192), 84: (22, 2, 8, 256), 124: (32, 2, 8, 384),
                128: (33, 1, 4, 416), 172: (44, 1, 4, 544), 248: (63, 1, 4, 768), 252: (64, 1, 4, 768)}


def test_wide_geometry_of_the_swept_widths():
    import test_wide_widths_gpu as W
    assert W.W == list(_WIDE_WIDTHS) and set(W.EDGE) <= set(W.W)
    for D, (lpr, G, NG, ld) in _WIDE_WIDTHS.items():
        assert A.col_blocks(D, 4, wide=True) == [(0, D, G, NG)]
        assert lpr == D // 4 + 1 and G == 64 // lpr and G * lpr <= 64 and NG == 4 * G
        assert W._fused_ld(D) == ld and ld % 32 == 0 and 0 <= ld - (3 * D + 4) < 32
        assert NG * (D + 4) <= 1024                      # (const_finish_body's shared rows: NG lane-groups of D + 4 floats)


@pytest.mark.parametrize("B,nconst,dom", [(1024, 13, 0), (777, 5, 3), (65, 2, 0)])
def test_hot_sums_at_252_obey_the_bound_of_their_own_order(B, nconst, dom):
    """A.sums(..., hot=...) at D = 252 (G = 1, NG = 4) against a plain float64 sum of the same contributions.  The allowed difference
    comes from the data: depth * 2^-24 * sum |x| per element, depth the additions on the longest path of the restated order (63 inside a
    chunk of 64 samples, per - 1 over a lane-group's chunks, the lane-groups' sums - 1)."""
    rng = np.random.default_rng(B + nconst + dom)
    D, F, V, aw = 252, 39, 5000, 8
    ids = np.minimum(rng.zipf(1.1, size=(B, F)) + 64, V - 1).astype(np.int32)
    ids[:, :nconst] = np.arange(nconst, dtype=np.int32)[None, :] + 7
    for d in range(dom):
        ids[rng.random(B) < 0.4 + 0.1 * d, 20 + d] = 30 + d
    hot = {f: f + 7 for f in range(nconst)}
    hot.update({20 + d: 30 + d for d in range(dom)})
    n = B * F
    g = O.round16(rng.standard_normal((n, D)).astype(np.float32), "bf16")
    rs = (rng.random(n) + 0.25).astype(np.float32)
    gw = rng.standard_normal(B).astype(np.float32)
    x, xw = A.contributions(g, rs, 0.37), A.contributions(np.repeat(gw, F), rs, 0.37)
    idx = A.Index(ids)
    G = A.sums(idx, x, D, 4, aw, xw=xw, hot=hot, ids2d=ids)
    Gw = A.sums(idx, x, D, 4, aw, xw=xw)                                     # the same ids through the windows
    (_, _, _, NG), = A.col_blocks(D, 4, True)
    nlg = (B + 63) // 64
    per = (nlg + NG - 1) // NG
    depth = 63 + (per - 1) + ((nlg + per - 1) // per - 1)
    xa = np.concatenate([x, xw[:, None]], axis=1).astype(np.float64).reshape(B, F, D + 1)
    where = {int(k): u for u, k in enumerate(idx.uniq.tolist())}
    hrows = np.array([where[h] for h in hot.values()])
    for f, h in hot.items():
        sel = ids[:, f] == h
        assert sel.sum() >= B // 8 and not (np.delete(ids, f, axis=1) == h).any()
        exact, absum = xa[sel, f].sum(axis=0), np.abs(xa[sel, f]).sum(axis=0)
        err = np.abs(G[where[h]] - exact)
        assert (err <= depth * 2.0 ** -24 * absum).all(), (f, float((err / absum).max() / 2.0 ** -24), depth)
        assert np.abs(G[where[h]]).min() > 0
    other = np.ones(idx.U, bool)
    other[hrows] = False
    assert np.array_equal(G[other].view(np.uint32), Gw[other].view(np.uint32))        # only the hot ids' sums take the other order
    assert not np.array_equal(G[hrows], Gw[hrows])
