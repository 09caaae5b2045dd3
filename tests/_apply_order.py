"""TEST INFRASTRUCTURE ONLY: the sparse apply's order of additions (mindrec_amd/csrc/mrec_apply.hip) restated on the host, so that every
row of every path of the apply can be required to match bit for bit (the library is built with -ffp-contract=off, like the oracle).

What is restated, each rule with the kernel lines it follows:
  * the sorted index: oracle.unique, then a stable argsort of inv (mrec_group_by_inverse; test_gpu_parity.test_unique_and_group);
    with skip_negative the negative ids have no group and no entry (include/mrec.h, MREC_PLAN_SKIP_NEGATIVE);
  * a position's contribution x_i = fp32(fp32(g_i * rs_i) * grad_scale) (apply_main_body: gwiden, vmul rscale, vmul gscale); the wide
    lane's is the same with gw[i / F] in place of the row (vzero + vset_x);
  * the geometry of a column block (apply_impl / apply_cols): vec = 4 / 2 / 1 by alignment, CB = 64 vec columns per launch,
    lpr = Dc / vec (+ 1 wide lane), G = 64 // lpr lane-groups per wave, NG = 4 G lane-groups per workgroup, AW from
    mrec_sparse_apply_window (the caller passes it: ops.apply_window(D, vec == 4));
  * a (run, window) piece is summed in ascending sorted order, starting from its first contribution (apply_main_body: acc = x at a
    run start, vadd after it);
  * a run whose pieces are P_0 (the owner's tail) .. P_k (the heads) is finished per column block as k_apply_long does: lane-group j
    sums P_t, t = j (mod NG), in ascending t (pass B's round-robin), and the result is S_0 + S_1 + .. + S_{min(k + 1, NG) - 1}
    added left to right (group 0's loop over `red`).  For k + 1 <= NG every S_j is one partial: that is pass A's loop over the
    heads in order.  A straddling pair that k_apply_main sums in place (MREC_PAIRS: head_pair / tail_pair) needs no rule of its
    own: its sum is a + b whichever window forms it, and a + b is what pass A adds too;
  * the hot columns (const_part_body / const_finish_body): chunks of 64 samples, each summed in sample order over the samples that
    hold the hot id (an empty chunk is +0.0); with per = ceil(nlg / NG), lane-group j sums chunks [j per, (j + 1) per) in order and
    group 0 adds the lane-groups' sums in order.  Constant and dominant ids alike: every entry of a hot id is hot.
The updates then go through the oracle with G as the gradient (row_scale None, grad_scale 1.0: multiplying by 1.0 is exact, and the
oracle's element formulas are adam_elem / ftrl_elem of mrec_optim.h operation for operation)."""
import numpy as np

from oracle import oracle as O

# mrec_apply.hip's defaults for the macros the census needs (a build that overrides them changes who sums what, not the order)
MREC_PAIRS_DUP_DIV = 16        # mrec_apply.hip: "#define MREC_PAIRS_DUP_DIV 16" (pairs_on: (n - groups) * 16 <= n)
MREC_APPLY_MAXB = 4096         # mrec_apply.hip: "#define MREC_APPLY_MAXB 4096u" (k_apply_main's grid cap)
MREC_LONG_AB = 16              # mrec_apply.hip: "#define MREC_LONG_AB 16" (partials in flight per lane-group in pass B)


# ---- the sorted index ---------------------------------------------------------------------------------------------------------------
class Index:
    """uniq (first-occurrence order), spos / sseg (the sorted index proper: positions grouped, ascending inside a group), offs [U + 1]."""

    def __init__(self, ids, skip_negative=False):
        flat = np.ascontiguousarray(ids).ravel()
        if skip_negative:
            self.uniq, inv = O.unique_skip_negative(flat)
        else:
            self.uniq, inv = O.unique(flat)
        inv = inv.astype(np.int64)
        pos = np.nonzero(inv >= 0)[0]
        self.spos = pos[np.argsort(inv[pos], kind="stable")]
        self.sseg = inv[self.spos]
        self.U = self.uniq.size
        self.n = self.spos.size
        self.offs = np.concatenate([[0], np.cumsum(np.bincount(self.sseg, minlength=self.U))]).astype(np.int64)


def lane_width(D, ld, ldg, state_ptrs, g_ptr, g_elem_bytes):
    """apply_impl's vec: 16-byte lanes where rows and pointers allow it and D % 4 == 0, else 8-byte lanes (D % 2 == 0), else 4."""
    a16 = ld % 4 == 0 and ldg % 4 == 0 and g_ptr % (4 * g_elem_bytes) == 0 and all(p % 16 == 0 for p in state_ptrs)
    a8 = ld % 2 == 0 and ldg % 2 == 0 and g_ptr % (2 * g_elem_bytes) == 0 and all(p % 8 == 0 for p in state_ptrs)
    return 4 if (a16 and D % 4 == 0) else (2 if (a8 and D % 2 == 0) else 1)


def col_blocks(D, vec, wide=False):
    """[(c0, Dc, G, NG)] of apply_impl's launches over columns [c0, c0 + Dc)."""
    out = []
    CB = 64 * vec
    for c0 in range(0, D, CB):
        Dc = min(CB, D - c0)
        lpr = Dc // vec + (1 if wide else 0)
        G = 64 // lpr
        out.append((c0, Dc, G, 4 * G))
    return out


def contributions(g, row_scale, grad_scale):
    """x_i = fp32(fp32(g_i * rs_i) * grad_scale), g already widened to fp32 (16-bit values widen exactly)"""
    x = np.asarray(g, np.float32)
    if row_scale is not None:
        x = x * np.asarray(row_scale, np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    return (x * np.float32(grad_scale)).astype(np.float32)


# ---- the sums -----------------------------------------------------------------------------------------------------------------------
def _pieces(idx, aw):
    """piece number of every sorted entry (a new piece at every run start and every window start), first piece and count per run"""
    e = np.arange(idx.n)
    win = e // aw
    new = np.ones(idx.n, bool)
    new[1:] = (idx.sseg[1:] != idx.sseg[:-1]) | (win[1:] != win[:-1])
    pid = np.cumsum(new) - 1
    ps = pid[idx.offs[:-1]]
    npc = pid[idx.offs[1:] - 1] - ps + 1
    return pid, ps, npc


def _combine(P, ps, npc, NG):
    """k_apply_long's tree: lane-group j sums partials t = j (mod NG) in order, group 0 adds the lane-group sums in group order"""
    out = P[ps].copy()
    cr = np.nonzero(npc > 1)[0]
    if cr.size == 0:
        return out
    p0, k1 = ps[cr], npc[cr]
    tot = None
    for j in range(min(NG, int(k1.max()))):
        has = np.nonzero(k1 > j)[0]
        S = P[p0[has] + j].copy()
        t = j + NG
        while True:
            more = k1[has] > t
            if not more.any():
                break
            S[more] = S[more] + P[p0[has[more]] + t]
            t += NG
        if j == 0:
            tot = S
        else:
            tot[has] = tot[has] + S
    out[cr] = tot
    return out


def _hot_sum(xh, b, nlg, NG):
    """const_part_body + const_finish_body over the contributions xh of samples b (ascending) of one hot column"""
    C = O.segment_sum(xh, (b // 64).astype(np.int32), nlg)                 # chunk sums, sample order; an empty chunk is +0.0
    per = (nlg + NG - 1) // NG
    ng = (nlg + per - 1) // per
    L = O.segment_sum(C, (np.arange(nlg) // per).astype(np.int32), ng)      # lane-group sums, chunk order
    acc = L[0].copy()
    for j in range(1, ng):
        acc = acc + L[j]
    return acc


def sums(idx, x, D, vec, aw, xw=None, hot=None, ids2d=None):
    """Per unique id (idx.uniq order), the fp32 gradient sum G as the apply forms it: [U, D] (+ the wide column: [U, D + 1]).
    x: [n, D] contributions by position; xw: [n] the wide lane's contributions (wide apply) or None; hot: {field: hot id} of the
    hot-column path (wide apply, [B, F] ids2d) or None."""
    wide = xw is not None
    xs = np.asarray(x, np.float32)[idx.spos]
    if wide:
        xs = np.concatenate([xs, np.asarray(xw, np.float32)[idx.spos][:, None]], axis=1)
    W = xs.shape[1]
    if idx.n == 0:
        return np.zeros((idx.U, W), np.float32)
    pid, ps, npc = _pieces(idx, aw)
    P = O.segment_sum(xs, pid.astype(np.int32), int(pid[-1]) + 1)
    G = np.empty((idx.U, W), np.float32)
    for c0, Dc, _, NG in col_blocks(D, vec, wide):
        cols = list(range(c0, c0 + Dc)) + ([D] if wide else [])
        G[:, cols] = _combine(P[:, cols], ps, npc, NG)
    if hot:
        B, F = ids2d.shape
        nlg = (B + 63) // 64
        NG = col_blocks(D, vec, wide)[0][3]
        xa = np.concatenate([np.asarray(x, np.float32), np.asarray(xw, np.float32)[:, None]], axis=1)
        where = {int(k): u for u, k in enumerate(idx.uniq.tolist())}
        for f, h in hot.items():
            b = np.nonzero(ids2d[:, f] == h)[0]
            G[where[int(h)]] = _hot_sum(xa[b * F + f], b, nlg, NG)
    return G


# ---- the updates --------------------------------------------------------------------------------------------------------------------
def lazy_adam(p, m, v, uniq, G, **kw):
    """LazyAdam with the restated sums (p, m, v: [V, D] numpy views, updated in place)"""
    D = p.shape[1]
    O.sparse_lazy_adam(p, m, v, uniq, np.ascontiguousarray(G[:, :D]), None, grad_scale=1.0, **kw)


def ftrl(var, accum, linear, uniq, G, **kw):
    D = var.shape[1]
    O.sparse_ftrl(var, accum, linear, uniq, np.ascontiguousarray(G[:, :D]), None, grad_scale=1.0, **kw)


def wide_ftrl(rec, uniq, G, **kw):
    """FTRL on the wide record [w, accum, linear, pad] (rec: a [V, 4] numpy view) with G's wide column"""
    O.sparse_ftrl(rec[:, 0:1], rec[:, 1:2], rec[:, 2:3], uniq, np.ascontiguousarray(G[:, -1:]), None, grad_scale=1.0, **kw)


# ---- the census ---------------------------------------------------------------------------------------------------------------------
def census(idx, D, vec, aw, wide=False, V=None, hot_ids=()):
    """What a batch's index makes the apply do.  Global: straddling pairs, pairs_on, windows wholly inside one run; per column block:
    crossing runs finished by pass A / pass B, runs of k + 1 = NG, NG + 1 and > 16 NG partials, whether the grid is capped; crossing runs
    whose row lies outside [0, V)."""
    n = idx.n
    L = np.diff(idx.offs)
    fw, lw = idx.offs[:-1] // aw, (idx.offs[1:] - 1) // aw
    npc = lw - fw + 1
    hot = np.isin(idx.uniq.astype(np.int64), np.asarray(list(hot_ids), np.int64))
    cross = (npc > 1) & ~hot
    pair = cross & (L == 2)
    groups = int(idx.sseg[n - 1]) + 1 if n else 0
    pairs_on = (n - groups) * MREC_PAIRS_DUP_DIV <= n
    fin = cross & ~(pair & pairs_on)                  # runs k_apply_long finishes
    c = dict(n=n, U=idx.U, crossing=int(cross.sum()), pairs=int(pair.sum()), pairs_on=bool(pairs_on),
             inside=int(np.maximum(npc[cross] - 2, 0).sum()), blocks=[])
    if V is not None:
        u = idx.uniq.astype(np.int64)
        c["oob_crossing"] = int((fin & ((u < 0) | (u >= V))).sum())
    nsw = -(-n // aw)
    for _, _, G, NG in col_blocks(D, vec, wide):
        c["blocks"].append(dict(NG=NG, pass_a=int((fin & (npc <= NG)).sum()), pass_b=int((fin & (npc > NG)).sum()),
                                at_ng=int((fin & (npc == NG)).sum()), at_ng1=int((fin & (npc == NG + 1)).sum()),
                                over_long=int((fin & (npc > NG * MREC_LONG_AB)).sum()),
                                capped=-(-nsw // (4 * G)) > MREC_APPLY_MAXB))
    return c


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
def layout_ids(lengths, keys, rng):
    """ids whose sorted index is exactly the run sequence `lengths` over groups keyed keys[0], keys[1], ..: the first occurrences in
    group order, then the remaining copies shuffled behind them (a run starts wherever the lengths in front of it put it)."""
    L = np.asarray(lengths, np.int64)
    U = L.size
    keys = np.asarray(keys)
    assert keys.size >= U and np.unique(keys[:U]).size == U
    rest = np.repeat(np.arange(U), L - 1)
    rng.shuffle(rest)
    return keys[np.concatenate([np.arange(U), rest])]


def run_lengths(ids):
    return np.diff(Index(ids).offs)


def _pad_to(seq, cur, off, aw):
    while cur % aw != off:
        seq.append(1)
        cur += 1
    return cur


def boundaries(aw):
    """every run length 1 .. 3 aw + 1 at every start offset 0 .. aw - 1 (singletons in between)"""
    seq, cur = [], 0
    for L in range(1, 3 * aw + 2):
        for o in range(aw):
            cur = _pad_to(seq, cur, o, aw)
            seq.append(L)
            cur += L
    return seq


def tree(aw, ngs, rng):
    """runs of k + 1 = NG - 1, NG, NG + 1, 16 NG, 16 NG + 1 partials for every NG in ngs, from a window start and from elsewhere"""
    seq, cur = [], 0
    for NG in sorted(set(ngs)):
        for P in (NG - 1, NG, NG + 1, MREC_LONG_AB * NG, MREC_LONG_AB * NG + 1):
            for o in (0, int(rng.integers(1, aw))):
                cur = _pad_to(seq, cur, o, aw)
                L = (aw - o) + (P - 2) * aw + int(rng.integers(1, aw + 1))
                seq.append(L)
                cur += L
    return seq


def pairs(aw, rate):
    """Nearly duplicate-free: singletons and straddling pairs, with the duplicate rate just under ('under'), at ('at') or just over
    ('over') the pairs_on threshold (n - U) * 16 <= n.  Around the pairs: runs of 3 that straddle a boundary 2 + 1 and 1 + 2, a pair
    with a run of 3 right in front of it and right behind it (seg_before2 / seg_after); 'under' and 'over' end on a pair whose
    second entry is the index's last and the final window's only entry."""
    body, cur = [], 0
    for _ in range(12):                                  # plain straddling pairs
        cur = _pad_to(body, cur, aw - 1, aw)
        body.append(2)
        cur += 2
    for o in (aw - 2, aw - 1):                           # runs of 3 across a boundary, 2 + 1 and 1 + 2
        cur = _pad_to(body, cur, o, aw)
        body.append(3)
        cur += 3
    cur = _pad_to(body, cur, aw - 4, aw)                 # run of 3, straddling pair, run of 3
    body += [3, 2, 3]
    cur += 8
    cur = _pad_to(body, cur, 0, aw)
    d0, n0 = sum(L - 1 for L in body), cur
    K = MREC_PAIRS_DUP_DIV
    for t in range(0, 800):                              # t blocks of aw entries in front: a of them [pair, singletons], b singletons
        for a in range(0, t + 1):
            d, base = d0 + a, n0 + aw * t
            if rate == "at":
                r = K * d - base
                if 0 <= r < aw:
                    return ([2] + [1] * (aw - 2)) * a + [1] * (aw * (t - a)) + body + [1] * r
            else:
                nn = base + aw + 1                         # + aw - 1 singletons and the closing pair
                d += 1
                if (rate == "under" and K * d <= nn < K * d + aw) or (rate == "over" and K * d - aw <= nn < K * d):
                    return ([2] + [1] * (aw - 2)) * a + [1] * (aw * (t - a)) + body + [1] * (aw - 1) + [2]
    raise AssertionError("no pairs layout")


def grow(seq, n_min):
    """the sequence repeated until it holds at least n_min entries (the grid-capped layouts)"""
    one, out, n = list(seq), [], 0
    while n < n_min:
        out += one
        n += sum(one)
    return out
