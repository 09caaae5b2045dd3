"""TEST INFRASTRUCTURE ONLY: the backward of the multitable Wide&Deep's input stage (mindrec_amd/csrc/mrec_multitable.hip,
mrec_mt_input_bwd; the contract: include/mrec.h) restated on the host in numpy float64.

A group is the list of _multitable_ref.Seg records that share a table (of a Seg only the table's width, ids, col, pooled and mask are
used).  Position i = b * Ls + s of the group's ids [B, Ls] lies in the segment whose slots hold s and contributes
  deep: g_x[b, c0 : c0 + D] * scale   (c0, scale) = (col + s_local * D, mask) for a single-hot segment, (col, fp32(mask * fp32(1 / L)))
                                       for a pooled one -- the scale is the kernel's fp32 value, widened: it is an INPUT of the sum
  wide: g_wide[b] * mask
summed per id (np.add.at over positions) and multiplied by grad_scale.  Every output comes with its first-order bound for an fp32
sum of n terms in any order: n * 2^-24 * sum |term| (n - 1 additions and the term's own product rounding) plus one rounding of the
result, (|result| + that) * 2^-24 * 2 (the multiplication by grad_scale and, for a long group, nothing more: its pieces are terms
of the same sum) -- the bound _multitable_ref.wide_sum's callers use for the forward."""
import numpy as np

EPS = 2.0 ** -24


def group_ids(segs):
    return np.concatenate([np.asarray(s.ids).reshape(s.ids.shape[0], -1) for s in segs], axis=1)


def group_sums(g_x, g_wide, segs, grad_scale=1.0, apply_bounds=False):
    """-> (uniq ids in first-occurrence order [U], sums [U, D], bound [U, D], wsums [U], wbound [U]) in float64, and, with
    apply_bounds, two more: the bounds of ops.segment_sum computing the same sums [U, D] / [U] -- its contribution is
    fp32(fp32(g * row_scale) * scale), ONE more product rounding per term than the kernel's, so n + 1 in place of n"""
    g_x, g_wide = np.asarray(g_x, np.float64), np.asarray(g_wide, np.float64)
    ids = group_ids(segs)
    B, Ls = ids.shape
    D = segs[0].table.shape[1]
    flat = ids.reshape(-1)
    uniq, first, inv = np.unique(flat, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                # first-occurrence order, as ops.sparse_plan numbers the groups
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    inv = rank[inv.reshape(-1)]
    U = uniq.size
    terms = np.zeros((B, Ls, D))
    wterms = np.zeros((B, Ls))
    s0 = 0
    for seg in segs:
        L = seg.ids.shape[1]
        m = np.ones((B, L), np.float32) if seg.mask is None else np.asarray(seg.mask, np.float32)
        for sl in range(L):
            if seg.pooled:
                c0 = seg.col
                scale = (m[:, sl] * (np.float32(1.0) / np.float32(L))).astype(np.float32)
            else:
                c0, scale = seg.col + sl * D, m[:, sl]
            terms[:, s0 + sl, :] = g_x[:, c0:c0 + D] * scale.astype(np.float64)[:, None]
            wterms[:, s0 + sl] = g_wide * m[:, sl].astype(np.float64)
        s0 += L
    terms, wterms = terms.reshape(B * Ls, D), wterms.reshape(B * Ls)
    sums, asum, cnt = np.zeros((U, D)), np.zeros((U, D)), np.zeros(U)
    ws, was = np.zeros(U), np.zeros(U)
    np.add.at(sums, inv, terms)
    np.add.at(asum, inv, np.abs(terms))
    np.add.at(ws, inv, wterms)
    np.add.at(was, inv, np.abs(wterms))
    np.add.at(cnt, inv, 1.0)
    gs = float(np.float32(grad_scale))
    bound = (cnt[:, None] * EPS * asum) * abs(gs)
    wbound = (cnt * EPS * was) * abs(gs)
    sums, ws = sums * gs, ws * gs
    bound += (np.abs(sums) + bound) * 2 * EPS
    wbound += (np.abs(ws) + wbound) * 2 * EPS
    if apply_bounds:
        ab, awb = ((cnt + 1)[:, None] * EPS * asum) * abs(gs), ((cnt + 1) * EPS * was) * abs(gs)
        return uniq[order], sums, bound, ws, wbound, ab + (np.abs(sums) + ab) * 2 * EPS, awb + (np.abs(ws) + awb) * 2 * EPS
    return uniq[order], sums, bound, ws, wbound


def cont_grads(g_wide, cont, grad_scale=1.0):
    """-> (d_wide_cont [C], its bound, d_wide_bias, its bound) in float64"""
    g, c = np.asarray(g_wide, np.float64), np.asarray(cont, np.float64)
    gs, B = float(np.float32(grad_scale)), g.shape[0]
    t = g[:, None] * c
    d, a = t.sum(0) * gs, np.abs(t).sum(0) * abs(gs)
    db, ab = g.sum() * gs, np.abs(g).sum() * abs(gs)
    bd = B * EPS * a
    bb = B * EPS * ab
    return d, bd + (np.abs(d) + bd) * 2 * EPS, db, bb + (abs(db) + bb) * 2 * EPS
