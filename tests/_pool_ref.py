"""TEST INFRASTRUCTURE ONLY: the multi-hot lookup (mindrec_amd/csrc/mrec_pool.hip) and the pooled sparse apply's contributions
restated on the host in np.float32, so that every output can be required to match bit for bit (the library is built with
-ffp-contract=off, like the oracle).

  gather_pool: per bag, slot by slot in ascending order: the row (a +0.0 row for an id outside [0, V)), its product with the slot's
    mask value (no product where mask is None), slot 0's product starts the sum and every later one is added to it; mode "mean": ONE
    division by np.float32(L) -- the bag's length, whatever the mask holds (ReduceMean over the bag axis, models/
    wide_and_deep_multitable/src/wide_and_deep.py:301-346); 16-bit outputs: ONE rounding, the oracle's round16.
  pooled_contributions: position i = b * L + l of the pooled apply contributes (g[i // L] * row_scale[i]) * grad_scale -- tests/
    _apply_order.contributions over the gradient rows indexed i // L; _apply_order.sums then adds them with no new rule.
  sums: _apply_order.sums, plus the one bit its restatement loses where a 0/1 mask is the row_scale: the kernels START a piece's sum
    from its first contribution (apply_main_body: acc = x at a run start) and add partial sums to each other, so a sum whose
    contributions are ALL -0.0 (a row whose every position is masked, under negative gradient values) is -0.0, while the oracle's
    segment sum starts from +0.0 and returns +0.0.  With any other contribution among them both give the same bits (x + -0.0 = x,
    +0.0 + -0.0 = +0.0, and an exact cancellation rounds to +0.0 either way).  The optimizers do not see the difference; a segment
    sum hands it out."""
import numpy as np

import _apply_order as A
from oracle import oracle as O


def gather_pool(table, ids, mask=None, mode="mean", out_dtype="f32"):
    """table [V, D] float32 (any row stride), ids [..., L], mask [..., L] float32 or None -> [..., D] float32 holding the values of
    out_dtype ('f32', 'bf16', 'f16')"""
    t = np.asarray(table)
    assert t.dtype == np.float32 and t.ndim == 2
    V, D = t.shape
    ids = np.asarray(ids)
    L = ids.shape[-1]
    flat = ids.reshape(-1, L).astype(np.int64)
    m = None if mask is None else np.asarray(mask, np.float32).reshape(-1, L)
    acc = None
    for l in range(L):
        r = flat[:, l]
        ok = (r >= 0) & (r < V)
        x = np.where(ok[:, None], t[np.where(ok, r, 0)], np.float32(0.0)).astype(np.float32)
        p = x if m is None else (x * m[:, l:l + 1]).astype(np.float32)
        acc = p if l == 0 else (acc + p).astype(np.float32)
    if mode == "mean":
        acc = (acc / np.float32(L)).astype(np.float32)
    else:
        assert mode == "sum"
    if out_dtype != "f32":
        acc = O.round16(acc, out_dtype)
    return np.ascontiguousarray(acc).reshape(tuple(ids.shape[:-1]) + (D,))


def expand(g, L, n):
    """the gradient row of every position: g[i // L], i < n"""
    return np.asarray(g)[np.arange(n) // L]


def pooled_contributions(g, L, n, row_scale, grad_scale):
    """x_i = fp32(fp32(g[i // L] * rs_i) * grad_scale) for the n positions of bags of L (g already widened to fp32)"""
    return A.contributions(expand(np.asarray(g, np.float32), L, n), row_scale, grad_scale)


def mean_scale(grad_scale, L, mode):
    """MultiHotEmbedding.apply_'s grad_scale: fp32(grad_scale / L) for the mean (ReduceMean's bprop), grad_scale for the sum"""
    return float(np.float32(grad_scale) / np.float32(L)) if mode == "mean" else float(grad_scale)


def sums(idx, x, D, vec, aw):
    """_apply_order.sums with the sign of the all-(-0.0) sums (see the module docstring)"""
    G = A.sums(idx, x, D, vec, aw)
    if idx.n == 0:
        return G
    neg0 = (np.ascontiguousarray(x, np.float32).view(np.uint32) == np.uint32(0x80000000)).astype(np.float32)
    cnt = O.segment_sum(neg0[idx.spos], idx.sseg.astype(np.int32), idx.U)          # (counts below 2^24: exact in fp32)
    all_neg0 = cnt == np.diff(idx.offs).astype(np.float32)[:, None]
    G[all_neg0] = np.float32(-0.0)
    return G
