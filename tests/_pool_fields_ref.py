"""TEST INFRASTRUCTURE ONLY: the fields form of the multi-hot path (mrec_gather_pool_fields, the fields form of mrec_apply_opts_t)
restated on the host in np.float32, on top of tests/_pool_ref.py and tests/_apply_order.py, which it does not change.

A sample is Ls = sum(field_len) slots, F bags back to back: field f holds slots off_f .. off_f + L_f - 1, off_f = L_0 + .. + L_{f-1}.
  gather_pool_fields: field f of every sample is _pool_ref.gather_pool of ids[:, off_f : off_f + L_f] -- the same slot-by-slot sum, the
    mean divided ONCE by np.float32(L_f), the FIELD's length -- written to columns f * D .. (f + 1) * D - 1.
  contributions: position i = b * Ls + s, s a slot of field f, contributes x_i = fp32(fp32(g[b * F + f] * rs_i) * fs_f): the rule of
    _apply_order.contributions with the gradient row of the position's BAG and the scale of its FIELD.  _pool_ref.sums then adds
    them over the plan's index with no new rule (the windows and the tree of partial sums do not know about fields).
  field_scales: MultiHotEmbedding.apply_'s scales, fp32(grad_scale / L_f) for the mean (ReduceMean's bprop), grad_scale for the sum."""
import numpy as np

import _pool_ref as P


def offsets(field_len):
    return np.concatenate([[0], np.cumsum(np.asarray(field_len, np.int64))])[:-1]


def slot_field(field_len):
    """field of every slot of a sample, [Ls]"""
    return np.repeat(np.arange(len(field_len)), np.asarray(field_len, np.int64))


def gather_pool_fields(table, ids, field_len, mask=None, mode="mean", out_dtype="f32"):
    """table [V, D], ids [B, Ls], mask [B, Ls] float32 or None -> [B, F * D] float32 holding the values of out_dtype"""
    ids = np.asarray(ids)
    assert ids.ndim == 2 and ids.shape[1] == sum(field_len)
    cols = []
    for off, L in zip(offsets(field_len), field_len):
        m = None if mask is None else np.asarray(mask, np.float32)[:, off:off + L]
        cols.append(P.gather_pool(table, ids[:, off:off + L], m, mode, out_dtype))
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def bag_rows(field_len, n):
    """(gradient row b * F + f, field f) of every position i < n"""
    Ls, F = sum(field_len), len(field_len)
    i = np.arange(n)
    f = slot_field(field_len)[i % Ls]
    return (i // Ls) * F + f, f


def expand(g, field_len, n):
    """the gradient row of every position: g[b * F + f]"""
    return np.asarray(g)[bag_rows(field_len, n)[0]]


def contributions(g, field_len, n, row_scale, field_scale):
    """x_i = fp32(fp32(g[b * F + f] * rs_i) * fs_f) for the n positions (g [B * F, D] already widened to fp32)"""
    rows, f = bag_rows(field_len, n)
    x = np.asarray(g, np.float32)[rows]
    if row_scale is not None:
        x = (x * np.asarray(row_scale, np.float32).reshape(-1, 1)).astype(np.float32)
    return (x * np.asarray(field_scale, np.float32)[f][:, None]).astype(np.float32)


def field_scales(grad_scale, field_len, mode):
    return tuple(P.mean_scale(grad_scale, L, mode) for L in field_len)
