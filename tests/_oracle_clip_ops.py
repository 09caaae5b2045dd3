"""TEST INFRASTRUCTURE ONLY: tests/_oracle_ops.py with max_norm -- the clip of HashEmbeddingLookup / nn.EmbeddingLookup(max_norm=c)
(ClipByNorm per looked-up row, mindspore_rec/ops/embedding.py:156-161) restated in float64 on top of the oracle:
  gather_rows: each fp32 row x becomes x * (c / |x|) where |x| > c (float64), then row_scale, rounded to fp32 once;
  sparse_lazy_adam_: the oracle's per-position contributions (g * row_scale) * grad_scale summed per unique id in position order
  (fp32), each sum G replaced by J(x) G = (c / n)(G - (x.G / n^2) x) in float64 where n = |x| > c (x = the row before the
  update), then the oracle's LazyAdam over the unique ids with those sums."""
import numpy as np
import torch

import _oracle_ops
from _oracle_ops import *  # noqa: F401,F403
from _oracle_ops import _np
from oracle import oracle as O


def clip_rows64(x, c):
    """float64 rows of x clipped to norm c (ties and zero rows untouched); also returns the mask of clipped rows"""
    x = np.asarray(x, np.float64)
    n = np.sqrt((x * x).sum(axis=-1, keepdims=True))
    hit = n > c
    return np.where(hit, x * (c / np.where(hit, n, 1.0)), x), hit[..., 0]


def jacobian_apply64(x, G, c):
    """J(x) G per row in float64 (G where |x| <= c)"""
    x = np.asarray(x, np.float64)
    G = np.asarray(G, np.float64)
    n2 = (x * x).sum(axis=1, keepdims=True)
    n = np.sqrt(n2)
    hit = n > c
    d = (x * G).sum(axis=1, keepdims=True)
    safe = np.where(hit, n2, 1.0)
    return np.where(hit, (c / np.sqrt(safe)) * (G - (d / safe) * x), G)


def gather_rows(table, ids, row_scale=None, max_norm=None):
    if max_norm is None:
        return _oracle_ops.gather_rows(table, ids, row_scale)
    t = _np(table)
    flat = _np(ids).reshape(-1).astype(np.int64)
    ok = (flat >= 0) & (flat < t.shape[0])
    x = np.where(ok[:, None], t[np.where(ok, flat, 0)], 0.0)
    y, _ = clip_rows64(x, max_norm)
    if row_scale is not None:
        y = y * _np(row_scale).reshape(-1, 1).astype(np.float64)
    return torch.from_numpy(y.astype(np.float32))


def clipped_sums(p, ids, g, row_scale, grad_scale, c):
    """(unique ids in [0, V), their J(x)-transformed gradient sums as fp32)"""
    t = _np(p) if isinstance(p, torch.Tensor) else p
    flat = np.asarray(ids).reshape(-1).astype(np.int64)
    D = t.shape[1]
    gg = np.asarray(g, np.float32).reshape(flat.size, D)
    contrib = gg * np.asarray(row_scale, np.float32).reshape(-1, 1) if row_scale is not None else gg.copy()
    contrib = (contrib * np.float32(grad_scale)).astype(np.float32)
    ok = (flat >= 0) & (flat < t.shape[0])
    u, inv = np.unique(flat[ok], return_inverse=True)
    sums = np.zeros((u.size, D), np.float32)
    np.add.at(sums, inv, contrib[ok])                    # position order per id, fp32
    return u, jacobian_apply64(t[u], sums, c).astype(np.float32)


def sparse_lazy_adam_(p, m, v, plan, g, row_scale=None, lr=3.5e-4, beta1=0.9, beta2=0.999, eps=1e-8, beta1_power=0.9,
                      beta2_power=0.999, grad_scale=1.0, use_nesterov=False, max_norm=None):
    if max_norm is None:
        return _oracle_ops.sparse_lazy_adam_(p, m, v, plan, g, row_scale, lr, beta1, beta2, eps, beta1_power, beta2_power, grad_scale,
                                             use_nesterov)
    u, sums = clipped_sums(p, plan.ids, _np(g), _np(row_scale) if row_scale is not None else None, grad_scale, max_norm)
    O.sparse_lazy_adam(_np(p), _np(m), _np(v), u, sums, None, lr=lr, b1=beta1, b2=beta2, eps=eps, b1_pow=beta1_power,
                       b2_pow=beta2_power, grad_scale=1.0, nesterov=use_nesterov)
