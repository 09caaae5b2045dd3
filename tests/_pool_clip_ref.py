"""TEST INFRASTRUCTURE ONLY: inputs and the lookup reference of tests/test_pool_clip_gpu.py (max_norm over multi-hot fields).

  special_table: rows whose norms spread around c (median c: both branches of the clip run), plus the rows a clip gets wrong first --
    a zero row, a row whose norm is EXACTLY c ((c, 0, ..): a tie is not clipped) and rows scaled to within a few ulps of c on either
    side.
  clipped_pool: the pooled lookup with max_norm built from an existing, separately tested kernel and the host restatement of the
    pooling: `rows` [n, D] -- one CLIPPED fp32 row per slot, ops.gather_rows(.., max_norm=c) of the slot's id or of the slot's
    MapTensorGet row, a zero row where the dense form's id is out of range -- are the "table" of _pool_fields_ref.gather_pool_fields
    under the ids arange(n).reshape(B, Ls): product with the mask, slot-order adds, one division, one rounding."""
import numpy as np

import _pool_fields_ref as FR

ZERO_ROW, TIE_ROW, NEAR0, NEAR1 = 0, 1, 2, 10           # rows NEAR0 .. NEAR1 - 1: within a few ulps of c


def special_table(rng, V, D, c):
    """[V, D] float32; c must be a float32 whose square is exact (0.75, 0.5, 0.078125, ..) so that the tie row's fp32 norm is c"""
    c32 = np.float32(c)
    assert float(c32) == c and float(np.float32(c32 * c32)) == c * c
    t = rng.standard_normal((V, D))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    scale = np.exp(rng.standard_normal((V, 1)) * 0.5)                  # log-normal around 1: the median norm is c
    tab = (t * scale * c).astype(np.float32)
    tab[ZERO_ROW] = 0.0
    tab[TIE_ROW] = 0.0
    tab[TIE_ROW, 0] = c32
    k = np.arange(NEAR0, NEAR1)
    tab[k] = (t[k] * (c * (1.0 + (k - (NEAR0 + NEAR1) // 2 + 0.5)[:, None] * 2.0 ** -23))).astype(np.float32)
    return tab


def ids_with_outsiders(rng, B, Ls, V, dtype):
    """ids over the whole table, -1 and V among them, every special row present"""
    ids = rng.integers(-1, V + 1, size=(B, Ls))
    flat = ids.reshape(-1)
    flat[: NEAR1 + 2] = np.concatenate([np.arange(NEAR1), [-1, V]])[: flat.size]
    return rng.permutation(flat).reshape(B, Ls).astype(dtype)


def clipped_pool(rows, B, lens, mask, mode, kind="f32"):
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    assert n == B * sum(lens)
    return FR.gather_pool_fields(rows, np.arange(n).reshape(B, sum(lens)), lens, mask, mode, kind)
