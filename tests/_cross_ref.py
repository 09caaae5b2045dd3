"""Host references for the DCN-v1 cross stack (mindrec_amd/csrc/mrec_cross.hip), numpy only.

cross_f64            the stack layer by layer, y = x0 * (x_l . w_l) + b_l + x_l, and its reverse-mode gradient, in float64:
                     the judge.  It knows nothing of the kernel's closed form.
cross_bwd_closed_f32 the closed form the backward kernel evaluates (the comment at the top of mrec_cross.hip) in float32 with
                     numpy's own summation: the kernel's algebra and precision, not its order of additions -- what fp32 can
                     deliver on these expressions, the yardstick the kernel's error is held against.
cross_fwd_bits       the forward in float32 in the kernel's own order of operations (lane ownership, slot order, wave sum): what
                     ops.cross_layers must return BIT FOR BIT.  lane_tree / lane_butterfly are the two wave sums.
row_rel / layer_rel  max over rows of |a - r|_2 / |r|_2.
"""
import numpy as np

BUCKETS = (1, 2, 4, 8, 12, 16, 20, 24, 32)      # a row's padded width in 64-column passes (npl_bucket in mrec_cross.hip)

# The shapes at which the forward's bits are pinned.  B = 3: no wave has a second row of its pair; B = 33: every wave of the first
# workgroup has a first row and one of them a second.  (D, L): one column per lane up to D = 128, four from 129 on; (130, 9) is
# past the 8 layers that the four-column form stages in LDS, so w / b come from global memory.
BITS_B = (3, 33)
BITS_DL = ((2, 1), (64, 6), (65, 3), (128, 8), (100, 9), (129, 1), (257, 6), (1170, 6), (2048, 8), (130, 9))


def inputs(B, D, L):
    """The inputs of tests/test_gpu_parity.py::test_cross_layers, seeded from the shape."""
    rng = np.random.default_rng([B, D, L])
    x0 = (rng.standard_normal((B, D)) * 0.5).astype(np.float32)
    w = (rng.standard_normal((L, D)) / np.sqrt(D)).astype(np.float32)
    b = (rng.standard_normal((L, D)) * 0.1).astype(np.float32)
    dy = rng.standard_normal((B, D)).astype(np.float32)
    return x0, w, b, dy


def cross_f64(x0, w, b, dy=None):
    """y, dx0, dw, db in float64 (dx0, dw, db are None without dy)."""
    x0 = np.asarray(x0, np.float64); w = np.asarray(w, np.float64); b = np.asarray(b, np.float64)
    L = w.shape[0]
    xs = [x0]
    for l in range(L):
        xl = xs[-1]
        xs.append(x0 * (xl @ w[l])[:, None] + b[l] + xl)
    if dy is None:
        return xs[-1], None, None, None
    gy = np.asarray(dy, np.float64).copy()          # d loss / d x_{l+1}
    gx0 = np.zeros_like(x0)
    dw = np.zeros_like(w); db = np.zeros_like(b)
    for l in range(L - 1, -1, -1):
        xl = xs[l]
        s = xl @ w[l]                               # [B]
        t = (gy * x0).sum(axis=1)                   # [B]: gy . x0
        db[l] = gy.sum(axis=0)
        dw[l] = t @ xl
        gx0 += gy * s[:, None]
        gy = gy + t[:, None] * w[l]
    return xs[-1], gx0 + gy, dw, db


def lane_tree(t):
    """[B, 64] -> [B]: the lanes pairwise in lane order, six levels (wave_sum_dpp)"""
    while t.shape[1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]


def lane_butterfly(t):
    """[B, 64] -> [B]: t = t + t[lane ^ d] for d = 32, 16, 8, 4, 2, 1 (wave_sum); every lane ends with the same bits"""
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        t = t + t[:, lanes ^ d]
    return t[:, 0]


def cross_fwd_bits(x0, w, b, swap_sums=False):
    """x_L [B, D] in float32, every multiply and add rounded on its own (-ffp-contract=off), in the forward kernel's order:
      D <= 128: lane l owns columns l + 64 j;  p = +0;  p += x_l[j] w_l[j] for j in slot order;  s = lane_butterfly(p)
      D > 128:  lane l owns columns 256 q + 4 l + {0..3};  p = (+0, +0, +0, +0);  p += x_l[q] * w_l[q] componentwise for q in slot
                order;  s = lane_tree((p.x + p.y) + (p.z + p.w))
      x_{l+1} = (x0 * s + b_l) + x_l per element, layer after layer
    with the slots past D holding +0 in both operands up to the width bucket.  swap_sums: a WRONG variant, each layout with the
    other's wave sum."""
    f = np.float32
    x0 = np.asarray(x0, f); w = np.asarray(w, f); b = np.asarray(b, f)
    B, D = x0.shape
    four = D > 128
    DP = 64 * next(v for v in BUCKETS if D <= 64 * v)
    wave_sum = lane_tree if four != swap_sums else lane_butterfly
    xp = np.zeros((B, DP), f); wp = np.zeros((w.shape[0], DP), f); bp = np.zeros((w.shape[0], DP), f)
    xp[:, :D], wp[:, :D], bp[:, :D] = x0, w, b
    xl = xp
    for l in range(w.shape[0]):
        prod = xl * wp[l][None, :]
        if four:
            prod = prod.reshape(B, DP // 256, 64, 4)
            p = np.zeros((B, 64, 4), f)
            for q in range(DP // 256):
                p = p + prod[:, q]
            p = (p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3])
        else:
            prod = prod.reshape(B, DP // 64, 64)
            p = np.zeros((B, 64), f)
            for j in range(DP // 64):
                p = p + prod[:, j]
        s = wave_sum(p)
        xl = (xp * s[:, None] + bp[l][None, :]) + xl
    assert xl.dtype == f
    return np.ascontiguousarray(xl[:, :D])


def cross_bwd_closed_f32(x0, w, b, dy):
    """dx0, dw, db by the closed form, every operation in float32:
        x_l = a_l x0 + beta_l,  beta_l = sum_{l'<l} b_l',  c_l = beta_l . w_l,  P_l = x0 . w_l,
        s_l = a_l P_l + c_l,  a_0 = 1,  a_{l+1} = a_l + s_l,
        t_l = dy . x0 + sum_{l'>l} t_l' P_l',  u_l = t_l a_l,  T_l = sum_rows t_l
        dx0 = a_L dy + sum_l u_l w_l,  dw_l = sum_rows u_l x0 + beta_l T_l,  db_l = colsum(dy) + sum_{l'>l} w_l' T_l'."""
    f = np.float32
    x0 = np.asarray(x0, f); w = np.asarray(w, f); b = np.asarray(b, f); dy = np.asarray(dy, f)
    B, D = x0.shape
    L = w.shape[0]
    beta = np.zeros((L, D), f)
    for l in range(1, L):
        beta[l] = beta[l - 1] + b[l - 1]
    c = (beta * w).sum(axis=1, dtype=f)             # [L]
    P = x0 @ w.T                                    # [B, L]
    a = np.ones((B, L + 1), f)
    for l in range(L):
        a[:, l + 1] = a[:, l] + (a[:, l] * P[:, l] + c[l])
    q = (dy * x0).sum(axis=1, dtype=f)
    t = np.zeros((B, L), f)
    run = np.zeros(B, f)
    for l in range(L - 1, -1, -1):
        t[:, l] = q + run
        run = run + t[:, l] * P[:, l]
    u = t * a[:, :L]
    T = t.sum(axis=0, dtype=f)                      # [L]
    dx0 = a[:, L:L + 1] * dy + u @ w
    dw = u.T @ x0 + beta * T[:, None]
    cs = dy.sum(axis=0, dtype=f)
    db = np.empty((L, D), f)
    tail = np.zeros(D, f)
    for l in range(L - 1, -1, -1):
        db[l] = cs + tail
        tail = tail + w[l] * T[l]
    assert dx0.dtype == f and dw.dtype == f and db.dtype == f
    return dx0, dw, db


def row_rel(a, r):
    """max over rows of |a_row - r_row|_2 / |r_row|_2 (0 for an empty tensor)."""
    a = np.asarray(a, np.float64); r = np.asarray(r, np.float64)
    assert a.shape == r.shape and a.ndim == 2
    if a.size == 0:
        return 0.0
    den = np.maximum(np.sqrt((r * r).sum(axis=1)), 1e-300)
    return float((np.sqrt(((a - r) ** 2).sum(axis=1)) / den).max())


layer_rel = row_rel      # dw, db are [L, D]: one row per layer
