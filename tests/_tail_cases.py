"""Case table, input builders and host restatements of the fused tail launch's oracle tests (test_tail_oracle.py checks them
without a device, test_tail_oracle_gpu.py runs them).

A case names the batch (a multiple of 64: one workgroup per 64 rows), the wide branch (F = 0: a per-sample value [B]; F > 0: the
[B, F, 2] products of gather_rows_wide, slot 1 of every pair 0), the extra columns of the buffer x is a view of, the Dropout
descriptor (keep_prob, row0, index of the first tail layer) and the input family:
  "rand"  activations, weights and biases with the distributions of test_tail_gpu.py; x carries some negative entries and some -0.0
  "int"   x in {0, 1, 2}, w2 / w3 in {-1, 0, 1} with a fixed number of nonzeros per column, integer biases, dyadic w5 / b5 / wide
          terms: every 16-bit value is an integer of magnitude <= 256 (exact in bf16 and f16) and every fp32 partial sum is exact in
          any order, so y2 and the logit equal the float64 oracle bit for bit."""
from collections import namedtuple

import numpy as np

K2, N2, N3 = 512, 256, 128
R = 64                                      # rows per workgroup
PW = 2 * N3 + 4 + N2 + K2                   # floats per partial row: dW5 | db4 | db5, loss, 0, 0 | column sums of dz3 | of dz2
U = 2.0 ** -24
SEED, STEP = 1004, 3                        # of every Dropout descriptor here
FULL_ORACLE_B = 576                         # above it only the first and the last 64-row tile meet the oracle row by row
UNDECIDABLE_CAP = 0.005

Case = namedtuple("Case", "name B F pad drop family")      # drop: None or (keep_prob, row0, first tail layer)

BIG_ROW0 = 2 ** 33 + 64
CASES = [
    # block counts 1 2 7 8 9 (finish_column: chunk = ceil(nblk / 8) goes 1 -> 2 between 8 and 9), strides, Dropout variants
    Case("b1", 64, 0, 0, None, "rand"),
    Case("b2", 128, 1, 8, (0.5, 0, 2), "rand"),
    Case("b7", 448, 15, 24, (0.8, 128, 13), "rand"),
    Case("b8", 512, 16, 0, None, "rand"),
    Case("b9", 576, 17, 8, (0.5, BIG_ROW0, 13), "rand"),
    # the wide-field loader's four quads of 16 lanes
    Case("f32", 64, 32, 24, (0.8, BIG_ROW0, 2), "rand"),
    Case("f33", 128, 33, 0, None, "rand"),
    Case("f48", 64, 48, 8, (0.5, 128, 2), "rand"),
    Case("f49", 64, 49, 0, (0.8, 0, 13), "rand"),
    Case("f63", 128, 63, 24, None, "rand"),
    Case("f64", 64, 64, 0, (0.8, 0, 2), "rand"),
    # many workgroups: 63, 65 and the limit of 512
    Case("b63", 64 * 63, 0, 0, None, "rand"),
    Case("b65", 64 * 65, 26, 8, (0.5, 128, 2), "rand"),
    Case("b512", 32768, 39, 0, (0.8, BIG_ROW0, 13), "rand"),
    # exact
    Case("int", 128, 17, 8, None, "int"),
    Case("int_drop", 128, 33, 0, (0.5, 128, 2), "int"),
]
BY_NAME = {c.name: c for c in CASES}
# seeds at which every case keeps its undecidable share under the cap and the integer family its magnitudes (test_tail_oracle.py)
SEEDS = {c.name: 100 + i for i, c in enumerate(CASES)}


def tiles(B):
    """the row ranges that meet the oracle row by row"""
    if B <= FULL_ORACLE_B:
        return [slice(0, B)]
    return [slice(0, R), slice(B - R, B)]


def drop_scale(case):
    return float(np.float32(1.0) / np.float32(case.drop[0])) if case.drop else 1.0


def masks(oracle, case, sl, which):
    """the oracle's mask of the input of tail layer `which` (0: x [., K2], 1: y2 [., N2], 2: y3 [., N3]) for the rows sl; None: no Dropout"""
    if not case.drop:
        return None
    keep, row0, layer = case.drop
    return oracle.dropout_mask(sl.stop - sl.start, (K2, N2, N3)[which], SEED, STEP, layer + which, keep, row0 + sl.start)


# ---- the fragment order, restated from the comment above tail_pack_chunk -----------------------------------------------------------
def pack_fwd(W):
    """F[ks][nt][l][j] = W[ks*32 + 8*(l>>4) + j][nt*16 + (l&15)]"""
    K, N = W.shape
    ks, nt, l, j = np.ogrid[:K // 32, :N // 16, :64, :8]
    return W[ks * 32 + 8 * (l >> 4) + j, nt * 16 + (l & 15)]


def pack_bwd(W):
    """G[ks][kt][l][j] = W[kt*16 + (l&15)][ks*32 + 8*(l>>4) + j]"""
    K, N = W.shape
    ks, kt, l, j = np.ogrid[:N // 32, :K // 16, :64, :8]
    return W[kt * 16 + (l & 15), ks * 32 + 8 * (l >> 4) + j]


def pack_ref(w2, w3):
    """W2 forward | W3 forward | W3 backward | W2 backward, flat"""
    return np.concatenate([pack_fwd(w2).ravel(), pack_fwd(w3).ravel(), pack_bwd(w3).ravel(), pack_bwd(w2).ravel()])


def index_patterns(rows, cols, first=0):
    """int16 [rows, cols] whose bit patterns encode the element's index: (first + index) mod 65521"""
    return ((first + np.arange(rows * cols, dtype=np.int64)) % 65521).astype(np.uint16).view(np.int16).reshape(rows, cols)


TRANSPOSE_SHAPES = [(72, 40), (136, 264), (8, 8), (200, 64)]      # ragged last 64-tiles; 3 and 4 of them run beside the tail pack


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def wide_sum_f32(prod, wb):
    """(((0 + p0) + p1) + ...) + wide_b in fp32: the head's adds"""
    acc = np.zeros(prod.shape[0], np.float32)
    for f in range(prod.shape[1]):
        acc = acc + prod[:, f, 0]
    return acc + np.float32(wb)


def _wide(rng, case, dyadic):
    B, F = case.B, case.F
    # (sized so that the logit stays within a few units: test_head_fwd_bwd's dlogit tolerance, which these tests take over, is
    # met by fp32 arithmetic only while the sigmoid is not saturated)
    if dyadic:
        val = lambda *s: (rng.integers(-16, 17, s) * 2.0 ** rng.integers(-7, -3, s)).astype(np.float32)
    else:
        c = min(0.5, 1.5 / max(F, 1) ** 0.5)
        val = lambda *s: (rng.standard_normal(s) * c * 10.0 ** rng.uniform(-4, 0, s)).astype(np.float32)     # mixed magnitudes
    if not F:
        return val(B), None
    prod = np.zeros((B, F, 2), np.float32)
    prod[:, :, 0] = val(B, F)
    return prod, (np.float32(-0.375) if dyadic else np.float32(rng.standard_normal() * 0.1))


def _sparse_signs(rng, K, N, nnz):
    """[K, N] in {-1, 0, 1}: nnz nonzeros in every column"""
    w = np.zeros((K, N), np.float32)
    rows = np.argsort(rng.random((K, N)), axis=0)[:nnz]
    w[rows, np.arange(N)[None, :]] = rng.choice(np.float32([-1, 1]), (nnz, N))
    return w


def inputs(oracle, case, dt):
    """dict of numpy arrays: x, w2, w3 hold 16-bit values as float32; x is the (dropped-out, when the case has Dropout) input of the first
    tail layer"""
    rng = np.random.default_rng([SEEDS.get(case.name, 0), case.B, case.F])
    B = case.B
    if case.family == "int":
        x = rng.integers(1, 3, (B, K2)).astype(np.float32) * (rng.random((B, K2)) < 0.5)
        w2, w3 = _sparse_signs(rng, K2, N2, 24), _sparse_signs(rng, N2, N3, 8)
        b2, b3 = rng.integers(-2, 3, N2).astype(np.float32), rng.integers(-2, 3, N3).astype(np.float32)
        w5 = (rng.integers(1, 9, N3) * rng.choice([-1, 1], N3) / 2048.0).astype(np.float32)      # the logit stays of order 1
        b5 = np.float32([0.25])
    else:
        x = oracle.round16(np.maximum(rng.standard_normal((B, K2)), 0).astype(np.float32), dt)
        w2 = oracle.round16((rng.standard_normal((K2, N2)) * 0.06).astype(np.float32), dt)
        w3 = oracle.round16((rng.standard_normal((N2, N3)) * 0.08).astype(np.float32), dt)
        b2, b3 = (rng.standard_normal(N2) * 0.1).astype(np.float32), (rng.standard_normal(N3) * 0.1).astype(np.float32)
        # |w5| >= 0.02: no element of dz4 = round16(dlogit * w5 [/ keep]) underflows to 0 in f16, so dz4's zeros are the mask's alone
        w5 = (rng.choice([-1.0, 1.0], N3) * (0.02 + 0.05 * np.abs(rng.standard_normal(N3)))).astype(np.float32)
        b5 = (rng.standard_normal(1) * 0.1).astype(np.float32)
    if case.drop:
        x = oracle.dropout(x, masks(oracle, case, slice(0, B), 0), dt)
    if case.family == "rand":
        # what a ReLU never writes but pos16 must mask all the same: negative values and the negative zero
        u = rng.random((B, K2))
        x = np.where(u < 0.01, -oracle.round16((np.abs(rng.standard_normal((B, K2))) * 0.5 + 0.01).astype(np.float32), dt), x)
        x = np.where((u >= 0.01) & (u < 0.02), np.float32(-0.0), x).astype(np.float32)
    wide, wb = _wide(rng, case, case.family == "int")
    label = (rng.random(B) < 0.3).astype(np.float32)
    return dict(x=x, w2=w2, w3=w3, b2=b2, b3=b3, w5=w5, b5=b5, wide=wide, wb=wb, label=label, dscale=1024.0 / B)


# ---- the forward stages in float64 with their derived bounds --------------------------------------------------------------------
def stage(oracle, a, w, b, dt, mask, eps16, tiny):
    """One tail DenseLayer on the 16-bit input a: dict of
      pre     a . w + b in float64 (before the ReLU)
      ref     round16(relu(pre)), then oracle.dropout with `mask` when given: round, scale, round again, zero
      lo, hi  the interval the kernel's value must lie in: its pre-Dropout value v (a 16-bit number) has |v - round16(relu(pre))| <=
              delta = ulp16 + TINY + 2 K 2^-24 (|a| . |w| + |b|) (tests/test_dense_gpu.py), and Dropout's scale-and-round is monotone,
              so the value lies between the oracle's Dropout of (round16(relu(pre)) - delta, clipped at 0) and of (... + delta)
      delta   the pre-Dropout bound; dev = max(hi - ref, ref - lo): the bound on the value the next stage reads"""
    K = a.shape[1]
    pre = np.asarray(a, np.float64) @ np.asarray(w, np.float64) + np.asarray(b, np.float64)[None, :]
    r0 = oracle.dense_layer(a, w, b, True, dt)
    delta = eps16 * np.abs(r0) + tiny + 2 * K * U * (np.abs(a).astype(np.float64) @ np.abs(w) + np.abs(b)[None, :])
    lo, hi = np.maximum(r0 - delta, 0.0), r0 + delta
    if mask is None:
        ref = r0
    else:
        ref = oracle.dropout(r0, mask, dt)
        lo = oracle.dropout(lo.astype(np.float32), mask, dt).astype(np.float64)
        hi = oracle.dropout(np.nextafter(hi.astype(np.float32), np.float32(np.inf)), mask, dt).astype(np.float64)
    return dict(pre=pre, ref=ref, lo=lo, hi=hi, delta=delta, dev=np.maximum(hi - ref, ref - lo))


def undecidable(st):
    """where the sign of the pre-activation is within the accumulation bound: the kernel's ReLU may fall on either side"""
    return np.abs(st["pre"]) <= st["delta"]
