"""Case tables, input builders and references of the one-launch Deep&Cross evaluation forward (csrc/mrec_cross.hip: k_dcn_predict at
either lane layout, behind ops.dcn_predict; test_dcn_predict_ref.py checks them without a device, test_dcn_predict_gpu.py runs them).

The kernel computes logit = [d2 | c] . w3 + b3 with c = x_L, the cross stack's output, held in registers.  The references take c as
GIVEN (on the device: ops.cross_layers' own output, whose per-row device code the kernel shares) and restate what happens behind it.

The logit in fp32, compared with the device BIT FOR BIT (the library is built with -ffp-contract=off), in the order the kernel
documents:
  deep half: lane l owns the float4 slots of columns 256 q + 4 l + {0..3} < H, q < 4 (a slot it does not own holds +0 in both
      operands);  dd = +0;  dd += (x.x w.x + x.y w.y) + (x.z w.z + x.w w.w)  for q = 0 .. 3
  cross half, X <= 128 (one column per lane: columns l + 64 j):  pc = +0;  pc += c_j w_j  for j = 0, 1
  cross half, X > 128 (four columns per lane: columns 256 q + 4 l + {0..3}):  p = (+0, +0, +0, +0);  p += c_q * w_q componentwise
      for q = 0 .. ceil(X / 256) - 1;  pc = (p.x + p.y) + (p.z + p.w)
  each half's 64 lane sums by themselves through a balanced tree in lane order: (t_0 + t_1), (t_2 + t_3), ..; those pairwise; .. six levels
  logit = (tree(pc) + tree(dd)) + b3
(slots past the kernel's own padding hold +0 x +0 and change no bit: a running sum that starts at +0 is never -0.)

The float64 bound.  The longest path from a product to the logit is the cross half's at four columns per lane: the product's own
rounding (1), at most 8 additions into p (X <= 2048), 2 inside pc, 6 tree levels, the add of the deep half, the bias: n = 19 (the
deep half: 1 + 2 + 4 + 6 + 2 = 15; one column per lane: 1 + 2 + 6 + 2 = 11).  Every rounding is relative 2^-24 =: u of a partial sum
that is no larger than the sum of the absolute products and |b3|, so to first order
    |logit - logit64| <= 19 u (sum |x| |w| + |b3|)
with logit64 the float64 value from the same fp32 inputs.  Derived, not measured.

Behind the logit: prob is held to the float64 sigmoid of the float64 logit within 0.25 bound + 2^-23 (the sigmoid's slope is at most
1/4; one fp32 rounding of a value below 1 and expf's error), the loss to float64 BCE of the DEVICE'S OWN logit within
_dcn_head_cases.loss64's (B + 8) u T / B: a sum of B terms in ANY fixed order takes at most B - 1 inexact additions (the kernel's: a
wave its rows in row order, the block its 16 waves in wave order, one wave the blocks: four a lane, then the tree; adding a wave or
block that had no row adds +0, exactly), 6 roundings for the row's own arithmetic and one for the product with the rounded 1 / B."""
from collections import namedtuple

import numpy as np

from _cross_ref import lane_tree       # the balanced tree over the 64 lane sums in lane order, shared with the stack's restatement
from _dcn_head_cases import VALUE_LABELS, VALUE_LOGITS, loss64  # noqa: F401  (the values and the loss model of the head's tests)

U = 2.0 ** -24
F32 = np.float32
HQ, HMAX, XMAX = 4, 1024, 2048
NROUND = 19

Case = namedtuple("Case", "B H X L kind")    # kind: "moderate" or "values" (saturated logits, soft labels)

WIDTHS = [2, 64, 65, 128, 129, 256, 257, 1170, 1280, 2048]        # both sides of the path edge (128) and of the width buckets
WIDTH_CASES = [Case(37, 64, X, L, "moderate") for X in WIDTHS for L in (1, 6, 8)]
GLOBAL_W_CASES = [Case(37, 64, 130, 9, "moderate"), Case(37, 64, 257, 9, "moderate")]     # L > 8: w / b (and W3[H:]) from global memory
NO_LAYER_CASES = [Case(37, 64, 30, 0, "moderate"), Case(37, 64, 1170, 0, "moderate")]     # the cross half is x0 . W3[H:]
DEEP_CASES = [Case(37, H, 30, 6, "moderate") for H in (4, 252, 256, 260, 1020, 1024)]
ROW_B = [1, 2, 31, 32, 33, 65]
ROW_CASES = [Case(B, H, X, 6, "moderate") for (H, X) in ((64, 30), (1024, 1170)) for B in ROW_B]
# the forward kernel's grid stops growing at 256 workgroups x 16 waves x 2 rows = 8192 rows a pass: past 16384 rows a wave walks a
# second pair of rows
SECOND_PAIR_CASE = Case(16384 + 33, 4, 64, 1, "moderate")
STRIDE_CASE = Case(33, 260, 130, 6, "moderate")
VALUES_CASE = Case(64, 64, 30, 6, "values")
REFUSED = [dict(H=6), dict(H=1028), dict(X=2049), dict(offset=1)]      # over (H, X) = (64, 30): raise before any launch


def all_cases():
    return WIDTH_CASES + GLOBAL_W_CASES + NO_LAYER_CASES + DEEP_CASES + ROW_CASES + [SECOND_PAIR_CASE, STRIDE_CASE, VALUES_CASE]


def name(c):
    return f"{c.kind[0]}-B{c.B}-H{c.H}-X{c.X}-L{c.L}"


def four_columns(X):
    """the kernel's path: four columns per lane from the 4 x 64 width bucket on"""
    return X > 128


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def cross64(x0, cw, cb):
    """CrossLayer x L in float64 (deep_and_cross.py:139-149): x_{l+1} = x0 (x_l . w_l) + b_l + x_l"""
    x0 = x0.astype(np.float64)
    xl = x0
    for l in range(cw.shape[0]):
        xl = x0 * (xl @ cw[l].astype(np.float64))[:, None] + cb[l].astype(np.float64)[None, :] + xl
    return xl


def inputs(case):
    """dict: x0 [B, X], cw, cb [L, X], d2 [B, H] (a ReLU's output: about half zeros, some of them -0.0), w3 [H + X], b3 [1],
    label [B]"""
    B, H, X, L = case.B, case.H, case.X, case.L
    rng = np.random.default_rng([B, H, X, L, len(case.kind)])
    x0 = rng.standard_normal((B, X)).astype(F32)
    cw = (rng.standard_normal((L, X)) * (0.3 / np.sqrt(X))).astype(F32)
    cb = (rng.standard_normal((L, X)) * 0.1).astype(F32)
    w3 = (rng.standard_normal(H + X) * (1.5 / np.sqrt(H + X))).astype(F32)
    b3 = np.array([0.1], F32)
    if case.kind == "moderate":
        d2 = np.maximum(rng.standard_normal((B, H)), 0).astype(F32)
        d2[:, H - 1] = np.abs(rng.standard_normal(B)).astype(F32) + F32(0.25)      # (the last deep slot is never empty)
        label = (rng.random(B) < 0.3).astype(F32)
    else:
        # the row's logit lands on its target: the deep half makes up what the cross half leaves, on the columns whose weight has the
        # sign that is needed -- d2 stays a ReLU's output, about half of it zeros
        target = np.array([VALUE_LOGITS[r % len(VALUE_LOGITS)] for r in range(B)]) + rng.uniform(-0.01, 0.01, B)
        need = target - 0.1 - cross64(x0, cw, cb) @ w3[H:].astype(np.float64)
        base = np.abs(rng.standard_normal((B, H))) * (np.sign(w3[None, :H]) == np.sign(need)[:, None])
        d2 = (base * (need / (base @ w3[:H].astype(np.float64)))[:, None]).astype(F32)
        label = np.array([VALUE_LABELS[(r // len(VALUE_LOGITS)) % len(VALUE_LABELS)] for r in range(B)], F32)
    d2[(d2 == 0) & (rng.random((B, H)) < 0.25)] = F32(-0.0)
    return dict(x0=x0, cw=cw, cb=cb, d2=d2, w3=w3, b3=b3, label=label)


# ---- the logit ---------------------------------------------------------------------------------------------------------------------
def logit64(d2, c, w3, b3):
    H = d2.shape[1]
    return d2.astype(np.float64) @ w3[:H].astype(np.float64) + c.astype(np.float64) @ w3[H:].astype(np.float64) + float(b3[0])


def logit32(d2, c, w3, b3, drop=None):
    """The kernel's logit, bit for bit.  drop: a wrong variant -- "deep" / "cross": the last owned slot of that half is left out."""
    d2, c, w3 = d2.astype(F32), c.astype(F32), w3.astype(F32)
    B, H = d2.shape
    X = c.shape[1]
    xa, wa = np.zeros((B, HMAX), F32), np.zeros(HMAX, F32)
    xa[:, :H], wa[:H] = d2, w3[:H]
    if drop == "deep":
        wa[H - 4:H] = 0
    pa = (xa * wa[None, :]).reshape(B, HQ, 64, 4)
    dd = np.zeros((B, 64), F32)
    for q in range(HQ):
        dd = dd + ((pa[:, q, :, 0] + pa[:, q, :, 1]) + (pa[:, q, :, 2] + pa[:, q, :, 3]))
    if four_columns(X):
        nq = -(-X // 256)
        xc, wc = np.zeros((B, nq * 256), F32), np.zeros(nq * 256, F32)
        xc[:, :X], wc[:X] = c, w3[H:]
        if drop == "cross":
            wc[(X - 1) // 4 * 4:X] = 0
        pr = (xc * wc[None, :]).reshape(B, nq, 64, 4)
        p = np.zeros((B, 64, 4), F32)
        for q in range(nq):
            p = p + pr[:, q]
        pc = (p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3])
    else:
        npl = -(-X // 64)
        xc, wc = np.zeros((B, npl * 64), F32), np.zeros(npl * 64, F32)
        xc[:, :X], wc[:X] = c, w3[H:]
        if drop == "cross":
            wc[X - 1] = 0
        pr = (xc * wc[None, :]).reshape(B, npl, 64)
        pc = np.zeros((B, 64), F32)
        for j in range(npl):
            pc = pc + pr[:, j]
    z = (lane_tree(pc) + lane_tree(dd)) + b3.astype(F32)[0]
    assert z.dtype == F32
    return z


def logit_bound(d2, c, w3, b3):
    H = d2.shape[1]
    return NROUND * U * (np.abs(d2).astype(np.float64) @ np.abs(w3[:H]).astype(np.float64) +
                         np.abs(c).astype(np.float64) @ np.abs(w3[H:]).astype(np.float64) + abs(float(b3[0])))


def sigmoid64(z):
    z = z.astype(np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
