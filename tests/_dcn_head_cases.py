"""Case tables, input builders and references of the Deep&Cross output head's edge tests (csrc/mrec_dcn.hip; test_dcn_head_ref.py
checks them without a device, test_dcn_head_edges_gpu.py runs them).

The logit is restated in fp32 and compared with the device BIT FOR BIT (the library is built with -ffp-contract=off): lane l owns the
float4 slots (q 64 + l) 4 < H, q < 4, of the deep half and the float2 slots (q 64 + l) 2 < X, q < 10, of the cross half (a slot it
does not own holds +0 in both operands); dot starts at +0 and takes + ((x.x w.x + x.y w.y) + (x.z w.z + x.w w.w)) for q = 0 .. 3,
then + (x.x w.x + x.y w.y) for q = 0 .. 9; the 64-lane xor butterfly d = 32 .. 1; + b3.  That is at most 24 roundings on any path
from a product to the logit (1 product, 2 inside the slot, 14 slots, 6 butterfly steps, the bias):
    |logit - logit64| <= 24 u (sum |x| |w| + |b3|),  u = 2^-24.

Everything behind expf and log1pf is held to float64 computed from the DEVICE'S OWN logit, so that a logit error is not counted
twice: dlogit = (sigmoid(z) - y) dscale, dd2 = dlogit w3[:H] where d2 > 0 (exactly 0 elsewhere, at -0.0 too), dc = dlogit w3[H:],
with the tolerances of test_dcn_head_vs_float64 (|err| <= 1e-7 dscale + 1e-4 |ref|).

The batch sums are held to the float64 sum of the per-row terms the device itself added up.  w3's first cross weight is exactly 1.0
in every case, so dc[:, 0] IS the device's dlogit, to the bit; the terms are d2 dlogit and c dlogit (dW3), dlogit (db3) and the
device's dd2 (db2).  With T the sum of a column's |terms|:
    |sum - sum64| <= (B + 2) u T.
Derivation: a term is one fp32 product (1 rounding); a wave adds its rows in order, min(B, 8) - 1 roundings (the add to +0 is
exact); the four waves' sums take 3 adds, the workgroups' ceil(B / 32) - 1: no more than B + 2 in all for any B, far fewer from
B = 16 on, which is where the terms of second order go.
The loss: the per-row terms are max(z, 0), -z y and log1p(exp(-|z|)) in float64 from the device's z, T the sum of their absolute
values over the batch, and
    |loss - mean64| <= (B + 8) u T / B:
the summation as above, and 6 more for the row's own arithmetic (z y, the subtraction, the add; expf and log1pf, whose errors touch
only the third term, at most log 2 of a row's share of T) and the product with the rounded 1 / B."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
F32 = np.float32
NA, NC, ROWS = 4, 10, 32                     # float4 slots per lane, float2 slots per lane, rows per workgroup (8 per wave)
HMAX, XMAX = 64 * 4 * NA, 64 * 2 * NC

Case = namedtuple("Case", "B H X kind")      # kind: "moderate" (|logit| <= 4, hard labels) or "values" (saturated logits, soft labels)

SLOT_CASES = [Case(37, H, 30, "moderate") for H in (4, 252, 256, 260, 1020, 1024)] + \
             [Case(37, 64, X, "moderate") for X in (2, 126, 128, 130, 1170, 1278, 1280)]
ROW_B = [1, 7, 8, 9, 31, 32, 33, 65]
ROW_CASES = [Case(B, H, X, "moderate") for (H, X) in ((64, 30), (1024, 1170)) for B in ROW_B]
STRIDE_CASES = [Case(33, 260, 130, "moderate"), Case(9, 1024, 1170, "moderate")]
VALUES_CASE = Case(64, 64, 30, "values")
VALUE_LOGITS = [0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
VALUE_LABELS = [0.0, 1.0, 0.3]
REFUSED_SHAPES = [(6, 30), (64, 3), (1028, 30), (64, 1282)]      # (H, X)
ZMAX = 4.0


def all_cases():
    return SLOT_CASES + ROW_CASES + STRIDE_CASES + [VALUES_CASE]


def name(c):
    return f"{c.kind[0]}-B{c.B}-H{c.H}-X{c.X}"


def dscale(case):
    """(the value the kernel receives: fp32)"""
    return float(F32(1000.0 / case.B))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def logit64(d2, c, w3, b3):
    H = d2.shape[1]
    return d2.astype(np.float64) @ w3[:H].astype(np.float64) + c.astype(np.float64) @ w3[H:].astype(np.float64) + float(b3[0])


def inputs(case):
    """dict: d2 [B, H] (a ReLU's output: about half zeros, some of them -0.0), c [B, X], w3 [H + X] with w3[H] = 1.0 exactly,
    b3 [1], label [B]"""
    B, H, X = case.B, case.H, case.X
    rng = np.random.default_rng([B, H, X, len(case.kind)])
    d2 = np.maximum(rng.standard_normal((B, H)), 0).astype(F32)
    c = rng.standard_normal((B, X)).astype(F32)
    c[:, 0] *= F32(0.03)                                     # (the column under the unit weight adds what the others add)
    w3 = (rng.standard_normal(H + X) * 0.03).astype(F32)
    w3[H] = 1.0
    b3 = np.array([0.1], F32)
    if case.kind == "moderate":
        # no row's dlogit is small against the others': |z| <= 4 keeps |sigmoid(z) - y| >= 0.018 at hard labels.  (The logit less its
        # bias is linear in the row, and a positive factor keeps the ReLU's zeros.)
        k = np.minimum(1.0, 3.5 / np.maximum(np.abs(logit64(d2, c, w3, b3) - 0.1), 1e-30))
        d2, c = (d2 * k[:, None]).astype(F32), (c * k[:, None]).astype(F32)
        label = (rng.random(B) < 0.3).astype(F32)
    else:
        # the row's logit lands on its target: the cross half is scaled (either sign), the ReLU's output is left as it is
        target = np.array([VALUE_LOGITS[r % len(VALUE_LOGITS)] for r in range(B)]) + rng.uniform(-0.01, 0.01, B)
        zd, zc = d2.astype(np.float64) @ w3[:H], c.astype(np.float64) @ w3[H:]
        c = (c * ((target - 0.1 - zd) / zc)[:, None]).astype(F32)
        label = np.array([VALUE_LABELS[(r // len(VALUE_LOGITS)) % len(VALUE_LABELS)] for r in range(B)], F32)
    d2[(d2 == 0) & (rng.random((B, H)) < 0.25)] = F32(-0.0)
    return dict(d2=d2, c=c, w3=w3, b3=b3, label=label)


# ---- the logit in fp32 ----------------------------------------------------------------------------------------------------------------
def logit32(d2, c, w3, b3, drop=None):
    """The kernel's logit, bit for bit.  drop: a wrong variant -- "deep" / "cross": the last owned slot of that half is left out."""
    B, H = d2.shape
    X = c.shape[1]
    xa, wa = np.zeros((B, HMAX), F32), np.zeros(HMAX, F32)
    xc, wc = np.zeros((B, XMAX), F32), np.zeros(XMAX, F32)
    xa[:, :H], wa[:H], xc[:, :X], wc[:X] = d2, w3[:H], c, w3[H:]
    if drop == "deep":
        wa[H - 4:H] = 0
    if drop == "cross":
        wc[X - 2:X] = 0
    pa = (xa * wa[None, :]).reshape(B, NA, 64, 4)
    pc = (xc * wc[None, :]).reshape(B, NC, 64, 2)
    dot = np.zeros((B, 64), F32)
    for q in range(NA):
        dot = dot + ((pa[:, q, :, 0] + pa[:, q, :, 1]) + (pa[:, q, :, 2] + pa[:, q, :, 3]))
    for q in range(NC):
        dot = dot + (pc[:, q, :, 0] + pc[:, q, :, 1])
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        dot = dot + dot[:, lane ^ d]
    return (dot[:, 0] + b3[0]).astype(F32)


def logit_bound(d2, c, w3, b3):
    H = d2.shape[1]
    return 24 * U * (np.abs(d2).astype(np.float64) @ np.abs(w3[:H]) + np.abs(c).astype(np.float64) @ np.abs(w3[H:]) + abs(float(b3[0])))


# ---- float64 behind the logit --------------------------------------------------------------------------------------------------------
def row_terms(z, label):
    """float64 [B, 3]: max(z, 0), -z y, log1p(exp(-|z|)) -- SigmoidCrossEntropyWithLogits as the kernel splits it"""
    z, y = z.astype(np.float64), label.astype(np.float64)
    return np.stack([np.maximum(z, 0.0), -z * y, np.log1p(np.exp(-np.abs(z)))], axis=1)


def dlogit64(z, label, ds):
    z = z.astype(np.float64)
    e = np.exp(-np.abs(z))
    return (np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e)) - label.astype(np.float64)) * ds


def grads64(x, z, label, ds):
    """(dd2, dc) in float64 from the logit z"""
    H = x["d2"].shape[1]
    dl = dlogit64(z, label, ds)
    return np.where(x["d2"] > 0, dl[:, None] * x["w3"][None, :H].astype(np.float64), 0.0), dl[:, None] * x["w3"][None, H:].astype(np.float64)


def grad_tol(ref, ds):
    """test_dcn_head_vs_float64's: allclose(rtol=1e-4, atol=1e-7 dscale)"""
    return 1e-7 * ds + 1e-4 * np.abs(ref)


def sums64(x, dl, dd2, rows=None):
    """The float64 batch sums of the per-row terms and their bounds: dict name -> (sum, bound).  dl [B]: the dlogit the terms are
    built from; dd2 [B, H]: db2's terms.  rows: weights per row (1 everywhere; 0 drops a row, 2 doubles it)."""
    B = dl.shape[0]
    w = np.ones(B) if rows is None else np.asarray(rows, np.float64)
    dl = dl.astype(np.float64)
    terms = dict(dw3=np.concatenate([x["d2"], x["c"]], axis=1).astype(np.float64) * dl[:, None], db2=dd2.astype(np.float64), db3=dl[:, None])
    return {k: ((t * w[:, None]).sum(axis=0), (B + 2) * U * np.abs(t).sum(axis=0)) for k, t in terms.items()}


def loss64(z, label, rows=None):
    """(float64 mean, bound)"""
    t = row_terms(z, label)
    B = t.shape[0]
    w = np.ones(B) if rows is None else np.asarray(rows, np.float64)
    return float((t.sum(axis=1) * w).sum() / B), float((B + 8) * U * np.abs(t).sum() / B)
