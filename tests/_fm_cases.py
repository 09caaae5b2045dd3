"""Case tables, input builders and host restatements of the FM term's edge tests (csrc/mrec_fm.hip; test_fm_ref.py checks them
without a device, test_fm_edges_gpu.py runs them).

The library is built with -ffp-contract=off and every sum in these kernels has a fixed order, so the restatements below -- numpy
fp32, one rounding per operation, vectorised over the batch -- are compared with the device BIT FOR BIT:

  fm4   k_fm_fwd4: a lane-group of lpr = D / 4 lanes owns a sample; s and q are summed in field order; per lane
        part = ((sx^2 - qx) + (sy^2 - qy)) + ((sz^2 - qz) + (sw^2 - qw)); for off = 32 .. 1 every lane with sub + off < lpr adds the
        value lane sub + off held BEFORE the step; fm = [add +] 0.5f * part[0]
  fm1   k_fm_fwd: lane l owns the columns l + 64 j; part starts at +0 and takes + (s s - q) for j = 0 .. 3 in order where the column
        exists; the 64-lane xor butterfly d = 32 .. 1, x = x + x[l ^ d]
  bwd   g + dout (colsum - vx), every kernel of the backward (k_fm_bwd, k_fm_bwd4, k_fm_bwd4_mix with g the widened 16-bit gradient)

The float64 bound.  fm64 is the float64 value of the fp32 inputs, A = 0.5 sum_d [(sum_f |x|)^2 + sum_f x^2], u = 2^-24:
    |fm - fm64| <= (2 F + 12) u A  [+ u |add|]
Derivation: s carries F - 1 roundings (the first add, to +0, is exact) relative to sum |x|, so s^2 carries 2 (F - 1) + 1 relative to
(sum |x|)^2; q carries one rounding per square and F - 1 per add, F relative to sum x^2; the subtraction adds 1 to each.  fm4 then
adds 2 levels inside the lane and 6 tree steps (2 F + 8 in all), fm1 up to 4 sequential adds inside the lane and 6 butterfly steps
(2 F + 10); the product with 0.5 is exact, and the sum with `add` rounds once more, relative to |add| + the term (2 F + 11).  The
terms of second order in u (below F^2 u^2) fit into what is left of 12.  A derivation, not a measurement: test_fm_ref.py holds both
restatements to it on every case, test_fm_edges_gpu.py the device.

The wrong variants (test_fm_ref.py shows that every case where a variant applies tells it from the right restatement):
  "noguard"   the tree without `if (sub + off < lpr)`: lane 0 of a group then pulls in the lanes behind its group.  In a wave whose
              other lanes hold +0 (G = 1, or a single live sample) that changes no bit, so it applies from two samples in a wave on
  "inplace"   the tree applied in place lane by lane, highest lane first (lowest first reads only lanes not yet updated and equals
              the simultaneous step): a lane then reads a neighbour that already took this step's addend.  Applies from lpr = 3 on
  "norem"     the F % 4 remainder fields dropped.  Applies where F % 4 != 0
  "nolast"    the last lane of the lane-group (fm1: the last column) dropped.
  "first64"   fm1 only: the columns past the first 64 dropped.  Applies where D > 64
At F = 1 every lane's part is s s - q = x x - x x = +0 exactly, whatever the tree does: fm is exactly +0 [+ add] (an fma contraction
would leave the rounding error of x x there), so the tree variants apply from F = 2 on; "norem" shows in the column sums at F = 1."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
F32 = np.float32
FM_MAXD = 256

VEC_D = [4, 8, 12, 20, 64, 80, 84, 128, 132, 252, 256]      # lpr 1 2 3 5 16 20 21 32 33 63 64
SCALAR_D = [1, 2, 3, 30, 63, 65, 129, 193, 254, 255]
MISALIGNED_D = [64, 80, 256]
FS = [1, 3, 4, 5, 39]
SCALAR_B = [1, 3, 4, 5]
COPY_D, COPY_F = [4, 20, 132, 256], [3, 4, 5]
REFUSED_D = [257, 260]
# (B, F, D) -> the kernel whose grid-stride loop takes a second trip
SECOND_TRIPS = {"fwd4": (8200, 2, 256), "fwd1": (8200, 2, 3), "bwd4": (8200, 2, 256), "bwd4_mix": (8200, 2, 256), "bwd1": (8200, 2, 65)}

Case = namedtuple("Case", "path B F D")      # path: "vec" (k_fm_fwd4) or "scalar" (k_fm_fwd)


def lanes(D):
    """(lpr, G) of k_fm_fwd4"""
    lpr = D // 4
    return lpr, 64 // lpr


def vec_B(D):
    G = lanes(D)[1]
    return [1, 4 * G - 1, 4 * G, 4 * G + 1]      # a workgroup is 4 waves of G samples


def vec_cases(D):
    return [Case("vec", B, F, D) for F in FS for B in vec_B(D)]


def scalar_cases(D):
    return [Case("scalar", B, F, D) for F in FS for B in SCALAR_B]


def all_cases():
    out = []
    for D in VEC_D:
        out += vec_cases(D)
    for D in SCALAR_D + MISALIGNED_D:
        out += scalar_cases(D)
    return out + [Case("vec", *SECOND_TRIPS["fwd4"]), Case("scalar", *SECOND_TRIPS["fwd1"])]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def inputs(B, F, D, seed=0):
    """dict: vx [B, F, D], add [B], dout [B], g [B, F, D] (fp32).  Per-sample scales from 1e-3 to 1e2; in about a fifth of the samples
    whole fields are zero (masked fields); sample 1 is all zero (where there are three or more); dout holds exact zeros and both signs."""
    rng = np.random.default_rng([seed, B, F, D])
    vx = rng.standard_normal((B, F, D)) * 10.0 ** rng.uniform(-3, 2, (B, 1, 1))
    masked = (rng.random((B, 1, 1)) < 0.2) & (rng.random((B, F, 1)) < 0.5)
    masked[0] = False                               # (sample 0 keeps every field: it is all there is at B = 1)
    vx = np.where(masked, 0.0, vx).astype(F32)
    if B >= 3:
        vx[1] = 0.0
    add = (rng.standard_normal(B) * 10.0 ** rng.uniform(-2, 2, B)).astype(F32)
    dout = rng.standard_normal(B).astype(F32)
    dout[rng.random(B) < 0.25] = 0.0
    if B >= 3:
        dout[0], dout[2] = F32(-0.75), F32(1.5)
    g = rng.standard_normal((B, F, D)).astype(F32)
    return dict(vx=vx, add=add, dout=dout, g=g)


def _bits32(words):
    return np.asarray(words, np.uint32).view(F32)


# fp32 values on bf16 rounding ties (low half 0x8000: to even, down and up), just beside them, of both signs, a tie in fp32's subnormal
# range and two whose rounding carries into the exponent
BF16_PLANTS = _bits32([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x00008000, 0x477FFFFF, 0x3FFF8000])
# ... on f16 ties (low 13 bits 0x1000), above the largest f16 (65504; 65520 is the tie that rounds to inf), in f16's subnormal range
# (ties there fall on other bits) and below its smallest subnormal 2^-24 ~ 5.96e-8 (2^-25 is the tie that rounds to zero)
F16_PLANTS = np.concatenate([_bits32([0x3F801000, 0x3F803000, 0x3F800FFF, 0x3F801001, 0xBF801000, 0xBF803000]),
                             F32([65504.0, 65519.0, 65520.0, 65536.0, 1e5, -65520.0, -7e4, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25,
                                  np.nextafter(F32(2.0 ** -25), F32(1)), 2.5 * 2.0 ** -24, 3.5 * 2.0 ** -24, -(2.0 ** -25), 5e-8, 6e-8, -3e-8,
                                  1e-9, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -15 + 2.0 ** -25])])


def plant(vx, values, seed=0):
    """a copy of vx with `values` written over elements chosen at random (every value at least once where vx has room)"""
    out = vx.copy()
    flat = out.reshape(-1)
    rng = np.random.default_rng([seed, flat.size])
    n = min(values.size, flat.size)
    flat[rng.choice(flat.size, n, replace=False)] = values[:n]
    return out


# ---- the restatements --------------------------------------------------------------------------------------------------------------
def col_sums(vx, fields=None):
    """(s, q) [B, D] fp32: ReduceSum(vx, 1) and ReduceSum(Square(vx), 1) in field order from +0"""
    B, F, D = vx.shape
    s, q = np.zeros((B, D), F32), np.zeros((B, D), F32)
    for f in range(F if fields is None else fields):
        x = vx[:, f, :]
        s = s + x
        q = q + x * x
    return s, q


def _finish(part0, add):
    half = F32(0.5) * part0
    return (add + half if add is not None else half).astype(F32)


def _tree(part, lpr, variant, G):
    """part [B, lpr] -> the value of each group's lane 0 after the shuffle tree"""
    B = part.shape[0]
    if variant == "noguard":
        # the wave as the kernel lays it out: G samples of lpr lanes, then spare lanes holding +0; a sample missing from the last
        # wave holds +0 too.  __shfl_down past lane 63 returns the lane's own value.
        nw = -(-B // G)
        wave = np.zeros((nw, 64), F32)
        full = np.zeros((nw * G, lpr), F32)
        full[:B] = part
        wave[:, :G * lpr] = full.reshape(nw, G * lpr)
        for off in (32, 16, 8, 4, 2, 1):
            o = wave.copy()
            o[:, :64 - off] = wave[:, off:]
            wave = wave + o
        return wave[:, :G * lpr].reshape(nw * G, lpr)[:B, 0]
    part = part.copy()
    for off in (32, 16, 8, 4, 2, 1):
        n = lpr - off
        if n <= 0:
            continue
        if variant == "inplace":
            for sub in range(n - 1, -1, -1):
                part[:, sub] = part[:, sub] + part[:, sub + off]
        else:
            part[:, :n] = part[:, :n] + part[:, off:off + n]      # (numpy evaluates the right-hand side before it stores)
    return part[:, 0]


def fm4(vx, add=None, variant=None):
    """k_fm_fwd4 (D % 4 == 0): (fm [B], colsum [B, D]) fp32.  variant: None or one of the wrong variants named above."""
    B, F, D = vx.shape
    lpr, G = lanes(D)
    s, q = col_sums(vx, F - F % 4 if variant == "norem" else None)
    t = (s * s - q).reshape(B, lpr, 4)
    part = (t[:, :, 0] + t[:, :, 1]) + (t[:, :, 2] + t[:, :, 3])
    if variant == "nolast":
        part[:, lpr - 1] = 0.0
    return _finish(_tree(part, lpr, variant, G), add), s


def fm1(vx, add=None, variant=None):
    """k_fm_fwd (any D <= 256): (fm [B], colsum [B, D]) fp32"""
    B, F, D = vx.shape
    s, q = col_sums(vx)
    t = np.zeros((B, FM_MAXD), F32)
    own = np.zeros(FM_MAXD, bool)
    keep = D - 1 if variant == "nolast" else min(D, 64) if variant == "first64" else D
    t[:, :keep] = (s * s - q)[:, :keep]
    own[:keep] = True
    t, own = t.reshape(B, 4, 64), own.reshape(4, 64)
    part = np.zeros((B, 64), F32)
    for j in range(4):
        part = np.where(own[j][None, :], part + t[:, j, :], part)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lane ^ d]
    return _finish(part[:, 0], add), s


def restate(case):
    return fm4 if case.path == "vec" else fm1


def variants(case):
    """the wrong variants that apply to the case"""
    B, F, D = case.B, case.F, case.D
    out = []
    if case.path == "vec":
        lpr, G = lanes(D)
        if F >= 2 and G >= 2 and B >= 2:
            out.append("noguard")
        if F >= 2 and lpr >= 3:
            out.append("inplace")
        if F % 4:
            out.append("norem")
        if F >= 2:
            out.append("nolast")
    elif F >= 2:
        out.append("nolast")
        if D > 64:
            out.append("first64")
    return out


def backward(g, vx, colsum, dout):
    """g + dout (colsum - vx) in fp32, one rounding per operation"""
    return (g + dout[:, None, None] * (colsum[:, None, :] - vx)).astype(F32)


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------
def fm64(vx, add=None):
    x = vx.astype(np.float64)
    fm = 0.5 * (x.sum(axis=1) ** 2 - (x * x).sum(axis=1)).sum(axis=1)
    return fm + add.astype(np.float64) if add is not None else fm


def bound(vx, add=None):
    """(2 F + 12) u A [+ u |add|], derived in the module's docstring"""
    x = np.abs(vx.astype(np.float64))
    A = 0.5 * (x.sum(axis=1) ** 2 + (x * x).sum(axis=1)).sum(axis=1)
    b = (2 * vx.shape[1] + 12) * U * A
    return b + U * np.abs(add.astype(np.float64)) if add is not None else b


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)
