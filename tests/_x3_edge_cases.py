"""Case tables and input generators of the three-part fp32 GEMM edge tests (test_x3_edges.py checks them without a device,
test_x3_edges_gpu.py runs them).

Roles.  A case is written as (form, p, red, q): p = rows of the output (the P side), red = the reduction length, q = the output's
width (the Q side).  As (M, K, N) of ops.x3_gemm: form 0 (p, red, q), form 1 (p, q, red), form 2 (red, p, q).

The tile rule (csrc/mrec_gemm_x3.hip, x3_tile_rows): with t8 / t4 = the launch's workgroups in 256- / 128-row tiles, 128-row tiles
iff ceil(t4 / 256) * 0.55 < ceil(t8 / 256) -- the 256 is literal, not the device's CU count.  While t8 <= 256 that reads: 256-row
tiles iff t4 > 256.  Every case written for one tile shape asks ops.x3_tile_rows whether it still lands there.

Exact families.  Inputs for which every retained bf16 part product is an integer and sum_k (sum of |parts of a_k|) (sum of |parts of
b_k|) < 2^24, so that every partial sum in any order is an integer below 2^24 and an fp32 accumulation is exact:
  "p"  P side odd 19-bit integers (three nonzero parts), sparse along the reduction; Q side +-1       products a1b1 a2b1 a3b1
  "q"  the mirror image                                                                               products a1b1 a1b2 a1b3
  "m"  both sides odd 9-bit integers (two nonzero parts, no third); the P side sparse                 products a1b1 a1b2 a2b1 a2b2
The sparse side has the same number of nonzeros, at least one, in every 64-long K-tile of every dot product (as many as the tile
holds, at most BUDGET // K-tiles), so that every K-tile of every segment contributes to every output."""
import numpy as np
import torch

U = 2.0 ** -24
FAMILIES = ["p", "q", "m"]
BUDGET = {"p": 26, "q": 26, "m": 56}        # nonzeros per dot product: 26 (2^19 + 2^11 + 2^3) < 2^24; 56 . 513^2 < 2^24
PADS = [6, 8]                               # extra columns of the buffer an output is a window of: with W % 4 in {0, 2} all four
                                            # classes (W % 4, ld % 4)


def up64(x):
    return (int(x) + 63) // 64 * 64


def mkn(form, p, red, q):
    return {0: (p, red, q), 1: (p, q, red), 2: (red, p, q)}[form]


def classes(widths, pads=PADS):
    return {(w % 4, (w + pad) % 4) for w in widths for pad in pads}


# ---- the rule, restated --------------------------------------------------------------------------------------------
def rule_rows(form, M, K, N, S=1):
    cd = lambda a, b: -(-a // b)
    p, q = (K if form == 2 else M), (K if form == 1 else N)
    t8, t4 = cd(p, 256) * cd(q, 256) * S, cd(p, 128) * cd(q, 256) * S
    return 128 if cd(t4, 256) * 0.55 < cd(t8, 256) else 256


def require_rows(ops, form, M, K, N, rows, S=1):
    got = ops.x3_tile_rows(form, M, K, N, S)
    assert got == rows, (f"x3 form {form} (M, K, N, S) = ({M}, {K}, {N}, {S}) runs {got}-row tiles, this case was written for {rows}: the "
                         "tile rule (x3_tile_rows: 128-row tiles iff ceil(t4 / 256) * 0.55 < ceil(t8 / 256)) moved -- resize the case, "
                         "do not drop it")


def split_plan(M, K, N):
    """(S, c0, rem, ldw) of the split input gradient as csrc/mrec_gemm_x3.hip (dgrad_split) decides it; S = 0: one launch"""
    cd = lambda a, b: -(-a // b)
    ntp, ntq = cd(M, 256), cd(K, 256)
    rem = K - 256 * (ntq - 1)
    if ntq < 2 or rem >= 224 or cd(ntp * ntq, 256) == cd(ntp * (ntq - 1), 256):
        return 0, 0, 0, 0
    S, T = min(4, 256 // ntp), 6 * (up64(N) // 64)
    while S > 1 and cd(T, S) * (S - 1) >= T:
        S -= 1
    return (0, 0, 0, 0) if S < 2 else (S, 256 * (ntq - 1), rem, (rem + 3) // 4 * 4)


def require_split(_lib, M, K, N, S, rem):
    """the workspace query pins the decision and S: S * M * ldw * 4 + 256 bytes when the split is taken, 0 when not"""
    got = _lib.query_bytes("mrec_x3_gemm_dgrad_workspace_bytes", M, K, N)
    want = S * M * ((rem + 3) // 4 * 4) * 4 + 256 if S else 0
    assert got == want, (f"x3 input gradient (M, K, N) = ({M}, {K}, {N}): workspace {got} bytes, this case was written for {want} "
                         f"(S = {S}, rem = {rem}): the split rule (dgrad_split) moved -- resize the case, do not drop it")


# ---- tables -----------------------------------------------------------------------------------------------------------------
BASE = (129, 66, 258)                                   # (p, red, q) the 128-row sweeps vary one extent of
SWEEP_RED = [2, 62, 64, 66, 128, 130, 190]              # seg_tiles 1 1 1 2 2 3 3, with and without a zero-padded tail
SWEEP_P = [1, 63, 64, 65, 127, 129, 257]
SWEEP_Q = [2, 6, 62, 66, 254, 256, 258, 518]
SIMPLEST = (0, 128, 64, 256)                            # one interior tile, seg_tiles = 1: the first exact case


def sweep_cases():
    """[(p, red, q)] one extent at a time around BASE"""
    p0, r0, q0 = BASE
    return [(p0, r, q0) for r in SWEEP_RED] + [(p, r0, q0) for p in SWEEP_P if p != p0] + [(p0, r0, q) for q in SWEEP_Q if q != q0]


SLAB_M = [1, 64, 65, 129, 190]                          # T = 6 ceil(M / 64) = 6 6 12 18 18
SLAB_KN = [(66, 62), (258, 130)]


def slab_counts(T):
    """(valid, refused): S in 1..T by the rule of include/mrec.h -- every slab a non-empty share of the T reduction tiles"""
    ok = [S for S in range(1, T + 1) if S == 1 or -(-T // S) * (S - 1) < T]
    return ok, [S for S in range(2, T + 1) if S not in ok]


# 256-row tiles: [(name, form, (M, K, N), S)]
MR8_GEMM = [("fwd_square", 0, (3969, 66, 2050), 1),     # 16 x 9 tiles: the last tile row 129 rows, the last tile column 2 columns
            ("fwd_tall", 0, (16385, 130, 258), 1),      # 65 x 2 tiles: the last tile row one row
            ("dgrad", 1, (3969, 2050, 66), 1),
            ("wgrad_s13", 2, (777, 1000, 1016), 13),    # T = 78: six K-tiles per slab
            ("wgrad_s16", 2, (777, 1000, 1016), 16)]    # five per slab: slabs cross the interleaved segments' boundaries
MR8_FWD = (3969, 66, 2050)                              # fused forward: bias, ReLU, parts ...
MR8_FWD_DROP = (3969, 66, 2052)                         # ... and its neighbour with drop_next (N % 4 == 0)
MR8_DGRAD = (3969, 2050, 66)                            # fused input gradient: 63 column-sum groups, the last of one row

SPLIT_TAKEN = [((21761, 514, 64), 2, 2),                # ((M, K, N), S, rem)
               ((21761, 518, 66), 2, 6),
               ((21505, 914, 64), 3, 146),
               ((21761, 734, 64), 2, 222)]              # the last width that takes the split
SPLIT_NOT_TAKEN = (21761, 736, 64)

POST_R = [1, 63, 65, 300]
POST_C = [2, 62, 66, 130, 254, 258, 1170]


def expected_configs():
    """[(what, form, (M, K, N), S, tile rows)] of every case above that was written for one tile shape"""
    out = [("simplest", SIMPLEST[0], mkn(*SIMPLEST), 1, 128)]
    for form in (0, 1, 2):
        for c in sweep_cases():
            out.append((f"sweep {c}", form, mkn(form, *c), 1, 128))
    for M in SLAB_M:
        for K, N in SLAB_KN:
            for S in slab_counts(6 * (up64(M) // 64))[0]:
                out.append(("slabs", 2, (M, K, N), S, 128))
    for name, form, shape, S in MR8_GEMM:
        out.append((name, form, shape, S, 256))
    out += [("fused fwd", 0, MR8_FWD, 1, 256), ("fused fwd drop", 0, MR8_FWD_DROP, 1, 256), ("fused dgrad", 1, MR8_DGRAD, 1, 256)]
    return out


# ---- the host's three-part split ----------------------------------------------------------------------------------------------
def split3(x):
    """fp32 array [R, C] -> torch.bfloat16 [3, R, C] on the CPU: x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2)"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    a = t.to(torch.bfloat16)
    r = t - a.float()
    b = r.to(torch.bfloat16)
    c = (r - b.float()).to(torch.bfloat16)
    return torch.stack([a, b, c])


def parts_image(x):
    """the zero-padded parts image [3, Rp, Cp] of include/mrec.h, made on the host"""
    R, C = x.shape
    img = torch.zeros((3, up64(R), up64(C)), dtype=torch.bfloat16)
    img[:, :R, :C] = split3(x)
    return img


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _wide(rng, shape, bits):
    """odd `bits`-bit integers with random sign; 19 bits: redrawn until all three bf16 parts are nonzero"""
    lo = 1 << (bits - 1)
    v = (rng.integers(lo // 2, lo, shape) * 2 + 1).astype(np.float32)
    if bits == 19:
        for _ in range(64):
            bad = (split3(v.reshape(1, -1)).float().numpy() == 0).any(axis=0).reshape(shape)
            if not bad.any():
                break
            v[bad] = (rng.integers(lo // 2, lo, int(bad.sum())) * 2 + 1).astype(np.float32)
        assert not bad.any()
    return v * rng.choice(np.float32([-1, 1]), shape)


def _sparse_rows(rng, rows, red, bits, budget):
    """[rows, red]: in every row the same number of nonzeros in every 64-long K-tile"""
    tiles = -(-red // 64)
    assert tiles <= budget, (red, budget)
    a = np.zeros((rows, red), np.float32)
    for t in range(tiles):
        w = min(64, red - 64 * t)
        n = max(1, min(w, budget // tiles))
        cols = np.argsort(rng.random((rows, w)), axis=1)[:, :n] + 64 * t
        a[np.arange(rows)[:, None], cols] = _wide(rng, (rows, n), bits)
    return a


def exact_inputs(family, form, p, red, q, seed=0):
    """(A [p, red], B [red, q]) fp32, integer valued: the output is A . B; as the operands the form takes (operands())"""
    rng = np.random.default_rng([seed, form, p, red, q, FAMILIES.index(family)])
    sign = lambda *s: rng.choice(np.float32([-1, 1]), s)
    if family == "p":
        return _sparse_rows(rng, p, red, 19, BUDGET["p"]), sign(red, q)
    if family == "q":
        return sign(p, red), np.ascontiguousarray(_sparse_rows(rng, q, red, 19, BUDGET["q"]).T)
    return _sparse_rows(rng, p, red, 9, BUDGET["m"]), _wide(rng, (red, q), 9)


def general_inputs(form, p, red, q, seed=0):
    """(A [p, red], B [red, q]) with the distributions of test_x3_products_have_fp32_accuracy in the form's roles: activations x with
    rows over six decades, weights w of sigma 0.05, gradients dy with rows down to e^-20"""
    rng = np.random.default_rng([seed, form, p, red, q])
    x = lambda r, c: (rng.standard_normal((r, c)) * np.exp(rng.uniform(-12, 2, (r, 1)))).astype(np.float32)
    w = lambda r, c: (rng.standard_normal((r, c)) * 0.05).astype(np.float32)
    dy = lambda r, c: (rng.standard_normal((r, c)) * np.exp(rng.uniform(-20, 0, (r, 1)))).astype(np.float32)
    if form == 0:
        return x(p, red), w(red, q)                                     # x [M, K] . w [K, N]
    if form == 1:
        return dy(p, red), np.ascontiguousarray(w(q, red).T)            # dy [M, N] . (w [K, N])^T
    return np.ascontiguousarray(x(red, p).T), dy(red, q)                # (x [M, K])^T . dy [M, N]


def operands(form, A, B):
    """the fp32 matrices whose parts images the form takes as P and Q: A, B as stored by the caller"""
    if form == 0:
        return A, B
    if form == 1:
        return A, np.ascontiguousarray(B.T)             # w [K, N]
    return np.ascontiguousarray(A.T), B                 # x [M, K]


def exact_margin(A, B):
    """max over outputs of sum_k (sum of |parts of a_k|) (sum of |parts of b_k|), as a share of 2^24"""
    pa = split3(A).double().abs().sum(0).numpy()
    pb = split3(B).double().abs().sum(0).numpy()
    return float((pa @ pb).max()) / 2.0 ** 24
