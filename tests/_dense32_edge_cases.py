"""Case tables, input generators and host restatements of the fp32-MFMA DenseLayer edge tests (csrc/mrec_gemm_f32.hip;
test_dense32_edges.py checks the tables without a device, test_dense32_edges_gpu.py runs them).

Roles.  A case is written as (form, p, red, q): p = rows of the output, red = the reduction length, q = the output's width.
As (M, K, N) of ops.dense32_*: form 0 fwd (p, red, q), form 1 dgrad (p, q, red), form 2 wgrad (red, p, q).

Operands.  A = the P side, B = the Q side, as the kernel stages them:
  form 0   A = x  [M, K]  contiguous extent K      B = w  [K, N]  contiguous extent N
  form 1   A = dy [M, N]  contiguous extent N      B = w  [K, N]  contiguous extent N   (the same N: mixed widths need other
                                                                                          offsets or strides)
  form 2   A = x  [M, K]  contiguous extent K      B = dy [M, N]  contiguous extent N
The load width of an operand is vec_of(pointer, row stride, contiguous extent) -> 4 / 2 / 1 floats, restated below as `vec_of`.

Exact family.  Every operand, bias and dy a nonzero integer in [-8, 8]: sum |a| |b| (+ |bias|, and over the 64 rows of a column
sum) stays below 2^24, so every partial sum in any order, fused or not, is an integer fp32 holds exactly, and the device's
result IS the int64 product -- whatever order the matrix instruction adds in, and a dropped term always changes a sum."""
import numpy as np

BK = 32                                                 # the kernel's K-tile
SIMPLEST = (128, 32, 128)                               # one interior tile, one K-tile
BASE = (129, 66, 130)                                   # 2 x 2 tiles, all partial; three K-tiles, the last holding 2
SWEEP_RED = [1, 2, 31, 32, 33, 34, 63, 64, 65, 96, 100]                             # T = 1..4, k_last_valid 1, 2, 31, 32
SWEEP_P = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 257]                    # every 32-row block boundary of a tile; 257: full
                                                                                    # tiles above a one-row tile
SWEEP_Q = [1, 2, 4, 31, 32, 33, 64, 65, 96, 97, 127, 128, 130, 258]
COLSUM_M = [1, 63, 64, 65, 127, 128, 129, 257]
SLAB_M = [1, 31, 32, 33, 64, 65, 100, 257]
SLAB_KN = [(66, 62), (129, 130)]
NEAR0_CAP = 1e-3                                        # share of a forward output that may lie in the ReLU's corner


def cdiv(a, b):
    return -(-a // b)


def align32(x):
    return cdiv(x, BK) * BK


def mkn(form, p, red, q):
    return {0: (p, red, q), 1: (p, q, red), 2: (red, p, q)}[form]


def sweep_cases():
    """[(p, red, q)] one extent at a time around BASE"""
    p0, r0, q0 = BASE
    return [(p0, r, q0) for r in SWEEP_RED] + [(p, r0, q0) for p in SWEEP_P] + [(p0, r0, q) for q in SWEEP_Q]


def k_tiles(red):
    """(T, k_last_valid) of an unsplit reduction"""
    T = cdiv(red, BK)
    return T, red - (T - 1) * BK


# ---- load widths ----------------------------------------------------------------------------------------------------------------
def vec_of(ptr_mod16, ld, ext):
    """gf32::vec_of: the widest load such that rows `ld` floats apart stay aligned and no vector straddles the extent's end"""
    if ptr_mod16 % 16 == 0 and ld % 4 == 0 and ext % 4 == 0:
        return 4
    if ptr_mod16 % 8 == 0 and ld % 2 == 0 and ext % 2 == 0:
        return 2
    return 1


FRONT, BACK = 4, 2                                      # poisoned rows in front of and behind a window (4 rows: 4 ld floats are a
                                                        # multiple of 16 bytes, so the window's alignment is its column offset's)


def ld_of(rows, ext, off, pad):
    """the row stride ops.dense32_* passes for a [rows, ext] window at column `off` of a buffer off + ext + pad wide (a single
    row has no stride: ops._mat32 passes its length)"""
    return off + ext + pad if rows > 1 else ext


def layout_vec(rows, ext, off, pad):
    """the width the kernel picks for such a window, the buffer's base 16-byte aligned"""
    return vec_of(4 * (FRONT * (off + ext + pad) + off) % 16, ld_of(rows, ext, off, pad), ext)


# how each width is reached: (extent % 4, column offset of the window, row stride % 4)
WAYS = {4: [(0, 0, 0)],
        2: [(2, 0, 0), (0, 2, 0), (0, 0, 2), (2, 2, 2)],
        1: [(1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 1, 2), (1, 2, 1)]}
EXT_NEAR = {66: {0: 68, 2: 66, 1: 65}, 129: {0: 132, 2: 130, 1: 129}, 130: {0: 132, 2: 130, 1: 129}}     # extents near BASE's, by % 4


def _pad_for(ext, off, ldmod):
    """1..4 poisoned columns right of the window such that the row stride is ldmod mod 4"""
    return next(pad for pad in range(1, 5) if (off + ext + pad) % 4 == ldmod)


def width_cases():
    """[(form, (p, red, q), (offA, padA), (offB, padB), (VA, VB))]: all 9 pairs per form, the ways of reaching a width taken in
    turn (form 1: among those where both operands have the same extent % 4)"""
    out = []
    p0, r0, q0 = BASE
    for form in (0, 1, 2):
        for va in (4, 2, 1):
            for vb in (4, 2, 1):
                pairs = [(wa, wb) for wa in WAYS[va] for wb in WAYS[vb] if form != 1 or wa[0] == wb[0]]
                wa, wb = pairs[len(out) % len(pairs)]
                # the contiguous extents: form 0 (red, q), form 1 (red, red), form 2 (p, q)
                if form == 0:
                    red, q, p = EXT_NEAR[r0][wa[0]], EXT_NEAR[q0][wb[0]], p0
                    ea, eb = red, q
                elif form == 1:
                    red, q, p = EXT_NEAR[r0][wa[0]], q0, p0
                    ea, eb = red, red
                else:
                    p, q, red = EXT_NEAR[p0][wa[0]], EXT_NEAR[q0][wb[0]], r0
                    ea, eb = p, q
                out.append((form, (p, red, q), (wa[1], _pad_for(ea, wa[1], wa[2])), (wb[1], _pad_for(eb, wb[1], wb[2])), (va, vb)))
    return out


def operand_shapes(form, p, red, q):
    """((rows, contiguous extent) of A, of B) as stored by the caller"""
    M, K, N = mkn(form, p, red, q)
    return {0: ((M, K), (K, N)), 1: ((M, N), (K, N)), 2: ((M, K), (M, N))}[form]


def case_widths(form, shape, la, lb):
    (ra, ea), (rb, eb) = operand_shapes(form, *shape)
    return layout_vec(ra, ea, *la), layout_vec(rb, eb, *lb)


GENERAL_WIDTHS = {0: (2, 4), 1: (4, 1), 2: (1, 2)}       # the mixed pair of each form that also runs general inputs
SWEEP_LAYOUT = ((0, 3), (0, 3))                         # the sweeps' operand windows: offset 0, three poisoned columns


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _ints(rng, shape):
    """nonzero integers in [-8, 8]"""
    return (rng.integers(1, 9, shape) * rng.choice([-1, 1], shape)).astype(np.float32)


def exact_inputs(form, p, red, q, seed=0):
    """dict of fp32 arrays as the caller stores them: form 0 x w bias; form 1 dy w h; form 2 x dy -- integer valued; h drawn from
    negative values, +0.0, -0.0 and positive values"""
    rng = np.random.default_rng([seed, form, p, red, q, 1])
    M, K, N = mkn(form, p, red, q)
    if form == 0:
        return dict(x=_ints(rng, (M, K)), w=_ints(rng, (K, N)), bias=_ints(rng, N))
    if form == 1:
        h = rng.choice(np.float32([-3.0, -0.5, 0.0, -0.0, 0.25, 7.0]), (M, K))
        return dict(dy=_ints(rng, (M, N)), w=_ints(rng, (K, N)), h=h)
    return dict(x=_ints(rng, (M, K)), dy=_ints(rng, (M, N)))


def general_inputs(form, p, red, q, seed=0):
    """the distributions of tests/test_dense32_gpu.py in the form's roles"""
    rng = np.random.default_rng([seed, form, p, red, q, 2])
    M, K, N = mkn(form, p, red, q)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    if form == 0:
        return dict(x=n(M, K), w=(rng.standard_normal((K, N)) * 0.05).astype(np.float32), bias=(rng.standard_normal(N) * 0.1).astype(np.float32))
    if form == 1:
        return dict(dy=n(M, N), w=(rng.standard_normal((K, N)) * 0.05).astype(np.float32), h=n(M, K))
    return dict(x=n(M, K), dy=n(M, N))


def product(form, d):
    """the float64 product of the form's operands (exact for the exact family: integers far below 2^53), without epilogue"""
    f = lambda a: a.astype(np.float64)
    if form == 0:
        return f(d["x"]) @ f(d["w"])
    if form == 1:
        return f(d["dy"]) @ f(d["w"]).T
    return f(d["x"]).T @ f(d["dy"])


def magnitude(form, d):
    """sum |a| |b| per output"""
    return product(form, {k: np.abs(v) for k, v in d.items()})


def bound(form, d):
    """tests/test_dense32_gpu.py's _bound: |fl(sum) - sum| <= red * 2^-24 * sum |a| |b| for red fp32 fma's in any order, with its
    headroom of 1.5"""
    red = d["x"].shape[1] if form == 0 else d["w"].shape[1] if form == 1 else d["x"].shape[0]
    return 1.5 * red * 2.0 ** -24 * magnitude(form, d) + 1e-30


def forward_reference(d):
    """(pre, tol, near0) of a forward with bias + ReLU as test_dense32_gpu.py judges it: tol = bound + 2^-23 |pre|; near0 = the
    ReLU's corner, where either side is right"""
    pre = product(0, d) + d["bias"].astype(np.float64)
    tol = bound(0, d) + 2.0 ** -23 * np.abs(pre)
    return pre, tol, np.abs(pre) <= tol


def general_forward_cases():
    """every (p, red, q) the device tests run a general-family forward at"""
    return sorted({BASE} | {shape for form, shape, _, _, v in width_cases() if form == 0 and v == GENERAL_WIDTHS[0]})


def exact_margin(form, d):
    """the largest sum of magnitudes any partial sum of the case can reach, as a share of 2^24: the dot products (+ the bias), and
    for form 1 the sums of 64 rows of them"""
    m = magnitude(form, d)
    if form == 0:
        m = m + np.abs(d["bias"]).astype(np.float64)
    if form == 1:
        m = np.stack([m[r:r + 64].sum(0) for r in range(0, m.shape[0], 64)])
    return float(m.max()) / 2.0 ** 24


# ---- column sums: the epilogue's order ------------------------------------------------------------------------------------------
def colsum_restated(dx):
    """[ceil(M / 64), W] fp32 from the device's own dx [M, W], in the order of the kernel's epilogue: for a 64-row block, S(mi, kh)
    = the sequential sum over r = 0..15 of row 32 mi + (r & 3) + 8 (r >> 2) + 4 kh, rows >= M skipped; the block's sum is
    (S(0, 0) + S(0, 1)) + (S(1, 0) + S(1, 1))"""
    assert dx.dtype == np.float32
    M, W = dx.shape
    out = np.empty((cdiv(M, 64), W), np.float32)
    for b in range(out.shape[0]):
        S = np.zeros((2, 2, W), np.float32)
        for mi in range(2):
            for kh in range(2):
                for r in range(16):
                    i = 64 * b + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * kh
                    if i < M:
                        S[mi, kh] = S[mi, kh] + dx[i]
        out[b] = (S[0, 0] + S[0, 1]) + (S[1, 0] + S[1, 1])
    return out


# ---- weight-gradient slabs ---------------------------------------------------------------------------------------------------------
def rows_per_slab(M, S):
    return align32(cdiv(M, S))


def slab_valid(M, S):
    """mrec_dense32_bwd_weight takes S iff no slab stays empty"""
    return S >= 1 and (S == 1 or rows_per_slab(M, S) * (S - 1) < M)


def slab_counts(M):
    """(valid, refused) among S = 1 .. ceil(M / 32)"""
    allS = range(1, max(1, cdiv(M, 32)) + 1)
    return [S for S in allS if slab_valid(M, S)], [S for S in allS if not slab_valid(M, S)]


def proposed_slabs(M, K, N):
    """mrec_dense32_bwd_weight_slabs, restated: fewest rounds of 512 workgroup slots x rows per workgroup, plus a slab's trip to
    memory and back; at least 256 batch rows per slab, at most 64 slabs; among equals the smallest"""
    best, best_cost = 1, None
    for S in range(1, min(64, max(1, M // 256)) + 1):
        rows = align32(cdiv(M, S))
        if S > 1 and rows * (S - 1) >= M:
            continue
        rounds = cdiv(cdiv(K, 128) * cdiv(N, 128) * S, 512)
        cost = rounds * (128 * rows + 8192) + S * (K * N // 600)
        if best_cost is None or cost < best_cost:
            best, best_cost = S, cost
    return best
