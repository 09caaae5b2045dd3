"""Case tables of the dense MFMA GEMM edge tests (test_dense_edges.py checks them without a device,
test_dense_edges_gpu.py runs them).

The tile rule (csrc/mrec_dense.hip, pick_mr): a launch runs 256 x 256 tiles when it has at least 3/4 . CU-count of them,
else 128 x 256 tiles.  Shapes that have to reach the 256 x 256 body are sized from the CU count: tiles = ceil(0.75 . CUs),
rounded up to the grid; at 256 CUs they are the figures in the comments.  Every test asks ops.dense_tile_rows whether its
shape still lands where this table says, so a retuned rule fails these tests instead of silently emptying them."""
import math

FWD, BWD_INPUT, BWD_WEIGHT = "fwd", "bwd_input", "bwd_weight"
DTYPES = ["bf16", "f16"]


def need_tiles(cus):
    return math.ceil(0.75 * cus)


def square_grid(cus):
    """g with g * g >= ceil(0.75 CUs): 14 at 256 CUs (196 tiles)"""
    return math.ceil(math.sqrt(need_tiles(cus)))


def fwd_mr8_cases(cus):
    """[(name, M, K, N)].  Square: the last tile row holds 129 rows (wave row 1 of it: one row), the last tile column
    8 columns.  Tall: two tile columns (the second 8 wide), the last tile row again 129 rows.  tall_1row: the same grid whose
    last tile row holds ONE row (wave row 0 nearly empty, wave row 1 entirely).  square_k32: one K-tile, exactly the half-tile
    boundary (krem = 32)."""
    g = square_grid(cus)
    rows = math.ceil(need_tiles(cus) / 2)
    sq_m, sq_n = (g - 1) * 256 + 129, (g - 1) * 256 + 8                 # 3457, 3336
    return [("square", sq_m, 72, sq_n),
            ("tall", (rows - 1) * 256 + 129, 136, 264),                 # 24449
            ("square_k32", sq_m, 32, sq_n),
            ("tall_1row", (rows - 1) * 256 + 1, 136, 264)]              # 24321


def bwd_input_mr8_cases(cus):
    """[(M, K, N)]: output [M, K]; the second has K % 8 == 4 and a reduction of one K-tile with krem = 40"""
    g = square_grid(cus)
    m = (g - 1) * 256 + 129
    return [(m, (g - 1) * 256 + 8, 72), (m, (g - 1) * 256 + 4, 40)]     # (3457, 3336, 72), (3457, 3332, 40)


BWD_WEIGHT_MR8 = (777, 1000, 1016)          # 16 tiles x 13 slabs at 256 CUs: batch tail 9, P edge 232, Q edge 248
BWD_WEIGHT_MR8_SPLITS = (13, 16, 8)         # one K-tile per slab; the same with three empty slabs; two per slab, slab 7 empty


def fused_cases(cus):
    """[(name, rows of the input gradient's tiles, rows of the weight gradient's tiles, (M, K, N), extra problem?)]"""
    m8 = 256 * math.ceil(need_tiles(cus) / 4)                           # 12288: K = 1024 gives four tile columns
    return [("<4,4>", 128, 128, (300, 264, 136), False),
            ("<4,8>", 128, 256, BWD_WEIGHT_MR8, True),
            ("<8,4>", 256, 128, (m8, 1024, 264), True),
            ("<8,8>", 256, 256, (m8 + 1, 1024, 8), False)]


EXTRA_KN_S = (136, 72, 3)                   # the extra weight-gradient problem riding a fused launch


def expected_configs(cus):
    """[(what, op, (M, K, N), tile rows)] of every case above that was written for one configuration"""
    out = []
    for name, M, K, N in fwd_mr8_cases(cus):
        out.append((f"forward {name}", FWD, (M, K, N), 256))
    for M, K, N in bwd_input_mr8_cases(cus):
        out.append(("input gradient", BWD_INPUT, (M, K, N), 256))
    out.append(("weight gradient", BWD_WEIGHT, BWD_WEIGHT_MR8, 256))
    for name, rd, rw, mkn, _ in fused_cases(cus):
        out.append((f"fused {name} dx", BWD_INPUT, mkn, rd))
        out.append((f"fused {name} dw", BWD_WEIGHT, mkn, rw))
    return out


def require_rows(ops, op, M, K, N, rows):
    got = ops.dense_tile_rows(op, M, K, N)
    assert got == rows, (f"{op} (M, K, N) = ({M}, {K}, {N}) runs {got}-row tiles, this case was written for {rows}: the tile rule "
                         "(pick_mr: 256 x 256 tiles from 3/4 . CU-count tiles on) moved -- resize the case, do not drop it")


# ---- the 128 x 256 sweeps -------------------------------------------------------------------------------------
FWD_K_SWEEP = [8, 24, 32, 40, 56, 64, 72, 96, 104, 128, 136, 160, 192, 200, 264]       # T = 1..5, krem in {0, 8, 24, 32, 40, 56}
FWD_K_SWEEP_MN = [(129, 264), (300, 8)]
FWD_EXTENT_K = [72, 128]
FWD_EXTENT_M = [1, 16, 127, 128, 129, 257]
FWD_EXTENT_N = [8, 24, 248, 256, 264, 520]
FWD_EXTENT_NO_BIAS_N = 248

BWD_INPUT_K = [4, 12, 68, 252, 260, 8, 264]          # output widths: the K % 8 == 4 classes (260: in a Q-edge tile), and two plain
BWD_INPUT_N = [8, 32, 40, 72, 136]                   # reduction lengths
BWD_INPUT_M = [1, 129, 300]
BWD_INPUT_TALL = (4225, 72, 8)                       # 34 tile rows of 128: k_colsum_tiles takes a second, partly filled trip

BWD_WEIGHT_M = [1, 7, 63, 64, 65, 100, 129, 193, 257]
BWD_WEIGHT_KN = [(8, 8), (136, 264), (264, 248)]
BWD_WEIGHT_EMPTY = (520, 8)                          # Ttot = 9, S = 8: two K-tiles per slab, slabs 5 to 7 empty
BWD_WEIGHT_ENGINE = (576, 512, 1024)                 # a 512 x 1024 layer at batch 513..576 with the library's own S


def slab_rows(M, S):
    """[(r0, r1)] batch rows of each of the S slabs (include/mrec.h: slab s = rows [s c, (s + 1) c), c = 64 ceil(ceil(M / 64) / S))"""
    kt = -(-(-(-M // 64)) // S)
    return [(min(M, s * kt * 64), min(M, (s + 1) * kt * 64)) for s in range(S)]


# ---- inputs: the distributions of tests/test_dense_gpu.py, through its own generator --------------------------------
def fwd_inputs(oracle, rng, M, K, N, dtype):
    """x (30 % zeros: post-ReLU activations are sparse), w, bias of test_dense_fwd_matches_oracle"""
    from test_dense_gpu import _vals
    x = _vals(rng, (M, K), 1.0, dtype, oracle)
    x[rng.random((M, K)) < 0.3] = 0.0
    w = _vals(rng, (K, N), 0.05, dtype, oracle)
    b = (rng.standard_normal(N) * 0.1).astype("float32")
    return x, w, b


def bwd_input_inputs(oracle, rng, M, K, N, dtype):
    """dy, w, h of test_dense_bwd_input_matches_oracle"""
    import numpy as np
    from test_dense_gpu import _vals
    dy = _vals(rng, (M, N), 1e-2, dtype, oracle)
    w = _vals(rng, (K, N), 0.05, dtype, oracle)
    h = np.maximum(_vals(rng, (M, K), 1.0, dtype, oracle), 0)
    return dy, w, h


def bwd_weight_inputs(oracle, rng, M, K, N, dtype):
    """x, dy of test_dense_bwd_weight_matches_oracle"""
    import numpy as np
    from test_dense_gpu import _vals
    x = np.maximum(_vals(rng, (M, K), 1.0, dtype, oracle), 0)
    dy = _vals(rng, (M, N), 1e-2, dtype, oracle)
    return x, dy
