"""mrec_dense_tile_rows (the read-only query for the dense GEMM's tile configuration) and the case tables of
test_dense_edges_gpu.py, checked without a device: the library's rule falls back to 256 CUs there."""
import ctypes as C

import numpy as np
import pytest

import _dense_edge_cases as T


def _cus():
    import torch
    if torch.cuda.is_available():
        return torch.cuda.get_device_properties(0).multi_processor_count
    return 256          # what cu_count() in csrc/mrec_dense.hip assumes without a device


def test_tile_rows_argument_errors():
    from mindrec_amd import _lib, ops
    l = _lib.lib()
    out = C.c_int32(-7)
    for args in [(-1, 64, 64, 64), (3, 64, 64, 64), (0, 0, 64, 64), (1, -5, 64, 64), (2, 64, 0, 64), (0, 64, 64, 0), (0, 64, -8, 64)]:
        assert l.mrec_dense_tile_rows(*args, C.byref(out)) == -1, args          # MREC_EINVAL
        assert out.value == -7                                                  # ... and nothing written
    assert l.mrec_dense_tile_rows(0, 64, 64, 64, None) == -1
    with pytest.raises(_lib.MrecError) as e:
        ops.dense_tile_rows("fwd", 0, 8, 8)
    assert e.value.code == -1
    with pytest.raises(_lib.MrecError):
        ops.dense_tile_rows(7, 8, 8, 8)
    with pytest.raises(ValueError, match="bwd_weight"):
        ops.dense_tile_rows("forward", 8, 8, 8)
    assert ops.dense_tile_rows("fwd", 64, 8, 8) == ops.dense_tile_rows(0, 64, 8, 8) == 128


def test_tile_rows_follow_the_rule_in_both_directions():
    """forward / input gradient: 256-row tiles exactly from ceil(0.75 CUs) tiles of 256 x 256 on; the reduction length plays no part"""
    from mindrec_amd import ops
    cus = _cus()
    need = T.need_tiles(cus)
    for tiles_m, tiles_n in [(need, 1), (1, need), (T.square_grid(cus), T.square_grid(cus))]:
        M, N = tiles_m * 256, tiles_n * 256
        for k in (8, 4096):
            assert ops.dense_tile_rows(T.FWD, M, k, N) == 256
            assert ops.dense_tile_rows(T.BWD_INPUT, M, N, k) == 256
    M = (need - 1) * 256
    assert ops.dense_tile_rows(T.FWD, M, 64, 256) == 128 and ops.dense_tile_rows(T.FWD, M + 1, 64, 256) == 256
    assert ops.dense_tile_rows(T.BWD_INPUT, M, 256, 64) == 128 and ops.dense_tile_rows(T.BWD_INPUT, M + 1, 256, 64) == 256
    # weight gradient: tiles x the slabs it would take alone; one K-tile of batch cannot split
    assert ops.dense_tile_rows(T.BWD_WEIGHT, 64, 512, 512) == 128
    assert ops.dense_tile_rows(T.BWD_WEIGHT, 1 << 20, 2080, 1024) == (256 if need <= 36 * max(1, cus // 36) else 128)


def test_case_table_reaches_the_configurations_it_was_written_for():
    from mindrec_amd import ops
    cus = _cus()
    table = T.expected_configs(cus)
    assert len(table) == 4 + 2 + 1 + 8
    for what, op, (M, K, N), rows in table:
        T.require_rows(ops, op, M, K, N, rows)
    assert {(rd, rw) for _, rd, rw, _, _ in T.fused_cases(cus)} == {(128, 128), (128, 256), (256, 128), (256, 256)}
    if cus == 256:      # the figures the cases were proposed with
        assert [c[1:] for c in T.fwd_mr8_cases(cus)] == [(3457, 72, 3336), (24449, 136, 264), (3457, 32, 3336), (24321, 136, 264)]
        assert T.bwd_input_mr8_cases(cus) == [(3457, 3336, 72), (3457, 3332, 40)]
        assert [c[3] for c in T.fused_cases(cus)] == [(300, 264, 136), (777, 1000, 1016), (12288, 1024, 264), (12289, 1024, 8)]
        # the engine-reachable split with empty slabs: the library's own S for a 512 x 1024 layer at batch 576
        M, K, N = T.BWD_WEIGHT_ENGINE
        S = ops.dense_bwd_weight_slabs(M, K, N)
        assert any(r0 == r1 for r0, r1 in T.slab_rows(M, S)), S
    # the 128-row sweeps stay below the rule at any CU count worth the name
    for M, N in T.FWD_K_SWEEP_MN + [(max(T.FWD_EXTENT_M), max(T.FWD_EXTENT_N))]:
        T.require_rows(ops, T.FWD, M, 64, N, 128)
    T.require_rows(ops, T.BWD_INPUT, *T.BWD_INPUT_TALL, 128)
    T.require_rows(ops, T.BWD_INPUT, max(T.BWD_INPUT_M), max(T.BWD_INPUT_K), 8, 128)
    for K, N in T.BWD_WEIGHT_KN:
        T.require_rows(ops, T.BWD_WEIGHT, max(T.BWD_WEIGHT_M), K, N, 128)
    T.require_rows(ops, T.BWD_WEIGHT, *T.BWD_WEIGHT_ENGINE, 128)


def test_slab_rows_restates_the_header():
    assert T.slab_rows(520, 8) == [(0, 128), (128, 256), (256, 384), (384, 512), (512, 520), (520, 520), (520, 520), (520, 520)]
    assert T.slab_rows(777, 13)[-1] == (768, 777) and T.slab_rows(777, 8)[6:] == [(768, 777), (777, 777)]
    assert T.slab_rows(1, 4) == [(0, 1), (1, 1), (1, 1), (1, 1)]
    assert T.slab_rows(129, 1) == [(0, 129)]


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_exactly_rounded_share_is_reachable(oracle, dtype):
    """The forward cases require > 98 % of the outputs to BE the float64 reference's 16-bit value.  That is a condition on the
    kernel only while an honest fp32 accumulation meets it with room: an fp32 matmul of the very inputs (any summation order the
    host BLAS likes), rounded to 16 bits, must agree with the reference on >= 99 % -- over the reduction lengths of the sweep and
    of the 256-row cases (the big ones on a slice of their rows: the share is a per-element property)."""
    shapes = [(129, K, 264) for K in T.FWD_K_SWEEP] + [(257, 128, 520)]
    shapes += [(min(M, 1024), K, N) for _, M, K, N in T.fwd_mr8_cases(256)]
    for M, K, N in shapes:
        rng = np.random.default_rng(M + K + N)
        x, w, b = T.fwd_inputs(oracle, rng, M, K, N, dtype)
        ref = oracle.dense_layer(x, w, b, True, dtype)
        f32 = np.maximum(x @ w + b[None, :], np.float32(0))
        assert f32.dtype == np.float32
        share = float(np.mean(oracle.round16(f32, dtype) == ref))
        assert share >= 0.99, (M, K, N, share)
