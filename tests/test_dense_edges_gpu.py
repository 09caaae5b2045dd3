"""The dense MFMA GEMM body (csrc/mrec_gemm.h through csrc/mrec_dense.hip) at both tile shapes, every edge and slab split,
against the oracle's float64 restatements (oracle.dense_layer / dense_bwd_input / dense_bwd_weight) -- the same inputs and
the same derived bounds as tests/test_dense_gpu.py (see its docstring; helpers imported from there, cases from
_dense_edge_cases.py):
  16-bit outputs      |gpu - ref| <= ulp16(|ref|) + TINY + 2 R 2^-24 (|a| . |b|)      R = reduction length
  fp32 weight slabs   |gpu - ref| <= 2 rows 2^-24 (|x|^T . |dy|) over the slab's own batch rows; an empty slab is exactly 0
and, forward, > 98 % of the elements ARE the reference's 16-bit value.  That share is asserted for every case (fp32 accumulation
misses well under 1 %: test_dense_edges.py::test_exactly_rounded_share_is_reachable); an output of fewer than 50 elements, where
"> 98 %" would demand bit equality of every one, may miss one, and the outputs under 2048 elements of a test are held to the
share once more as a pool.  The ReLU-mask assertions of the input gradient are those of test_dense_bwd_input_matches_oracle
with ONE exception, stated in _check_dx: the issue behind these tests asked for them verbatim, and verbatim the first of them
fails on correct results at 10^7 outputs.

What the existing tests do not reach and these do: reductions shorter than the software pipeline is deep (1..3 K-tiles) with
every class of partial K-tile (none, under / exactly / over the half tile); batch tails of any length in the weight gradient's
strided reduction; slab splits that leave workgroups with nothing to add up (they still owe their zeros); input-gradient widths
that are multiples of 4 only; more than 32 tile rows in the bias-sum finish; the 256 x 256 body with ragged extents in all three
roles; all four instantiations of the fused backward launch.  Every output is a window of a larger sentinel-filled allocation
(16-bit: 7.0 in 8 extra columns and 2 extra rows; contiguous fp32 slabs and bias sums: NaN in two rows + 8 elements on either
side, and NaN inside before the call), and the sentinel must be intact afterwards.

Each test asks ops.dense_tile_rows for the tile configuration its shape runs in and FAILS when that is not the one it was
written for."""
import numpy as np
import pytest
import torch

import _dense_edge_cases as T
from test_dense_gpu import DT, EPS16, TINY, _dev

pytestmark = pytest.mark.gpu

FILL = 7.0
NAN = float("nan")
POOL = 2048          # outputs with fewer elements pool their exactly-rounded counts per test


def _tall(a, dtype, dev, width=None):
    """a [rows, cols] on the device as the [:rows, :cols] view of a buffer 64 rows taller (and `width` columns wide) that holds NaN
    everywhere else: a reduction-strided operand (the forward's w, the weight gradient's x and dy) whose staging reads one row
    past its last finds NaN there, not the zeros or the range check a tight allocation would answer with"""
    rows, cols = a.shape
    buf = torch.full((rows + 64, width or cols), NAN, dtype=DT[dtype], device=dev)
    buf[:rows, :cols] = _dev(a, dtype, dev)
    return buf[:rows, :cols]


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---- sentinel-guarded outputs ---------------------------------------------------------------------------------------
def _window16(M, W, dtype, dev):
    buf = torch.full((M + 2, W + 8), FILL, dtype=DT[dtype], device=dev)
    return buf, buf[:M, :W]


def _read16(buf, M, W, what):
    g = buf.float().cpu().numpy()
    assert (g[M:, :] == FILL).all(), f"{what}: rows below M = {M} written"
    assert (g[:M, W:] == FILL).all(), f"{what}: columns right of {W} written"
    return g[:M, :W]


def _guarded32(shape, dev):
    """contiguous fp32 NaN window of `shape` with NaN guards of two rows + 8 elements before and behind (16-byte aligned)"""
    n, guard = int(np.prod(shape)), 2 * shape[-1] + 8
    guard += -guard % 4
    buf = torch.full((n + 2 * guard,), NAN, dtype=torch.float32, device=dev)
    return buf, buf[guard:guard + n].view(shape)


def _read32(buf, win, what):
    g = buf.cpu().numpy()
    guard = (g.size - win.numel()) // 2
    assert np.isnan(g[:guard]).all() and np.isnan(g[guard + win.numel():]).all(), f"{what}: written outside its extent"
    out = g[guard:guard + win.numel()].reshape(tuple(win.shape))
    assert not np.isnan(out).any(), f"{what}: {int(np.isnan(out).sum())} elements never written"
    return out


# ---- the bounds of tests/test_dense_gpu.py --------------------------------------------------------------------------
def _check_fwd(y, ref, x, w, b, K, dtype, what):
    """-> number of exactly rounded elements"""
    absb = np.abs(b) if b is not None else 0.0
    bound = EPS16[dtype] * np.abs(ref) + TINY[dtype] + 2 * K * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(w) + absb)
    err = np.abs(y.astype(np.float64) - ref)
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} of {err.size} outside the bound, worst ratio {float((err / bound).max()):.3g}"
    return int((y == ref).sum())


def _check_share(equal, total, what, pooled=None):
    """> 98 % of the elements are the exactly rounded value.  An output of fewer than 50 elements may miss ONE (there "> 98 %"
    would mean every element, which fp32 accumulation does not promise: it misses about one element in a thousand); outputs
    under POOL elements are, besides, added to `pooled` = [equal, total], which the caller holds to > 98 % as a whole."""
    assert equal > 0.98 * total or total - equal <= 1, f"{what}: only {equal} of {total} elements are the exactly rounded value"
    if pooled is not None and total < POOL:
        pooled[0] += equal; pooled[1] += total


def _check_dx(dx, ref, dy, w, h, N, dtype, what):
    bound = EPS16[dtype] * np.abs(ref) + TINY[dtype] + 2 * N * 2.0 ** -24 * (np.abs(dy).astype(np.float64) @ np.abs(w).T)
    err = np.abs(dx.astype(np.float64) - ref)
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} of {err.size} outside the bound, worst ratio {float((err / bound).max()):.3g}"
    if h is not None:
        # test_dense_bwd_input_matches_oracle's two mask assertions.  Its first reads "the oracle's zeros are zeros" and takes every
        # zero of the oracle for the mask's; among 10^7 outputs a few UNMASKED sums round to zero by themselves (seen: a float64
        # sum of exactly 0.0 where fp32 accumulation leaves 2^-32; an f16 sum of 2.96e-8, just under half the smallest subnormal),
        # and there the fp32 result may be one step off zero -- the bound above holds it.  Those elements alone are left out.
        own_zero = (h > 0) & (ref == 0)
        assert np.array_equal((dx == 0)[~own_zero], ((ref == 0) | (dx == 0))[~own_zero]) and ((h > 0) | (dx == 0)).all(), f"{what}: ReLU mask"
        # (a sum of N >= 8 products of sigma 1e-2 * 0.05 each lands under 2^-25 with probability < 2 * 2^-25 / (1.4e-3 sqrt(2 pi)) = 1.7e-5)
        assert own_zero.sum() <= 1e-4 * ref.size + 1, f"{what}: {int(own_zero.sum())} unmasked zeros in the oracle"


def _check_db(db, dx, ref_db, M, what):
    """fp32 sum of the ROUNDED dx in a fixed order: against the float64 sum of the GPU's own dx, and against the oracle's"""
    own = dx.astype(np.float64).sum(axis=0)
    assert np.allclose(db, own, rtol=0, atol=M * 2.0 ** -24 * np.abs(dx).sum(axis=0).max() + 1e-30), f"{what}: bias sum vs own dx"
    assert np.allclose(db, ref_db, rtol=1e-2, atol=1e-3 * np.abs(ref_db).max()), f"{what}: bias sum vs oracle"


def _check_slabs(sl, x, dy, M, S, oracle, what):
    """every slab against the oracle over its own batch rows; empty slabs exactly zero"""
    assert sl.shape[0] == S
    for s, (r0, r1) in enumerate(T.slab_rows(M, S)):
        if r0 == r1:
            assert (sl[s] == 0.0).all(), f"{what}: empty slab {s} of {S} is not all zeros"
            continue
        ref = oracle.dense_bwd_weight(x[r0:r1], dy[r0:r1])
        bound = 2 * (r1 - r0) * 2.0 ** -24 * (np.abs(x[r0:r1]).astype(np.float64).T @ np.abs(dy[r0:r1])) + 1e-30
        err = np.abs(sl[s].astype(np.float64) - ref)
        assert np.all(err <= bound), f"{what}: slab {s} of {S} (rows {r0}..{r1}) worst ratio {float((err / bound).max()):.3g}"


def _check_slab_sum(slabs_dev, sl, x, dy, M, oracle, what, ref=None):
    """sum_slabs == the sequential fp32 host sum, bit for bit, and within the weight-gradient bound of the oracle"""
    from mindrec_amd import ops
    out = torch.empty(tuple(slabs_dev.shape[1:]), dtype=torch.float32, device=slabs_dev.device)
    ops.sum_slabs(slabs_dev, out)
    acc = sl[0].copy()
    for s in range(1, sl.shape[0]):
        acc = acc + sl[s]
    got = out.cpu().numpy()
    assert np.array_equal(got, acc), f"{what}: sum_slabs is not the sequential sum"
    if ref is None:
        ref = oracle.dense_bwd_weight(x, dy)
    bound = 2 * M * 2.0 ** -24 * (np.abs(x).astype(np.float64).T @ np.abs(dy)) + 1e-30
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= bound), f"{what}: sum worst ratio {float((err / bound).max()):.3g}"


# ---- 1. forward, 128-row tiles: reductions shorter than the pipeline, every tail class ------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("M,N", T.FWD_K_SWEEP_MN)
def test_fwd_reduction_length_sweep(dev, oracle, dtype, M, N):
    from mindrec_amd import ops
    T.require_rows(ops, T.FWD, M, max(T.FWD_K_SWEEP), N, 128)
    assert sorted({(k + 63) // 64 for k in T.FWD_K_SWEEP}) == [1, 2, 3, 4, 5] and sorted({k % 64 for k in T.FWD_K_SWEEP}) == [0, 8, 24, 32, 40, 56]
    pooled = [0, 0]
    for K in T.FWD_K_SWEEP:
        what = f"{dtype} M={M} K={K} N={N}"
        rng = np.random.default_rng(M + K + N)
        x, w, b = T.fwd_inputs(oracle, rng, M, K, N, dtype)
        buf, out = _window16(M, N, dtype, dev)
        ops.dense_fwd(_dev(x, dtype, dev), _tall(w, dtype, dev), torch.from_numpy(b).to(dev), relu=True, out=out)
        y = _read16(buf, M, N, what)
        eq = _check_fwd(y, oracle.dense_layer(x, w, b, True, dtype), x, w, b, K, dtype, what)
        _check_share(eq, y.size, what, pooled)
    if pooled[1]:
        _check_share(pooled[0], pooled[1], f"{dtype} M={M} N={N}, all K")


# ---- 2. forward, 128-row tiles: extents ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("K", T.FWD_EXTENT_K)
def test_fwd_extent_sweep(dev, oracle, dtype, K):
    """x is a view of a wider buffer (ldx = K + 24) whose other columns hold NaN: a read past K would show"""
    from mindrec_amd import ops
    T.require_rows(ops, T.FWD, max(T.FWD_EXTENT_M), K, max(T.FWD_EXTENT_N), 128)
    pooled = [0, 0]
    for M in T.FWD_EXTENT_M:
        for N in T.FWD_EXTENT_N:
            rng = np.random.default_rng(M + K + N)
            x, w, b = T.fwd_inputs(oracle, rng, M, K, N, dtype)
            if N == T.FWD_EXTENT_NO_BIAS_N:
                b = None
            xb = torch.full((M, K + 24), NAN, dtype=DT[dtype], device=dev)
            xb[:, :K] = _dev(x, dtype, dev)
            wd, bd = _tall(w, dtype, dev), torch.from_numpy(b).to(dev) if b is not None else None
            for relu in (True, False):
                what = f"{dtype} M={M} K={K} N={N} relu={relu} bias={b is not None}"
                buf, out = _window16(M, N, dtype, dev)
                ops.dense_fwd(xb[:, :K], wd, bd, relu=relu, out=out)
                y = _read16(buf, M, N, what)
                eq = _check_fwd(y, oracle.dense_layer(x, w, b, relu, dtype), x, w, b, K, dtype, what)
                _check_share(eq, y.size, what, pooled)
    _check_share(pooled[0], pooled[1], f"{dtype} K={K}, the small outputs")


# ---- 3. forward, 256-row tiles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("case", [0, 1, 2, 3], ids=["square", "tall", "square_k32", "tall_1row"])
def test_fwd_256_row_tiles(dev, oracle, dtype, case):
    """... and the transposed-weight forward of the same case: bit-equal, hence within the same bound"""
    from mindrec_amd import ops
    name, M, K, N = T.fwd_mr8_cases(_cus(dev))[case]
    T.require_rows(ops, T.FWD, M, K, N, 256)
    what = f"{dtype} {name} M={M} K={K} N={N}"
    rng = np.random.default_rng(M + K + N)
    x, w, b = T.fwd_inputs(oracle, rng, M, K, N, dtype)
    xd, wd, bd = _dev(x, dtype, dev), _tall(w, dtype, dev), torch.from_numpy(b).to(dev)
    buf, out = _window16(M, N, dtype, dev)
    ops.dense_fwd(xd, wd, bd, relu=True, out=out)
    buf_t, out_t = _window16(M, N, dtype, dev)
    ops.dense_fwd(xd, None, bd, relu=True, out=out_t, wt=wd.t().contiguous())
    y = _read16(buf, M, N, what)
    ref = oracle.dense_layer(x, w, b, True, dtype)
    _check_share(_check_fwd(y, ref, x, w, b, K, dtype, what), y.size, what)
    y_t = _read16(buf_t, M, N, what + " wt")
    assert np.array_equal(y_t, y), f"{what}: the transposed-weight forward differs in {int((y_t != y).sum())} elements"
    assert torch.equal(buf, buf_t)


# ---- 4. input gradient, 128-row tiles: widths that are multiples of 4 only, short reductions ------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("M", T.BWD_INPUT_M)
def test_bwd_input_width_and_reduction_sweep(dev, oracle, dtype, M):
    from mindrec_amd import ops
    assert sorted(k for k in T.BWD_INPUT_K if k % 8 == 4) == [4, 12, 68, 252, 260]
    for K in T.BWD_INPUT_K:
        for N in T.BWD_INPUT_N:
            T.require_rows(ops, T.BWD_INPUT, M, K, N, 128)
            rng = np.random.default_rng(M * 3 + K + N)
            dy, w, h = T.bwd_input_inputs(oracle, rng, M, K, N, dtype)
            dyd, wd = _dev(dy, dtype, dev), _dev(w, dtype, dev)
            hb = torch.full((M, K + 8), NAN, dtype=DT[dtype], device=dev)       # the mask source has the output's row stride
            hb[:, :K] = _dev(h, dtype, dev)
            ref, ref_db = oracle.dense_bwd_input(dy, w, h, dtype)
            ref_nomask, _ = oracle.dense_bwd_input(dy, w, None, dtype)
            # no mask
            what = f"{dtype} M={M} K={K} N={N} no mask"
            buf, out = _window16(M, K, dtype, dev)
            ops.dense_bwd_input(dyd, wd, out=out)
            _check_dx(_read16(buf, M, K, what), ref_nomask, dy, w, None, N, dtype, what)
            # mask + db_out
            what = f"{dtype} M={M} K={K} N={N} mask db_out"
            buf, out = _window16(M, K, dtype, dev)
            dbuf, db = _guarded32((K,), dev)
            ops.dense_bwd_input(dyd, wd, h=hb[:, :K], db_out=db, out=out)
            dx = _read16(buf, M, K, what)
            _check_dx(dx, ref, dy, w, h, N, dtype, what)
            _check_db(_read32(dbuf, db, what), dx, ref_db, M, what)
            # mask + db_slabs
            what = f"{dtype} M={M} K={K} N={N} mask db_slabs"
            buf, out = _window16(M, K, dtype, dev)
            rows = ops.dense_bwd_bias_slabs(M, K, N, False)
            assert rows == -(-M // 128)
            sbuf, slabs = _guarded32((rows, K), dev)
            ops.dense_bwd_input(dyd, wd, h=hb[:, :K], db_slabs=slabs, out=out)
            dx2 = _read16(buf, M, K, what)
            assert np.array_equal(dx2, dx), what
            sl = _read32(sbuf, slabs, what)
            for t in range(rows):
                part = dx[t * 128:(t + 1) * 128]
                assert np.allclose(sl[t], part.astype(np.float64).sum(axis=0), rtol=0,
                                   atol=128 * 2.0 ** -24 * np.abs(part).sum(axis=0).max() + 1e-30), f"{what}: tile row {t}"
            tot = torch.empty(K, dtype=torch.float32, device=dev)
            ops.sum_slabs(slabs, tot)
            _check_db(tot.cpu().numpy(), dx, ref_db, M, what)


# ---- 5. input gradient: more than 32 tile rows in the bias-sum finish ------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_bwd_input_bias_sum_over_34_tile_rows(dev, oracle, dtype):
    from mindrec_amd import ops
    M, K, N = T.BWD_INPUT_TALL
    T.require_rows(ops, T.BWD_INPUT, M, K, N, 128)
    assert ops.dense_bwd_bias_slabs(M, K, N, False) == 34
    what = f"{dtype} M={M} K={K} N={N}"
    rng = np.random.default_rng(M * 3 + K + N)
    dy, w, h = T.bwd_input_inputs(oracle, rng, M, K, N, dtype)
    hb = torch.full((M, K + 8), NAN, dtype=DT[dtype], device=dev)
    hb[:, :K] = _dev(h, dtype, dev)
    buf, out = _window16(M, K, dtype, dev)
    dbuf, db = _guarded32((K,), dev)
    ops.dense_bwd_input(_dev(dy, dtype, dev), _dev(w, dtype, dev), h=hb[:, :K], db_out=db, out=out)
    dx = _read16(buf, M, K, what)
    ref, ref_db = oracle.dense_bwd_input(dy, w, h, dtype)
    _check_dx(dx, ref, dy, w, h, N, dtype, what)
    _check_db(_read32(dbuf, db, what), dx, ref_db, M, what)


# ---- 6. input gradient, 256-row tiles --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("case", [0, 1], ids=["k8", "k4"])
def test_bwd_input_256_row_tiles(dev, oracle, dtype, case):
    from mindrec_amd import ops
    M, K, N = T.bwd_input_mr8_cases(_cus(dev))[case]
    T.require_rows(ops, T.BWD_INPUT, M, K, N, 256)
    assert K % 8 == (0, 4)[case]
    what = f"{dtype} M={M} K={K} N={N}"
    rng = np.random.default_rng(M * 3 + K + N)
    dy, w, h = T.bwd_input_inputs(oracle, rng, M, K, N, dtype)
    dyd, wd = _dev(dy, dtype, dev), _dev(w, dtype, dev)
    hb = torch.full((M, K + 8), NAN, dtype=DT[dtype], device=dev)
    hb[:, :K] = _dev(h, dtype, dev)
    buf, out = _window16(M, K, dtype, dev)
    dbuf, db = _guarded32((K,), dev)
    ops.dense_bwd_input(dyd, wd, h=hb[:, :K], db_out=db, out=out)
    rows = ops.dense_bwd_bias_slabs(M, K, N, False)
    assert rows == -(-M // 256)
    buf2, out2 = _window16(M, K, dtype, dev)
    sbuf, slabs = _guarded32((rows, K), dev)
    ops.dense_bwd_input(dyd, wd, h=hb[:, :K], db_slabs=slabs, out=out2)
    tot = torch.empty(K, dtype=torch.float32, device=dev)
    ops.sum_slabs(slabs, tot)
    dx = _read16(buf, M, K, what)
    ref, ref_db = oracle.dense_bwd_input(dy, w, h, dtype)
    _check_dx(dx, ref, dy, w, h, N, dtype, what)
    _check_db(_read32(dbuf, db, what), dx, ref_db, M, what)
    assert torch.equal(buf, buf2), f"{what}: dx differs between the db_out and the db_slabs call"
    sl = _read32(sbuf, slabs, what)
    for t in range(rows):
        part = dx[t * 256:(t + 1) * 256]
        assert np.allclose(sl[t], part.astype(np.float64).sum(axis=0), rtol=0,
                           atol=256 * 2.0 ** -24 * np.abs(part).sum(axis=0).max() + 1e-30), f"{what}: tile row {t}"
    _check_db(tot.cpu().numpy(), dx, ref_db, M, what + " slabs")


# ---- 7. weight gradient, 128-row tiles: batch tails and slab splits -------------------------------------------------------
def _run_bwd_weight(dev, oracle, dtype, M, K, N, S, x=None, dy=None, ref=None):
    from mindrec_amd import ops
    what = f"{dtype} M={M} K={K} N={N} S={S}"
    if x is None:
        x, dy = T.bwd_weight_inputs(oracle, np.random.default_rng(M + 7 * K + N), M, K, N, dtype)
    buf, slabs = _guarded32((S, K, N), dev)
    ops.dense_bwd_weight(_tall(x, dtype, dev), _tall(dy, dtype, dev), slabs)
    sl = _read32(buf, slabs, what)
    _check_slabs(sl, x, dy, M, S, oracle, what)
    _check_slab_sum(slabs, sl, x, dy, M, oracle, what, ref)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("K,N", T.BWD_WEIGHT_KN)
def test_bwd_weight_batch_tail_and_split_sweep(dev, oracle, dtype, K, N):
    from mindrec_amd import ops
    for M in T.BWD_WEIGHT_M + [T.BWD_WEIGHT_EMPTY[0]]:
        T.require_rows(ops, T.BWD_WEIGHT, M, K, N, 128)
        ttot = -(-M // 64)
        splits = sorted({1, ttot, ttot + 3}) if M != T.BWD_WEIGHT_EMPTY[0] else [T.BWD_WEIGHT_EMPTY[1]]
        x, dy = T.bwd_weight_inputs(oracle, np.random.default_rng(M + 7 * K + N), M, K, N, dtype)
        ref = oracle.dense_bwd_weight(x, dy)
        for S in splits:
            _run_bwd_weight(dev, oracle, dtype, M, K, N, S, x, dy, ref)
    M, S = T.BWD_WEIGHT_EMPTY
    assert T.slab_rows(M, S)[4:] == [(512, 520), (520, 520), (520, 520), (520, 520)]


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_bwd_weight_library_split_leaves_empty_slabs(dev, oracle, dtype):
    """a 512 x 1024 layer at batch 576: nine K-tiles in the eight slabs the library itself proposes on 256 CUs -- two per slab,
    the last three slabs empty"""
    from mindrec_amd import ops
    M, K, N = T.BWD_WEIGHT_ENGINE
    T.require_rows(ops, T.BWD_WEIGHT, M, K, N, 128)
    S = ops.dense_bwd_weight_slabs(M, K, N)
    assert any(r0 == r1 for r0, r1 in T.slab_rows(M, S)), (
        f"dense_bwd_weight_slabs({M}, {K}, {N}) = {S} on {_cus(dev)} CUs leaves no slab empty any more: find the batch that does")
    _run_bwd_weight(dev, oracle, dtype, M, K, N, S)


# ---- 8. weight gradient, 256-row tiles -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES)
def test_bwd_weight_256_row_tiles(dev, oracle, dtype):
    from mindrec_amd import ops
    M, K, N = T.BWD_WEIGHT_MR8
    T.require_rows(ops, T.BWD_WEIGHT, M, K, N, 256)
    x, dy = T.bwd_weight_inputs(oracle, np.random.default_rng(M + 7 * K + N), M, K, N, dtype)
    ref = oracle.dense_bwd_weight(x, dy)
    empties = []
    for S in T.BWD_WEIGHT_MR8_SPLITS:
        empties.append(sum(r0 == r1 for r0, r1 in T.slab_rows(M, S)))
        _run_bwd_weight(dev, oracle, dtype, M, K, N, S, x, dy, ref)
    assert empties == [0, 3, 1]


# ---- 9. the fused backward launch, all four instantiations ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("case", [0, 1, 2, 3], ids=["d128_w128", "d128_w256", "d256_w128", "d256_w256"])
def test_bwd_fused_launch_every_instantiation(dev, oracle, dtype, case):
    """k_gemm256_bwd<MRD, MRW>: bit-equal to the two separate launches (dx, dw slabs, db slabs); dx and the dw sum within the
    oracle bounds; an extra weight-gradient problem of another width riding the launch, checked slab by slab"""
    from mindrec_amd import ops
    name, rows_d, rows_w, (M, K, N), with_extra = T.fused_cases(_cus(dev))[case]
    T.require_rows(ops, T.BWD_INPUT, M, K, N, rows_d)
    T.require_rows(ops, T.BWD_WEIGHT, M, K, N, rows_w)
    what = f"{dtype} {name} M={M} K={K} N={N}"
    rng = np.random.default_rng(M + K)
    dy, w, x = T.bwd_input_inputs(oracle, rng, M, K, N, dtype)                  # x: the layer's input and the mask source
    dyd, wd = _tall(dy, dtype, dev), _dev(w, dtype, dev)
    xd = _tall(x, dtype, dev, width=K + 8)                                      # ... with the output's row stride
    S = ops.dense_bwd_weight_slabs(M, K, N)
    rows = ops.dense_bwd_bias_slabs(M, K, N, True)
    assert rows == ops.dense_bwd_bias_slabs(M, K, N, False) == -(-M // rows_d)
    extra, ex = None, None
    if with_extra:
        Ke, Ne, Se = T.EXTRA_KN_S
        if (-(-M // 64)) % Se == 0:
            Se = 5              # a split whose last slab is short, where three slabs would divide the K-tiles evenly
        assert (-(-M // 64)) % Se != 0
        xe, dye = T.bwd_weight_inputs(oracle, rng, M, Ke, Ne, dtype)
        ebuf, eslabs = _guarded32((Se, Ke, Ne), dev)
        extra = [(_tall(xe, dtype, dev), _tall(dye, dtype, dev), eslabs)]
        ex = (xe, dye, Se, ebuf, eslabs)
    buf1, out1 = _window16(M, K, dtype, dev)
    wbuf1, dw1 = _guarded32((S, K, N), dev)
    bbuf1, db1 = _guarded32((rows, K), dev)
    ops.dense_bwd(dyd, wd, xd, dw1, mask=True, db_slabs=db1, out=out1, extra=extra)
    buf2, out2 = _window16(M, K, dtype, dev)
    wbuf2, dw2 = _guarded32((S, K, N), dev)
    bbuf2, db2 = _guarded32((rows, K), dev)
    ops.dense_bwd_input(dyd, wd, h=xd, db_slabs=db2, out=out2)
    ops.dense_bwd_weight(xd, dyd, dw2)
    dx = _read16(buf1, M, K, what)
    sl = _read32(wbuf1, dw1, what + " dw")
    _read32(bbuf1, db1, what + " db")
    assert torch.equal(buf1, buf2), f"{what}: dx differs from the separate launch"
    assert np.array_equal(sl, _read32(wbuf2, dw2, what + " dw separate")), f"{what}: dw slabs differ from the separate launch"
    assert torch.equal(db1, db2), f"{what}: db slabs differ from the separate launch"
    ref, ref_db = oracle.dense_bwd_input(dy, w, x, dtype)
    _check_dx(dx, ref, dy, w, x, N, dtype, what)
    tot = torch.empty(K, dtype=torch.float32, device=dev)
    ops.sum_slabs(db1, tot)
    _check_db(tot.cpu().numpy(), dx, ref_db, M, what)
    empty = [s for s, (r0, r1) in enumerate(T.slab_rows(M, S)) if r0 == r1]
    for s in empty:
        assert (sl[s] == 0.0).all(), f"{what}: empty slab {s} of {S}"
    _check_slab_sum(dw1, sl, x, dy, M, oracle, what + " dw")
    if ex is not None:
        xe, dye, Se, ebuf, eslabs = ex
        esl = _read32(ebuf, eslabs, what + " extra")
        _check_slabs(esl, xe, dye, M, Se, oracle, what + " extra")
        _check_slab_sum(eslabs, esl, xe, dye, M, oracle, what + " extra")
