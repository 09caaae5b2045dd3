"""mrec_clip_group_sums_f32 (ops.clip_group_sums_) on the GPU against the float64 model of the clip's Jacobian (tests/_clip_sums_ref.py):
every width class of the lane-group geometry (nd = D / 4 a power of two or not, one row per wave .. 64 rows per wave, more than one
workgroup, a partial last wave), groups the call must leave alone bit for bit (rows outside the table, groups past the device count,
unclipped rows, a zero row, an exact tie), the clip decision against the lookup's over rows a few ulps around the bound, and the call
inside a captured HIP graph."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _clip_sums_ref as R  # noqa: E402

V = 97
C = 0.75                      # (its square is an exact float32: the tie row's fp32 norm is c whatever the summation order)
WIDTHS = (4, 12, 20, 64, 128, 252, 256)
ZERO_ROW, TIE_ROW = 5, 7
U_LIVE, U_ALL = 300, 320      # groups below the device count / in the buffer (D = 4: 64 groups per wave, 256 per workgroup)


def _row_rel(a, b):
    den = np.maximum(np.abs(b).max(axis=1), 1e-30)
    return float((np.abs(a.astype(np.float64) - b).max(axis=1) / den).max()) if a.size else 0.0


def _table(rng, D):
    """rows of norm 0.4 c .. 0.9 c or 1.1 c .. 3 c (either side of the bound, far from it), a zero row and an exact tie"""
    x = rng.standard_normal((V, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    f = np.where(rng.random(V) < 0.5, rng.uniform(0.4, 0.9, V), rng.uniform(1.1, 3.0, V))
    p = (x * (C * f)[:, None]).astype(np.float32)
    p[ZERO_ROW] = 0.0
    p[TIE_ROW] = 0.0
    p[TIE_ROW, D // 2] = C
    return p


def _groups(rng):
    """the groups' rows: every table row at least once (0 and V - 1 among them), repeats, a -1 and a row >= V; U_ALL entries of which
    the first U_LIVE count"""
    u = np.concatenate([rng.permutation(V), rng.integers(0, V, size=U_ALL - V)]).astype(np.int32)
    u[11], u[200] = -1, V + 3
    u[20], u[21] = ZERO_ROW, TIE_ROW
    u[U_LIVE - 1], u[U_LIVE], u[U_LIVE + 1] = V - 1, 0, V - 1      # the last live group and the first two behind the count
    return u


def _plan(u, n_live, dev):
    return SimpleNamespace(uniq_buf=torch.from_numpy(u).to(dev), n_uniq_dev=torch.tensor([n_live], dtype=torch.int64, device=dev))


def _build_cases():
    out = {}
    for D in WIDTHS:
        rng = np.random.default_rng(100 + D)
        p, u = _table(rng, D), _groups(rng)
        G = (rng.standard_normal((U_ALL, D)) * 0.01).astype(np.float32)
        live = (np.arange(U_ALL) < U_LIVE) & (u >= 0) & (u < V)
        ref64 = G.astype(np.float64)
        hit = np.zeros(U_ALL, bool)
        g = np.flatnonzero(live)
        ref64[g] = R.jacobian_apply64(p[u[g]], G[g], C)
        hit[g] = R.clip_sums64(p[u[g]], G[g], C)[1]
        out[D] = (p, u, G, ref64, hit)
    return out


@pytest.fixture(scope="module")
def cases():
    """per width: (table, groups' rows, sums, the float64 model's sums, clipped groups) -- built once, never written"""
    return _build_cases()


@pytest.mark.parametrize("D", WIDTHS)
def test_group_sums_match_the_float64_jacobian(dev, cases, D):
    from mindrec_amd import ops
    p, u, G, ref64, hit = cases[D]
    assert 0.2 * U_LIVE < hit.sum() < 0.8 * U_LIVE and not hit[U_LIVE:].any()
    zero_g, tie_g = np.flatnonzero(u[:U_LIVE] == ZERO_ROW), np.flatnonzero(u[:U_LIVE] == TIE_ROW)
    assert zero_g.size and tie_g.size and not hit[zero_g].any() and not hit[tie_g].any()
    tp, sums = torch.from_numpy(p).to(dev), torch.from_numpy(G).to(dev)
    back = ops.clip_group_sums_(sums, _plan(u, U_LIVE, dev), tp, C)
    assert back is sums
    got = sums.cpu().numpy()
    assert np.isfinite(got).all()
    # unclipped groups -- norm <= c, the tie, the zero row, rows outside the table, everything behind the device count: bit for bit
    assert np.array_equal(got[~hit].view(np.int32), G[~hit].view(np.int32))
    assert (got[hit] != G[hit]).any(axis=1).all()                          # every clipped group was rewritten
    err = _row_rel(got[hit], ref64[hit])
    print(f"D={D}: {int(hit.sum())} clipped groups, row-relative error {err:.3g}")
    assert err <= 1e-5
    assert np.array_equal(tp.cpu().numpy(), p)                              # the table is only read


@pytest.mark.parametrize("D", WIDTHS)
def test_device_count_above_the_buffer(dev, cases, D):
    """min(U, *n_uniq_dev): a device count past the buffer's length touches the buffer's groups only"""
    from mindrec_amd import ops
    p, u, G, _, _ = cases[D]
    tp = torch.from_numpy(p).to(dev)
    ok = (u >= 0) & (u < V)
    ref, hit = G.copy(), np.zeros(U_ALL, bool)
    ref[ok], hit[ok] = R.clip_sums64(p[u[ok]], G[ok], C)
    guard = np.full((8, D), 7.0, np.float32)                                # rows behind the U groups of a longer buffer
    sums = torch.from_numpy(np.concatenate([G, guard])).to(dev)
    ops.clip_group_sums_(sums, _plan(u, U_ALL + 1000, dev), tp, C)
    got = sums.cpu().numpy()
    assert np.array_equal(got[U_ALL:], guard)
    assert np.array_equal(got[:U_ALL][~hit].view(np.int32), G[~hit].view(np.int32))
    assert _row_rel(got[:U_ALL][hit], ref[hit].astype(np.float64)) <= 1e-5


@pytest.mark.parametrize("D", WIDTHS)
def test_the_decision_is_the_lookups(dev, D):
    """Rows whose fp32 norm lies within a few ulps of c: the groups the call changed are exactly the rows gather_rows(max_norm=c)
    scaled -- one sum of squares, one decision."""
    from mindrec_amd import ops
    rng = np.random.default_rng(300 + D)
    x = rng.standard_normal((V, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = (x * C * (1.0 + rng.integers(-6, 7, size=(V, 1)) * 2.0 ** -24)).astype(np.float32)
    G = (rng.standard_normal((V, D)) * 0.01).astype(np.float32)
    tp = torch.from_numpy(x).to(dev)
    ids = torch.arange(V, dtype=torch.int32, device=dev)
    clipped_fwd = (ops.gather_rows(tp, ids, max_norm=C).cpu().numpy() != x).any(axis=1)
    assert 10 < clipped_fwd.sum() < V - 10                                  # both decisions occur among the near-ties
    sums = torch.from_numpy(G).to(dev)
    ops.clip_group_sums_(sums, ops.sparse_plan(ids), tp, C)                 # (a real plan: its groups are the ids in order)
    changed = (sums.cpu().numpy() != G).any(axis=1)
    assert np.array_equal(clipped_fwd, changed), int((clipped_fwd != changed).sum())


def test_captured_call_replays_to_the_eager_bits(dev, cases):
    from mindrec_amd import ops
    D = 20
    p, u, G, _, hit = cases[D]
    tp, G0 = torch.from_numpy(p).to(dev), torch.from_numpy(G).to(dev)
    plan = _plan(u, U_LIVE, dev)
    eager = ops.clip_group_sums_(G0.clone(), plan, tp, C)
    static = G0.clone()
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        ops.clip_group_sums_(static, plan, tp, C)
    assert torch.equal(static, G0)                                          # capturing runs nothing
    for _ in range(2):
        static.copy_(G0)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(static, eager)
    assert hit.any() and not torch.equal(eager, G0)


def test_wrapper_checks_its_arguments(dev, cases):
    from mindrec_amd import _lib, ops
    p, u, G, _, _ = cases[12]
    tp, plan = torch.from_numpy(p).to(dev), _plan(u, U_LIVE, dev)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            ops.clip_group_sums_(torch.from_numpy(G).to(dev), plan, tp, bad)
    with pytest.raises(TypeError, match="sums"):
        ops.clip_group_sums_(torch.from_numpy(G[:U_ALL - 1]).to(dev), plan, tp, C)            # fewer rows than groups
    with pytest.raises(TypeError, match="sums"):
        ops.clip_group_sums_(torch.from_numpy(G).to(dev).double(), plan, tp, C)
    with pytest.raises(_lib.MrecError):
        ops.clip_group_sums_(torch.zeros((U_ALL, 6), device=dev), plan, torch.zeros((V, 6), device=dev), C)      # D % 4 != 0
