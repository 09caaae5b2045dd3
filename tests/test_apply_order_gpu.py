"""The sparse apply (mindrec_amd/csrc/mrec_apply.hip) bit for bit against the host restatement of its order of additions
(tests/_apply_order.py): every row of every path -- LazyAdam, FTRL, the segment sum, the wide-folded LazyAdam + FTRL with its finishing
pass launched or deferred into the dense Adam, the hot-column path, the skip-negative plan, max_norm -- on layouts of the sorted index
built to reach window boundaries at every offset, straddling pairs around the pairs_on threshold, runs at the pass A / pass B boundary
and past 16 NG partials, out-of-range rows in crossing runs, and grids past the cap.  Each case first asserts its own census, so that a
layout cannot silently stop covering what it claims.  Untouched rows and the padding columns of ld > D tables are compared too."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _apply_order as A  # noqa: E402
import _oracle_clip_ops as OC  # noqa: E402
from oracle import oracle as O  # noqa: E402

_G16 = {torch.bfloat16: "bf16", torch.float16: "f16"}
_NP = {torch.int32: np.int32, torch.int64: np.int64}
STEPS = ((0.9, 0.999), (0.81, 0.998001))        # beta powers of the two steps every case takes


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, ref, what):
    bad = got.view(np.uint32) != ref.view(np.uint32)
    rows = np.nonzero(bad.reshape(bad.shape[0], -1).any(axis=1))[0]
    assert rows.size == 0, f"{what}: {rows.size} rows differ from the restatement, e.g. {rows[:6].tolist()}"


def _aw(D, vec):
    from mindrec_amd import ops
    return ops.apply_window(D, vec == 4)


def _seq(layout, aw, ngs, rng):
    if layout in ("boundaries", "oob"):
        return A.boundaries(aw)
    if layout == "tree":
        return A.tree(aw, ngs, rng)
    if layout.startswith("pairs_"):
        return A.pairs(aw, layout[len("pairs_"):])
    raise ValueError(layout)


def _keys(U, rng, idt, oob):
    """U distinct keys and the table size V: rows of the table, with every fifth key below 0 and every fifth past V where oob (and,
    with 64-bit keys, keys >= 2^31)"""
    V = U + 97
    keys = rng.permutation(V)[:U].astype(np.int64)
    if oob:
        keys[1::5] = -1 - np.arange(keys[1::5].size)
        keys[3::5] = V + np.arange(keys[3::5].size)
        if idt == np.int64:
            keys[3::10] += 2 ** 31
    return keys.astype(idt), V


def _check_census(c, layout, aw):
    if layout in ("boundaries", "oob"):
        assert c["crossing"] > 50 and c["inside"] > 0 and c["pairs"] > 0 and not c["pairs_on"], c
        assert all(b["pass_a"] > 50 for b in c["blocks"]), c
    if layout == "oob":
        assert c["oob_crossing"] > 10, c
    if layout == "tree":
        for b in c["blocks"]:
            assert b["at_ng"] >= 2 and b["at_ng1"] >= 2 and b["over_long"] >= 2 and b["pass_a"] > 0 and b["pass_b"] > 0, c
    if layout.startswith("pairs_"):
        assert c["pairs_on"] == (layout != "pairs_over") and c["pairs"] >= 12, c
        assert abs((c["n"] - c["U"]) * 16 - c["n"]) <= aw + 1, c
    if layout == "capped":
        assert c["blocks"][0]["capped"] and c["crossing"] > 1000, c


def _grads(rng, n, D, gdt, ldg=None):
    """gradient rows (fp32 values of the dtype the kernel reads) and the device tensor, rows ldg apart"""
    g = rng.standard_normal((n, D)).astype(np.float32)
    if gdt in _G16:
        g = O.round16(g, _G16[gdt])
    buf = np.zeros((n, ldg or D), np.float32)
    buf[:, :D] = g
    return g, buf, gdt


def _dev_grads(buf, D, gdt, dev):
    return T(buf, dev).to(gdt)[:, :D]


def _ld(D):
    """a row stride past D that keeps D's lane width"""
    return D + 4 if D % 4 == 0 else D + 2 if D % 2 == 0 else D + 1


def _state(rng, V, ld, kind):
    """[V, ld] state arrays, padding columns included (they must come back untouched)"""
    a = (rng.standard_normal((V, ld)) * 0.01).astype(np.float32)
    if kind == "adam":
        return [a, (rng.standard_normal((V, ld)) * 1e-3).astype(np.float32), (rng.random((V, ld)) * 1e-5).astype(np.float32)]
    return [a, (rng.random((V, ld)) + 0.5).astype(np.float32), (rng.standard_normal((V, ld)) * 1e-3).astype(np.float32)]


# ---- LazyAdam -----------------------------------------------------------------------------------------------------------------------
_LAYOUTS = ["boundaries", "tree", "pairs_under", "pairs_at", "pairs_over", "oob"]
_ADAM = []
for _i, (_D, _lay) in enumerate((d, l) for d in (80, 16, 128, 1, 30, 7, 260, 512) for l in _LAYOUTS):
    _ADAM.append((_D, _lay, (torch.float32, torch.bfloat16, torch.float16)[_i % 3], (torch.int32, torch.int64)[(_i // 3) % 2],
                  _i % 4 != 3, _D == 80 and _lay == "boundaries", None, None))
_ADAM += [(80, "boundaries", torch.float32, torch.int32, True, False, 82, None),      # 8-byte lanes at D % 4 == 0
          (80, "tree", torch.bfloat16, torch.int64, True, False, 81, None),           # 4-byte lanes
          (16, "tree", torch.float32, torch.int32, True, False, None, 20),            # gradient rows 20 apart
          (128, "capped", torch.bfloat16, torch.int32, True, False, None, None)]      # past k_apply_main's grid cap


@pytest.mark.parametrize("D,layout,gdt,idt,use_rs,nesterov,ld,ldg", _ADAM)
def test_sparse_lazy_adam_bitwise(dev, D, layout, gdt, idt, use_rs, nesterov, ld, ldg):
    from mindrec_amd import ops
    rng = np.random.default_rng(D * 101 + len(layout) + (ld or 0))
    ld = ld or _ld(D)
    vec = A.lane_width(D, ld, ldg or D, [0], 0, 4)
    aw = _aw(D, vec)
    ngs = [b[3] for b in A.col_blocks(D, vec)]
    seq = A.grow(A.boundaries(aw), A.MREC_APPLY_MAXB * 4 * 2 * aw + 1) if layout == "capped" else _seq(layout, aw, ngs, rng)
    keys, V = _keys(len(seq), rng, _NP[idt], layout == "oob")
    ids = A.layout_ids(seq, keys, rng)
    n = ids.size
    idx = A.Index(ids)
    _check_census(A.census(idx, D, vec, aw, V=V), layout, aw)
    st = _state(rng, V, ld, "adam")
    tst = [T(a, dev) for a in st]
    plan = ops.sparse_plan(T(ids, dev))
    for b1p, b2p in STEPS:                                       # two steps, state carried over
        g, gbuf, _ = _grads(rng, n, D, gdt, ldg)
        rs = (rng.random(n) + 0.25).astype(np.float32) if use_rs else None
        gs = 0.37
        ops.sparse_lazy_adam_(*(t[:, :D] for t in tst), plan, _dev_grads(gbuf, D, gdt, dev), T(rs, dev) if use_rs else None,
                              beta1_power=b1p, beta2_power=b2p, grad_scale=gs, use_nesterov=nesterov)
        G = A.sums(idx, A.contributions(g, rs, gs), D, vec, aw)
        A.lazy_adam(*(a[:, :D] for a in st), idx.uniq, G, b1_pow=b1p, b2_pow=b2p, nesterov=nesterov)
    for name, t, a in zip("pmv", tst, st):
        _same(t.cpu().numpy(), a, name)


# ---- FTRL ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["boundaries", "tree", "pairs_under", "oob"])
@pytest.mark.parametrize("D", [1, 16, 30, 7])
def test_sparse_ftrl_bitwise(dev, D, layout):
    from mindrec_amd import ops
    rng = np.random.default_rng(D * 7 + len(layout))
    idt = np.int64 if layout == "oob" else np.int32
    ld = _ld(D)
    vec = A.lane_width(D, ld, D, [0], 0, 4)
    aw = _aw(D, vec)
    seq = _seq(layout, aw, [b[3] for b in A.col_blocks(D, vec)], rng)
    keys, V = _keys(len(seq), rng, idt, layout == "oob")
    ids = A.layout_ids(seq, keys, rng)
    idx = A.Index(ids)
    _check_census(A.census(idx, D, vec, aw, V=V), layout, aw)
    st = _state(rng, V, ld, "ftrl")
    tst = [T(a, dev) for a in st]
    plan = ops.sparse_plan(T(ids, dev))
    for _ in range(2):
        g = rng.standard_normal((ids.size, D)).astype(np.float32)
        rs = (rng.random(ids.size) + 0.25).astype(np.float32)
        ops.sparse_ftrl_(*(t[:, :D] for t in tst), plan, T(g, dev), T(rs, dev), grad_scale=0.37)
        A.ftrl(*(a[:, :D] for a in st), idx.uniq, A.sums(idx, A.contributions(g, rs, 0.37), D, vec, aw))
    for name, t, a in zip(("var", "accum", "linear"), tst, st):
        _same(t.cpu().numpy(), a, name)


# ---- segment sum --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["boundaries", "tree"])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [80, 300, 130, 7])
def test_segment_sum_bitwise(dev, D, gdt, layout):
    from mindrec_amd import ops
    rng = np.random.default_rng(D + len(layout) + (gdt == torch.float32))
    vec = A.lane_width(D, D, D, [0], 0, 2 if gdt in _G16 else 4)
    aw = _aw(D, vec)
    ngs = [b[3] for b in A.col_blocks(D, vec)]
    seq = _seq(layout, aw, ngs if D < 64 else [min(ngs)], rng)
    ids = A.layout_ids(seq, np.arange(len(seq), dtype=np.int32) * 3, rng)
    idx = A.Index(ids)
    c = A.census(idx, D, vec, aw)
    assert c["crossing"] > (50 if layout == "boundaries" else 4) and c["blocks"][0]["pass_a"] > 0
    if layout == "tree":
        assert c["blocks"][0]["pass_b"] > 0 and c["blocks"][0]["at_ng"] > 0 and c["blocks"][0]["over_long"] > 0
    g, gbuf, _ = _grads(rng, ids.size, D, gdt)
    rs = (rng.random(ids.size) + 0.25).astype(np.float32)
    out = ops.segment_sum(ops.sparse_plan(T(ids, dev)), _dev_grads(gbuf, D, gdt, dev), T(rs, dev), grad_scale=0.37)[: idx.U]
    _same(out.cpu().numpy(), A.sums(idx, A.contributions(g, rs, 0.37), D, vec, aw), "segment sum")


# ---- the wide-folded apply ----------------------------------------------------------------------------------------------------------
_WKW = dict(lr=3.5e-4, grad_scale=0.37)


def _wide_case(dev, rng, ids, F, gdt, V, defer, skip_negative=False, const=None, max_norm=None, p0=None, D=80):
    """one step of sparse_lazy_adam_wide_ on fused [p | w accum linear pad | m | v | pad] rows (the engine's 128-byte padded stride: ld 256
    at D = 80) and its restatement; returns (device rows, restated rows, device dense buffers, restated dense buffers, the index, the hot
    columns found)"""
    from mindrec_amd import ops
    ld = -(-(3 * D + 4) // 32) * 32
    n = ids.size
    buf = _state(rng, V, ld, "adam")[0]
    if p0 is not None:
        buf[:, :D] = p0
    buf[:, D + 1] = 1.0 + rng.random(V).astype(np.float32)             # FTRL accum
    buf[:, 2 * D + 4:3 * D + 4] = np.abs(buf[:, 2 * D + 4:3 * D + 4]) * 1e-3
    g, gbuf, _ = _grads(rng, n, D, gdt)
    gw = rng.standard_normal(n // F).astype(np.float32)
    rs = (rng.random(n) + 0.25).astype(np.float32)
    tb = T(buf, dev)
    tid = T(ids, dev)
    plan = ops.sparse_plan(tid.reshape(-1), skip_negative=skip_negative)
    cc = None
    if const is not None:
        cc = (ops.const_cols_detect(tid, V, min_count=const), tid)
    b1p, b2p = STEPS[0]
    fin = ops.sparse_lazy_adam_wide_(tb[:, :D], tb[:, D + 4:2 * D + 4], tb[:, 2 * D + 4:3 * D + 4], plan, _dev_grads(gbuf, D, gdt, dev),
                                     T(rs, dev), T(gw, dev), F, D, beta1_power=b1p, beta2_power=b2p, defer=defer, const_cols=cc,
                                     max_norm=max_norm, **_WKW)
    nd = 4096
    dn = [(rng.standard_normal(nd) * 0.01).astype(np.float32), (rng.standard_normal(nd) * 1e-3).astype(np.float32),
          (rng.random(nd) * 1e-5).astype(np.float32), rng.standard_normal(nd).astype(np.float32)]
    tdn = [T(a, dev) for a in dn]
    if defer:
        ops.dense_adam_slabs_(*tdn, [], finish=fin, lr=3.5e-4, beta1_power=b1p, beta2_power=b2p, grad_scale=0.37)
        O.dense_adam(dn[0], dn[1], dn[2], dn[3], lr=3.5e-4, b1_pow=b1p, b2_pow=b2p, grad_scale=0.37)
    hot = ops.const_cols_ids(cc[0]) if cc is not None else None
    idx = A.Index(ids, skip_negative=skip_negative)
    x = A.contributions(g, rs, 0.37)
    xw = A.contributions(np.repeat(gw, F), rs, 0.37)
    G = A.sums(idx, x, D, 4, _aw(D, 4), xw=xw, hot=hot, ids2d=ids.reshape(-1, F) if hot else None)
    ref = buf.copy()
    if max_norm is not None:
        rows = idx.uniq.astype(np.int64)
        ok = (rows >= 0) & (rows < V)
        Gc = G.copy()
        Gc[ok, :D] = OC.jacobian_apply64(ref[rows[ok], :D], G[ok, :D], max_norm).astype(np.float32)
        A.lazy_adam(ref[:, :D], ref[:, D + 4:2 * D + 4], ref[:, 2 * D + 4:3 * D + 4], idx.uniq, Gc, b1_pow=b1p, b2_pow=b2p, lr=3.5e-4)
    else:
        A.lazy_adam(ref[:, :D], ref[:, D + 4:2 * D + 4], ref[:, 2 * D + 4:3 * D + 4], idx.uniq, G, b1_pow=b1p, b2_pow=b2p, lr=3.5e-4)
    A.wide_ftrl(ref[:, D:D + 4], idx.uniq, G)
    torch.cuda.synchronize()
    return tb.cpu().numpy(), ref, [t.cpu().numpy() for t in tdn], dn, idx, hot


def _wide_ids(seq, rng, F, oob=False):
    """layout ids padded with singletons to a multiple of F (a batch of n / F samples)"""
    seq = list(seq) + [1] * ((-sum(seq)) % F)
    keys, V2 = _keys(len(seq), rng, np.int32, oob)
    return A.layout_ids(seq, keys, rng), V2


@pytest.mark.parametrize("layout,defer", [(lay, d) for lay in ("boundaries", "tree", "pairs_under", "pairs_over", "oob", "skip_negative")
                                          for d in (False, True)] + [("capped", False)])
def test_sparse_lazy_adam_wide_bitwise(dev, layout, defer):
    rng = np.random.default_rng(len(layout) * 3 + defer)
    D, aw = 80, _aw(80, 4)
    ngs = [b[3] for b in A.col_blocks(D, 4, True)]
    if layout == "capped":
        seq = A.grow(A.boundaries(aw), A.MREC_APPLY_MAXB * 4 * 3 * aw + 1)
    else:
        seq = _seq("boundaries" if layout == "skip_negative" else layout, aw, ngs, rng)
    F = 1 if layout in ("skip_negative", "capped") or layout.startswith("pairs_") else 13
    ids, V = _wide_ids(seq, rng, F, oob=layout == "oob")
    gdt = (torch.bfloat16, torch.float16, torch.float32)[len(layout) % 3]
    if layout == "skip_negative":                                   # padding slots spread through the message and a tail of them
        total = ids.size + ids.size // 4 + 400
        pad = np.zeros(total, bool)
        pad[-400:] = True
        pad[rng.choice(total - 400, size=ids.size // 4, replace=False)] = True
        full = np.full(total, -1, np.int32)
        full[~pad] = ids
        ids = full
    idx = A.Index(ids, skip_negative=layout == "skip_negative")
    _check_census(A.census(idx, D, 4, aw, wide=True, V=V), "boundaries" if layout == "skip_negative" else layout, aw)
    got, ref, dgot, dref, _, _ = _wide_case(dev, rng, ids, F, gdt, V, defer, skip_negative=layout == "skip_negative")
    _same(got, ref, "fused rows")
    for name, a, b in zip("pmv", dgot, dref):
        _same(a, b, "dense " + name)


def _cc_ids(rng, B, F, V, nconst, dom):
    ids = np.minimum(rng.zipf(1.1, size=(B, F)) + 64, V - 1).astype(np.int32)
    ids[:, :nconst] = np.arange(nconst, dtype=np.int32)[None, :] + 7
    for d in range(dom):
        ids[rng.random(B) < 0.4 + 0.1 * d, 20 + d] = 30 + d
    return ids


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("B,nconst,dom,gdt", [(1024, 13, 0, torch.float16), (2000, 18, 3, torch.bfloat16), (777, 0, 5, torch.float32),
                                              (96, 1, 0, torch.bfloat16)])
def test_wide_hot_columns_bitwise(dev, defer, B, nconst, dom, gdt):
    """constant and dominant ids through the hot-column path (const_part_body / const_finish_body), every other id through the windows"""
    rng = np.random.default_rng(B + nconst + dom)
    V, F = 5000, 39
    ids = _cc_ids(rng, B, F, V, nconst, dom)
    got, ref, dgot, dref, idx, hot = _wide_case(dev, rng, ids, F, gdt, V, defer, const=B // 8 if dom else B)
    want = {f: f + 7 for f in range(nconst)}
    want.update({20 + d: 30 + d for d in range(dom)})
    assert hot == want
    c = A.census(idx, 80, 4, _aw(80, 4), wide=True, hot_ids=list(want.values()))
    assert c["crossing"] > 20 and c["blocks"][0]["pass_a"] > 0, c
    _same(got, ref, "fused rows")
    for name, a, b in zip("pmv", dgot, dref):
        _same(a, b, "dense " + name)


# ---- max_norm -----------------------------------------------------------------------------------------------------------------------
def _clip_rows(rng, V, D, c, idx, aw, NG):
    """rows at 3 c (clipped) or 0.5 c (not), and zero rows; the rows of crossing runs alternate between 3 c and 0.5 c"""
    t = rng.standard_normal((V, D))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    scale = rng.choice([3.0, 0.5, 0.0], size=V, p=[0.45, 0.45, 0.1])
    _, _, npc = A._pieces(idx, aw)
    for sel in (npc <= NG, npc > NG):                  # (crossing runs of pass A and of pass B: both kinds of rows in each)
        r = idx.uniq.astype(np.int64)[(npc > 1) & sel]
        scale[r] = np.where(np.arange(r.size) % 2 == 0, 3.0, 0.5)
    return (t * scale[:, None] * c).astype(np.float32)


def _row_rel(a, b):
    den = np.maximum(np.abs(b).max(axis=1), 1e-30)
    return float((np.abs(a.astype(np.float64) - b).max(axis=1) / den).max()) if a.size else 0.0


def _check_clip(got, ref, rows_clipped, V, what):
    """rows the clip leaves alone (norm <= c, untouched rows): bit for bit; clipped rows: within test_max_norm_gpu's 1e-5"""
    other = np.ones(V, bool)
    other[rows_clipped] = False
    _same(got[other], ref[other], what)
    assert _row_rel(got[rows_clipped], ref[rows_clipped]) <= 1e-5, what


def _clip_census(idx, p0, c, aw, NG):
    """both the clipped and the unclipped rows include runs finished by pass A and by pass B"""
    _, ps, npc = A._pieces(idx, aw)
    rows = idx.uniq.astype(np.int64)
    clipped = np.linalg.norm(p0[rows].astype(np.float64), axis=1) > c
    for sel in (clipped, ~clipped):
        assert ((npc > 1) & (npc <= NG) & sel).sum() > 0 and ((npc > NG) & sel).sum() > 0
    return rows[clipped]


@pytest.mark.parametrize("layout", ["boundaries", "tree"])
def test_sparse_lazy_adam_max_norm(dev, layout):
    from mindrec_amd import ops
    rng = np.random.default_rng(40 + len(layout))
    D, ld, c = 80, 84, 0.09
    aw = _aw(D, 4)
    NG = A.col_blocks(D, 4)[0][3]
    seq = _seq(layout, aw, [NG], rng)
    if layout == "boundaries":
        seq = seq + A.tree(aw, [NG], rng)                                 # (runs for pass B)
    keys, V = _keys(len(seq), rng, np.int32, False)
    ids = A.layout_ids(seq, keys, rng)
    idx = A.Index(ids)
    st = _state(rng, V, ld, "adam")
    st[0][:, :D] = _clip_rows(rng, V, D, c, idx, aw, NG)
    clipped = _clip_census(idx, st[0][:, :D], c, aw, NG)
    tst = [T(a, dev) for a in st]
    g = (rng.standard_normal((ids.size, D)) * 0.5).astype(np.float32)
    rs = (rng.random(ids.size) + 0.25).astype(np.float32)
    ops.sparse_lazy_adam_(*(t[:, :D] for t in tst), ops.sparse_plan(T(ids, dev)), T(g, dev), T(rs, dev), grad_scale=0.37, max_norm=c)
    G = A.sums(idx, A.contributions(g, rs, 0.37), D, 4, aw)
    rows = idx.uniq.astype(np.int64)
    G[:, :] = OC.jacobian_apply64(st[0][rows, :D], G, c).astype(np.float32)     # (G itself where |x| <= c)
    A.lazy_adam(*(a[:, :D] for a in st), idx.uniq, G)
    for name, t, a in zip("pm", tst, st):
        _check_clip(t.cpu().numpy(), a, clipped, V, name)
    _same(tst[2].cpu().numpy()[np.setdiff1d(np.arange(V), clipped)], st[2][np.setdiff1d(np.arange(V), clipped)], "v")


@pytest.mark.parametrize("layout", ["boundaries", "tree"])
@pytest.mark.parametrize("defer", [False, True])
def test_sparse_lazy_adam_wide_max_norm(dev, layout, defer):
    rng = np.random.default_rng(50 + len(layout) + defer)
    D, c, F = 80, 0.09, 13
    aw = _aw(D, 4)
    NG = A.col_blocks(D, 4, True)[0][3]
    seq = _seq(layout, aw, [NG], rng)
    if layout == "boundaries":
        seq = seq + A.tree(aw, [NG], rng)
    ids, V = _wide_ids(seq, rng, F)
    idx = A.Index(ids)
    p0 = _clip_rows(rng, V, D, c, idx, aw, NG)
    clipped = _clip_census(idx, p0, c, aw, NG)
    got, ref, dgot, dref, _, _ = _wide_case(dev, rng, ids, F, torch.bfloat16, V, defer, max_norm=c, p0=p0)
    _check_clip(got[:, :D], ref[:, :D], clipped, V, "p")
    _check_clip(got[:, D + 4:2 * D + 4], ref[:, D + 4:2 * D + 4], clipped, V, "m")
    _same(got[:, D:D + 4], ref[:, D:D + 4], "wide record")                   # FTRL is not clipped
    _same(got[:, 3 * D + 4:], ref[:, 3 * D + 4:], "padding")
    for name, a, b in zip("pmv", dgot, dref):
        _same(a, b, "dense " + name)
