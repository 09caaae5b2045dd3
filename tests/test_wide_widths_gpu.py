"""The folded wide path swept over embedding widths.  Four kernel families take the width D as a run-time geometry (lpr = D / 4 + 1
lanes per row, the extra one the wide lane; G = 64 // lpr lane-groups per wave; NG = 4 G): the fused-row lookup (mrec_gather.hip), the
wide-folded sparse apply with its finishing pass launched or deferred (mrec_apply.hip), the hot-column path of the same launch, and the
engine around them, which folds every D % 4 == 0, D <= 252.  Everything here runs at the widths of W below: the apply and the hot
columns bit for bit against the restatement of their order of additions (tests/_apply_order.py), the lookup exactly against the oracle,
max_norm at the edge widths, and the engine end to end at the widths the kernels alone cannot vouch for."""
import copy
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
from test_apply_order_gpu import (T, _aw, _cc_ids, _check_census, _check_clip, _clip_census, _clip_rows, _same, _seq, _state,  # noqa: E402
                                  _wide_case, _wide_ids)
from test_const_cols_gpu import _detect_ref  # noqa: E402
from test_max_norm_gpu import _TINY, _ULP, _rows  # noqa: E402

#    D  lpr   G   NG  fused ld   what it reaches
#    4    2  32  128     32      most lane-groups per wave, one data lane + the wide lane
#   12    4  16   64     64      D % 8 == 4: the plain gather kernel, power-of-two lpr
#   60   16   4   16    192      D % 8 == 4, lpr divides 64
#   84   22   2    8    256      3 D + 4 = 256 exactly: a fused row with no pad word after v; 20 idle lanes
#  124   32   2    8    384      lpr = 32 exactly, no idle lane
#  128   33   1    4    416      the first width with G = 1, 31 idle lanes, a row of 1664 B (13 lines)
#  172   44   1    4    544      D % 8 == 4 with G = 1
#  248   63   1    4    768      one idle lane, D % 8 == 0 (the 16-byte-store gather)
#  252   64   1    4    768      no idle lane: a 64-bit sample mask of all ones in const_part_body; 3 D + 4 = 760, gm.D = 256
# (ld = ceil((3 D + 4) / 32) * 32 floats, the engine's 128-byte padded row; the geometry is _apply_order.col_blocks(D, 4, wide=True))
W = [4, 12, 60, 84, 124, 128, 172, 248, 252]
EDGE = [12, 124, 248, 252]            # lpr - 1 = 3, 31, 62, 63 data lanes: where a wrong shuffle width in the clip's reduction shows
_GDT = (torch.float32, torch.bfloat16, torch.float16)


def _fused_ld(D):
    return -(-(3 * D + 4) // 32) * 32


def _ng(D):
    (c0, Dc, G, NG), = A.col_blocks(D, 4, True)
    assert c0 == 0 and Dc == D
    return NG


# ---- 1. the wide apply, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,layout,defer,gdt", [(D, lay, d, _GDT[(wi + li + d) % 3]) for wi, D in enumerate(W)
                                                for li, lay in enumerate(("boundaries", "tree", "oob")) for d in (False, True)])
def test_wide_apply_bitwise_at_width(dev, D, layout, defer, gdt):
    rng = np.random.default_rng(D * 31 + len(layout) * 3 + defer)
    aw, NG, F = _aw(D, 4), _ng(D), 13
    ids, V = _wide_ids(_seq(layout, aw, [NG], rng), rng, F, oob=layout == "oob")
    idx = A.Index(ids)
    c = A.census(idx, D, 4, aw, wide=True, V=V)
    assert c["blocks"][0]["NG"] == NG
    _check_census(c, layout, aw)
    got, ref, dgot, dref, _, _ = _wide_case(dev, rng, ids, F, gdt, V, defer, D=D)
    assert got.shape[1] == _fused_ld(D)
    _same(got, ref, "fused rows")
    for name, a, b in zip("pmv", dgot, dref):
        _same(a, b, "dense " + name)


# ---- 2. the hot columns -------------------------------------------------------------------------------------------------------------
_HOT_SHAPES = [(1024, 13, 0), (777, 5, 3), (65, 2, 0)]      # (B, constant columns, dominant ids); 777 and 65 end on a partial chunk of 64
_HOT = [(D, d) + _HOT_SHAPES[(wi + d) % 3] + (_GDT[(wi + d) % 3],) for wi, D in enumerate(W) if D != 252 for d in (False, True)]
_HOT += [(252, d) + s + (_GDT[(si + d) % 3],) for si, s in enumerate(_HOT_SHAPES) for d in (False, True)]


def _initial_rows(rng, V, D, p0):
    """the fused rows _wide_case starts from, given the generator in the state _wide_case received it in"""
    buf = _state(rng, V, _fused_ld(D), "adam")[0]
    buf[:, :D] = p0
    buf[:, D + 1] = 1.0 + rng.random(V).astype(np.float32)
    buf[:, 2 * D + 4:3 * D + 4] = np.abs(buf[:, 2 * D + 4:3 * D + 4]) * 1e-3
    return buf


@pytest.mark.parametrize("D,defer,B,nconst,dom,gdt", _HOT)
def test_wide_hot_columns_bitwise_at_width(dev, D, defer, B, nconst, dom, gdt):
    """constant and dominant ids through the hot-column path (const_part_body / const_finish_body), every other id through the windows"""
    V, F = 5000, 39
    want = {f: f + 7 for f in range(nconst)}
    want.update({20 + d: 30 + d for d in range(dom)})
    for salt in range(16):         # (a dominant id is planted in 40 % of a field's samples: redraw until it also leads the first 16, which
        rng = np.random.default_rng(1000 * D + B + nconst + dom + defer + 100_000 * salt)       # is where the detection looks first)
        ids = _cc_ids(rng, B, F, V, nconst, dom)
        if _detect_ref(ids, V, B // 8 if dom else B) == want:
            break
    else:
        raise AssertionError("no batch whose planted hot columns the detection rule accepts")
    p0 = (rng.standard_normal((V, D)) * 0.01).astype(np.float32)
    rng0 = copy.deepcopy(rng)
    got, ref, dgot, dref, idx, hot = _wide_case(dev, rng, ids, F, gdt, V, defer, const=B // 8 if dom else B, p0=p0, D=D)
    assert hot == want
    c = A.census(idx, D, 4, _aw(D, 4), wide=True, hot_ids=list(want.values()))
    assert c["crossing"] > 20 and c["blocks"][0]["pass_a"] > 0, c
    # a hot id whose chunk sums were dropped gets an update with a zero gradient: say so before the row-by-row comparison does
    buf0 = _initial_rows(rng0, V, D, p0)
    untouched = np.setdiff1d(np.arange(V), idx.uniq)
    assert untouched.size > 0 and np.array_equal(buf0[untouched].view(np.uint32), ref[untouched].view(np.uint32))
    zero = buf0.copy()
    hrows = np.array(sorted(want.values()), np.int32)
    A.lazy_adam(zero[:, :D], zero[:, D + 4:2 * D + 4], zero[:, 2 * D + 4:3 * D + 4], hrows, np.zeros((hrows.size, D + 1), np.float32),
                b1_pow=0.9, b2_pow=0.999, lr=3.5e-4)
    for h in hrows:
        assert (got[h, :D] != p0[h]).any(), f"hot id {h}: p unchanged"
        assert not np.array_equal(got[h, D + 4:2 * D + 4], zero[h, D + 4:2 * D + 4]), f"hot id {h}: updated with a zero gradient"
    _same(got, ref, "fused rows")
    for name, a, b in zip("pmv", dgot, dref):
        _same(a, b, "dense " + name)


# ---- 4. the wide lookup -------------------------------------------------------------------------------------------------------------
def _lookup_case(rng, dev, D, n, idt, table_p):
    """fused rows of the engine's stride holding table_p [V, D] and a wide weight; ids with -1, V, V + 3 and a duplicate-heavy tail"""
    V = table_p.shape[0]
    buf = rng.standard_normal((V, _fused_ld(D))).astype(np.float32)           # (m, v and the pad words: never looked up)
    buf[:, :D] = table_p
    buf[:, D] = rng.standard_normal(V).astype(np.float32) * 5
    ids = rng.integers(0, V, size=n).astype(np.int64)
    ids[n - n // 4:] = rng.integers(0, 5, size=n // 4)
    ids[[3, n // 2, n - 1]] = [-1, V, V + 3]
    wts = rng.random(n).astype(np.float32)
    return buf, ids, wts, T(buf, dev), T(ids.astype({torch.int32: np.int32, torch.int64: np.int64}[idt]), dev), T(wts, dev)


def _guarded_out(n, D, odt, dev):
    """[n, D] output rows with eight sentinel rows behind them"""
    big = torch.full((n + 8, D), -3.0, dtype=odt, device=dev)
    return big, big[:n]


@pytest.mark.parametrize("D,n,odt,idt", [(D, n, (torch.bfloat16, torch.float16)[(wi + ni) % 2], (torch.int32, torch.int64)[(wi // 2 + ni) % 2])
                                         for wi, D in enumerate(W) for ni, n in enumerate((4096, 4094))])
def test_wide_lookup_exact_at_width(dev, D, n, odt, idt):
    """n = 4096: the 16-byte-store kernel where D % 8 == 0, the plain one elsewhere; n = 4094: the plain one.  The lookup multiplies by
    the row scale once in fp32 and rounds once: exact equality, no tolerance to choose."""
    from mindrec_amd import ops
    rng = np.random.default_rng(D * 13 + n)
    V = 1500
    buf, ids, wts, tb, tid, twt = _lookup_case(rng, dev, D, n, idt, (rng.standard_normal((V, D)) * 0.01).astype(np.float32))
    ok = (ids >= 0) & (ids < V)
    assert (~ok).sum() == 3
    dname = "bf16" if odt == torch.bfloat16 else "f16"
    ref = O.round16(O.gather_rows(buf[:, :D], ids, wts), dname)
    refw = O.gather_rows(buf[:, D:D + 1], ids, wts)[:, 0]
    assert not ref[~ok].any() and not refw[~ok].any() and ref[ok].any(axis=1).all()
    emb, wprod = ops.gather_rows_wide(tb[:, :D], tid, twt, D, out_dtype=odt)
    assert np.array_equal(emb.float().cpu().numpy(), ref)
    assert np.array_equal(wprod[:, 0].cpu().numpy(), refw) and (wprod[:, 1] == 0).all()
    # into a caller's buffer (the wrapper takes rows D apart only): the rows behind the n-th keep their sentinel
    big, out = _guarded_out(n, D, odt, dev)
    emb2, wprod2 = ops.gather_rows_wide(tb[:, :D], tid, twt, D, out=out, out_dtype=odt)
    assert emb2.data_ptr() == big.data_ptr() and torch.equal(emb2, emb) and torch.equal(wprod2, wprod)
    assert (big[n:] == -3.0).all()
    assert torch.equal(tb.cpu(), torch.from_numpy(buf))                       # the table is only read


# The clip's acceptance rule is test_max_norm_gpu.test_gather_wide_clip's: one ulp of the output type plus 8 * 2^-24 for the fp32 norm
# and the two multiplies.  Where that figure comes from, for the widest row here (63 data lanes): the sum of squares is a product (1
# rounding), three lane-local additions and ceil(log2(63)) = 6 additions of mrec_group_sum's butterfly, 10 roundings on its longest
# path; the square root halves their relative error (5) and adds its own (1), the division c / n adds 1, the multiply by the scale 1:
# 8 roundings of 2^-24 in front of the row-scale multiply.  That multiply's own rounding (one more 2^-24) and the rounding to the
# output type (half an ulp of it) sit inside the whole ulp of the output type the rule grants.
_CLIP_FP32_ROUNDINGS = 8


@pytest.mark.parametrize("D", EDGE)
@pytest.mark.parametrize("n", [4096, 4094])
@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float16])
def test_wide_lookup_clip_at_width(dev, D, n, odt):
    """the deep columns clipped to max_norm, the wide word (column D of the same rows) not"""
    from mindrec_amd import ops
    rng = np.random.default_rng(D * 17 + n)
    V, c = 2000, 0.5
    buf, ids, wts, tb, tid, twt = _lookup_case(rng, dev, D, n, torch.int32, _rows(rng, V, D, c))
    ok = (ids >= 0) & (ids < V)
    nrm = np.linalg.norm(buf[np.where(ok, ids, 0), :D].astype(np.float64), axis=1)
    assert ((nrm > 2 * c) & ok).sum() > 100 and ((nrm < 0.9999 * c) & (nrm > 0) & ok).sum() > 100 and ((nrm == 0) & ok).sum() > 100
    emb, wprod = ops.gather_rows_wide(tb[:, :D], tid, twt, D, out_dtype=odt, max_norm=c)
    ref = OC.gather_rows(torch.from_numpy(buf[:, :D].copy()), torch.from_numpy(ids), torch.from_numpy(wts), max_norm=c).numpy()
    got = emb.float().cpu().numpy()
    err = np.abs(got - ref.astype(np.float64))
    tol = np.abs(ref) * (_ULP[odt] + _CLIP_FP32_ROUNDINGS * 2.0 ** -24) + _TINY[odt]
    print(f"D={D} n={n} {odt}: max err / tol = {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    assert not got[~ok].any()
    assert np.array_equal(wprod[:, 0].cpu().numpy(), O.gather_rows(buf[:, D:D + 1], ids, wts)[:, 0]) and (wprod[:, 1] == 0).all()
    plain, _ = ops.gather_rows_wide(tb[:, :D], tid, twt, D, out_dtype=odt)
    assert not torch.equal(plain, emb)


# ---- 5. the wide apply with max_norm at the edge widths -----------------------------------------------------------------------------
@pytest.mark.parametrize("D", EDGE)
@pytest.mark.parametrize("layout", ["boundaries", "tree"])
@pytest.mark.parametrize("defer", [False, True])
def test_wide_apply_max_norm_at_width(dev, D, layout, defer):
    rng = np.random.default_rng(D * 5 + len(layout) + defer)
    c, F = 0.09, 13
    aw, NG = _aw(D, 4), _ng(D)
    seq = _seq(layout, aw, [NG], rng)
    if layout == "boundaries":
        seq = seq + A.tree(aw, [NG], rng)
    ids, V = _wide_ids(seq, rng, F)
    idx = A.Index(ids)
    p0 = _clip_rows(rng, V, D, c, idx, aw, NG)
    clipped = _clip_census(idx, p0, c, aw, NG)
    got, ref, dgot, dref, _, _ = _wide_case(dev, rng, ids, F, torch.bfloat16, V, defer, max_norm=c, p0=p0, D=D)
    _check_clip(got[:, :D], ref[:, :D], clipped, V, "p")
    _check_clip(got[:, D + 4:2 * D + 4], ref[:, D + 4:2 * D + 4], clipped, V, "m")
    _same(got[:, D:D + 4], ref[:, D:D + 4], "wide record")                   # FTRL is not clipped
    _same(got[:, 3 * D + 4:], ref[:, 3 * D + 4:], "padding")
    for name, a, b in zip("pmv", dgot, dref):
        _same(a, b, "dense " + name)


# ---- 6. the engine ------------------------------------------------------------------------------------------------------------------
def _engine_kw(D, **kw):
    base = dict(vocab_size=6000, emb_dim=D, field_size=8, batch_size=512, deep_layer_dim=[128, 64], mlp_dtype="bf16")
    base.update(kw)
    return base


@pytest.mark.parametrize("D", [12, 124, 252])
def test_engine_fold_equals_separate_wide_kernels_at_width(dev, D):
    """fold_wide against the separate wide kernels on uniform ids, bit for bit: the claim of
    test_folded_wide_branch_equals_separate_wide_kernels at D = 80.  It holds where no run of duplicates needs pass B's tree (pass A
    adds a run's partials in order whichever the number of lane-groups); the batches are checked for that first."""
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch
    a = WideDeepEngine(WideDeepConfig(fold_wide=True, **_engine_kw(D)), dev)
    b = WideDeepEngine(WideDeepConfig(fold_wide=False, **_engine_kw(D)), dev)
    assert a._fold_wide and not b._fold_wide
    assert a.deep_state.shape[1] == _fused_ld(D)
    w0 = a.wide.clone()
    for s in range(4):
        batch = synthetic_batch(a.cfg, "cpu", "uniform", seed=90 + s)
        c = A.census(A.Index(batch[0].numpy()), D, 4, _aw(D, 4), wide=True)
        assert c["crossing"] > 20 and all(blk["pass_b"] == 0 for blk in c["blocks"]), c
        batch = tuple(t.to(dev) for t in batch)
        la, lb = float(a.train_step(*batch)), float(b.train_step(*batch))
        assert la == lb, (s, la, lb)
    assert torch.equal(a.deep, b.deep) and torch.equal(a.wide, b.wide) and torch.equal(a.wide_accum, b.wide_accum)
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach())
    assert not torch.equal(a.wide, w0)


def _criteo_batch(cfg, dev, seed):
    """13 dense fields on the constant ids 0 .. 12 (weights in [0, 1)), the other fields Zipf over their own slots: the shape of
    synthetic_batch's 39-field batches at a field count of the caller's choice"""
    rng = np.random.default_rng(seed)
    B, F, V = cfg.batch_size, cfg.field_size, cfg.vocab_size
    ncat = F - 13
    slot = (V - 13) // ncat
    ids = np.empty((B, F), np.int32)
    ids[:, :13] = np.arange(13, dtype=np.int32)
    ids[:, 13:] = np.minimum(rng.zipf(1.05, size=(B, ncat)) - 1, slot - 1) + 13 + slot * np.arange(ncat)[None, :]
    wts = np.ones((B, F), np.float32)
    wts[:, :13] = rng.random((B, 13)).astype(np.float32)
    label = (rng.random((B, 1)) < 0.25).astype(np.float32)
    return T(ids, dev), T(wts, dev), T(label, dev)


def test_engine_constant_columns_at_252(dev):
    """Criteo-shaped batches at emb_dim = 252 (63 data lanes + the wide lane: the whole wave): the hot-column path inside the replayed
    graphs against the same engine with the path off, to test_engine_takes_the_constant_columns_path's tolerances."""
    from mindrec_amd import ops
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine
    kw = _engine_kw(252, vocab_size=20000, field_size=40, batch_size=1024)
    a = WideDeepEngine(WideDeepConfig(**kw), dev)
    b = WideDeepEngine(WideDeepConfig(const_columns=False, **kw), dev)
    assert a._fold_wide and b._fold_wide
    d0 = a.deep[:13].clone()
    batches = [_criteo_batch(a.cfg, dev, 170 + s) for s in range(10)]
    la = [float(a.train_step(*x)) for x in batches[:6]] + [float(x) for x in a.train_steps(batches[6:])]
    lb = [float(b.train_step(*x)) for x in batches[:6]] + [float(x) for x in b.train_steps(batches[6:])]
    assert a._hot_seen and a._cc is not None and not b._hot_seen and getattr(b, "_cc", None) is None
    assert a._step_graph is not None and any(v for v in a._sink_graphs.values())          # (graphs replayed: the path is inside them)
    assert ops.const_cols_mask(a._cc[0]) == (1 << 13) - 1 and ops.const_cols_ids(a._cc[0]) == {f: f for f in range(13)}
    assert la[0] == lb[0]                                                                  # (the first loss: before any update)
    moved = (a.deep[:13] != d0).float().mean(dim=1)
    print("losses", la, lb, "max rel", max(abs(x - y) / abs(y) for x, y in zip(la, lb)))
    for name, x, y in (("deep", a.deep, b.deep), ("wide", a.wide, b.wide), ("dense", a.dense_flat.detach(), b.dense_flat.detach())):
        print(name, float((x - y).abs().max()) / float(y.abs().max()))
    assert (moved > 0.9).all(), moved                                                     # the constant ids' rows were trained
    assert max(abs(x - y) / abs(y) for x, y in zip(la, lb)) <= 1e-4, (la, lb)
    for x, y in ((a.deep, b.deep), (a.wide, b.wide), (a.dense_flat.detach(), b.dense_flat.detach())):
        assert float((x - y).abs().max()) <= 2e-4 * float(y.abs().max())
