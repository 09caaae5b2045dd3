"""DeepCrossEngine.predict_fused -- the evaluation forward as lookup -> the two hidden layers on the GEMMs the training step runs at
that batch size -> ops.dcn_predict (cross stack, output layer over [deep | cross], sigmoid, loss: one launch), replayed as one HIP
graph.

References: the same engine's predict() (the path this one stands beside); float64 binary_cross_entropy_with_logits of the returned
logit for the loss; the oracle-side CPU engine (tests/_clip_sums_ref.py over tests/_torch_net.py) within the bound
tests/test_engine_max_norm_gpu.py puts on predict (rtol 1e-3, atol 1e-4).

predict_fused against predict with fp32_matmul="exact": d2 and the cross stack's output c are the same bits on both paths (asserted
on the ops, called the way each path calls them), so the logits differ by the summation order of two fp32 dots of H + X terms in all
and the order and rounding of the adds behind them (predict: (d2 . W3[:H]) + (c . W3[H:] + b3); predict_fused: the order documented at
the kernel).  Per row
    |d logit| <= 2 (H + X) 2^-24 sum |x| |w|  +  4 * 2^-24 (|deep| + |cross| + |b3|)
-- twice the worst-case error of an fp32 dot in any order, plus four roundings of partial sums no larger than the three terms'
magnitudes together.  Derived, not measured; computed in float64 from the engine's own activations and weights.  prob follows through
the sigmoid's slope (at most 1/4) plus one fp32 rounding of a value below 1: |d prob| <= 0.25 bound + 2^-23.  The loss is a fp32 mean
of B terms: B * 2^-24 relative plus 2^-23 absolute against the float64 value."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

V, FIELDS = 4000, 39
NETS = [([64, 32], 16), ([64, 32], 30), ([1024, 1024], 30)]                 # (deep_layer_dim, emb_dim)
NET_IDS = ["x".join(map(str, n)) + f"-D{d}" for n, d in NETS]


def _cfg(layers, D, B=128, **over):
    from mindrec_amd.deep_cross import DeepCrossConfig
    return DeepCrossConfig(**{**dict(vocab_size=V, emb_dim=D, field_size=FIELDS, batch_size=B, deep_layer_dim=list(layers)), **over})


def _batch(dev, seed, D, B=128):
    from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch
    return synthetic_batch(WideDeepConfig(vocab_size=V, emb_dim=D, field_size=FIELDS, batch_size=B), dev, "zipf", seed=seed, signal=True)


def _trained(dev, cfg, steps=3, oracle_too=False):
    """an engine trained `steps` steps and, optionally, the oracle-side engine on the CPU trained on the same batches"""
    from mindrec_amd.deep_cross import DeepCrossEngine
    e = DeepCrossEngine(cfg, dev)
    assert e._native
    c = None
    if oracle_too:
        from _clip_sums_ref import OracleClipDeepCrossEngine
        c = OracleClipDeepCrossEngine(cfg, "cpu")
    for s in range(steps):
        ids, wts, label = _batch("cpu", 10 + s, cfg.emb_dim, cfg.batch_size)
        e.train_step(ids.to(dev), wts.to(dev), label.to(dev))
        if c is not None:
            c.train_step(ids, wts, label)
    return e, c


def _bits(t):
    return t.contiguous().view(torch.int32)


def _params(e):
    return [p.detach() for p in e.dense]


def _hidden_as_the_step(e, emb):
    """(d1, d2) from the ops called the way _step_native's forward calls them at this batch size, on buffers of the test's own"""
    from mindrec_amd import ops
    B, X = emb.shape
    h1, h2 = e.cfg.deep_layer_dim
    W1, b1, W2, b2 = _params(e)[:4]
    d1, d2 = torch.empty((B, h1), device=emb.device), torch.empty((B, h2), device=emb.device)
    if e._x3(B):
        P = {"emb": ops.x3_parts(B, X, emb.device), "W1": ops.x3_parts(X, h1, emb.device), "W2": ops.x3_parts(h1, h2, emb.device),
             "d1": ops.x3_parts(B, h1, emb.device)}
        ops.x3_split(emb, out=P["emb"])
        ops.x3_split(W1, out=P["W1"])
        ops.x3_split(W2, out=P["W2"])
        ops.x3_fwd(P["emb"], P["W1"], B, X, h1, d1, bias=b1, relu=True, parts_out=P["d1"])
        ops.x3_fwd(P["d1"], P["W2"], B, h1, h2, d2, bias=b2, relu=True)
    else:
        ops.dense32_fwd(emb, W1, b1, relu=True, out=d1)
        ops.dense32_fwd(d1, W2, b2, relu=True, out=d2)
    return d1, d2


def _fused_hidden(e, B):
    """d2 as the last predict_fused left it"""
    bf = e._bufs.get(B) or e._eval_bufs[B]
    return bf["d2"].clone()


def _logit_bound(e, d2, c):
    W3, b3 = _params(e)[4].double().view(-1), _params(e)[5].double().view(1)
    H, X = d2.shape[1], c.shape[1]
    deep, cross = d2.double() @ W3[:H], c.double() @ W3[H:]
    mag = d2.double().abs() @ W3[:H].abs() + c.double().abs() @ W3[H:].abs()
    return (2 * (H + X) * 2.0 ** -24 * mag + 4 * 2.0 ** -24 * (deep.abs() + cross.abs() + b3.abs())).view(-1, 1)


def _check_loss_and_forms(e, ids, wts, label, lf, pf, loss):
    B = ids.shape[0]
    assert tuple(lf.shape) == (B, 1) and tuple(pf.shape) == (B, 1) and loss.dim() == 0 and lf.dtype == pf.dtype == loss.dtype == torch.float32
    ref = float(torch.nn.functional.binary_cross_entropy_with_logits(lf.double(), label.double().view(B, 1)))
    print("  loss", float(loss), "float64", ref)
    assert abs(float(loss) - ref) <= B * 2.0 ** -24 * abs(ref) + 2.0 ** -23, (float(loss), ref)
    lu, pu = e.predict_fused(ids, wts)                      # the unlabelled form: the same logit and prob bits
    assert torch.equal(_bits(lu), _bits(lf)) and torch.equal(_bits(pu), _bits(pf))


def _check_against_predict(e, ids, wts, label):
    """fp32_matmul="exact": predict_fused against the same engine's predict within the derived bound.  Returns the fused logit."""
    from mindrec_amd import ops
    B = ids.shape[0]
    lp, pp = e.predict(ids, wts)
    lf, pf, loss = [t.clone() for t in e.predict_fused(ids, wts, label)]
    # d2 and c of the two paths: the same bits
    W1, b1, W2, b2, W3, b3, cw, cb = _params(e)
    emb = ops.gather_rows(e.table, ids, wts, **e._clip_kw()).view(B, -1)
    d2_p = ops.dense32_fwd(ops.dense32_fwd(emb, W1, b1, relu=True), W2, b2, relu=True)          # forward()'s calls
    assert not e._x3(B)
    d2_f = _hidden_as_the_step(e, emb)[1]
    assert torch.equal(_bits(d2_p), _bits(d2_f)) and torch.equal(_bits(d2_f), _bits(_fused_hidden(e, B))), "the hidden activations differ"
    c = ops.cross_layers(emb, cw, cb)
    # the fused launch on these very activations returns the engine's logit: c inside it is cross_layers' c
    assert torch.equal(_bits(ops.dcn_predict(emb, cw, cb, d2_f, W3.view(-1), b3)[0].view(B, 1)), _bits(lf))
    bound = _logit_bound(e, d2_f, c)
    d = (lf.double() - lp.double()).abs()
    print("  logit max |d|", float(d.max()), "smallest slack", float((bound - d).min()))
    assert bool((d <= bound).all()), (float(d.max()), float(bound.min()))
    dp = (pf.double() - pp.double()).abs()
    print("  prob max |d|", float(dp.max()))
    assert bool((dp <= 0.25 * bound + 2.0 ** -23).all()), float(dp.max())
    _check_loss_and_forms(e, ids, wts, label, lf, pf, loss)
    return lf


@pytest.mark.parametrize("layers,D", NETS, ids=NET_IDS)
def test_exact_matmul_predict_fused_matches_predict(dev, oracle, layers, D):
    e, _ = _trained(dev, _cfg(layers, D, graphs="none", fp32_matmul="exact"))
    assert e.fused_predict_supported
    ids, wts, label = _batch(dev, 99, D)
    _check_against_predict(e, ids, wts, label)
    e.close()


@pytest.mark.parametrize("layers,D", [([64, 64], 16), ([1024, 1024], 30)], ids=["64x64-D16", "1024x1024-D30"])
def test_x3_matmul_runs_the_training_forward(dev, oracle, layers, D):
    """B = 256: the step's three-part GEMMs.  Against the oracle-side engine's predict within the bound the existing tests put on
    DeepCrossEngine.predict; the hidden activations are the bits of _step_native's forward"""
    from mindrec_amd import ops
    B = 256
    e, c = _trained(dev, _cfg(layers, D, B=B, graphs="none", fp32_matmul="x3"), oracle_too=True)
    assert e._x3(B) and e.fused_predict_supported
    ids, wts, label = _batch("cpu", 99, D, B)
    gi, gw, gl = ids.to(dev), wts.to(dev), label.to(dev)
    lf, pf, loss = [t.clone() for t in e.predict_fused(gi, gw, gl)]
    lc, _ = c.predict(ids, wts)
    print("  max |d logit| against the oracle-side engine", float((lf.cpu() - lc).abs().max()))
    assert np.allclose(lf.cpu().numpy(), lc.numpy(), rtol=1e-3, atol=1e-4)
    emb = ops.gather_rows(e.table, gi, gw).view(B, -1)
    d2 = _hidden_as_the_step(e, emb)[1]
    assert torch.equal(_bits(d2), _bits(_fused_hidden(e, B))), "predict_fused's hidden layers are not the step's"
    assert not torch.equal(d2, ops.dense32_fwd(ops.dense32_fwd(emb, *_params(e)[:2]), *_params(e)[2:4]))      # (the exact GEMMs round differently)
    _check_loss_and_forms(e, gi, gw, gl, lf, pf, loss)
    e.close()


def _clip_bound(table, ids):
    """tests/test_engine_max_norm_gpu.py::_bound"""
    n = np.linalg.norm(table.astype(np.float64), axis=1)
    c = float(np.round(np.median(n[ids.reshape(-1)]), 4))
    assert np.abs(n / c - 1.0).min() > 1e-5
    return c, float((n[ids.reshape(-1)] > c).mean())


def test_predict_fused_with_max_norm(dev, oracle):
    from mindrec_amd.deep_cross import DeepCrossConfig
    D = 16
    c0, frac = _clip_bound(oracle.fill_normal(DeepCrossConfig().seed, V, D, 1.0 / float(np.sqrt(D))), _batch("cpu", 10, D)[0].numpy())
    assert 0.2 < frac < 0.8, frac
    e, c = _trained(dev, _cfg([64, 32], D, graphs="none", fp32_matmul="exact", max_norm=c0), oracle_too=True)
    ids, wts, label = _batch("cpu", 99, D)
    n = e.table[ids.long().view(-1).to(dev)].norm(dim=1)
    assert 0.2 < float((n > c0).float().mean()) < 0.8                           # after training the clip still acts on part of this batch
    lf = _check_against_predict(e, ids.to(dev), wts.to(dev), label.to(dev))
    assert np.allclose(lf.cpu().numpy(), c.predict(ids, wts)[0].numpy(), rtol=1e-3, atol=1e-4)
    plain, _ = _trained(dev, _cfg([64, 32], D, graphs="none", fp32_matmul="exact"))
    assert not torch.equal(plain.predict_fused(ids.to(dev), wts.to(dev))[0], lf)      # the clip is part of the result
    e.close()
    plain.close()


def test_graph_from_the_third_call_equals_an_eager_twin(dev):
    """calls 1-2 eager, 3 and later the graph: every call's bits are those of a twin engine that never captures, on new inputs of the
    same shape too; the outputs are static buffers; another batch shape and the unlabelled form get graphs of their own;
    release_graphs() and close() drop them"""
    D = 16
    a, _ = _trained(dev, _cfg([64, 32], D, graphs="step"))
    b, _ = _trained(dev, _cfg([64, 32], D, graphs="none"))
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach()) and torch.equal(a.table, b.table)

    def both(ids, wts, label, what):
        ra = [t.clone() for t in a.predict_fused(ids, wts, label)]
        rb = [t.clone() for t in b.predict_fused(ids, wts, label)]
        for n, x, y in zip(("logit", "prob", "loss"), ra, rb):
            assert torch.equal(_bits(x.view(-1)), _bits(y.view(-1))), (what, n)

    for s in range(5):
        ids, wts, label = _batch(dev, 200 + s, D)
        both(ids, wts, label, s)
        key = (tuple(ids.shape), ids.dtype, True)
        assert (a._predict_graphs[key]["g"] is not None) == (s >= 2), s
    assert not b._predict_graphs
    ptrs = [t.data_ptr() for t in a.predict_fused(ids, wts, label)]
    ids2, wts2, label2 = _batch(dev, 300, D)
    assert [t.data_ptr() for t in a.predict_fused(ids2, wts2, label2)] == ptrs           # static outputs: overwritten by the next call
    for s in range(4):                                                                    # another batch shape: a graph of its own
        both(ids2[:48], wts2[:48], label2[:48], ("B48", s))
    key48 = ((48, ids.shape[1]), ids.dtype, True)
    assert a._predict_graphs[key48]["g"] is not None and a._predict_graphs[key]["g"] is not None
    for s in range(3):                                                                    # ... and the unlabelled form its own
        lu, pu = a.predict_fused(ids2, wts2)
        lb, pb = b.predict_fused(ids2, wts2)
        assert torch.equal(_bits(lu), _bits(lb)) and torch.equal(_bits(pu), _bits(pb))
    assert a._predict_graphs[(tuple(ids.shape), ids.dtype, False)]["g"] is not None
    both(ids, wts, label, "back to 128")
    a.release_graphs()
    assert a._predict_graphs == {} and a._graph is None
    both(ids, wts, label, "after release_graphs")                                         # eager again, captured again on demand
    for s in range(2):
        a.predict_fused(ids, wts, label)
    assert a._predict_graphs[key]["g"] is not None
    a.close()
    assert a._predict_graphs == {}
    b.close()


def test_predict_fused_leaves_training_alone(dev):
    """after predict_fused (eager calls and graph replays) the parameters, the table, the moments, step_count and Adam's powers are
    bitwise unchanged, and the next train_steps return the loss bits of a twin engine that never evaluated"""
    D = 16
    cfg = _cfg([64, 32], D)
    a, _ = _trained(dev, cfg)
    b, _ = _trained(dev, cfg)
    assert cfg.graphs == "step" and a._graph is not None
    snap = lambda e: [e.dense_flat.detach().clone(), e.dense_m.clone(), e.dense_v.clone(), e.table.clone(), e.table_m.clone(),      # noqa: E731
                      e.table_v.clone()]
    before, steps, powers = snap(a), a.step_count, (a.beta1_power, a.beta2_power)
    for s in range(4):
        a.predict_fused(*_batch(dev, 99, D))
    assert a._predict_graphs and a.step_count == steps and (a.beta1_power, a.beta2_power) == powers
    for x, y in zip(before, snap(a)):
        assert torch.equal(x, y)
    for s in range(2):
        batch = _batch(dev, 50 + s, D)
        la, lb = a.train_step(*batch).clone(), b.train_step(*batch).clone()
        assert torch.equal(_bits(la.view(1)), _bits(lb.view(1))), (s, float(la), float(lb))
    for x, y in zip(snap(a), snap(b)):
        assert torch.equal(x, y)
    a.close()
    b.close()


def test_refusals(dev):
    from mindrec_amd.deep_cross import DeepCrossEngine
    D = 16
    ids, wts, label = _batch(dev, 1, D)
    e = DeepCrossEngine(_cfg([64, 30], D), dev)             # a last hidden width that is no multiple of 4: no hand-written output end
    assert e.fused_predict_supported is False and not e._native
    table = e.table.clone()
    with pytest.raises(ValueError, match="use predict"):
        e.predict_fused(ids, wts, label)
    with pytest.raises(ValueError, match=r"predict_fused is not supported with .*: use predict"):
        e.predict_fused(ids, wts)
    assert torch.equal(e.table, table) and e._predict_graphs == {} and e._eval_bufs == {} and e._bufs == {}
