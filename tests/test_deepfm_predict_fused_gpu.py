"""DeepFMEngine.predict_fused / DeepFMHashEngine.predict_fused -- the evaluation forward as ops.fm_lookup (the masked rows in the net's
dtype, the linear term and the FM term: one launch) -> DenseNetMixin.mlp_predict, on DeepFMEngine replayed as one HIP graph.

References: the same engine's predict() (the path this one stands beside); float64 binary_cross_entropy_with_logits of the returned
logit for the loss; for the fp32 net the oracle-side CPU engine (tests/_clip_sums_ref.py over tests/_torch_net.py) within the bound
tests/test_engine_max_norm_gpu.py puts on predict (rtol 1e-3, atol 1e-4).

predict_fused against predict: the last hidden activations are the same bits (asserted on the two lookups and the two layer stacks,
called the way each path calls them), so the logits differ by the summation order of one K5-term fp32 dot and the order and rounding
of the adds behind it (predict: (linear + fm) + (h . w5 + b5); predict_fused: lin_fm, the dot and b5 added inside the head).  Per row
    |d logit| <= 2 * K5 * 2^-24 * sum_k |h_k * w5_k|  +  4 * 2^-24 * (|deep| + |lin_fm| + |b5|)
-- twice the worst-case error of an fp32 dot in any order, plus four roundings of partial sums no larger than the three terms'
magnitudes together.  Derived, not measured; computed in float64 from the engine's own last activation and weights.  prob follows
through the sigmoid's slope (at most 1/4) plus one fp32 rounding of a value below 1: |d prob| <= 0.25 * bound + 2^-23.
The loss is a fp32 mean of B terms: B * 2^-24 relative plus 2^-23 absolute against the float64 value."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KW = dict(data_vocab_size=4000, data_emb_dim=16, data_field_size=39, batch_size=128)
NETS = [([64, 32], "fp16"), ([64, 32], "bf16"), ([64, 32], "fp32"), ([1024, 512, 256, 128], "fp16")]
NET_IDS = ["x".join(map(str, n)) + "-" + d for n, d in NETS]


def _cfg(layers, dt, **over):
    from mindrec_amd.deepfm import DeepFMConfig
    return DeepFMConfig(**{**KW, "deep_layer_dims": list(layers), "mlp_dtype": dt, **over})


def _batch(dev, seed, B=128):
    from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch
    bcfg = WideDeepConfig(vocab_size=KW["data_vocab_size"], emb_dim=KW["data_emb_dim"], field_size=KW["data_field_size"], batch_size=B)
    return synthetic_batch(bcfg, dev, "zipf", seed=seed, signal=True)


def _trained(dev, cfg, steps=3, oracle_too=False):
    """an engine trained `steps` steps (the weights and the 16-bit shadows have moved) and, optionally, the oracle-side engine on the
    CPU trained on the same batches"""
    from mindrec_amd.deepfm import DeepFMEngine
    e = DeepFMEngine(cfg, dev)
    c = None
    if oracle_too:
        from _clip_sums_ref import OracleClipDeepFMEngine
        c = OracleClipDeepFMEngine(cfg, "cpu")
    for s in range(steps):
        ids, wts, label = _batch("cpu", 10 + s)
        e.train_step(ids.to(dev), wts.to(dev), label.to(dev))
        if c is not None:
            c.train_step(ids, wts, label)
    return e, c


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _stacks(e, V, W, ids_v, ids_w, wts):
    """(the last hidden activation, lin_fm of the fused lookup): the activation as predict() computes it and as predict_fused() does, from
    the two lookups and the two layer stacks called the way each path calls them -- asserted to be the same bits"""
    from mindrec_amd import ops
    n = len(e.dims) - 1
    B = ids_v.shape[0]
    with torch.no_grad():
        vx = ops.gather_rows(V, ids_v, wts, **e._clip_kw()).view(B, -1)              # predict's lookup
        rows, lin_fm = ops.fm_lookup(V, W, ids_v, wts, ids_w=ids_w, out_dtype=e._amp if e._mfma else torch.float32, **e._clip_kw())
        rows = rows.view(B, -1)
        if e._mfma:
            h_p = vx.to(e._amp)                                                       # mlp()'s cast
            assert rows.dtype == e._amp and torch.equal(_bits(h_p), _bits(rows)), "the 16-bit lookup differs from the cast fp32 lookup"
            h_f = rows
            for i in range(n - 1):
                h_p = ops.dense_fwd(h_p, e.dense16[2 * i], e.dense[2 * i + 1].detach(), relu=True)
                h_f = ops.dense_fwd(h_f, e.dense16[2 * i], e.dense[2 * i + 1].detach(), relu=True, wt=e._dense16_t.get(i))
        else:
            assert e._f32net and rows.dtype == torch.float32 and torch.equal(_bits(vx), _bits(rows)), "the fp32 lookups differ"
            h_p = vx.contiguous()
            for i in range(n - 1):
                h_p = ops.dense32_fwd(h_p, e.dense[2 * i].detach(), e.dense[2 * i + 1].detach(), relu=True)
            h_f = h_p
    assert torch.equal(_bits(h_p), _bits(h_f)), "the hidden activations of the two paths differ"
    return h_p, lin_fm


def _logit_bound(e, h, lin_fm):
    n = len(e.dims) - 1
    K5 = e.dims[n - 1]
    w5, b5 = e.dense[2 * (n - 1)].detach().double().view(-1, 1), e.dense[2 * (n - 1) + 1].detach().double().view(1, 1)
    hw = h.double().abs() @ w5.abs()
    deep = h.double() @ w5
    return 2 * K5 * 2.0 ** -24 * hw + 4 * 2.0 ** -24 * (deep.abs() + lin_fm.double().view(-1, 1).abs() + b5.abs())


def _check_against_predict(e, ids, wts, label, tables=None):
    """predict_fused against the same engine's predict within the derived bound; the loss against float64 BCE of the returned logit.
    tables: (V, W, ids_v, ids_w) of the lookups (default: the dense engine's).  Returns (logit, prob) of predict_fused as clones."""
    lp, pp = e.predict(ids, wts)
    lf, pf, loss = [t.clone() for t in e.predict_fused(ids, wts, label)]
    B = ids.shape[0]
    assert tuple(lf.shape) == (B, 1) and tuple(pf.shape) == (B, 1) and loss.dim() == 0 and lf.dtype == pf.dtype == loss.dtype == torch.float32
    V, W, ids_v, ids_w = tables if tables is not None else (e.V_l2, e.W_l2, ids, None)
    h, lin_fm = _stacks(e, V, W, ids_v, ids_w, wts)
    bound = _logit_bound(e, h, lin_fm)
    d = (lf.double() - lp.double()).abs()
    print("  logit max |d|", float(d.max()), "smallest slack", float((bound - d).min()))
    assert bool((d <= bound).all()), (float(d.max()), float(bound.min()))
    dp = (pf.double() - pp.double()).abs()
    print("  prob max |d|", float(dp.max()))
    assert bool((dp <= 0.25 * bound + 2.0 ** -23).all()), float(dp.max())
    ref = float(torch.nn.functional.binary_cross_entropy_with_logits(lf.double(), label.double().view(B, 1)))
    print("  loss", float(loss), "float64", ref)
    assert abs(float(loss) - ref) <= B * 2.0 ** -24 * abs(ref) + 2.0 ** -23, (float(loss), ref)
    lu, pu = e.predict_fused(ids, wts)                      # the unlabelled form: the same logit and prob bits
    assert torch.equal(_bits(lu), _bits(lf)) and torch.equal(_bits(pu), _bits(pf))
    return lf, pf


@pytest.mark.parametrize("layers,dt", NETS, ids=NET_IDS)
def test_predict_fused_matches_predict(dev, oracle, layers, dt):
    cfg = _cfg(layers, dt, graphs="none")
    e, c = _trained(dev, cfg, oracle_too=(dt == "fp32"))
    assert e.fused_predict_supported and (e._mfma if dt != "fp32" else e._f32net)
    ids, wts, label = _batch("cpu", 99)
    lf, pf = _check_against_predict(e, ids.to(dev), wts.to(dev), label.to(dev))
    if c is not None:                                       # the fp32 net: the oracle-side engine's predict, the existing bound on predict
        lc, _ = c.predict(ids, wts)
        print("  max |d logit| against the oracle-side engine", float((lf.cpu() - lc).abs().max()))
        assert np.allclose(lf.cpu().numpy(), lc.numpy(), rtol=1e-3, atol=1e-4)
    e.close()


def _clip_bound(table, ids):
    """tests/test_engine_max_norm_gpu.py::_bound"""
    n = np.linalg.norm(table.astype(np.float64), axis=1)
    c = float(np.round(np.median(n[ids.reshape(-1)]), 4))
    assert np.abs(n / c - 1.0).min() > 1e-5
    return c, float((n[ids.reshape(-1)] > c).mean())


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_predict_fused_with_max_norm(dev, oracle, dt):
    from mindrec_amd.deepfm import DeepFMConfig
    c0, frac = _clip_bound(oracle.fill_normal(DeepFMConfig().seed, KW["data_vocab_size"], KW["data_emb_dim"], 0.01), _batch("cpu", 10)[0].numpy())
    assert 0.2 < frac < 0.8, frac
    e, c = _trained(dev, _cfg([64, 32], dt, graphs="none", max_norm=c0), oracle_too=(dt == "fp32"))
    ids, wts, label = _batch("cpu", 99)
    n = e.V_l2[ids.long().view(-1).to(dev)].norm(dim=1)
    assert 0.05 < float((n > c0).float().mean()) < 0.95                         # after training the clip still acts on part of this batch
    lf, _ = _check_against_predict(e, ids.to(dev), wts.to(dev), label.to(dev))
    if c is not None:
        assert np.allclose(lf.cpu().numpy(), c.predict(ids, wts)[0].numpy(), rtol=1e-3, atol=1e-4)
    plain, _ = _trained(dev, _cfg([64, 32], dt, graphs="none"))
    assert not torch.equal(plain.predict_fused(ids.to(dev), wts.to(dev))[0], lf)      # the clip is part of the result


def test_graph_from_the_third_call_equals_an_eager_twin(dev):
    """calls 1-2 eager, 3 and later the graph: every call's bits are those of a twin engine that never captures, call 4 on new inputs
    of the same shape included; the outputs are static buffers; another batch shape gets a graph of its own; close() drops them"""
    a, _ = _trained(dev, _cfg([64, 32], "fp16", graphs="mlp"))
    b, _ = _trained(dev, _cfg([64, 32], "fp16", graphs="none"))
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach()) and torch.equal(a.V_l2, b.V_l2)

    def both(ids, wts, label, what):
        ra = [t.clone() for t in a.predict_fused(ids, wts, label)]
        rb = [t.clone() for t in b.predict_fused(ids, wts, label)]
        for n, x, y in zip(("logit", "prob", "loss"), ra, rb):
            assert torch.equal(_bits(x.view(-1)), _bits(y.view(-1))), (what, n)

    for s in range(5):
        ids, wts, label = _batch(dev, 200 + s)
        both(ids, wts, label, s)
        key = (tuple(ids.shape), ids.dtype, True)
        assert (a._predict_graphs[key]["g"] is not None) == (s >= 2), s
    assert not b._predict_graphs
    ptrs = [t.data_ptr() for t in a.predict_fused(ids, wts, label)]
    ids2, wts2, label2 = _batch(dev, 300)
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
    assert a._predict_graphs == {}
    both(ids, wts, label, "after release_graphs")                                         # eager again, captured again on demand
    a.close()
    assert a._predict_graphs == {}
    b.close()


def test_predict_fused_leaves_training_alone(dev):
    """after predict_fused (eager calls and graph replays) the parameters, tables and optimizer state are bitwise unchanged, and the
    next train_steps return the loss bits of a twin engine that never evaluated"""
    cfg = _cfg([64, 32], "fp16")
    a, _ = _trained(dev, cfg)
    b, _ = _trained(dev, cfg)
    snap = lambda e: [e.dense_flat.detach().clone(), e.dense_m.clone(), e.dense_v.clone(), e.dense16_flat.clone(), e.V_l2.clone(),      # noqa: E731
                      e.W_l2.clone()] + [t.clone() for pair in e.state.values() for t in pair]
    before, steps, powers = snap(a), a.step_count, (a.beta1_power, a.beta2_power)
    for s in range(4):
        a.predict_fused(*_batch(dev, 99))
    assert a.step_count == steps and (a.beta1_power, a.beta2_power) == powers
    for x, y in zip(before, snap(a)):
        assert torch.equal(x, y)
    for s in range(2):
        batch = _batch(dev, 50 + s)
        la, lb = a.train_step(*batch).clone(), b.train_step(*batch).clone()
        assert torch.equal(_bits(la.view(1)), _bits(lb.view(1))), (s, float(la), float(lb))
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach()) and torch.equal(a.V_l2, b.V_l2)
    a.close()
    b.close()


def _hash_engine(dev, dt="fp16", **kw):
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMHashEngine
    cfg = DeepFMConfig(data_emb_dim=16, data_field_size=39, batch_size=48, deep_layer_dims=[64, 32], learning_rate=1e-2, mlp_dtype=dt)
    return DeepFMHashEngine(cfg, dev, key_dtype=torch.int64, capacity=1 << 12, **kw)


def _keys(seed, B=48, F=39, pool=600):
    """keys drawn from the first `pool` of 600 fixed int64 keys"""
    g = torch.Generator().manual_seed(seed)
    pool_keys = torch.randint(1, 2 ** 40, (600,), generator=torch.Generator().manual_seed(5))
    keys = pool_keys[torch.randint(0, pool, (B, F), generator=g)]
    wts = torch.rand((B, F), generator=g)
    label = (torch.rand((B, 1), generator=g) < 0.3).float()
    return keys, wts, label


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_hash_engine_predict_fused(dev, dt):
    """int64 keys, capacity 1 << 12, B 48: predict_fused against predict within the derived bound; keys first seen in evaluation are
    inserted exactly as predict inserts them (twin engines: the same key count, the same rows); never a graph"""
    a, b = _hash_engine(dev, dt), _hash_engine(dev, dt)
    for s in range(3):
        keys, wts, label = (t.to(dev) for t in _keys(20 + s, pool=300))                  # training sees the first 300 keys of the pool only
        a.train_step(keys, wts, label)
        b.train_step(keys, wts, label)
    assert a.fused_predict_supported and len(a.V) == len(b.V)
    seen = len(a.V)
    keys, wts, label = (t.to(dev) for t in _keys(99))
    a.predict_fused(keys, wts, label)                                                    # a: first sees the new keys in predict_fused,
    b.predict(keys, wts)                                                                 # b: in predict
    assert len(a.V) == len(b.V) > seen and len(a.W) == len(b.W) == len(a.V)
    n = len(a.V)
    assert torch.equal(a.V.values[:n], b.V.values[:n]) and torch.equal(a.W.values[:n], b.W.values[:n])
    assert torch.equal(a.V.get_keys().sort().values, b.V.get_keys().sort().values)
    B, Fd = keys.shape
    _, _, pos_v, _, pos_w = a._lookup(keys, insert=True)
    assert len(a.V) == n                                                                 # (resident by now: nothing more is inserted)
    _check_against_predict(a, keys, wts, label, tables=(a.V.values, a.W.values, pos_v.view(B, Fd), pos_w.view(B, Fd)))
    for _ in range(3):
        a.predict_fused(keys, wts, label)
    assert not hasattr(a, "_predict_graphs") or not a._predict_graphs
    la, lb = a.train_step(keys, wts, label), b.train_step(keys, wts, label)              # evaluation left the training state alone
    assert torch.equal(_bits(la.view(1)), _bits(lb.view(1)))


def test_refusals(dev):
    from mindrec_amd.deepfm import DeepFMEngine
    ids, wts, label = _batch(dev, 1)
    e = _hash_engine(dev)
    e.world = 2                                             # key shards, without a process group: refused before anything is touched
    assert e.fused_predict_supported is False
    with pytest.raises(ValueError, match=r"key shards \(world > 1\).*use predict"):
        e.predict_fused(ids.long(), wts, label)
    assert len(e.V) == 0
    e = DeepFMEngine(_cfg([60, 30], "fp16"), dev)           # widths that are no multiple of 8: no hand-written net
    assert e.fused_predict_supported is False and not e._mfma
    with pytest.raises(ValueError, match="dense net.*use predict"):
        e.predict_fused(ids, wts)
    e = DeepFMEngine(_cfg([64, 32], "fp16", data_emb_dim=18), dev)      # rows that are no multiple of 4 floats
    assert e.fused_predict_supported is False
    with pytest.raises(ValueError, match="data_emb_dim.*use predict"):
        e.predict_fused(ids, wts, label)
    e = DeepFMEngine(_cfg([64, 36], "fp32"), dev)           # fp32 net, last hidden width 36: the evaluation head takes multiples of 8
    assert e.fused_predict_supported is False
    with pytest.raises(ValueError, match="use predict"):
        e.predict_fused(ids, wts)
