"""WideDeepEngine.predict_fused -- the evaluation forward on the training step's kernels (the 16-bit lookup with the wide branch
folded in, the K-contiguous forward GEMMs, ops.head_predict), replayed as one HIP graph -- and WideDeepRunner(fused_eval=True).

References: the same engine's predict() (the code this path stands beside); OracleWideDeepEngine.predict on the CPU with the
tolerances the existing tests apply to predict (max |d prob| <= 2e-2 for a 16-bit net against the fp32 oracle-side engine,
test_head_any_engine_gpu.py; the fp32 net 1e-5); float64 binary_cross_entropy_with_logits of the returned logit for the loss.

predict_fused against predict: the hidden activations are the same bits (asserted on the two lookups and layer stacks), so the
logits differ by the summation order of one K5-term fp32 dot and the order of the two adds behind it:
|d| <= 2 * K5 * 2^-24 * sum_k |h_k * w5_k| + 4 * 2^-24 * |logit| per row -- twice the worst-case error of an fp32 dot in any order,
plus the roundings of the adds.  Derived, not measured; computed from the engine's own last activation and W5."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KW = dict(vocab_size=20_000, emb_dim=16, field_size=26, batch_size=256)
NETS = [([64, 512], "fp16"), ([64, 512], "bf16"), ([48, 24], "fp16"), ([48, 24], "bf16"), ([64, 1024], "fp16"), ([64, 1024], "bf16"),
        ([64, 32], "fp32"), ([1024, 512, 256, 128], "fp16")]
NET_IDS = ["x".join(map(str, n)) + "-" + d for n, d in NETS]


def _cfg(layers, dt, **over):
    from mindrec_amd.wide_deep import WideDeepConfig
    return WideDeepConfig(**{**KW, "deep_layer_dim": layers, "mlp_dtype": dt, **over})


def _trained(dev, cfg, steps=3, oracle_too=False, kind="zipf"):
    """an engine trained `steps` steps (weights and 16-bit shadows have moved) and, optionally, the oracle-side fp32 engine on the CPU
    trained on the same batches"""
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch
    e = WideDeepEngine(cfg, dev)
    c = None
    if oracle_too:
        from _oracle_engine import OracleWideDeepEngine
        c = OracleWideDeepEngine(WideDeepConfig(**{**cfg.__dict__, "mlp_dtype": "fp32"}), "cpu")
    for s in range(steps):
        ids, wts, label = synthetic_batch(cfg, "cpu", kind, seed=10 + s, signal=True)
        e.train_step(ids.to(dev), wts.to(dev), label.to(dev))
        if c is not None:
            c.train_step(ids, wts, label)
    return e, c


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _stacks(e, ids, wts):
    """the last hidden activation as predict() computes it and as predict_fused() does: (h_predict, h_fused), from the two lookups
    and the two layer stacks called the way each path calls them"""
    from mindrec_amd import ops
    n = len(e.dims) - 1
    with torch.no_grad():
        if e.index is not None:
            ids, _ = e._translate_keys(ids)
        emb_p, _, _ = e.lookup(ids, wts)                      # predict's lookup: grad mode off
        if e._mfma:
            assert emb_p.dtype == torch.float32
            h_p = emb_p.to(e._amp)
            emb_f = e._lookup_folded(ids, wts)[0] if e._fold_wide else e._lookup_rows(ids, wts, out_dtype=e._amp)
            assert emb_f.dtype == e._amp and torch.equal(_bits(h_p), _bits(emb_f)), "the 16-bit lookup differs from the cast fp32 lookup"
            h_f = emb_f
            for i in range(n - 1):
                h_p = ops.dense_fwd(h_p, e.dense16[2 * i], e.dense[2 * i + 1].detach(), relu=True)
                h_f = ops.dense_fwd(h_f, e.dense16[2 * i], e.dense[2 * i + 1].detach(), relu=True, wt=e._dense16_t.get(i))
        else:
            h_p = h_f = emb_p.contiguous()
            for i in range(n - 1):
                h_p = ops.dense32_fwd(h_p, e.dense[2 * i].detach(), e.dense[2 * i + 1].detach(), relu=True)
            h_f = h_p
    assert torch.equal(_bits(h_p), _bits(h_f)), "the hidden activations of the two paths differ"
    return h_p, h_f


def _logit_bound(e, h, logit_ref):
    n = len(e.dims) - 1
    K5 = e.dims[n - 1]
    hw = h.double().abs() @ e.dense[2 * (n - 1)].detach().double().abs().view(-1, 1)
    return 2 * K5 * 2.0 ** -24 * hw + 4 * 2.0 ** -24 * logit_ref.double().abs()


def _check_against_predict(e, ids, wts, label):
    """predict_fused against the same engine's predict within the derived bound; the loss against float64 BCE of the returned logit.
    Returns (logit, prob) of predict_fused as clones."""
    lp, pp = e.predict(ids, wts)
    out = [t.clone() for t in e.predict_fused(ids, wts, label)]
    lf, pf, loss = out
    B = ids.shape[0]
    assert tuple(lf.shape) == (B, 1) and tuple(pf.shape) == (B, 1) and loss.dim() == 0 and lf.dtype == pf.dtype == torch.float32
    h_p, _ = _stacks(e, ids, wts)
    bound = _logit_bound(e, h_p, lp)
    d = (lf.double() - lp.double()).abs()
    print("  logit max |d|", float(d.max()), "smallest slack", float((bound - d).min()))
    assert bool((d <= bound).all()), (float(d.max()), float(bound.min()))
    assert np.allclose(pf.cpu().numpy(), torch.sigmoid(lf.double()).cpu().numpy(), rtol=1e-4, atol=1e-7)
    ref = float(torch.nn.functional.binary_cross_entropy_with_logits(lf.double(), label.double().view(B, 1)))
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (float(loss), ref)
    lu, pu = e.predict_fused(ids, wts)                      # the unlabelled form: the same logit and prob bits
    assert torch.equal(_bits(lu), _bits(lf)) and torch.equal(_bits(pu), _bits(pf))
    return lf, pf


@pytest.mark.parametrize("layers,dt", NETS, ids=NET_IDS)
def test_predict_fused_matches_predict_and_the_oracle_engine(dev, oracle, layers, dt):
    from mindrec_amd.wide_deep import synthetic_batch
    cfg = _cfg(layers, dt, graphs="none")
    e, c = _trained(dev, cfg, oracle_too=True)
    assert e.fused_predict_supported and (e._mfma or e._f32net) and (e._fold_wide == (dt != "fp32"))
    ids, wts, label = synthetic_batch(cfg, "cpu", "zipf", seed=99, signal=True)
    lf, pf = _check_against_predict(e, ids.to(dev), wts.to(dev), label.to(dev))
    pc = c.predict(ids, wts)[1].numpy()
    dmax = float(np.abs(pf.cpu().numpy() - pc).max())
    print("  max |d prob| against the oracle-side engine", dmax)
    assert dmax <= (1e-5 if dt == "fp32" else 2e-2), dmax


def test_predict_fused_without_the_folded_wide_branch(dev):
    """fold_wide=False: the 16-bit row lookup + wide_sum, the wide branch per sample into the head"""
    from mindrec_amd.wide_deep import synthetic_batch
    cfg = _cfg([64, 1024], "bf16", fold_wide=False, graphs="none")
    e, _ = _trained(dev, cfg)
    assert e._mfma and not e._fold_wide
    _check_against_predict(e, *synthetic_batch(cfg, dev, "zipf", seed=99, signal=True))


def test_predict_fused_with_max_norm(dev):
    from mindrec_amd.wide_deep import synthetic_batch
    cfg = _cfg([64, 1024], "fp16", max_norm=0.03, graphs="none")
    e, _ = _trained(dev, cfg)
    ids, wts, label = synthetic_batch(cfg, dev, "zipf", seed=99, signal=True)
    assert float(e.deep[ids.long().view(-1)].norm(dim=1).max()) > 0.03          # the clip acts on this batch
    _check_against_predict(e, ids, wts, label)


@pytest.mark.parametrize("dropout", [False, True])
def test_predict_fused_leaves_the_training_state_alone(dev, dropout):
    """after predict_fused (eager calls and graph replays): step_count, the dense parameters, the tables and the optimizer moments are
    bitwise unchanged and the next train_step gives the loss bits of a twin engine that never evaluated; with Dropout on, the mask
    stream has not moved and evaluation applies no mask (its result does not depend on the engine's training flag)"""
    from mindrec_amd.wide_deep import synthetic_batch
    cfg = _cfg([64, 512], "bf16", dropout_flag=dropout)
    a, _ = _trained(dev, cfg)
    b, _ = _trained(dev, cfg)
    assert a._dropout == dropout
    snap = lambda e: [e.dense_flat.detach().clone(), e.dense_m.clone(), e.dense_v.clone(), e.deep_state.clone(), e.dense16_flat.clone()]      # noqa: E731
    before, steps = snap(a), a.step_count
    outs = []
    for s in range(4):
        ids, wts, label = synthetic_batch(cfg, dev, "zipf", seed=99, signal=True)
        a._training = bool(s % 2)                   # whatever _training says, evaluation draws no mask
        try:
            outs.append([t.clone() for t in a.predict_fused(ids, wts, label)])
        finally:
            a._training = False
    for o in outs[1:]:
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(outs[0], o))
    assert a.step_count == steps and not a._emb_dropped
    for x, y in zip(before, snap(a)):
        assert torch.equal(x, y)
    for s in range(2):
        batch = synthetic_batch(cfg, dev, "zipf", seed=50 + s, signal=True)
        la, lb = a.train_step(*batch).clone(), b.train_step(*batch).clone()
        assert torch.equal(_bits(la.view(1)), _bits(lb.view(1))), (s, float(la), float(lb))
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach()) and torch.equal(a.deep_state, b.deep_state)


def test_predict_fused_graph_replays_equal_eager(dev):
    """calls 1-2 (eager) and 3-5 (replayed, other batches) are the bits of an engine that never captures; close() drops the graph; another
    batch size captures its own graph"""
    from mindrec_amd.wide_deep import synthetic_batch
    a, _ = _trained(dev, _cfg([64, 1024], "fp16", graphs="step"))
    b, _ = _trained(dev, _cfg([64, 1024], "fp16", graphs="none"))
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach())

    def both(ids, wts, label, what):
        ra = [t.clone() for t in a.predict_fused(ids, wts, label)]
        rb = [t.clone() for t in b.predict_fused(ids, wts, label)]
        for n, x, y in zip(("logit", "prob", "loss"), ra, rb):
            assert torch.equal(_bits(x.view(-1)), _bits(y.view(-1))), (what, n)

    key = None
    for s in range(5):
        ids, wts, label = synthetic_batch(a.cfg, dev, "zipf", seed=200 + s, signal=True)
        both(ids, wts, label, s)
        key = (tuple(ids.shape), ids.dtype, True)
        assert (a._predict_graphs[key]["g"] is not None) == (s >= 2), s
    assert not b._predict_graphs
    static = a.predict_fused(ids, wts, label)
    ptrs = [t.data_ptr() for t in static]
    ids2, wts2, label2 = synthetic_batch(a.cfg, dev, "zipf", seed=300, signal=True)
    assert [t.data_ptr() for t in a.predict_fused(ids2, wts2, label2)] == ptrs           # static outputs: overwritten by the next call
    # another batch size: two eager calls, then a graph of its own beside the first
    for s in range(4):
        both(ids2[:128], wts2[:128], label2[:128], ("B128", s))
    key128 = ((128, ids.shape[1]), ids.dtype, True)
    assert a._predict_graphs[key128]["g"] is not None and a._predict_graphs[key]["g"] is not None
    both(ids, wts, label, "back to 256")
    a.close()
    assert a._predict_graphs == {}
    both(ids, wts, label, "after close")                                                  # eager again, captured again on demand
    a.close()
    b.close()


def test_predict_fused_hash_tables_run_eagerly(dev):
    """dynamic_embedding=True: keys translated as predict does (unseen keys read default rows), never captured"""
    from mindrec_amd.wide_deep import synthetic_batch
    cfg = _cfg([64, 1024], "bf16", dynamic_embedding=True, hash_capacity=1 << 16, graphs="step")
    e, _ = _trained(dev, cfg)
    assert e.index is not None and e.fused_predict_supported
    ids, wts, label = synthetic_batch(cfg, dev, "uniform", seed=99, signal=True)          # uniform ids: almost all unseen in training
    for _ in range(4):
        _check_against_predict(e, ids, wts, label)
    assert not e._predict_graphs
    e.close()


def test_predict_fused_refusals(dev):
    from mindrec_amd.wide_deep import WideDeepEngine, synthetic_batch
    from mindrec_amd.wide_deep_mlp import UnsupportedNet
    cfg = _cfg([64, 512], "bf16", host_cache_rows=8192)
    e = WideDeepEngine(cfg, dev)
    assert e.fused_predict_supported is False
    ids, wts, label = synthetic_batch(cfg, dev, "zipf", seed=1)
    with pytest.raises(ValueError, match="host cache"):
        e.predict_fused(ids, wts, label)
    cfg = _cfg([60, 30], "bf16")                     # widths that are no multiple of 8: no hand-written net
    e = WideDeepEngine(cfg, dev)
    assert e.fused_predict_supported and not e._mfma
    with pytest.raises(UnsupportedNet, match="MREC_EUNSUPPORTED"):
        e.predict_fused(ids, wts)
    with pytest.raises(UnsupportedNet, match="MREC_EUNSUPPORTED"):
        e.predict_fused(ids, wts, label)


def test_runner_fused_eval(dev):
    """WideDeepRunner(fused_eval=True).eval over 4 batches of the planted-signal stream: the AUC of the fused_eval=False runner within
    the difference test_auc_parity_on_planted_signal allows, and the float64 log-loss of the concatenated logits"""
    from mindrec_amd.metrics import DeviceAUCMetric
    from mindrec_amd.wide_deep import synthetic_batch
    from mindrec_amd.wide_deep_run import WideDeepRunner
    cfg = _cfg([64, 1024], "fp16")
    e, _ = _trained(dev, cfg, steps=6, kind="uniform")
    data = [synthetic_batch(cfg, dev, "uniform", seed=900 + s, signal=True) for s in range(4)]
    plain = WideDeepRunner(e, {"auc": DeviceAUCMetric()}).eval(data)
    fused = WideDeepRunner(e, {"auc": DeviceAUCMetric()}, fused_eval=True).eval(data)
    assert "logloss" not in plain and set(fused) == {"auc", "logloss"}
    print("  auc", plain["auc"], fused["auc"], "logloss", fused["logloss"])
    assert abs(plain["auc"] - fused["auc"]) <= 2e-3
    logits = torch.cat([e.predict_fused(i, w)[0].clone() for i, w, _ in data]).double()
    labels = torch.cat([y for _, _, y in data]).double().view(-1, 1)
    ref = float(torch.nn.functional.binary_cross_entropy_with_logits(logits, labels))
    assert abs(fused["logloss"] - ref) <= 1e-5 * abs(ref), (fused["logloss"], ref)
    e.close()
