"""predict_fused through ops.tail_predict (fused_tail_eval=True: the last two hidden layers and the output head as one launch)
against the twin engine that runs those three launches (fused_tail_eval=False): the same parameters, the same lookup, the same first
hidden layer, so logit and prob must be IDENTICAL; the loss is the same B terms added over other partial groupings and agrees within
2e-6 relative (the tolerance tests/test_tail_gpu.py allows between the two groupings of this sum).  Whole tiles (B = 256) and a ragged
last tile (B = 200), with a label and without, eager and replayed from the captured graph, WideDeepEngine and DeepFMEngine; the
training state is not touched, and nets or switches without the tail never reach the op."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KW = dict(vocab_size=20_000, emb_dim=16, field_size=26, batch_size=256)
TAIL_NET = [64, 512, 256, 128]
SIZES = (256, 200)


def _cfg(dt, layers=TAIL_NET, **over):
    from mindrec_amd.wide_deep import WideDeepConfig
    return WideDeepConfig(**{**KW, "deep_layer_dim": list(layers), "mlp_dtype": dt, **over})


def _trained(dev, cfg, steps=3):
    """tests/test_predict_fused_gpu.py::_trained: an engine trained `steps` steps (weights and 16-bit shadows have moved)"""
    from mindrec_amd.wide_deep import WideDeepEngine, synthetic_batch
    e = WideDeepEngine(cfg, dev)
    for s in range(steps):
        ids, wts, label = synthetic_batch(cfg, "cpu", "zipf", seed=10 + s, signal=True)
        e.train_step(ids.to(dev), wts.to(dev), label.to(dev))
    return e


def _batch(cfg, dev, seed, B):
    from mindrec_amd.wide_deep import synthetic_batch
    ids, wts, label = synthetic_batch(cfg, dev, "zipf", seed=seed, signal=True)
    return ids[:B].contiguous(), wts[:B].contiguous(), label[:B].contiguous()


def _bits(t):
    return t.contiguous().view(-1).view(torch.int16 if t.element_size() == 2 else torch.int32)


class _Counted:
    """ops.tail_predict behind a counting wrapper; restores the op on exit"""

    def __enter__(self):
        from mindrec_amd import ops
        self.ops, self.real, self.calls = ops, ops.tail_predict, 0

        def counted(*a, **kw):
            self.calls += 1
            return self.real(*a, **kw)
        ops.tail_predict = counted
        return self

    def __exit__(self, *exc):
        self.ops.tail_predict = self.real
        return False


def _same(ra, rb, what, loss_rel=2e-6):
    assert torch.equal(_bits(ra[0]), _bits(rb[0])), (what, "logit", int((_bits(ra[0]) != _bits(rb[0])).sum()))
    assert torch.equal(_bits(ra[1]), _bits(rb[1])), (what, "prob", int((_bits(ra[1]) != _bits(rb[1])).sum()))
    if len(ra) == 3:
        la, lb = float(ra[2]), float(rb[2])
        print(f"  {what}: loss {la!r} twin {lb!r}")
        assert abs(la - lb) <= loss_rel * abs(lb), (what, la, lb)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_predict_fused_equals_the_twin_without_the_fused_eval_tail(dev, dt):
    a = _trained(dev, _cfg(dt, graphs="none", fused_tail_eval=True))
    b = _trained(dev, _cfg(dt, graphs="none", fused_tail_eval=False))
    assert a._tail_ok and b._tail_ok and a._tail_eval and not b._tail_eval
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach()) and torch.equal(a.deep_state, b.deep_state)
    with _Counted() as c:
        for B in SIZES:
            ids, wts, label = _batch(a.cfg, dev, 99, B)
            for lab in (label, None):
                n0 = c.calls
                ra = [t.clone() for t in a.predict_fused(ids, wts, lab)]
                assert c.calls == n0 + 1, "one ops.tail_predict call per eager predict_fused"
                rb = [t.clone() for t in b.predict_fused(ids, wts, lab)]
                assert c.calls == n0 + 1, "the twin never calls ops.tail_predict"
                assert len(ra) == len(rb) == (3 if lab is not None else 2) and tuple(ra[0].shape) == (B, 1)
                _same(ra, rb, (dt, B, lab is not None))
    a.close()
    b.close()


def test_graph_replays_equal_eager(dev):
    """calls 1-2 (eager) and 3-5 (replayed, other batches) are the bits of an engine that never captures; the ragged batch size captures
    a graph of its own; close() drops both"""
    a = _trained(dev, _cfg("fp16", graphs="step", fused_tail_eval=True))
    b = _trained(dev, _cfg("fp16", graphs="none", fused_tail_eval=True))
    assert a._tail_eval and b._tail_eval and torch.equal(a.dense_flat.detach(), b.dense_flat.detach())
    keys = []
    with _Counted() as c:
        for B in SIZES:
            for s in range(5):
                ids, wts, label = _batch(a.cfg, dev, 200 + s, B)
                n0 = c.calls
                ra = [t.clone() for t in a.predict_fused(ids, wts, label)]
                assert c.calls == n0 + (0 if s >= 3 else 1), (B, s)          # (call 3 captures through the op, 4 and 5 replay)
                rb = [t.clone() for t in b.predict_fused(ids, wts, label)]
                _same(ra, rb, (B, s), loss_rel=0.0)
                key = (tuple(ids.shape), ids.dtype, True)
                assert (a._predict_graphs[key]["g"] is not None) == (s >= 2), (B, s)
            keys.append(key)
    assert keys[0] != keys[1] and all(a._predict_graphs[k]["g"] is not None for k in keys) and not b._predict_graphs
    a.close()
    assert a._predict_graphs == {}
    b.close()


def test_training_state_is_untouched(dev):
    a = _trained(dev, _cfg("bf16", fused_tail_eval=True))
    b = _trained(dev, _cfg("bf16", fused_tail_eval=True))
    snap = lambda e: [e.dense_flat.detach().clone(), e.dense_m.clone(), e.dense_v.clone(), e.deep_state.clone(), e.dense16_flat.clone(),      # noqa: E731
                      e._tail_packed.clone()]
    before, steps = snap(a), a.step_count
    with _Counted() as c:
        for s in range(4):                   # ragged batches: two eager calls, the capture, one replay
            a.predict_fused(*_batch(a.cfg, dev, 99 + s, 200))
        assert c.calls == 3
    assert a.step_count == steps
    for x, y in zip(before, snap(a)):
        assert torch.equal(_bits(x), _bits(y))
    batch = _batch(a.cfg, dev, 50, 256)
    la, lb = a.train_step(*batch).clone(), b.train_step(*batch).clone()
    assert torch.equal(_bits(la.view(1)), _bits(lb.view(1))), (float(la), float(lb))
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach()) and torch.equal(a.deep_state, b.deep_state)
    a.close()
    b.close()


def test_deepfm_equals_its_twin(dev):
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMEngine
    from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch
    kw = dict(data_vocab_size=4000, data_emb_dim=16, data_field_size=26, batch_size=256, deep_layer_dims=list(TAIL_NET), mlp_dtype="fp16",
              graphs="none")
    bcfg = WideDeepConfig(vocab_size=4000, emb_dim=16, field_size=26, batch_size=256)
    a, b = DeepFMEngine(DeepFMConfig(fused_tail_eval=True, **kw), dev), DeepFMEngine(DeepFMConfig(fused_tail_eval=False, **kw), dev)
    for s in range(3):
        batch = synthetic_batch(bcfg, dev, "zipf", seed=10 + s, signal=True)
        a.train_step(*batch)
        b.train_step(*batch)
    assert a._mfma and a._tail_eval and b._tail_ok and not b._tail_eval and a.fused_predict_supported
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach())
    with _Counted() as c:
        for B in SIZES:
            ids, wts, label = _batch(bcfg, dev, 99, B)
            for lab in (label, None):
                n0 = c.calls
                ra = [t.clone() for t in a.predict_fused(ids, wts, lab)]
                assert c.calls == n0 + 1
                rb = [t.clone() for t in b.predict_fused(ids, wts, lab)]
                assert c.calls == n0 + 1
                _same(ra, rb, ("deepfm", B, lab is not None))


@pytest.mark.parametrize("what,over", [("fused_tail off", dict(fused_tail=False)), ("a 64 x 1024 net", dict(layers=[64, 1024])),
                                       ("an fp32 net", dict(dt="fp32"))])
def test_engines_without_the_tail_never_call_the_op(dev, what, over):
    over = dict(over)
    e = _trained(dev, _cfg(over.pop("dt", "fp16"), layers=over.pop("layers", TAIL_NET), graphs="none", fused_tail_eval=True, **over), steps=1)
    assert not e._tail_ok and not e._tail_eval
    with _Counted() as c:
        for B in SIZES:
            ids, wts, label = _batch(e.cfg, dev, 99, B)
            lf, pf, loss = e.predict_fused(ids, wts, label)
            assert tuple(lf.shape) == (B, 1) and bool(torch.isfinite(loss))
        assert c.calls == 0, what
    e.close()
