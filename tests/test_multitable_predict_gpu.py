"""MultiTableWideDeep (mindrec_amd/multitable.py) on the GPU: predict_fused is ops.multitable_input -> ops.dense_fwd x5 -> ops.head_predict
and nothing in between (bit for bit), it computes the reference's WideDeepModel.construct + sigmoid (float64 restatement, tests/
_multitable_ref.py), load_parameters round-trips, evaluate is the metric fed by hand, and the loss is the mean sigmoid cross-entropy of
the returned logits.  Small tables (vocab 50 / 20 / 30 / 16), field counts 2 / 3 / 2, bags (3, 5, 4, 3, 4, 2), five layers of 64."""
import functools

import numpy as np
import pytest
import torch

import _multitable_ref as R

pytestmark = pytest.mark.gpu

BAGS = (3, 5, 4, 3, 4, 2)
N_IND, N_128, N_64 = 2, 3, 2
VOCAB = dict(emb128=50, emb64_single=20, emb64_multi=30, indicator=16)


def make_cfg(mlp_dtype="fp16"):
    from mindrec_amd.multitable import MultiTableConfig
    return MultiTableConfig(emb128_vocab=VOCAB["emb128"], emb64_single_vocab=VOCAB["emb64_single"], emb64_multi_vocab=VOCAB["emb64_multi"],
                            indicator_vocab=VOCAB["indicator"], n_indicator=N_IND, n_emb128=N_128, n_emb64_single=N_64, multi_bags=BAGS,
                            deep_dims=(64,) * 5, mlp_dtype=mlp_dtype, seed=3)


@functools.lru_cache(maxsize=None)
def named_params():
    """parameters by the reference's names, scaled so that activations stay O(1) and the logits spread over the sigmoid"""
    rng = np.random.default_rng(11)
    f = lambda *shape, s=1.0: (rng.standard_normal(shape) * s).astype(np.float32)
    p = {"emb128_embedding": f(VOCAB["emb128"], 128, s=0.5), "emb64_single": f(VOCAB["emb64_single"], 64, s=0.5),
         "emb64_multi": f(VOCAB["emb64_multi"], 64, s=0.5), "emb64_indicator": f(VOCAB["indicator"], 64, s=0.5),
         "wide_continue_w": f(32, s=0.1), "wide_emb128_w": f(VOCAB["emb128"], s=0.3), "wide_emb64_single_w": f(VOCAB["emb64_single"], s=0.3),
         "wide_emb64_multi_w": f(VOCAB["emb64_multi"], s=0.3), "wide_indicator_w": f(VOCAB["indicator"], s=0.3), "wide_bias": f(1, s=0.1)}
    dims = [32 + N_IND * 64 + N_128 * 128 + N_64 * 64 + 6 * 64] + [64] * 5 + [1]
    for i in range(6):
        name = f"dense_layer_{i + 1}" if i < 5 else "deep_predict"
        p[name + ".weight"] = f(dims[i], dims[i + 1], s=float(np.sqrt(2.0 / dims[i])))
        p[name + ".bias"] = f(dims[i + 1], s=0.1)
    for a in p.values():
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def batch_np(B, seed=0):
    rng = np.random.default_rng(100 + B + seed)
    b = {"continue_val": rng.random((B, 32)).astype(np.float32),
         "indicator_id": rng.integers(0, VOCAB["indicator"], (B, N_IND)).astype(np.int32),
         "emb_128_id": rng.integers(0, VOCAB["emb128"], (B, N_128)).astype(np.int32),
         "emb_64_single_id": rng.integers(0, VOCAB["emb64_single"], (B, N_64)).astype(np.int32)}
    for key, L in zip(R.MULTI_KEYS, BAGS):
        b[key] = rng.integers(0, VOCAB["emb64_multi"], (B, L)).astype(np.int32)
        b[key + "_mask"] = (rng.random((B, L)) < 0.7).astype(np.float32)
    b["label"] = (rng.random(B) < 0.3).astype(np.float32)
    b["label"][:2] = (0.0, 1.0)
    b["display_id"] = np.sort(rng.integers(0, max(B // 4, 2), B)).astype(np.int64)
    for a in b.values():
        a.setflags(write=False)
    return b


def to_dev(b, dev):
    return {k: torch.from_numpy(np.array(v)).to(dev) for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def net(mlp_dtype="fp16"):
    from mindrec_amd.multitable import MultiTableWideDeep
    n = MultiTableWideDeep(make_cfg(mlp_dtype))
    n.load_parameters(named_params())
    return n


@pytest.mark.parametrize("B", [5, 130])
def test_predict_fused_is_the_three_kinds_of_launch_bit_for_bit(dev, B):
    from mindrec_amd import ops
    m = net()
    batch = to_dev(batch_np(B), dev)
    logit, prob = m.predict_fused(batch)
    assert tuple(logit.shape) == (B, 1) and tuple(prob.shape) == (B, 1) and logit.dtype == torch.float32
    x, wide = m.input_row(batch)
    assert x.dtype == torch.float16 and tuple(x.shape) == (B, m.cfg.input_emb_dim) and tuple(wide.shape) == (B,)
    h = x
    for i in range(5):
        w16 = m.params[f"dense_layer_{i + 1}.weight"].to(torch.float16)
        h = ops.dense_fwd(h, None, m.params[f"dense_layer_{i + 1}.bias"], relu=True, wt=w16.t().contiguous())
    lg, pr = ops.head_predict(h, m.params["deep_predict.weight"].view(-1), m.params["deep_predict.bias"], wide=wide)
    assert torch.equal(lg, logit.view(-1)) and torch.equal(pr, prob.view(-1))
    # the input row itself, against the host restatement of the model's layout
    segs, K0 = R.model_segments(named_params(), batch_np(B))
    assert K0 == m.cfg.input_emb_dim
    ref_x = R.input_row(batch_np(B)["continue_val"], segs, K0, "f16")
    assert np.array_equal(x.float().cpu().numpy().view(np.uint32), ref_x.view(np.uint32))
    assert torch.equal(m.predict_fused(batch)[0], logit)                      # and the same bits on the next call


@pytest.mark.parametrize("mlp_dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("B", [5, 130])
def test_predict_fused_against_the_float64_restatement(dev, B, mlp_dtype):
    m = net(mlp_dtype)
    logit, prob = m.predict_fused(to_dev(batch_np(B), dev))
    ref_logit, ref_prob = R.model_forward(named_params(), batch_np(B), {"fp16": "f16", "fp32": "f32"}[mlp_dtype])
    assert ref_prob.std() > 0.05, "the case does not spread over the sigmoid"
    d = np.abs(prob.view(-1).cpu().numpy().astype(np.float64) - ref_prob).max()
    print(f"{mlp_dtype} B={B}: max |dprob| = {d:.3e}, max |dlogit| = {np.abs(logit.view(-1).cpu().numpy() - ref_logit).max():.3e}")
    assert d <= 2e-2


def test_load_parameters_round_trip_and_refusals(dev):
    from mindrec_amd.multitable import MultiTableWideDeep
    from mindrec_amd.wide_deep_mlp import UnsupportedNet
    m = MultiTableWideDeep(make_cfg())
    assert sorted(m.params) == sorted(named_params())
    before = m.predict_fused(to_dev(batch_np(5), dev))[0].clone()
    m.load_parameters(named_params())
    for name, a in named_params().items():
        assert np.array_equal(m.params[name].cpu().numpy(), a), name
    after = m.predict_fused(to_dev(batch_np(5), dev))[0]
    assert torch.equal(after, net().predict_fused(to_dev(batch_np(5), dev))[0]) and not torch.equal(after, before)
    with pytest.raises(ValueError, match="shape"):
        m.load_parameters({"emb64_multi": np.zeros((VOCAB["emb64_multi"], 32), np.float32)})
    with pytest.raises(ValueError, match="shape"):
        m.load_parameters({"wide_bias": np.zeros(1, np.float32), "dense_layer_3.weight": np.zeros((64, 32), np.float32)})
    with pytest.raises(ValueError, match="unknown"):
        m.load_parameters({"dense_layer_6.weight": np.zeros((64, 64), np.float32)})
    assert torch.equal(m.predict_fused(to_dev(batch_np(5), dev))[0], after)   # a refused load writes nothing
    # inputs of the wrong type are refused, and a net the kernels do not cover is UnsupportedNet
    bad = to_dev(batch_np(5), dev)
    bad["emb_128_id"] = bad["emb_128_id"].long()
    with pytest.raises(TypeError):
        m.predict_fused(bad)
    bad = to_dev(batch_np(5), dev)
    bad["multi_doc_ad_topic_id_mask"] = bad["multi_doc_ad_topic_id_mask"].double()
    with pytest.raises(TypeError):
        m.predict_fused(bad)
    cfg = make_cfg()
    cfg.deep_dims = (64, 60, 64)
    with pytest.raises(UnsupportedNet):
        MultiTableWideDeep(cfg).predict_fused(to_dev(batch_np(5), dev))


def test_evaluate_is_the_metric_fed_by_hand(dev, capsys):
    from mindrec_amd.metrics import DeviceAUCMAPMetric
    m = net()
    batches = [to_dev(batch_np(130, seed=s), dev) for s in range(3)]
    for s, b in enumerate(batches):
        b["display_id"] = b["display_id"] + 1000 * s                         # displays do not span batches
    metric = DeviceAUCMAPMetric(capacity=1024)
    auc = m.evaluate(batches, metric)
    by_hand = DeviceAUCMAPMetric(capacity=1024)
    for b in batches:
        logit, prob = m.predict_fused(b)
        by_hand.update(logit, prob, b["label"], b["display_id"])
    assert auc == by_hand.eval() and metric.map == by_hand.map and metric.rank_hist == by_hand.rank_hist and metric.groups == by_hand.groups
    assert 0.0 <= auc <= 1.0 and 0.0 <= metric.map <= 1.0
    assert m.evaluate(batches) == auc                                         # the default metric


@pytest.mark.parametrize("B", [5, 130])
def test_loss_is_the_mean_sigmoid_cross_entropy_of_the_logits(dev, B):
    m = net()
    batch = to_dev(batch_np(B), dev)
    logit, prob, loss = m.predict_fused(batch, label=batch["label"])
    assert loss.dim() == 0
    l2, p2 = m.predict_fused(batch)
    assert torch.equal(logit, l2) and torch.equal(prob, p2)
    z, y = logit.view(-1).cpu().numpy().astype(np.float64), batch_np(B)["label"].astype(np.float64)
    ref = np.mean(np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z))))
    print(f"B={B}: loss {float(loss):.8f}, float64 {ref:.8f}")
    assert np.isclose(float(loss), ref, rtol=2e-6, atol=0)
