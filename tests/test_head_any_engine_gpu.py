"""The engines on dense nets whose last hidden layer the first head kernel does not serve (K5 / 8 no power of two, or K5 > 512):
the 16-bit net takes its output end through ops.head_fwd_bwd_any, the fp32 net does where 1024 < K5 <= 2048.

The 16-bit [64, 1024] and [48, 24] cases below raised UnsupportedNet before the head for any width existed ("output head": the
engine had no HIP path for them); the fp32 [64, 2048] engine had _f32net false and raised it from the training step."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RESTATE_BATCH = 256


def _row_rel(a, b):
    den = np.maximum(np.abs(b).max(axis=1), 1e-30)
    return float((np.abs(a.astype(np.float64) - b).max(axis=1) / den).max())


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("layers", [[64, 512], [64, 1024], [48, 24], [64, 2048]], ids=lambda v: "x".join(map(str, v)))
def test_mlp_step_matches_torch_restatement(dev, layers, dt):
    """The comparison and the tolerances of test_mfma_mlp_step_matches_torch_fp32_reference: a plain PyTorch fp32 restatement with the
    same rounding points, through autograd on the same GPU.  [64, 512] is the control (the first head kernel) that calibrates the
    shape; the others run the head for any width."""
    from mindrec_amd import ops
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch
    from mindrec_amd.wide_deep_mlp import _WideProd
    cfg = WideDeepConfig(vocab_size=20_000, emb_dim=16, field_size=26, batch_size=RESTATE_BATCH, deep_layer_dim=layers, mlp_dtype=dt)
    e = WideDeepEngine(cfg, dev)
    assert e._mfma and e._fold_wide
    assert ops.head_supported(layers[-1]) == (layers[-1] == 512) and ops.head_any_supported(layers[-1])
    amp = e._amp
    ids, wts, label = synthetic_batch(cfg, dev, "zipf", seed=5)
    emb, wide, _ = e.lookup(ids, wts)
    assert isinstance(wide, _WideProd)
    loss, g_emb, g_wide = e._mlp_step_eager(emb, wide, label)
    e._sum_dw_slabs()
    gd1 = e.dense_grad_flat.detach().clone()
    n = len(e.dims) - 1
    params = [p.detach().clone().requires_grad_(True) for p in e.dense]
    x = emb.detach().clone().requires_grad_(True)
    wd = (wide.prod[..., 0].sum(dim=1) + e.wide_b).detach().clone().requires_grad_(True)
    with torch.enable_grad():
        h = x
        for i in range(n - 1):
            W16 = params[2 * i].to(amp)
            h = torch.relu(h.float() @ W16.float() + params[2 * i + 1]).to(amp)
        logit = h.float() @ params[2 * (n - 1)] + params[2 * (n - 1) + 1] + wd.view(-1, 1)
        loss2 = torch.nn.functional.binary_cross_entropy_with_logits(logit, label)
        (loss2 * cfg.sens).backward()
    ge1, ge2 = g_emb.float(), x.grad.float()
    fig = {"loss": abs(float(loss) - float(loss2.detach())) / abs(float(loss2.detach())),
           "g_emb max": float((ge1 - ge2).abs().max()) / float(ge2.abs().max()), "g_emb equal": float((ge1 == ge2).float().mean())}
    worst = 0.0
    for i, p in enumerate(params):
        ref = p.grad
        got = gd1[e.dense_grad[i].storage_offset(): e.dense_grad[i].storage_offset() + ref.numel()].view_as(ref)
        worst = max(worst, float((got - ref).abs().max()) / float(ref.abs().max()))
    fig["dense grad"] = worst
    print("  figures", layers, dt, fig)
    assert fig["loss"] <= 2e-5, (dt, fig)
    assert torch.allclose(g_wide, wd.grad, rtol=2e-3, atol=1e-6 * float(wd.grad.abs().max())), dt
    assert fig["g_emb max"] <= 0.1, (dt, fig)
    assert fig["g_emb equal"] >= 0.9, (dt, fig)
    for i, p in enumerate(params):
        ref = p.grad
        got = gd1[e.dense_grad[i].storage_offset(): e.dense_grad[i].storage_offset() + ref.numel()].view_as(ref)
        assert float((got - ref).abs().max()) <= 5e-3 * float(ref.abs().max()) + 1e-12, (dt, i)
    # the wide bias' gradient arrives in place: the sum of dlogit (g_wide's elementwise bound, summed)
    assert abs(float(e.wide_b_grad) - float(wd.grad.sum())) <= 2e-3 * float(wd.grad.abs().sum()) + 1e-6 * float(wd.grad.abs().max()) * len(wd)


def test_folded_wide_branch_equals_separate_wide_kernels_at_1024(dev):
    """as test_folded_wide_branch_equals_separate_wide_kernels on uniform ids: the head for any width adds the folded lookup's
    per-field products in the order the separate wide kernels do -- losses, tables and dense parameters bit for bit"""
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch
    kw = dict(vocab_size=40000, emb_dim=80, field_size=26, batch_size=2048, deep_layer_dim=[64, 1024], mlp_dtype="bf16")
    a = WideDeepEngine(WideDeepConfig(fold_wide=True, **kw), dev)
    b = WideDeepEngine(WideDeepConfig(fold_wide=False, **kw), dev)
    assert a._fold_wide and not b._fold_wide
    for s in range(6):
        batch = synthetic_batch(a.cfg, dev, "uniform", seed=40 + s)
        la, lb = float(a.train_step(*batch)), float(b.train_step(*batch))
        assert la == lb, (s, la, lb)
    assert torch.equal(a.deep, b.deep) and torch.equal(a.wide, b.wide) and torch.equal(a.wide_accum, b.wide_accum)
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach())


def test_mlp_graph_replay_is_bit_identical_to_eager_at_1024(dev):
    """as test_graph_replay_is_bit_identical_to_eager[mlp]: the captured MLP step holds the head for any width on the same workspace"""
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch
    kw = dict(vocab_size=50000, emb_dim=16, field_size=26, batch_size=2048, deep_layer_dim=[64, 1024], mlp_dtype="bf16")
    a = WideDeepEngine(WideDeepConfig(graphs="mlp", **kw), dev)
    b = WideDeepEngine(WideDeepConfig(graphs="none", **kw), dev)
    assert a._mfma and a._fold_wide
    for s in range(9):
        ids, wts, label = synthetic_batch(a.cfg, dev, "zipf", seed=70 + s)
        la, lb = float(a.train_step(ids, wts, label)), float(b.train_step(ids, wts, label))
        assert la == lb, (s, la, lb)
    assert a._mlp_graph is not None and b._mlp_graph is None
    assert torch.equal(a.deep, b.deep) and torch.equal(a.wide, b.wide)
    assert torch.equal(a.dense_flat.detach(), b.dense_flat.detach())


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_16bit_net_with_dropout_tracks_oracle_engine_at_1024(dev, oracle, dt):
    """Dropout (dh_scale = 1 / keep in the head) on [64, 1024]: three steps against the fp32 oracle-side engine, whose masks are the
    same function of (seed, step, layer, row, column).  Loss: 3e-3 relative, the project's bound for a 16-bit net against the fp32
    oracle (test_deepfm_engine_in_the_references_precision); parameters: within Adam's reach of a flipped gradient sign per step,
    as there."""
    from _oracle_engine import OracleWideDeepEngine
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch
    kw = dict(vocab_size=20_000, emb_dim=16, field_size=39, batch_size=128, deep_layer_dim=[64, 1024], dropout_flag=True)
    g = WideDeepEngine(WideDeepConfig(mlp_dtype=dt, **kw), dev)
    c = OracleWideDeepEngine(WideDeepConfig(mlp_dtype="fp32", **kw), "cpu")
    n = WideDeepEngine(WideDeepConfig(mlp_dtype=dt, **{**kw, "dropout_flag": False}), dev)
    assert g._mfma and g._dropout and not g.k.head_supported(1024)
    nd = c.dense_flat.numel()
    assert torch.equal(g.dense_flat.detach().cpu()[:nd], c.dense_flat.detach()[:g.dense_flat.numel()])
    for s in range(3):
        ids, wts, label = synthetic_batch(g.cfg, "cpu", "zipf", seed=31 + s)
        lc = float(c.train_step(ids, wts, label))
        lg = float(g.train_step(ids.to(dev), wts.to(dev), label.to(dev)))
        ln = float(n.train_step(ids.to(dev), wts.to(dev), label.to(dev)))
        print("  losses", dt, s, lg, lc, abs(lg - lc) / abs(lc))
        assert abs(lg - lc) <= 3e-3 * abs(lc), (s, lg, lc)
        assert lg != ln                                  # the masks do act
    lr = g.cfg.adam_lr
    d = np.abs(g.dense_flat.detach().cpu().numpy()[:nd] - c.dense_flat.detach().numpy()[:nd])
    assert d.max() <= 2 * lr * 3, d.max()
    assert np.abs(g.deep.cpu().numpy() - c.deep.numpy()).max() <= 2 * lr * 3


def test_deepfm_engine_in_the_references_precision_at_1024(dev):
    """test_deepfm_engine_in_the_references_precision with deep_layer_dims = [64, 1024], fp16"""
    from _oracle_engine import OracleDeepFMEngine
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMEngine
    from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch
    kw = dict(data_vocab_size=4000, data_emb_dim=16, data_field_size=39, batch_size=256, deep_layer_dims=[64, 1024])
    g = DeepFMEngine(DeepFMConfig(mlp_dtype="fp16", **kw), dev)
    c = OracleDeepFMEngine(DeepFMConfig(mlp_dtype="fp32", **kw), "cpu")
    assert g._mfma and torch.equal(g.dense_flat.detach().cpu()[:c.dense_flat.numel()], c.dense_flat.detach()[:g.dense_flat.numel()])
    bcfg = WideDeepConfig(vocab_size=4000, emb_dim=16, field_size=39, batch_size=256)
    for s in range(6):
        ids, wts, label = synthetic_batch(bcfg, "cpu", "zipf", seed=70 + s)
        lc = float(c.train_step(ids, wts, label))
        lg = float(g.train_step(ids.to(dev), wts.to(dev), label.to(dev)))
        assert abs(lg - lc) <= 3e-3 * abs(lc), (s, lg, lc)
    assert g._mlp_graph is not None
    for a, b, name in ((g.V_l2, c.V_l2, "V"), (g.W_l2, c.W_l2, "W")):
        a, b = a.cpu().numpy(), b.numpy()
        assert np.abs(a - b).max() <= 2 * g.cfg.learning_rate * 6, name
        assert np.mean(np.abs(a - b) <= 0.1 * g.cfg.learning_rate) > 0.97, name
    n = c.dense_flat.numel()
    d = np.abs(g.dense_flat.detach().cpu().numpy()[:n] - c.dense_flat.detach().numpy()[:n])
    assert d.max() <= 2 * g.cfg.learning_rate * 6 and np.mean(d <= 0.1 * g.cfg.learning_rate) > 0.9
    ids, wts, _ = synthetic_batch(bcfg, "cpu", "zipf", seed=99)
    pg, pc = g.predict(ids.to(dev), wts.to(dev))[1].cpu().numpy(), c.predict(ids, wts)[1].numpy()
    assert np.abs(pg - pc).max() <= 2e-2


@pytest.mark.parametrize("dropout", [False, True])
def test_fp32_net_with_a_2048_wide_last_layer_matches_oracle_engine(dev, oracle, dropout):
    """test_fp32_net_with_a_wide_last_layer_matches_oracle_engine one step wider: past the Deep&Cross head's 1024 columns the fp32
    net takes the head for any width on fp32 activations.  Same tolerances."""
    from _oracle_engine import OracleWideDeepEngine
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch
    cfg = WideDeepConfig(vocab_size=20_000, emb_dim=16, field_size=39, batch_size=128, deep_layer_dim=[64, 2048], mlp_dtype="fp32",
                         dropout_flag=dropout)
    g, c = WideDeepEngine(cfg, dev), OracleWideDeepEngine(cfg, "cpu")
    assert g._f32net and not g.k.head_supported(2048) and not g.k.dcn_head_supported(2048, 2)
    for s in range(3):
        ids, wts, label = synthetic_batch(cfg, "cpu", "zipf", seed=31 + s)
        lc = float(c.train_step(ids, wts, label))
        lg = float(g.train_step(ids.to(dev), wts.to(dev), label.to(dev)))
        assert abs(lc - lg) <= 1e-5 * max(abs(lc), 1e-3)
    assert _row_rel(g.deep.cpu().numpy(), c.deep.numpy()) <= 2e-5
    assert np.allclose(g.dense_flat.detach().cpu().numpy(), c.dense_flat.detach().numpy(), rtol=1e-4, atol=1e-6)
