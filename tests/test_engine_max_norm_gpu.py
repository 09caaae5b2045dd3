"""max_norm on DeepFMEngine, DeepCrossEngine and the one-GPU DeepFMHashEngine: three steps and predict on the GPU against the
oracle-side engine with the float64 clip (tests/_clip_sums_ref.py) at the shapes and tolerances of those engines' own step tests
(tests/test_wide_deep_gpu.py, tests/test_config5_gpu.py; Deep&Cross at emb_dim 32, the nearest width to its 30 that can clip), with a
bound that about half of the looked-up rows exceed; and max_norm=None: the launches and the bits of an engine built without the field."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def row_rel(a, b):
    den = np.maximum(np.abs(b).max(axis=1), 1e-30)
    return float((np.abs(a.astype(np.float64) - b).max(axis=1) / den).max())


def _bound(table, ids):
    """a bound about half of the looked-up rows exceed: the median of their norms at four digits, no row within 1e-5 of it (the
    float64 model and the fp32 kernels then take the same decisions at the start)"""
    n = np.linalg.norm(table.astype(np.float64), axis=1)
    c = float(np.round(np.median(n[ids.reshape(-1)]), 4))
    assert np.abs(n / c - 1.0).min() > 1e-5
    return c, float((n[ids.reshape(-1)] > c).mean())


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_deepfm_engine_with_max_norm_matches_oracle_engine(dev, oracle):
    from _clip_sums_ref import OracleClipDeepFMEngine
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMEngine
    from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch
    kw = dict(data_vocab_size=4000, data_emb_dim=16, data_field_size=39, batch_size=128, deep_layer_dims=[64, 32], mlp_dtype="fp32")
    bcfg = WideDeepConfig(vocab_size=4000, emb_dim=16, field_size=39, batch_size=128)
    batches = [synthetic_batch(bcfg, "cpu", "zipf", seed=40 + s) for s in range(3)]
    c0, frac = _bound(oracle.fill_normal(DeepFMConfig().seed, 4000, 16, 0.01), batches[0][0].numpy())
    assert 0.2 < frac < 0.8, frac
    cfg = DeepFMConfig(max_norm=c0, **kw)
    g = DeepFMEngine(cfg, dev)
    c = OracleClipDeepFMEngine(cfg, "cpu")
    plain = DeepFMEngine(DeepFMConfig(**kw), dev)
    assert np.array_equal(g.V_l2.cpu().numpy(), c.V_l2.numpy())
    for ids, wts, label in batches:
        lc = float(c.train_step(ids, wts, label))
        lg = float(g.train_step(ids.to(dev), wts.to(dev), label.to(dev)))
        plain.train_step(ids.to(dev), wts.to(dev), label.to(dev))
        assert abs(lc - lg) <= 2e-5 * max(abs(lc), 1e-3)
    assert row_rel(g.V_l2.cpu().numpy(), c.V_l2.numpy()) <= 5e-5
    assert np.abs(g.W_l2.cpu().numpy() - c.W_l2.numpy()).max() <= 1e-4 * np.abs(c.W_l2.numpy()).max()
    assert np.allclose(g.dense_flat.detach().cpu().numpy(), c.dense_flat.detach().numpy(), rtol=2e-4, atol=2e-6)
    assert not torch.equal(g.V_l2, plain.V_l2)                           # the clip changed the training
    logit, prob = g.predict(ids.to(dev), wts.to(dev))
    lc2, _ = c.predict(ids, wts)
    assert np.allclose(logit.cpu().numpy(), lc2.numpy(), rtol=1e-3, atol=1e-4)


def test_deep_cross_engine_with_max_norm_matches_oracle_engine(dev, oracle):
    """The third step is the captured whole-step graph's first replay: the clip kernel is one more node of it."""
    from _clip_sums_ref import OracleClipDeepCrossEngine
    from mindrec_amd.deep_cross import DeepCrossConfig, DeepCrossEngine
    from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch
    kw = dict(vocab_size=5000, emb_dim=32, field_size=39, batch_size=128, deep_layer_dim=[64, 32])
    bcfg = WideDeepConfig(vocab_size=5000, emb_dim=32, field_size=39, batch_size=128)
    batches = [synthetic_batch(bcfg, "cpu", "zipf", seed=21 + s) for s in range(3)]
    c0, frac = _bound(oracle.fill_normal(DeepCrossConfig().seed, 5000, 32, 1.0 / float(np.sqrt(32))), batches[0][0].numpy())
    assert 0.2 < frac < 0.8, frac
    cfg = DeepCrossConfig(max_norm=c0, **kw)
    g = DeepCrossEngine(cfg, dev)
    c = OracleClipDeepCrossEngine(cfg, "cpu")
    plain = DeepCrossEngine(DeepCrossConfig(**kw), dev)
    assert g._native and cfg.graphs == "step"
    assert np.array_equal(g.table.cpu().numpy(), c.table.numpy())
    for ids, wts, label in batches:
        lc = float(c.train_step(ids, wts, label))
        lg = float(g.train_step(ids.to(dev), wts.to(dev), label.to(dev)))
        plain.train_step(ids.to(dev), wts.to(dev), label.to(dev))
        assert abs(lc - lg) <= 2e-5 * max(abs(lc), 1e-3)
    assert g._graph is not None
    a, b = g.table.cpu().numpy(), c.table.numpy()
    assert row_rel(a, b) <= 5e-5, row_rel(a, b)
    assert np.allclose(g.dense_flat.detach().cpu().numpy(), c.dense_flat.detach().numpy(), rtol=2e-4, atol=2e-6)
    assert not torch.equal(g.table, plain.table)
    logit, prob = g.predict(ids.to(dev), wts.to(dev))
    lc2, _ = c.predict(ids, wts)
    assert logit.shape == (128, 1)
    assert np.allclose(logit.cpu().numpy(), lc2.numpy(), rtol=1e-3, atol=1e-4)      # (the DeepFM step test's bound on predict)
    g.close(); plain.close()


def _rows_view(oracle, m, cap, D):
    pr = oracle.lib().mrec_o_map_rows_ptr
    pr.restype = C.POINTER(C.c_float)
    return np.ctypeslib.as_array(pr(m._h), shape=(cap, D))


def test_deepfm_hash_engine_with_max_norm_matches_reference(dev, oracle):
    """tests/test_config5_gpu.py's reference at its small shape (admission after two hits, no eviction here) with the clip: V's
    looked-up rows clipped in float64, V's LazyAdam over the Jacobian-transformed sums (tests/_oracle_clip_ops.py); W plain."""
    import _oracle_clip_ops as OC
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMHashEngine
    B, Fd, cap, pool, D = 48, 6, 4096, 40, 128
    cfg = DeepFMConfig(data_emb_dim=D, data_field_size=Fd, batch_size=B, deep_layer_dims=[64, 32], learning_rate=1e-2, mlp_dtype="fp32")
    rng = np.random.default_rng(5)
    keys_pool = rng.integers(1, 2 ** 40, size=pool)
    tmp = oracle.Map(D, cap, seed=cfg.seed, sigma=0.01)                   # the pool's default rows, to place the bound
    c0, _ = _bound(_rows_view(oracle, tmp, cap, D)[tmp.find_or_insert(keys_pool.astype(np.int64), True)], np.arange(pool))
    eng = DeepFMHashEngine(cfg, dev, key_dtype=torch.int64, capacity=cap, permit_filter_value=2, max_norm=c0)
    oV, oW = oracle.Map(D, cap, seed=cfg.seed, sigma=0.01), oracle.Map(1, cap, seed=cfg.seed + 1, sigma=0.01)
    vV, vW = _rows_view(oracle, oV, cap, D), _rows_view(oracle, oW, cap, 1)
    st = {"V": (np.zeros((cap, D), np.float32), np.zeros((cap, D), np.float32)),
          "W": (np.zeros((cap, 1), np.float32), np.zeros((cap, 1), np.float32))}
    hits = {}
    dense = eng.dense_flat.detach().cpu().clone().requires_grad_(True)
    dm, dv = np.zeros(dense.numel(), np.float32), np.zeros(dense.numel(), np.float32)
    dims, offs = eng.dims, [p.storage_offset() for p in eng.dense]
    b1p = b2p = np.float32(1.0)

    def ref_mlp(x):
        h = x
        for i in range(len(dims) - 1):
            W = dense[offs[2 * i]:offs[2 * i] + dims[i] * dims[i + 1]].view(dims[i], dims[i + 1])
            b = dense[offs[2 * i + 1]:offs[2 * i + 1] + dims[i + 1]]
            h = torch.addmm(b, h, W)
            if i < len(dims) - 2:
                h = torch.relu(h)
        return h

    fracs, n_updated = [], 0
    for step in range(3):
        keys = rng.choice(keys_pool, size=(B, Fd)).astype(np.int64)
        wts = rng.random((B, Fd)).astype(np.float32)
        label = (rng.random((B, 1)) < 0.4).astype(np.float32)
        lg = float(eng.train_step(T(keys, dev), T(wts, dev), T(label, dev)))
        flat = keys.reshape(-1)
        rows_v, rows_w = oV.find_or_insert(flat, True), oW.find_or_insert(flat, True)
        uk = np.unique(flat)
        for k in uk.tolist():
            hits[k] = hits.get(k, 0) + 1
        fracs.append(float((np.linalg.norm(vV[rows_v].astype(np.float64), axis=1) > c0).mean()))
        vx = OC.gather_rows(torch.from_numpy(vV), torch.from_numpy(rows_v), torch.from_numpy(wts.reshape(-1)), max_norm=c0)
        vx = vx.reshape(B, Fd, D).requires_grad_(True)
        lin = torch.from_numpy(oracle.wide_sum(vW, rows_w.reshape(B, Fd), wts, 0.0)).requires_grad_(True)
        s = vx.sum(dim=1)
        fm = 0.5 * (s * s - (vx * vx).sum(dim=1)).sum(dim=1)
        logit = (lin + fm).view(-1, 1) + ref_mlp(vx.view(B, Fd * D))
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, torch.from_numpy(label))
        dense.grad = None
        (loss * cfg.loss_scale).backward()
        lr_ = float(loss.detach())
        assert abs(lr_ - lg) <= 2e-5 * max(abs(lr_), 1e-3), (step, lr_, lg)
        b1p = np.float32(b1p * np.float32(0.9)); b2p = np.float32(b2p * np.float32(0.999))
        kw = dict(lr=cfg.learning_rate, eps=cfg.epsilon, b1_pow=float(b1p), b2_pow=float(b2p))
        adm_u = np.fromiter((hits[k] >= 2 for k in uk.tolist()), bool, uk.size)
        admitted = adm_u[np.searchsorted(uk, flat)]
        n_updated += int(adm_u.sum())
        u, sums = OC.clipped_sums(vV, np.where(admitted, rows_v, -1), vx.grad.numpy().reshape(-1, D), wts.reshape(-1), 1.0 / cfg.loss_scale, c0)
        oracle.sparse_lazy_adam(vV, st["V"][0], st["V"][1], u, sums, None, grad_scale=1.0, **kw)
        gw = (lin.grad.numpy().reshape(B, 1) * wts).reshape(-1, 1)
        oracle.sparse_lazy_adam(vW, st["W"][0], st["W"][1], np.where(admitted, rows_w, -1), gw, None, grad_scale=1.0 / cfg.loss_scale, **kw)
        oracle.dense_adam(dense.detach().numpy(), dm, dv, dense.grad.numpy(), grad_scale=1.0 / cfg.loss_scale, **kw)
    assert 0.2 < fracs[0] < 0.8, fracs
    assert n_updated > pool                                               # admitted rows took the clipped apply, un-admitted ones were skipped
    keys = np.array(sorted(hits), np.int64)
    got, ref = eng.V.get(T(keys, dev), False).cpu().numpy(), oV.get(keys, False)
    assert row_rel(got, ref) <= 5e-5
    gw_, rw_ = eng.W.get(T(keys, dev), False).cpu().numpy(), oW.get(keys, False)
    assert np.abs(gw_ - rw_).max() <= 1e-4 * np.abs(rw_).max()
    got_d, ref_d = eng.dense_flat.detach().cpu().numpy(), dense.detach().numpy()
    over = np.abs(got_d - ref_d) - (2e-6 + 2e-4 * np.abs(ref_d))         # (tests/test_config5_gpu.py's bound on the dense net)
    assert (over > 0).sum() <= 1e-4 * got_d.size and np.abs(got_d - ref_d).max() <= 5e-3 * cfg.learning_rate
    # predict: the clipped lookup again, against the reference's forward
    pk, pw = rng.choice(keys_pool, size=(B, Fd)).astype(np.int64), rng.random((B, Fd)).astype(np.float32)
    logit, _ = eng.predict(T(pk, dev), T(pw, dev))
    rv, rw = oV.find_or_insert(pk.reshape(-1), True), oW.find_or_insert(pk.reshape(-1), True)
    with torch.no_grad():
        vx = OC.gather_rows(torch.from_numpy(vV), torch.from_numpy(rv), torch.from_numpy(pw.reshape(-1)), max_norm=c0).reshape(B, Fd, D)
        s = vx.sum(dim=1)
        ref_logit = (torch.from_numpy(oracle.wide_sum(vW, rw.reshape(B, Fd), pw, 0.0)) + 0.5 * (s * s - (vx * vx).sum(dim=1)).sum(dim=1)).view(-1, 1) \
            + ref_mlp(vx.view(B, Fd * D))
    assert np.allclose(logit.cpu().numpy(), ref_logit.numpy(), rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("which", ["deepfm", "deep_cross", "hash"])
def test_max_norm_none_runs_the_launches_and_bits_of_an_engine_without_the_field(dev, which, monkeypatch):
    from mindrec_amd import ops
    from mindrec_amd.deep_cross import DeepCrossConfig, DeepCrossEngine
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMEngine, DeepFMHashEngine
    from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch

    def build(explicit):
        kw = {"max_norm": None} if explicit else {}
        if which == "deepfm":
            e = DeepFMEngine(DeepFMConfig(data_vocab_size=4000, data_emb_dim=16, data_field_size=39, batch_size=128, deep_layer_dims=[64, 32],
                                          mlp_dtype="fp32", **kw), dev)
            return e, lambda: (e.V_l2, e.W_l2, e.dense_flat.detach())
        if which == "deep_cross":
            e = DeepCrossEngine(DeepCrossConfig(vocab_size=5000, emb_dim=32, field_size=39, batch_size=128, deep_layer_dim=[64, 32], **kw), dev)
            return e, lambda: (e.table, e.dense_flat.detach())
        cfg = DeepFMConfig(data_emb_dim=128, data_field_size=39, batch_size=128, deep_layer_dims=[64, 32], learning_rate=1e-2, mlp_dtype="fp32")
        e = DeepFMHashEngine(cfg, dev, key_dtype=torch.int64, capacity=8192, **kw)
        return e, lambda: (e.V.values, e.W.values, e.dense_flat.detach())

    D = {"deepfm": 16, "deep_cross": 32, "hash": 128}[which]
    bcfg = WideDeepConfig(vocab_size=4000, emb_dim=D, field_size=39, batch_size=128)
    batches = [synthetic_batch(bcfg, dev, "zipf", seed=60 + s) for s in range(3)]
    if which == "hash":
        batches = [(ids.to(torch.int64), wts, label) for ids, wts, label in batches]
    outs = []
    for explicit in (True, False):
        e, tables = build(explicit)
        if explicit:                                                      # None launches no clip kernel and passes no max_norm on
            def no_clip(*a, **k):
                raise AssertionError("clip_group_sums_ launched without max_norm")
            real_gather, real_apply = ops.gather_rows, ops.sparse_lazy_adam_

            def gather(*a, **k):
                assert "max_norm" not in k
                return real_gather(*a, **k)

            def apply(*a, **k):
                assert "max_norm" not in k
                return real_apply(*a, **k)
            monkeypatch.setattr(ops, "clip_group_sums_", no_clip)
            monkeypatch.setattr(ops, "gather_rows", gather)
            monkeypatch.setattr(ops, "sparse_lazy_adam_", apply)
        losses = [float(e.train_step(ids, wts, label)) for ids, wts, label in batches]
        logit, _ = e.predict(batches[0][0], batches[0][1])
        outs.append((losses, [t.clone() for t in tables()], logit.clone()))
        monkeypatch.undo()
        if hasattr(e, "close"):
            e.close()
    (la, ta, pa), (lb, tb, pb) = outs
    assert la == lb and torch.equal(pa, pb)
    assert all(torch.equal(x, y) for x, y in zip(ta, tb))
