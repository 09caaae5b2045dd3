"""MultiTableWideDeep.train_step on the GPU, on a small model (vocabs 16 / 40 / 50 / 30, field counts 2 / 3 / 2, bags (3, 5, 4, 3, 4, 2),
deep_dims (16, 8): the two smallest widths the dense kernels take, B = 64): (a) the gradient pieces of _backward against CPU torch
float64 autograd of the reference's network with the DenseLayer casts in place; (b) the optimizers, given those pieces, against the
tested ops driven by hand on copies, bit for bit; (c) three steps on one batch; (d) nothing new before the first train_step."""
import functools

import numpy as np
import pytest
import torch

import _multitable_ref as R

pytestmark = pytest.mark.gpu

BAGS = (3, 5, 4, 3, 4, 2)
VOCAB = dict(emb128=40, emb64_single=50, emb64_multi=30, indicator=16)
B = 64
TABLES = (("emb64_indicator", "wide_indicator_w"), ("emb128_embedding", "wide_emb128_w"), ("emb64_single", "wide_emb64_single_w"),
          ("emb64_multi", "wide_emb64_multi_w"))
# (a), fp16 net: the largest error of a gradient piece relative to the piece's largest magnitude, measured against the float64
# reference on an MI355X; the assertion allows four times that
FP16_MEASURED = 1.3e-3
# (a), fp32 net, first order: a gradient element is reached through at most 8 chained stages (3 layers forward, the head, 3 layers back,
# the group sum), each an fp32 sum of at most B * 21 = 1344 terms (the longest: the multi-hot table's groups; the widest dot has
# K0 = 1056), each stage adding at most terms * 2^-24 relative to the magnitudes it sums: 8 * 1344 * 2^-24 of the piece's largest magnitude
FP32_BOUND = 8 * 1344 * 2.0 ** -24


def make_cfg(mlp_dtype="fp16", **kw):
    from mindrec_amd.multitable import MultiTableConfig
    return MultiTableConfig(emb128_vocab=VOCAB["emb128"], emb64_single_vocab=VOCAB["emb64_single"], emb64_multi_vocab=VOCAB["emb64_multi"],
                            indicator_vocab=VOCAB["indicator"], multi_bags=BAGS, deep_dims=(16, 8), mlp_dtype=mlp_dtype, seed=5, **kw)


@functools.lru_cache(maxsize=None)
def named_params():
    rng = np.random.default_rng(21)
    f = lambda *shape, s=1.0: (rng.standard_normal(shape) * s).astype(np.float32)
    p = {"emb128_embedding": f(VOCAB["emb128"], 128, s=0.5), "emb64_single": f(VOCAB["emb64_single"], 64, s=0.5),
         "emb64_multi": f(VOCAB["emb64_multi"], 64, s=0.5), "emb64_indicator": f(VOCAB["indicator"], 64, s=0.5),
         "wide_continue_w": f(32, s=0.1), "wide_emb128_w": f(VOCAB["emb128"], s=0.3), "wide_emb64_single_w": f(VOCAB["emb64_single"], s=0.3),
         "wide_emb64_multi_w": f(VOCAB["emb64_multi"], s=0.3), "wide_indicator_w": f(VOCAB["indicator"], s=0.3), "wide_bias": f(1, s=0.1)}
    dims = [32 + 2 * 64 + 3 * 128 + 2 * 64 + 6 * 64, 16, 8, 1]
    for i in range(3):
        name = f"dense_layer_{i + 1}" if i < 2 else "deep_predict"
        p[name + ".weight"] = f(dims[i], dims[i + 1], s=float(np.sqrt(2.0 / dims[i])))
        p[name + ".bias"] = np.abs(f(dims[i + 1], s=0.1))
    for a in p.values():
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def batch_np(B=B):
    rng = np.random.default_rng(100 + B)
    b = {"continue_val": rng.random((B, 32)).astype(np.float32),
         "indicator_id": rng.integers(0, VOCAB["indicator"], (B, 2)).astype(np.int32),
         "emb_128_id": rng.integers(0, VOCAB["emb128"] - 4, (B, 3)).astype(np.int32),          # (rows 36 .. 39 stay untouched)
         "emb_64_single_id": rng.integers(0, VOCAB["emb64_single"] - 4, (B, 2)).astype(np.int32)}
    for key, L in zip(R.MULTI_KEYS, BAGS):
        b[key] = rng.integers(0, VOCAB["emb64_multi"], (B, L)).astype(np.int32)
        b[key + "_mask"] = (rng.random((B, L)) < 0.7).astype(np.float32)
    b["label"] = (rng.random(B) < 0.4).astype(np.float32)
    for a in b.values():
        a.setflags(write=False)
    return b


def dev_batch(B=B):
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in batch_np(B).items()}


def model(mlp_dtype="fp16", **kw):
    from mindrec_amd.multitable import MultiTableWideDeep
    net = MultiTableWideDeep(make_cfg(mlp_dtype, **kw))
    net.load_parameters(named_params())
    return net


@functools.lru_cache(maxsize=None)
def autograd_ref(mlp_dtype):
    """float64 autograd of WideDeepModel.construct + the mean sigmoid cross-entropy; the DenseLayers cast input, weight, bias and output
    to the net's type (a Cast's bprop is a Cast: the identity on the gradient's value) -> {parameter name: gradient}"""
    kind = {"fp16": "f16", "fp32": "f32"}[mlp_dtype]
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in named_params().items()}
    b = {k: torch.from_numpy(np.array(v)) for k, v in batch_np().items()}

    def q(t):
        if kind == "f32":
            return t
        return t + (torch.from_numpy(R.round16(t.detach().numpy().astype(np.float32), kind).astype(np.float64)) - t).detach()

    cols, wide = [b["continue_val"].double()], (b["continue_val"].double() * P["wide_continue_w"]).sum(1) + P["wide_bias"]
    for key, (table, w) in zip(("indicator_id", "emb_128_id", "emb_64_single_id"), TABLES[:3]):
        ids = b[key].long()
        cols.append(P[table][ids].reshape(B, -1))
        wide = wide + P[w][ids].sum(1)
    for key in R.MULTI_KEYS:
        ids, m = b[key].long(), b[key + "_mask"].double()
        cols.append((P["emb64_multi"][ids] * m[:, :, None]).sum(1) / ids.shape[1])
        wide = wide + (P["wide_emb64_multi_w"][ids] * m).sum(1)
    h = torch.cat(cols, dim=1)
    for name in ("dense_layer_1", "dense_layer_2", "deep_predict"):
        y = q(h) @ q(P[name + ".weight"]) + q(P[name + ".bias"])
        h = q(torch.relu(y) if name != "deep_predict" else y)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(wide + h[:, 0], b["label"].double())
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in P.items()}


@pytest.mark.parametrize("mlp_dtype", ["fp32", "fp16"])
def test_a_gradient_pieces_against_float64_autograd(mlp_dtype):
    net, batch = model(mlp_dtype), dev_batch()
    ref_loss, ref = autograd_ref(mlp_dtype)
    g = net._backward(batch, batch["label"])
    got = {}
    for table, w, plan, sums, wsums in g["groups"]:
        rows = plan.uniq.long().cpu().numpy()
        got[table] = np.zeros(ref[table].shape)
        got[table][rows] = sums[:plan.U].cpu().numpy()
        got[w] = np.zeros(ref[w].shape)
        got[w][rows] = wsums[:plan.U].cpu().numpy()
    got["wide_continue_w"], got["wide_bias"] = g["d_wide_cont"].cpu().numpy(), g["d_wide_bias"].cpu().numpy()
    got.update({k: v.cpu().numpy() for k, v in net.dense_gradients().items()})
    assert set(got) == set(ref)
    tol = FP32_BOUND if mlp_dtype == "fp32" else 4 * FP16_MEASURED
    worst = 0.0
    for k in sorted(ref):
        err = float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max())
        worst = max(worst, err)
        print(f"{mlp_dtype} {k}: max |err| / max |ref| = {err:.3e}")
    print(f"{mlp_dtype} worst = {worst:.3e} (allowed {tol:.3e}); loss {float(g['loss']):.6f} vs {ref_loss:.6f}")
    assert abs(float(g["loss"]) - ref_loss) <= tol * max(1.0, abs(ref_loss))
    assert worst <= tol


def test_b_optimizers_bit_for_bit_given_the_pieces():
    from mindrec_amd import ops
    net, batch = model("fp16"), dev_batch()
    cfg = net.cfg
    before = {k: v.clone() for k, v in net.params.items()}
    net.train_step(batch, batch["label"])
    # a second model from the same start: its pieces are the step's (the kernels give the same bits on every run)
    twin = model("fp16")
    g = twin._backward(batch, batch["label"])
    b1p, b2p = float(np.float32(0.9)), float(np.float32(0.999))
    for table, w, plan, sums, wsums in g["groups"]:
        p, m, v = before[table].clone(), torch.zeros_like(before[table]), torch.zeros_like(before[table])
        ops.dense_adam_rows_l2_(p, m, v, plan, sums, 0.0, lr=cfg.adam_lr, beta1=b1p, beta2=b2p, eps=cfg.adam_eps, beta1_power=b1p,
                                beta2_power=b2p, grad_scale=1.0)
        assert torch.equal(p, net.params[table]) and torch.equal(m, net._opt["adam"][table][0]) and torch.equal(v, net._opt["adam"][table][1])
        touched = torch.zeros(p.shape[0], dtype=torch.bool, device=p.device)
        touched[plan.uniq.long()] = True
        moved = (net.params[table] != before[table]).any(1)
        assert not (moved & ~touched).any()                     # first step: m = 0 on untouched rows, so they stay
        gb = torch.zeros_like(before[w])
        ops.scatter_unique_rows_(gb.view(-1, 1), plan, wsums.view(-1, 1))
        var, acc, lin = before[w].clone(), torch.full_like(gb, cfg.ftrl_initial_accum), torch.zeros_like(gb)
        ops.dense_ftrl_(var, acc, lin, gb, lr=cfg.ftrl_lr, l1=cfg.ftrl_l1, l2=cfg.ftrl_l2, lr_power=-0.5, grad_scale=1.0)
        assert torch.equal(var, net.params[w]) and torch.equal(acc, net._opt["ftrl"][w][0]) and torch.equal(lin, net._opt["ftrl"][w][1])
        assert not net._opt["gbuf"][w].any()                    # cleared again
        if (~touched).any():                                    # untouched weights follow dense FTRL: recomputed from linear and accum
            assert (net.params[w][~touched] != before[w][~touched]).any()
    for name, d in (("wide_continue_w", g["d_wide_cont"]), ("wide_bias", g["d_wide_bias"])):
        var, acc, lin = before[name].clone(), torch.full_like(before[name], cfg.ftrl_initial_accum), torch.zeros_like(before[name])
        ops.dense_ftrl_(var, acc, lin, d, lr=cfg.ftrl_lr, l1=cfg.ftrl_l1, l2=cfg.ftrl_l2, lr_power=-0.5, grad_scale=1.0)
        assert torch.equal(var, net.params[name]) and torch.equal(acc, net._opt["ftrl"][name][0]) and torch.equal(lin, net._opt["ftrl"][name][1])
    # a second step moves the untouched rows of a table only where m != 0: nowhere (their m is still 0)
    rows = torch.arange(VOCAB["emb128"] - 4, VOCAB["emb128"], device="cuda")
    net.train_step(batch, batch["label"])
    assert torch.equal(net.params["emb128_embedding"][rows], before["emb128_embedding"][rows])
    assert not net._opt["adam"]["emb128_embedding"][0][rows].any()
    # the dense net moved
    assert not torch.equal(net.params["dense_layer_1.weight"], before["dense_layer_1.weight"])


@pytest.mark.parametrize("mlp_dtype", ["fp16", "fp32"])
def test_c_three_steps_on_one_batch(mlp_dtype):
    from mindrec_amd.multitable import MultiTableWideDeep
    net, batch = model(mlp_dtype), dev_batch()
    logit0, _ = net.predict_fused(batch)
    logit0 = logit0.clone()
    losses = [float(l) for l in net.train([dict(batch)] * 3)]
    print(f"{mlp_dtype} losses: {losses}")
    assert losses[2] < losses[0]
    logit1, prob1 = net.predict_fused(batch)
    assert not torch.equal(logit1, logit0)
    fresh = MultiTableWideDeep(make_cfg(mlp_dtype))
    fresh.load_parameters({k: v.clone() for k, v in net.params.items()})
    logit2, prob2 = fresh.predict_fused(batch)
    assert torch.equal(logit1, logit2) and torch.equal(prob1, prob2)


def test_d_nothing_new_before_the_first_train_step():
    from mindrec_amd.multitable import MultiTableWideDeep
    from mindrec_amd.wide_deep_mlp import UnsupportedNet
    import dataclasses
    from mindrec_amd import ops
    batch = dev_batch()
    net = model("fp16")
    ref = [t.clone() for t in net.predict_fused(batch)]          # (the first call makes the kernels' workspaces)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    out = net.predict_fused(batch)
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
    del out
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0 and net._net is None and net._opt is None
    # the parent's code path, restated: the input launch, ops.dense_fwd on the K-contiguous copies, ops.head_predict
    h, wide = net.input_row(batch)
    for i in range(2):
        h = ops.dense_fwd(h, net._w16[i], net.params[f"dense_layer_{i + 1}.bias"], relu=True, wt=net._wt16[i])
    o = ops.head_predict(h, net.params["deep_predict.weight"].view(-1), net.params["deep_predict.bias"], wide=wide)
    assert torch.equal(o[0].view(B, 1), ref[0]) and torch.equal(o[1].view(B, 1), ref[1])
    # a net the mixin has no step for: refused before any state exists
    odd = MultiTableWideDeep(dataclasses.replace(make_cfg("fp16"), deep_dims=(12, 8)))
    with pytest.raises(UnsupportedNet):
        odd.train_step(batch, batch["label"])
    assert odd._net is None and odd._opt is None
    # no continuous values: wide_bias would go untrained -- refused as well
    nocont = MultiTableWideDeep(dataclasses.replace(make_cfg("fp16"), n_continue=0))
    with pytest.raises(UnsupportedNet):
        nocont.train_step({k: v for k, v in batch.items() if k != "continue_val"}, batch["label"])
    assert nocont._net is None and nocont._opt is None


def test_e_long_groups_in_the_step():
    """B = 4096: the 16 rows of emb64_indicator hold about 512 positions each and the 30 of emb64_multi about 2900 -- every group longer
    than MREC_MT_BWD_CHUNK, beginning anywhere inside a window of the sorted index, as at the reference's batch size.  The sums the step's
    backward launch leaves against the float64 restatement on the step's own g_x and g_wide, within its first-order bound; then the
    step trains."""
    import _multitable_bwd_cases as K
    import _multitable_bwd_ref as BR
    Bb = 4096
    assert Bb * 2 // VOCAB["indicator"] > K.chunk_len()
    net, batch = model("fp16"), dev_batch(Bb)
    g = net._backward(batch, batch["label"])
    segs, K0 = R.model_segments(named_params(), batch_np(Bb))
    gx, gw = g["g_x"].float().cpu().numpy(), g["g_wide"].cpu().numpy()
    parts = [segs[0:1], segs[1:2], segs[2:3], segs[3:]]
    for (table, w, plan, sums, wsums), sg in zip(g["groups"], parts):
        uniq, rs, rb, rw, rwb = BR.group_sums(gx, gw, sg, 1.0 / net.cfg.sens)
        U = plan.U
        assert U == uniq.size and np.array_equal(plan.uniq.cpu().numpy(), uniq)
        err, werr = np.abs(sums[:U].cpu().numpy() - rs), np.abs(wsums[:U].cpu().numpy() - rw)
        print(f"{table}: U={U} max err/bound deep {float((err / np.maximum(rb, 1e-300)).max()):.3f} wide {float((werr / np.maximum(rwb, 1e-300)).max()):.3f}")
        assert (err <= rb).all() and (werr <= rwb).all(), table
    d, bd, b, bb = BR.cont_grads(gw, batch_np(Bb)["continue_val"], 1.0 / net.cfg.sens)
    assert (np.abs(g["d_wide_cont"].cpu().numpy() - d) <= bd).all() and abs(float(g["d_wide_bias"].cpu()[0]) - b) <= bb
    losses = [float(l) for l in net.train([dict(batch)] * 3)]
    print(f"B = {Bb} losses: {losses}")
    assert losses[2] < losses[0]
