"""WideDeepEngine.q8_predictor() / serving.WideDeepQ8Predictor.  (b)'s yardstick is the engine's own predict_fused: the same launches
behind a lookup that rounds x * wt once, so against a float64 forward over ITS table (the records dequantized as include/mrec.h defines
it: an fp32 multiply, an fp32 add) the predictor's largest logit error over the batch may be at most twice the engine's over the fp32
table -- 2 for different inputs reaching different roundings.  How far q8 predictions sit from fp32 ones is data: printed only."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cfg(dt, layers, B, D, **over):
    from mindrec_amd.wide_deep import WideDeepConfig
    return WideDeepConfig(**{**dict(vocab_size=1000, emb_dim=D, field_size=5, batch_size=B, deep_layer_dim=layers, mlp_dtype=dt,
                                    graphs="none"), **over})


def _forward64(table, wide, wide_b, dense, ids, wts):
    """float64 logit [B]: sum_f wide[id] wt + wide_b + DenseLayers(table[ids] * wt), ReLU on all but the last"""
    ids, wts = ids.long().cpu(), wts.double().cpu()
    h = (table.double().cpu()[ids] * wts[..., None]).reshape(ids.shape[0], -1)
    for i in range(len(dense) // 2):
        h = h @ dense[2 * i].detach().double().cpu() + dense[2 * i + 1].detach().double().cpu()
        h = torch.relu(h) if i < len(dense) // 2 - 1 else h
    return h.view(-1) + (wide.double().cpu().view(-1)[ids] * wts).sum(dim=1) + float(wide_b)


def _bits(ts):
    return [t.detach().contiguous().view(-1).view(torch.int32).clone() for t in ts]


@pytest.mark.parametrize("D", [16, 80])
@pytest.mark.parametrize("B", [70, 256])
@pytest.mark.parametrize("dt,layers", [("fp16", [64, 32]), ("fp32", [64, 32]), ("fp16", [512, 256, 128])], ids=["fp16", "fp32", "fp16-tail"])
def test_q8_predictor(dev, dt, layers, B, D):
    from mindrec_amd import ops
    from mindrec_amd.wide_deep import WideDeepEngine, synthetic_batch
    from mindrec_amd.wide_deep_mlp import _WideProd
    cfg = _cfg(dt, layers, B, D)
    e = WideDeepEngine(cfg, dev)
    for s in range(2):
        e.train_step(*synthetic_batch(cfg, dev, "uniform", seed=10 + s, signal=True))
    p = e.q8_predictor()
    assert p.q8.row_bytes == ops.q8_row_bytes(D) and p.net.dense_m is None and e._tail_eval == (len(layers) == 3)
    ids, wts, label = synthetic_batch(cfg, dev, "uniform", seed=99, signal=True)
    out = p.predict_fused(ids, wts, label)
    assert [tuple(t.shape) for t in out] == [(B, 1), (B, 1), ()]
    got = _bits(out)
    # (a) the wiring: the engine's own evaluation launches fed by the dequantizing lookup
    rows, wprod = ops.gather_rows_q8(p.q8, ids, wts, out_dtype=e._amp if e._mfma else torch.float32)
    want = _bits(e.mlp_predict(rows.view(B, -1), _WideProd(wprod), label))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(_bits(p.predict_fused(ids, wts)), got[:2]))
    # (b) against float64 forwards: the engine's error over its fp32 table is the yardstick
    rec = p.q8.records.cpu()
    hdr = rec[:, :12].contiguous().view(torch.float32)
    deq = hdr[:, 0:1] + rec[:, 16:16 + D].float() * hdr[:, 1:2]
    le, pe = [t.clone() for t in e.predict_fused(ids, wts)]
    err_q = float((out[0].double().cpu().view(-1) - _forward64(deq, hdr[:, 2], e.wide_b, p.net.dense, ids, wts)).abs().max())
    err_e = float((le.double().cpu().view(-1) - _forward64(e.deep, e.wide, e.wide_b, e.dense, ids, wts)).abs().max())
    print(f"  logit error q8 {err_q:.3e} engine {err_e:.3e}; max |prob_q8 - prob_fp32| {float((out[1] - pe).abs().max()):.3e}")
    assert err_q <= 2 * err_e, (err_q, err_e)
    # (c) the predictor no longer depends on the engine
    e.train_step(*synthetic_batch(cfg, dev, "uniform", seed=12, signal=True))
    assert all(torch.equal(a, b) for a, b in zip(_bits(p.predict_fused(ids, wts, label)), got))
    e.close()


@pytest.mark.parametrize("over,kw,what", [(dict(max_norm=1.0), {}, "max_norm"),
                                          (dict(dynamic_embedding=True, hash_capacity=1 << 12), {}, "dynamic_embedding"),
                                          (dict(vocab_size=20_000, host_cache_rows=8192), {}, "host cache"),
                                          ({}, dict(shard_protocol=True), "row shards"),
                                          (dict(emb_dim=260, mlp_dtype="fp32"), {}, "emb_dim")])
def test_q8_predictor_refusals(dev, over, kw, what):
    from mindrec_amd.wide_deep import WideDeepEngine
    e = WideDeepEngine(_cfg("fp16", [64, 32], 64, 16, **over), dev, **kw)
    with pytest.raises(ValueError, match="q8_predictor is not supported with .*" + what):
        e.q8_predictor()
    e.release_graphs()
