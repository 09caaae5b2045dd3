"""DeepFMEngine.q8_predictor(): (a) the wiring -- the engine's own evaluation launches behind ops.fm_lookup_q8; (b) that lookup against the fp32
kernel ops.fm_lookup over the records dequantized on the host: both round the same fp32 x' * t once, so the rows agree bit for bit, and each
lin_fm lies within one bound of test_q8_fm_gpu.py of the exact value, the two within twice that; (c) independence from the engine."""
import pytest
import torch

pytestmark = pytest.mark.gpu
V, F = 1000, 5


def _engine(dev, dt, layers, B, D, **over):
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMEngine
    from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch
    cfg = dict(data_vocab_size=V, data_emb_dim=D, data_field_size=F, batch_size=B, deep_layer_dims=layers, mlp_dtype=dt, graphs="none")
    bcfg = WideDeepConfig(vocab_size=V, emb_dim=D, field_size=F, batch_size=B)
    return DeepFMEngine(DeepFMConfig(**{**cfg, **over}), dev), lambda seed: synthetic_batch(bcfg, dev, "uniform", seed=seed, signal=True)


def _bits(ts):
    return [t.detach().contiguous().view(-1).view(torch.int32).clone() for t in ts]


@pytest.mark.parametrize("D", [16, 80])
@pytest.mark.parametrize("B", [70, 256])
@pytest.mark.parametrize("dt,layers", [("fp16", [64, 32]), ("fp32", [64, 32]), ("fp16", [512, 256, 128])], ids=["fp16", "fp32", "fp16-tail"])
def test_q8_predictor(dev, dt, layers, B, D):
    from mindrec_amd import ops
    e, batch = _engine(dev, dt, layers, B, D)
    for s in range(2):
        e.train_step(*batch(10 + s))
    p = e.q8_predictor()
    assert p.q8.row_bytes == ops.q8_row_bytes(D) and p.net.dense_m is None
    ids, wts, label = batch(99)
    out = p.predict_fused(ids, wts, label)
    got, row_dt = _bits(out), e._amp if e._mfma else torch.float32
    rows, lin_fm = ops.fm_lookup_q8(p.q8, ids, wts, out_dtype=row_dt)                                  # (a)
    want = _bits(e.mlp_predict(rows.view(B, -1), lin_fm, label))
    assert all(torch.equal(a, b) for a, b in zip(got + got[:2], want + _bits(p.predict_fused(ids, wts))))
    rec, ic, w = p.q8.records.cpu(), ids.long().cpu(), wts.cpu()                                       # (b)
    hdr = rec[:, :12].contiguous().view(torch.float32)
    deq = hdr[:, 0:1] + rec[:, 16:16 + D].float() * hdr[:, 1:2]
    rows32, lin32 = ops.fm_lookup(deq.to(dev), hdr[:, 2:3].contiguous().to(dev), ids, wts, out_dtype=row_dt)
    assert torch.equal(rows32.view(torch.uint8), rows.view(torch.uint8))
    y, lin = (deq[ic] * w[..., None]).double(), (hdr[:, 2][ic] * w).double()
    bound = (2 * F + D + 4) * 2.0 ** -24 * (0.5 * (y.abs().sum(dim=1) ** 2 + (y ** 2).sum(dim=1)).sum(dim=1) + lin.abs().sum(dim=1))
    err, pe = (lin_fm.double() - lin32.double()).abs().cpu(), e.predict_fused(ids, wts)[1]
    print(f"  worst |lin_fm q8 - fp32| / bound {float((err / bound).max()):.3f}; max |prob_q8 - prob_fp32| {float((out[1] - pe).abs().max()):.3e}")
    assert bool((err <= 2 * bound).all())
    e.train_step(*batch(12))                                                                           # (c)
    assert all(torch.equal(a, b) for a, b in zip(_bits(p.predict_fused(ids, wts, label)), got))


@pytest.mark.parametrize("over", [dict(max_norm=1.0), dict(data_emb_dim=260, mlp_dtype="fp32")], ids=["max_norm", "emb_dim"])
def test_q8_predictor_refusals(dev, over):
    with pytest.raises(ValueError, match="q8_predictor is not supported with"):
        _engine(dev, "fp16", [64, 32], 64, 16, **over)[0].q8_predictor()
