"""DeepFMHashEngine.q8_predictor(): (a) the evaluation launches behind the keyed lookup; (b) frozen model against engine on seen keys, within
the bound of the records' quantization step; (c) an unseen key: a zero row, no insert; (d) independence from the engine; (e) refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B, F = 48, 5


def _engine(dev, dt="fp16", D=16, **kw):
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMHashEngine
    cfg = DeepFMConfig(data_emb_dim=D, data_field_size=F, batch_size=B, deep_layer_dims=[64, 32], learning_rate=1e-2, mlp_dtype=dt, graphs="none")
    return DeepFMHashEngine(cfg, dev, key_dtype=torch.int64, capacity=1 << 12, **kw)


def _batch(dev, seed, pool=300):
    g = torch.Generator().manual_seed(seed)
    pool_keys = torch.randint(1, 2 ** 40, (600,), generator=torch.Generator().manual_seed(5))
    keys = pool_keys[torch.randint(0, pool, (B, F), generator=g)]
    return keys.to(dev), torch.rand((B, F), generator=g).to(dev), torch.randint(0, 2, (B, 1), generator=g).float().to(dev)


def _bits(ts):
    return [t.detach().contiguous().view(-1).view(torch.int32).clone() for t in ts]


def _prob_bound(p, keys, wts, bits, sixteen):
    """|prob_frozen - prob_engine| <= bound.  A dequantized value is within scale / 2 of the fp32 one: y = x t moves by at most e = t scale / 2
    (the first-order weight is exact).  FM: 0.5 sum_d (s_d^2 - q_d) moves by at most sum_d (|s_d| ds_d + ds_d^2 / 2 + sum_f (|y| e + e^2 / 2)),
    ds_d = sum_f e.  Net: ReLU is 1-Lipschitz, a difference d travels as d |W|; both sides round rows and activations to 16 bits (eps 2^-10 the
    pair) and sum K terms in fp32 (K 2^-23), relative to the magnitudes a |W| + |b|.  The sigmoid's slope is at most 1 / 4."""
    rec, D = p.q8.records, p.q8.D
    hdr = rec[:, :12].contiguous().view(torch.float32).double()
    r = p.kidx.find(keys).long()
    t = wts.double()[..., None]
    e = (t * hdr[r, 1:2].view(B, F, 1) / 2).expand(B, F, D)
    code = rec[:, 16:].long()
    code = (torch.stack([code & 15, code >> 4], dim=2).reshape(rec.shape[0], -1) if bits == 4 else code)[:, :D].double()
    y = (hdr[:, 0:1] + code * hdr[:, 1:2])[r] * t
    ds = e.sum(dim=1)
    dfm = ((y.sum(dim=1).abs() + ds) * ds + ds ** 2 / 2 + (y.abs() * e + e ** 2 / 2).sum(dim=1)).sum(dim=1)
    eps = (2.0 ** -10 if sixteen else 0.0) + max(p.net.dims) * 2.0 ** -23
    a, d = y.abs().reshape(B, -1), e.reshape(B, -1) + eps * y.abs().reshape(B, -1)
    for i in range(len(p.net.dims) - 1):
        W, b = p.net.dense[2 * i].detach().double().abs(), p.net.dense[2 * i + 1].detach().double().abs()
        a = a @ W + b
        d = d @ W + eps * a
    fm_mag = 0.5 * (y.abs().sum(dim=1) ** 2 + (y ** 2).sum(dim=1)).sum(dim=1) + (hdr[r, 2] * wts.double()).abs().sum(dim=1)
    return 0.25 * (d[:, 0] + dfm + eps * (fm_mag + a[:, 0]))


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("D", [16, 80])
@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_hash_q8_predictor(dev, dt, D, bits):
    from mindrec_amd import ops
    e = _engine(dev, dt, D, permit_filter_value=2)
    for s in range(2):
        e.train_step(*_batch(dev, 10 + s))
    p = e.q8_predictor(bits=bits)
    n = len(e.V)
    assert p.q8.bits == bits and p.q8.V == p.kidx.n == n and p.net.dense_m is None and not hasattr(p, "engine")
    assert int((e.V.hits[: n] < 2).sum()) > 0, "the model holds no un-admitted key"
    keys, wts, label = _batch(dev, 11)                                                                  # seen keys only
    out = p.predict_fused(keys, wts, label)
    got = _bits(out)
    lookup = ops.fm_lookup_q4_keyed if bits == 4 else ops.fm_lookup_q8_keyed
    rows, lin_fm = lookup(p.q8, p.kidx, keys, wts, out_dtype=e._amp if e._mfma else torch.float32)     # (a)
    assert all(torch.equal(x, y) for x, y in zip(got, _bits(p.net.mlp_predict(rows.view(B, -1), lin_fm, label))))
    err = (out[1].double() - e.predict_fused(keys, wts)[1].double()).abs().view(B)                      # (b)
    bound = _prob_bound(p, keys, wts, bits, e._mfma)
    print(f"  worst |prob_q{bits} - prob_engine| {float(err.max()):.3e}, worst ratio to the bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()) and len(e.V) == n
    unseen = keys.clone()                                                                               # (c)
    unseen[:, 0] = -(2 ** 50) - torch.arange(B, device=dev)
    p.predict_fused(unseen, wts)
    assert len(e.V) == n and not bool(lookup(p.q8, p.kidx, unseen, wts)[0][:, 0].any())
    e.train_step(*_batch(dev, 12, pool=600))                                                            # (d)
    assert all(torch.equal(x, y) for x, y in zip(_bits(p.predict_fused(keys, wts, label)), got))


@pytest.mark.parametrize("kw,bits,D,world,why", [(dict(max_norm=1.0), 8, 16, 1, "max_norm"), ({}, 5, 16, 1, "bits"), ({}, 8, 260, 1, "data_emb_dim"),
                                                  ({}, 8, 16, 2, "key shards"), ({}, 8, 16, 1, "an empty model")], ids=lambda v: str(v)[:12])
def test_hash_q8_predictor_refusals(dev, kw, bits, D, world, why):                                      # (e)
    e = _engine(dev, "fp32", D, **kw)
    e.world = world
    with pytest.raises(ValueError, match="q8_predictor is not supported with " + why):
        e.q8_predictor(bits=bits)
