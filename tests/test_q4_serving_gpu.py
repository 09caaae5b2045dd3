"""4-bit records behind the serving classes.  DeepFMEngine.q8_predictor(bits=4): test_q8_deepfm_predict_gpu.py's checks over ops.fm_lookup_q4 --
(a) the wiring, (b) the lookup against ops.fm_lookup over the records dequantized on the host (rows bit for bit, lin_fm within twice
test_q8_fm_gpu.py's bound), (c) independence from the engine.  freeze_q8(bits=4): test_q8_multihot_gpu.py's checks, 15 codes for 255."""
import numpy as np
import pytest
import torch

from test_q8_deepfm_predict_gpu import F, _bits, _engine
from test_q8_multihot_gpu import BAG, B as BM
from test_q8_rows_gpu import V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D", [16, 80])
@pytest.mark.parametrize("B", [70, 256])
@pytest.mark.parametrize("dt,layers", [("fp16", [64, 32]), ("fp32", [64, 32]), ("fp16", [512, 256, 128])], ids=["fp16", "fp32", "fp16-tail"])
def test_deepfm_q4_predictor(dev, dt, layers, B, D):
    from mindrec_amd import ops
    e, batch = _engine(dev, dt, layers, B, D)
    for s in range(2):
        e.train_step(*batch(10 + s))
    p = e.q8_predictor(bits=4)
    assert p.q8.bits == 4 and p.q8.row_bytes == ops.q4_row_bytes(D) and p.net.dense_m is None
    ids, wts, label = batch(99)
    out = p.predict_fused(ids, wts, label)
    got, row_dt = _bits(out), e._amp if e._mfma else torch.float32
    rows, lin_fm = ops.fm_lookup_q4(p.q8, ids, wts, out_dtype=row_dt)                                  # (a)
    want = _bits(e.mlp_predict(rows.view(B, -1), lin_fm, label))
    assert all(torch.equal(a, b) for a, b in zip(got + got[:2], want + _bits(p.predict_fused(ids, wts))))
    rec, ic, w = p.q8.records.cpu(), ids.long().cpu(), wts.cpu()                                       # (b)
    hdr, nib = rec[:, :12].contiguous().view(torch.float32), rec[:, 16:16 + D // 2]
    deq = hdr[:, 0:1] + torch.stack([nib & 15, nib >> 4], dim=2).reshape(-1, D).float() * hdr[:, 1:2]
    rows32, lin32 = ops.fm_lookup(deq.to(dev), hdr[:, 2:3].contiguous().to(dev), ids, wts, out_dtype=row_dt)
    assert torch.equal(rows32.view(torch.uint8), rows.view(torch.uint8))
    y, lin = (deq[ic] * w[..., None]).double(), (hdr[:, 2][ic] * w).double()
    bound = (2 * F + D + 4) * 2.0 ** -24 * (0.5 * (y.abs().sum(dim=1) ** 2 + (y ** 2).sum(dim=1)).sum(dim=1) + lin.abs().sum(dim=1))
    err, pe = (lin_fm.double() - lin32.double()).abs().cpu(), e.predict_fused(ids, wts)[1]
    print(f"  worst |lin_fm q4 - fp32| / bound {float((err / bound).max()):.3f}; max |prob_q4 - prob_fp32| {float((out[1] - pe).abs().max()):.3e}")
    assert bool((err <= 2 * bound).all())
    e.train_step(*batch(12))                                                                           # (c)
    assert all(torch.equal(a, b) for a, b in zip(_bits(p.predict_fused(ids, wts, label)), got))


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("D", [64, 80])
def test_wide_deep_freeze_q4(dev, D, mode):
    from mindrec_amd import multi_hot, ops
    pair = multi_hot.MultiHotWideDeep(vocab=V, dim=D, bag=BAG, mode=mode, device=dev)
    rng = np.random.default_rng(D)
    ids, mask = rng.integers(0, V, size=(BM, sum(BAG))).astype(np.int32), rng.random((BM, sum(BAG))).astype(np.float32)
    tids, tmask, frozen = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), pair.freeze_q8(bits=4)
    (x, w), x0 = frozen.lookup(tids, tmask), pair.lookup(tids, tmask)[0]
    want = ops.gather_pool_fields_q4(ops.quantize_rows_q4(pair.deep.table, pair.wide.table), tids, BAG, tmask, mode=mode, wide=True)
    assert torch.equal(x.view(torch.int32), want[0].view(torch.int32)) and torch.equal(w.view(torch.int32), want[1].view(torch.int32))
    hdr = np.ascontiguousarray(frozen.q8.records.cpu().numpy()[:, :12]).view(np.float32).astype(np.float64)
    m, off = mask.astype(np.float64), np.concatenate([[0], np.cumsum(BAG)])
    bound = np.stack([(0.5 * (1 + 2.0 ** -12) * (m * hdr[ids, 1])[:, off[f]:off[f + 1]].sum(axis=1)
                       + (L + 5) * 2.0 ** -24 * (m * (np.abs(hdr[ids, 0]) + 15.0 * hdr[ids, 1]))[:, off[f]:off[f + 1]].sum(axis=1))
                      / (L if mode == "mean" else 1) for f, L in enumerate(BAG)], axis=1)
    err = np.abs((x.double() - x0.double()).cpu().numpy()).reshape(BM, len(BAG), D).max(axis=2)
    print("  worst |x_q4 - x_fp32| / bound", float((err / bound).max()))
    assert np.all(err <= bound)


def test_bits_and_code_widths_are_checked(dev):
    from mindrec_amd import multi_hot, ops
    ids, wts, table = torch.zeros((8, 2), dtype=torch.int32, device=dev), torch.ones((8, 2), device=dev), torch.zeros((V, 80), device=dev)
    other = {4: ops.quantize_rows_q8(table), 8: ops.quantize_rows_q4(table)}           # the table a lookup of that code width refuses
    for width, fm, pool in [(4, ops.fm_lookup_q4, ops.gather_pool_fields_q4), (8, ops.fm_lookup_q8, ops.gather_pool_fields_q8)]:
        for call in (lambda: fm(other[width], ids, wts), lambda: pool(other[width], ids, (2,))):
            with pytest.raises(TypeError, match=f"{width}-bit records"):
                call()
    for freeze in (_engine(dev, "fp16", [64, 32], 64, 16)[0].q8_predictor, multi_hot.MultiHotWideDeep(vocab=V, dim=64, bag=(2, 3), device=dev).freeze_q8):
        with pytest.raises(ValueError, match="bits must be 8 or 4"):
            freeze(bits=5)
