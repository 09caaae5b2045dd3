"""WideDeepEngine.q8_predictor(bits=4): serving.WideDeepQ8Predictor over row-wise 4-bit records, at tests/test_q8_predict_gpu.py's shapes and
by its yardstick -- against a float64 forward over ITS table (the records dequantized as include/mrec.h defines it) the predictor's largest
logit error may be at most twice the engine's own over the fp32 table.  How far 4-bit predictions sit from fp32 ones is data: printed."""
import pytest
import torch
from test_q8_predict_gpu import _bits, _cfg, _forward64

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D", [16, 80])
@pytest.mark.parametrize("B", [70, 256])
@pytest.mark.parametrize("dt,layers", [("fp16", [64, 32]), ("fp32", [64, 32]), ("fp16", [512, 256, 128])], ids=["fp16", "fp32", "fp16-tail"])
def test_q4_predictor(dev, dt, layers, B, D):
    from mindrec_amd import ops
    from mindrec_amd.wide_deep import WideDeepEngine, synthetic_batch
    from mindrec_amd.wide_deep_mlp import _WideProd
    cfg = _cfg(dt, layers, B, D)
    e = WideDeepEngine(cfg, dev)
    for s in range(2):
        e.train_step(*synthetic_batch(cfg, dev, "uniform", seed=10 + s, signal=True))
    p = e.q8_predictor(bits=4)
    assert p.q8.bits == 4 and p.q8.row_bytes == ops.q4_row_bytes(D) and p.net.dense_m is None
    with pytest.raises(ValueError, match="bits must be 8 or 4"):
        e.q8_predictor(bits=5)
    ids, wts, label = synthetic_batch(cfg, dev, "uniform", seed=99, signal=True)
    out = p.predict_fused(ids, wts, label)
    got = _bits(out)
    # (a) the wiring: the engine's own evaluation launches fed by the 4-bit lookup
    rows, wprod = ops.gather_rows_q4(p.q8, ids, wts, out_dtype=e._amp if e._mfma else torch.float32)
    assert all(torch.equal(a, b) for a, b in zip(got, _bits(e.mlp_predict(rows.view(B, -1), _WideProd(wprod), label))))
    assert all(torch.equal(a, b) for a, b in zip(_bits(p.predict_fused(ids, wts)), got[:2]))
    # (b) against float64 forwards: the engine's error over its fp32 table is the yardstick
    rec = p.q8.records.cpu()
    hdr, b = rec[:, :12].contiguous().view(torch.float32), rec[:, 16:16 + D // 2]
    deq = hdr[:, 0:1] + torch.stack([b & 15, b >> 4], dim=2).reshape(-1, D).float() * hdr[:, 1:2]
    le, pe = [t.clone() for t in e.predict_fused(ids, wts)]
    err_q = float((out[0].double().cpu().view(-1) - _forward64(deq, hdr[:, 2], e.wide_b, p.net.dense, ids, wts)).abs().max())
    err_e = float((le.double().cpu().view(-1) - _forward64(e.deep, e.wide, e.wide_b, e.dense, ids, wts)).abs().max())
    print(f"  logit error q4 {err_q:.3e} engine {err_e:.3e}; max |prob_q4 - prob_fp32| {float((out[1] - pe).abs().max()):.3e}")
    assert err_q <= 2 * err_e, (err_q, err_e)
    # (c) the predictor no longer depends on the engine
    e.train_step(*synthetic_batch(cfg, dev, "uniform", seed=12, signal=True))
    assert all(torch.equal(a, b) for a, b in zip(_bits(p.predict_fused(ids, wts, label)), got))
    e.close()
