"""ops.tail_predict (mrec_tail_predict: the last two hidden DenseLayers and the evaluation head in ONE launch; csrc/mrec_tail.hip
k_tail_predict) against the three launches it replaces -- ops.dense_fwd, ops.dense_fwd, ops.head_predict, which are the ones checked
against the oracle (tests/test_dense_gpu.py, test_head_predict_gpu.py).  Same products in the same order and the head's lane geometry
at K5 = 128: logit and prob must be IDENTICAL, at every batch size (whole tiles of 64 rows, ragged last tiles, one row), in both
forms of the wide branch and with x a view of a wider buffer.  The loss is a sum over other partial groupings than head_predict's: it
is held to float64 binary_cross_entropy_with_logits of the returned logits within 1e-5 relative (test_predict_fused_gpu.py's tolerance
for this quantity) and to itself bit for bit across runs.  Inputs: the distributions of tests/test_tail_gpu.py (its builder, copied)
and the exact integer family of tests/_tail_cases.py, on which the logit equals the float64 value bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

T16 = {"bf16": torch.bfloat16, "f16": torch.float16}
K2, N2, N3 = 512, 256, 128
SENTINEL = -77.0


def _inputs(dev, dt, B, seed, F=0):
    """tests/test_tail_gpu.py::_inputs"""
    rng = np.random.default_rng(seed)
    t16 = T16[dt]
    x = torch.from_numpy(np.maximum(rng.standard_normal((B, K2)), 0).astype(np.float32)).to(dev).to(t16)     # a ReLU output
    w2 = torch.from_numpy((rng.standard_normal((K2, N2)) * 0.06).astype(np.float32)).to(dev).to(t16)
    w3 = torch.from_numpy((rng.standard_normal((N2, N3)) * 0.08).astype(np.float32)).to(dev).to(t16)
    b2 = torch.from_numpy((rng.standard_normal(N2) * 0.1).astype(np.float32)).to(dev)
    b3 = torch.from_numpy((rng.standard_normal(N3) * 0.1).astype(np.float32)).to(dev)
    w5 = torch.from_numpy((rng.standard_normal(N3) * 0.1).astype(np.float32)).to(dev)
    b5 = torch.from_numpy(rng.standard_normal(1).astype(np.float32) * 0.1).to(dev)
    label = torch.from_numpy((rng.random(B) < 0.3).astype(np.float32)).to(dev)
    if F:
        wide = torch.zeros((B, F, 2), dtype=torch.float32, device=dev)
        wide[:, :, 0] = torch.from_numpy((rng.standard_normal((B, F)) * 0.05).astype(np.float32)).to(dev)
        wb = torch.from_numpy(rng.standard_normal(1).astype(np.float32) * 0.1).to(dev)
    else:
        wide = torch.from_numpy((rng.standard_normal(B) * 0.2).astype(np.float32)).to(dev)
        wb = None
    return x, w2, b2, w3, b3, w5, b5, wide, wb, label


def _view(x, pad):
    """x as a window of a NaN-filled buffer [B + 1, K2 + pad]: row stride K2 + pad, one more row behind the last"""
    buf = torch.full((x.shape[0] + 1, K2 + pad), float("nan"), dtype=x.dtype, device=x.device)
    buf[:-1, :K2] = x
    v = buf[:-1, :K2]
    assert v.stride(0) == K2 + pad or x.shape[0] == 1
    return v


def _bits(t):
    return t.contiguous().view(torch.int32)


def _chain(ops, x, w2, b2, w3, b3, w5, b5, wide, wb, label):
    """the three launches: (logit, prob, loss)"""
    y2 = ops.dense_fwd(x, w2, b2, relu=True)
    y3 = ops.dense_fwd(y2, w3, b3, relu=True)
    prod = wide.dim() == 3
    return ops.head_predict(y3, w5, b5, wide=None if prod else wide, wide_prod=wide if prod else None, wide_bias=wb, label=label)


def _check(dev, dt, B, F, pad):
    from mindrec_amd import ops
    x, w2, b2, w3, b3, w5, b5, wide, wb, label = _inputs(dev, dt, B, seed=1000 * B + F, F=F)
    x = _view(x, pad)
    assert ops.tail_predict_supported(B, K2, N2, N3)
    logit, prob, loss = _chain(ops, x, w2, b2, w3, b3, w5, b5, wide, wb, label)
    packed = ops.tail_pack_weights(w2, w3)
    # outputs longer than B, filled with a sentinel: the rows of a ragged last tile at or past B store nothing
    n_out = (B + 63) // 64 * 64 + 64
    out = {"logit": torch.full((n_out,), SENTINEL, device=dev), "prob": torch.full((n_out,), SENTINEL, device=dev)}
    tl, tp, tloss = ops.tail_predict(x, packed, b2, b3, w5, b5, wide, wide_bias=wb, label=label, out=out)
    torch.cuda.synchronize()
    assert tl.shape == (B,) and tp.shape == (B,) and tloss.shape == (1,)
    assert tl.data_ptr() == out["logit"].data_ptr() and tp.data_ptr() == out["prob"].data_ptr() and out["loss"] is tloss
    assert torch.equal(_bits(tl), _bits(logit)), ("logit", int((_bits(tl) != _bits(logit)).sum()))
    assert torch.equal(_bits(tp), _bits(prob)), ("prob", int((_bits(tp) != _bits(prob)).sum()))
    assert bool((out["logit"][B:] == SENTINEL).all()) and bool((out["prob"][B:] == SENTINEL).all()), "rows at or past B were written"
    ref = float(torch.nn.functional.binary_cross_entropy_with_logits(tl.double(), label.double()))
    print(f"  B {B} F {F} pad {pad} {dt}: loss {float(tloss)!r} float64 {ref!r} head_predict {float(loss)!r}")
    assert abs(float(tloss) - ref) <= 1e-5 * abs(ref), (float(tloss), ref)
    # the unlabelled call (one launch, no workspace): the same logit and prob bits
    ul, up = ops.tail_predict(x, packed, b2, b3, w5, b5, wide, wide_bias=wb)
    assert torch.equal(_bits(ul), _bits(logit)) and torch.equal(_bits(up), _bits(prob))
    # a second labelled run: the same loss bits
    first = _bits(tloss).clone()
    _, _, again = ops.tail_predict(x, packed, b2, b3, w5, b5, wide, wide_bias=wb, label=label)
    assert torch.equal(_bits(again), first)


# batch sizes: one row, a tile less one, a tile, a tile and one row, 3 tiles and 17 rows, 9 workgroups (finish_column's chunk goes
# 1 -> 2); wide forms: per sample (F = 0) and the edges of the field loader's four 16-lane quads; x's row stride 512 + {0, 8, 24}
CASES = [(1, 0, 0), (1, 64, 24), (63, 1, 8), (64, 16, 24), (65, 17, 0), (65, 0, 8), (209, 33, 8), (209, 0, 24), (576, 64, 24), (576, 0, 0)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("B,F,pad", CASES, ids=[f"B{b}-F{f}-pad{p}" for b, f, p in CASES])
def test_tail_predict_equals_the_three_launches(dev, dt, B, F, pad):
    _check(dev, dt, B, F, pad)


def test_tail_predict_at_65_workgroups(dev):
    _check(dev, "f16", 4160, 26, 8)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_exact_family_equals_float64(dev, oracle, dt):
    """the "int" inputs of tests/_tail_cases.py: every 16-bit value an integer, every fp32 partial sum exact in any order -- the logit is
    the float64 value bit for bit, in the whole batch of 128 and when its first 100 rows are a batch of their own (a ragged tile)"""
    import _tail_cases as T
    from mindrec_amd import ops
    case = T.BY_NAME["int"]
    inp = T.inputs(oracle, case, dt)
    f64 = lambda a: np.asarray(a, np.float64)      # noqa: E731
    y2 = np.maximum(f64(inp["x"]) @ f64(inp["w2"]) + f64(inp["b2"])[None, :], 0.0)
    y3 = np.maximum(y2 @ f64(inp["w3"]) + f64(inp["b3"])[None, :], 0.0)
    assert np.abs(y2).max() <= 256 and np.abs(y3).max() <= 256          # exact in both 16-bit formats
    z = y3 @ f64(inp["w5"]) + float(inp["b5"][0]) + f64(inp["wide"][:, :, 0]).sum(1) + float(inp["wb"])
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    x = _view(t(inp["x"]).to(T16[dt]), case.pad)
    packed = ops.tail_pack_weights(t(inp["w2"]).to(T16[dt]), t(inp["w3"]).to(T16[dt]))
    wide, wb, label = t(inp["wide"]), t(np.float32([inp["wb"]])), t(inp["label"])
    for B in (case.B, 100):
        logit, prob, loss = ops.tail_predict(x[:B], packed, t(inp["b2"]), t(inp["b3"]), t(inp["w5"]), t(inp["b5"]), wide[:B].contiguous(),
                                             wide_bias=wb, label=label[:B])
        got = logit.cpu().numpy()
        assert np.array_equal(got.view(np.int32), z[:B].astype(np.float32).view(np.int32)), (B, float(np.abs(got - z[:B]).max()))
        assert np.allclose(prob.cpu().numpy(), 1.0 / (1.0 + np.exp(-z[:B])), rtol=1e-4, atol=1e-7)      # (test_predict_fused_gpu.py's)
        ref = float(torch.nn.functional.binary_cross_entropy_with_logits(torch.from_numpy(z[:B]), torch.from_numpy(f64(inp["label"][:B]))))
        assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (B, float(loss), ref)


def test_python_side_refusals(dev):
    from mindrec_amd import ops
    x, w2, b2, w3, b3, w5, b5, wide, wb, label = _inputs(dev, "bf16", 64, seed=5, F=3)
    packed = ops.tail_pack_weights(w2, w3)
    refused = (ValueError, TypeError)
    big = torch.zeros((32832, K2), dtype=torch.bfloat16, device=dev)
    assert not ops.tail_predict_supported(32832, K2, N2, N3)
    with pytest.raises(refused):
        ops.tail_predict(big, packed, b2, b3, w5, b5, torch.zeros(32832, device=dev))
    with pytest.raises(refused):                           # other widths
        ops.tail_predict(x[:, :256], packed, b2, b3, w5, b5, wide, wide_bias=wb)
    with pytest.raises(refused):
        ops.tail_predict(x, packed, b2[:128].contiguous(), b3, w5, b5, wide, wide_bias=wb)
    with pytest.raises(refused):                           # F = 65
        ops.tail_predict(x, packed, b2, b3, w5, b5, torch.zeros((64, 65, 2), device=dev), wide_bias=wb)
    with pytest.raises(refused):                           # products without the bias
        ops.tail_predict(x, packed, b2, b3, w5, b5, wide)
    with pytest.raises(refused):                           # packed in another dtype
        ops.tail_predict(x, packed.to(torch.float16), b2, b3, w5, b5, wide, wide_bias=wb)
    with pytest.raises(refused):                           # an output buffer shorter than the batch
        ops.tail_predict(x, packed, b2, b3, w5, b5, wide, wide_bias=wb, out={"logit": torch.empty(63, device=dev)})
    with pytest.raises(refused):                           # a label of another length
        ops.tail_predict(x, packed, b2, b3, w5, b5, wide, wide_bias=wb, label=label[:63])
    logit, prob = ops.tail_predict(x, packed, b2, b3, w5, b5, wide, wide_bias=wb)          # the well-formed call runs
    assert bool(torch.isfinite(logit).all()) and bool(((prob > 0) & (prob < 1)).all())
