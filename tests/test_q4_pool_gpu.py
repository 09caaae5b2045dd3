"""ops.gather_pool_fields_q4 (k_q4_gather_pool_fields) against float64 over the records' own fields read back from the device:
ref = sum_s m_s (lo_s + code_sd scale_s) / (L_f or 1) per field, under test_q8_pool_gpu.py's derived bounds with 15 codes for 255:
|got - ref| <= (L_f + 5) u S / (L_f or 1) + u_out |ref|, S = sum_s |m_s| (|lo_s| + 15 scale_s); |w - ref| <= (Ls + 2) u sum_s |m_s wide_s|."""
import numpy as np
import pytest
import torch

from test_q4_rows_gpu import _records
from test_q8_rows_gpu import PADDED, U, V

pytestmark = pytest.mark.gpu
B = 67                  # the last wave holds a partial set of lane-groups at every D
FIELDS = [(1,), (4,), (5,), (9,), (3, 5, 4, 3, 4, 2), (1, 1, 1)]      # a lone slot, one batch of four, a partial second, a third, seams inside a batch, single-hot


@PADDED
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("fields", FIELDS, ids=lambda f: "x".join(map(str, f)))
@pytest.mark.parametrize("D", [4, 12, 20, 28, 32, 36, 80, 252, 256])
def test_gather_pool_fields_q4(dev, D, fields, mode, padded):
    from mindrec_amd import ops
    q4, lo, scale, wide, code = _records(dev, D, False, padded)
    F, Ls, rng = len(fields), sum(fields), np.random.default_rng(100 + sum(fields))
    ids, mask = rng.integers(0, V, size=(B, Ls)), rng.random((B, Ls)).astype(np.float32)
    ids[1] = [(-1, V)[k % 2] for k in range(Ls)]           # a sample with no id in range
    ids[2:6, 0], ids[B - 1, Ls - 1], mask[6, 0] = [0, 66, -1, V], 66, 0.0
    ic, m = np.where(ok := (ids >= 0) & (ids < V), ids, 0), np.where(ok, mask, 0).astype(np.float64)
    term = m[..., None] * (lo[ic].astype(np.float64)[..., None] + code[ic].astype(np.float64) * scale[ic].astype(np.float64)[..., None])
    S, gw = m * (np.abs(lo[ic]).astype(np.float64) + 15.0 * scale[ic]), m * wide[ic].astype(np.float64)
    off, den = np.concatenate([[0], np.cumsum(fields)]), [float(L) if mode == "mean" else 1.0 for L in fields]
    ref = np.concatenate([term[:, off[f]:off[f + 1]].sum(axis=1) / den[f] for f in range(F)], axis=1)
    arith = np.repeat(np.stack([(fields[f] + 5) * 2.0 ** -24 * S[:, off[f]:off[f + 1]].sum(axis=1) / den[f] for f in range(F)], axis=1), D, axis=1)
    wref, wbound = gw.sum(axis=1), (Ls + 2) * 2.0 ** -24 * np.abs(gw).sum(axis=1)
    tids, tmask, x32, wbits = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), None, None
    for dt, idt in [(k, torch.int32) for k in U] + [(torch.float32, torch.int64)] * (D == 80):
        x, w = ops.gather_pool_fields_q4(q4, tids.to(idt), fields, tmask, mode=mode, out_dtype=dt, wide=True)
        err, werr = np.abs(x.double().cpu().numpy() - ref), np.abs(w.double().cpu().numpy() - wref)
        bound = arith + U[dt] * np.abs(ref) + (2.0 ** -25 if dt == torch.float16 else 0.0)
        assert np.all(err <= bound) and np.all(werr <= wbound)
        assert not x[1].float().any() and float(w[1]) == 0, "a sample with every id out of range: a zero row, w 0"
        x32, wbits = (x, w) if x32 is None else (x32, wbits)
        assert torch.equal(x.view(torch.uint8), x32.to(dt).view(torch.uint8)), "not the fp32 row rounded once to nearest even / depends on the id width"
        assert torch.equal(w.view(torch.int32), wbits.view(torch.int32)), "w depends on the output kind or the id width"
    ones = ops.gather_pool_fields_q4(q4, tids.int(), fields, torch.ones_like(tmask), mode=mode, wide=True)
    none = ops.gather_pool_fields_q4(q4, tids.int(), fields, None, mode=mode, wide=True)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ones, none)), "mask=None is not a mask of ones"
    big, wbig = torch.full((B, F * D + 8), 7.0, dtype=torch.float16, device=dev), torch.full((B, 3), 7.0, device=dev)
    ops.gather_pool_fields_q4(q4, tids.int(), fields, tmask, mode=mode, out=big[:, 4:4 + F * D], wide=True, wide_out=wbig[:, 1])
    assert torch.equal(big[:, 4:4 + F * D], x32.half()) and torch.equal(wbig[:, 1], wbits), "a column block (8-byte aligned only), a strided wide column"
    assert bool((big[:, :4] == 7.0).all()) and bool((big[:, 4 + F * D:] == 7.0).all()) and bool((wbig[:, ::2] == 7.0).all()), "other columns touched"
