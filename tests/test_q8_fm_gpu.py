"""ops.fm_lookup_q8 (k_q8_fm_lookup).  rows: ops.gather_rows_q8's bit for bit (test_q8_rows_gpu.py holds those to float64).  lin_fm against
float64 over y = (lo + code * scale) * t restated in numpy float32: |got - ref| <= (2F + D + 4) 2^-24 (0.5 A + Lm), A = sum_d [(sum_f |y|)^2 +
sum_f y^2], Lm = sum_f |wide t| -- (2F - 1) u on each s_d^2, F u on q_d, u on the subtraction, (D - 1) u for any order of the column sum,
(F + 2) u on the linear term and the last add, + 4 for higher orders.  A dropped field or column chunk moves it by A / F or 16 A / D."""
import numpy as np
import pytest
import torch

from test_q8_rows_gpu import V, _quantize

pytestmark = pytest.mark.gpu
B = 67                  # the last wave holds a partial set of lane-groups at every D


@pytest.mark.parametrize("padded", [False, True], ids=["compact", "128B"])
@pytest.mark.parametrize("F", [1, 4, 7])               # a lone field, exactly one batch of four, a partial second batch
@pytest.mark.parametrize("D", [4, 12, 20, 24, 80, 252, 256])
def test_fm_lookup_q8(dev, D, F, padded):
    from mindrec_amd import ops
    q8, lo, scale, wide, code, _ = _quantize(dev, D, False, padded)
    rng = np.random.default_rng(100 + F)
    ids, wts = rng.integers(0, V, size=(B, F)), rng.random((B, F)).astype(np.float32)
    ids[0], ids[1] = 3, [(-1, V)[k % 2] for k in range(F)]  # one row in every field; a sample with no id in range
    ids[2:6, 0], ids[B - 1, F - 1], wts[6, 0] = [0, 66, -1, V], 66, 0.0
    ic = np.where(ok := (ids >= 0) & (ids < V), ids, 0)
    y = np.where(ok[..., None], (lo[ic][..., None] + code[ic].astype(np.float32) * scale[ic][..., None]) * wts[..., None], np.float32(0))
    lin = np.where(ok, wide[ic] * wts, np.float32(0))
    assert y.dtype == np.float32 and lin.dtype == np.float32, "the restatement rounds every step to fp32"
    y, lin = y.astype(np.float64), lin.astype(np.float64)
    ref = lin.sum(axis=1) + 0.5 * (y.sum(axis=1) ** 2 - (y ** 2).sum(axis=1)).sum(axis=1)
    bound = (2 * F + D + 4) * 2.0 ** -24 * (0.5 * (np.abs(y).sum(axis=1) ** 2 + (y ** 2).sum(axis=1)).sum(axis=1) + np.abs(lin).sum(axis=1))
    tids, twts, lin_bits = torch.from_numpy(ids).to(dev), torch.from_numpy(wts).to(dev), None
    for dt, idt in [(k, torch.int32) for k in (torch.float32, torch.bfloat16, torch.float16)] + [(torch.float16, torch.int64)] * (D == 80):
        rows, lin_fm = ops.fm_lookup_q8(q8, tids.to(idt), twts, out_dtype=dt)
        want = ops.gather_rows_q8(q8, tids.to(idt), twts, out_dtype=dt)[0]
        assert rows.dtype == dt and torch.equal(rows.view(torch.uint8), want.view(torch.uint8)), "rows are not gather_rows_q8's bit for bit"
        got = lin_fm.cpu().numpy()
        err = np.abs(got.astype(np.float64) - ref)
        print(f"  {dt} {idt}: worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound)
        assert not rows[1].float().any() and got[1] == 0, "a sample with every id out of range: zero rows, lin_fm 0"
        lin_bits = got.view(np.uint32) if lin_bits is None else lin_bits
        assert np.array_equal(got.view(np.uint32), lin_bits), "lin_fm depends on the output kind or the id width"


@pytest.mark.parametrize("D,row_bytes,code", [(6, 32, -3), (260, 288, -3), (80, 80, -1), (80, 100, -1)])
def test_refusals_leave_the_outputs_untouched(dev, D, row_bytes, code):
    from mindrec_amd import _lib, ops
    q8 = ops.Q8Table(torch.zeros((V, row_bytes), dtype=torch.uint8, device=dev), V, D, row_bytes)
    out = {"rows": torch.full((B, 4, D), 7.0, dtype=torch.float16, device=dev), "lin_fm": torch.full((B,), 7.0, device=dev)}
    with pytest.raises(_lib.MrecError) as e:
        ops.fm_lookup_q8(q8, torch.zeros((B, 4), dtype=torch.int32, device=dev), torch.ones((B, 4), device=dev), out=out)
    assert e.value.code == code and bool((out["rows"] == 7.0).all()) and bool((out["lin_fm"] == 7.0).all())
