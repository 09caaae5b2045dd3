"""ops.fm_lookup_q4 (k_q4_fm_lookup).  rows: ops.gather_rows_q4's bit for bit.  lin_fm against float64 over y = (lo + code * scale) * t restated
in numpy float32, under test_q8_fm_gpu.py's bound (2F + D + 4) 2^-24 (0.5 A + Lm), which holds for any order of the column sum.  The widths give
lane-groups of 2, 3, 4 and 9 lanes, a last chunk of 4 .. 32 valid columns and both store widths (D % 8 == 4)."""
import numpy as np
import pytest
import torch

from test_q4_rows_gpu import _records
from test_q8_rows_gpu import PADDED, V

pytestmark = pytest.mark.gpu
B = 67                  # the last wave holds a partial set of lane-groups at every D


@PADDED
@pytest.mark.parametrize("F", [1, 4, 7])               # a lone field, exactly one batch of four, a partial second batch
@pytest.mark.parametrize("D", [4, 12, 20, 28, 32, 36, 80, 252, 256])
def test_fm_lookup_q4(dev, D, F, padded):
    from mindrec_amd import ops
    q4, lo, scale, wide, code = _records(dev, D, False, padded)
    rng = np.random.default_rng(100 + F)
    ids, wts = rng.integers(0, V, size=(B, F)), rng.random((B, F)).astype(np.float32)
    ids[0], ids[1] = 3, [(-1, V)[k % 2] for k in range(F)]  # one row in every field; a sample with no id in range
    ids[2:6, 0], ids[B - 1, F - 1], wts[6, 0] = [0, 66, -1, V], 66, 0.0
    ic = np.where(ok := (ids >= 0) & (ids < V), ids, 0)
    y = np.where(ok[..., None], (lo[ic][..., None] + code[ic].astype(np.float32) * scale[ic][..., None]) * wts[..., None], np.float32(0))
    lin = np.where(ok, wide[ic] * wts, np.float32(0))
    y, lin = y.astype(np.float64), lin.astype(np.float64)
    ref = lin.sum(axis=1) + 0.5 * (y.sum(axis=1) ** 2 - (y ** 2).sum(axis=1)).sum(axis=1)
    bound = (2 * F + D + 4) * 2.0 ** -24 * (0.5 * (np.abs(y).sum(axis=1) ** 2 + (y ** 2).sum(axis=1)).sum(axis=1) + np.abs(lin).sum(axis=1))
    tids, twts, lin_bits = torch.from_numpy(ids).to(dev), torch.from_numpy(wts).to(dev), None
    for dt, idt in [(k, torch.int32) for k in (torch.float32, torch.bfloat16, torch.float16)] + [(torch.float16, torch.int64)] * (D == 80):
        rows, lin_fm = ops.fm_lookup_q4(q4, tids.to(idt), twts, out_dtype=dt)
        want = ops.gather_rows_q4(q4, tids.to(idt), twts, out_dtype=dt)[0]
        assert rows.dtype == dt and torch.equal(rows.view(torch.uint8), want.view(torch.uint8)), "rows are not gather_rows_q4's bit for bit"
        got = lin_fm.cpu().numpy()
        assert np.all(np.abs(got.astype(np.float64) - ref) <= bound)
        assert not rows[1].float().any() and got[1] == 0, "a sample with every id out of range: zero rows, lin_fm 0"
        lin_bits = got.view(np.uint32) if lin_bits is None else lin_bits
        assert np.array_equal(got.view(np.uint32), lin_bits), "lin_fm depends on the output kind or the id width"


@pytest.mark.parametrize("D,row_bytes,code", [(6, 32, -3), (260, 160, -3), (80, 48, -1), (80, 72, -1)])
def test_refusals_leave_the_outputs_untouched(dev, D, row_bytes, code):
    from mindrec_amd import _lib, ops
    q4 = ops.Q8Table(torch.zeros((V, row_bytes), dtype=torch.uint8, device=dev), V, D, row_bytes, 4)
    out = {"rows": torch.full((B, 4, D), 7.0, dtype=torch.float16, device=dev), "lin_fm": torch.full((B,), 7.0, device=dev)}
    with pytest.raises(_lib.MrecError) as e:
        ops.fm_lookup_q4(q4, torch.zeros((B, 4), dtype=torch.int32, device=dev), torch.ones((B, 4), device=dev), out=out)
    assert e.value.code == code and bool((out["rows"] == 7.0).all()) and bool((out["lin_fm"] == 7.0).all())
