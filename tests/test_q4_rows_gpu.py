"""Row-wise 4-bit records (csrc/mrec_q8.hip) against a float64 restatement of include/mrec.h's formulas, over tests/test_q8_rows_gpu.py's
table and with its bounds at 15 codes instead of 255 (derived there, not tuned).  The widths cover every `valid` = 4 .. 32 of a row's last
chunk, lane-groups of 2, 3, 4 and 9 lanes and both store widths (D % 8 == 4); N = 1031 is three workgroups of the 2-lane geometry."""
import numpy as np
import pytest
import torch
from test_q8_rows_gpu import PADDED, U, V, _table

pytestmark = pytest.mark.gpu
DIMS = pytest.mark.parametrize("D", [4, 8, 12, 16, 20, 24, 28, 32, 36, 80, 252, 256])


def _records(dev, D, fused, padded):
    """quantizes _table(D) into a buffer of 0xAB, holds the records to the format, returns (Q8Table, lo, scale, wide, codes [V, D])"""
    from mindrec_amd import ops
    x, w = _table(D)
    rb = 16 + 16 * ((D + 31) // 32)
    rb = -(-rb // 128) * 128 if padded else rb
    buf = torch.from_numpy(np.concatenate([x, w, np.zeros((V, 11), np.float32)], axis=1)).to(dev)      # a fused row: D + 12 floats
    table, wide = (buf[:, :D], buf[:, D:D + 1]) if fused else (buf[:, :D].contiguous(), buf[:, D:D + 1].contiguous())
    out = torch.full((V, rb), 0xAB, dtype=torch.uint8, device=dev)      # no memset is needed in front
    q4 = ops.quantize_rows_q4(table, wide, row_bytes=rb, out=out)
    assert (q4.V, q4.D, q4.row_bytes, q4.bits) == (V, D, rb, 4) and (padded or ops.q4_row_bytes(D) == rb)
    rec = q4.records.cpu().numpy()
    f, b = np.ascontiguousarray(rec[:, :12]).view(np.float32), rec[:, 16:16 + D // 2]
    lo, scale, code = f[:, 0], f[:, 1], np.stack([b & 15, b >> 4], axis=2).reshape(V, D)     # byte j: column 2 j low, 2 j + 1 high
    assert np.array_equal(lo.view(np.uint32), x.min(axis=1).view(np.uint32)), "lo is not the row minimum bit for bit"
    ref = (x.max(axis=1).astype(np.float64) - x.min(axis=1).astype(np.float64)) / 15.0
    assert np.all(np.abs(scale.astype(np.float64) - ref) <= np.spacing(ref.astype(np.float32)).astype(np.float64)), "scale"
    assert np.array_equal(f[:, 2].view(np.uint32), w[:, 0].view(np.uint32)), "wide is not copied unchanged"
    assert not rec[:, 12:16].any() and not rec[:, 16 + D // 2:].any(), "bytes 12..15, or behind the ceil(D / 2) code bytes, are not zero"
    s64 = scale.astype(np.float64)[:, None]
    err, bound = np.abs(lo.astype(np.float64)[:, None] + code.astype(np.float64) * s64 - x.astype(np.float64)), 0.5 * s64 * (1 + 2.0 ** -12)
    assert np.all(err <= bound), float((err - bound).max())
    assert scale[0] == 0 and scale[1] == 0 and not code[:2].any(), "a constant row has scale 0 and all codes 0"
    return q4, lo, scale, f[:, 2], code


@PADDED
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@DIMS
def test_quantize(dev, D, fused, padded):
    _records(dev, D, fused, padded)


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("dt", list(U), ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("N", [131, 1031])
@PADDED
@DIMS
def test_gather(dev, D, padded, N, dt, idt, scaled):
    from mindrec_amd import ops
    q4, lo, scale, wide, code = _records(dev, D, False, padded)
    rng = np.random.default_rng(7)
    ids = rng.integers(0, V, size=N)
    ids[:8] = [3, 3, -1, V, 0, 66, 4, 3]                    # duplicates, both sides out of range, the first and the last row
    rs = rng.random(N).astype(np.float32) if scaled else np.ones(N, np.float32)
    rows, wprod = ops.gather_rows_q4(q4, torch.from_numpy(ids).to(dev).to(idt), torch.from_numpy(rs).to(dev) if scaled else None,
                                     out_dtype=dt)
    assert rows.dtype == dt and tuple(rows.shape) == (N, D) and tuple(wprod.shape) == (N, 2)
    got, wp = rows.double().cpu().numpy(), wprod.cpu().numpy()
    ok = (ids >= 0) & (ids < V)
    ic, rs64 = np.where(ok, ids, 0), rs.astype(np.float64)[:, None]
    ref = (lo.astype(np.float64)[ic, None] + code[ic].astype(np.float64) * scale.astype(np.float64)[ic, None]) * rs64
    bound = (U[dt] * np.abs(ref) + 2.0 ** -22 * (np.abs(lo[ic]) + 15.0 * scale[ic]).astype(np.float64)[:, None] * rs64
             + (2.0 ** -25 if dt == torch.float16 else 0.0))
    assert np.all(np.abs(got - ref)[ok] <= bound[ok]), float((np.abs(got - ref) - bound)[ok].max())
    assert not got[~ok].any() and not wp[~ok].any(), "an id outside [0, V) gives exact zeros"
    assert np.array_equal(wp[:, 0].view(np.uint32)[ok], (wide[ic] * rs).view(np.uint32)[ok]) and not wp[:, 1].any()


@pytest.mark.parametrize("D,row_bytes,code", [(6, 32, -3), (260, 160, -3), (80, 48, -1), (80, 72, -1)])
def test_refusals_leave_the_output_untouched(dev, D, row_bytes, code):
    from mindrec_amd import _lib, ops
    rec = torch.full((V, row_bytes), 0xAB, dtype=torch.uint8, device=dev)
    out, ids = torch.full((131, D), 7.0, dtype=torch.float16, device=dev), torch.zeros(131, dtype=torch.int32, device=dev)
    for call in (lambda: ops.quantize_rows_q4(torch.zeros((V, D), dtype=torch.float32, device=dev), row_bytes=row_bytes, out=rec),
                 lambda: ops.gather_rows_q4(ops.Q8Table(rec, V, D, row_bytes, 4), ids, out=out)):
        with pytest.raises(_lib.MrecError) as e:
            call()
        assert e.value.code == code
    torch.cuda.synchronize()
    assert bool((rec == 0xAB).all()) and bool((out == 7.0).all())


def test_a_table_is_read_by_the_lookup_of_its_own_code_width_only(dev):
    from mindrec_amd import ops
    ids, table = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros((V, 80), dtype=torch.float32, device=dev)
    with pytest.raises(TypeError, match="8-bit records"):
        ops.gather_rows_q8(ops.quantize_rows_q4(table), ids)
    with pytest.raises(TypeError, match="4-bit records"):
        ops.gather_rows_q4(ops.quantize_rows_q8(table), ids)
