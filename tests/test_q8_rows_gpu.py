"""Row-wise 8-bit records (csrc/mrec_q8.hip) against a float64 restatement of include/mrec.h's two formulas.  Quantize: |x' - x| <=
0.5 scale (1 + 2^-12) -- half a code step plus the two fp32 roundings (subtraction, division) of a quotient of at most 255, each at most
255 * 2^-24 codes.  Gather: |out - ref| <= u |ref| + 2^-22 (|lo| + 255 scale) |row_scale| -- u the output rounding (0, 2^-8, 2^-11; f16
with its 2^-25 subnormal floor), the rest the multiply, the add and the product with row_scale in fp32.  Derived, not tuned."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
V, N = 67, 131          # the last wave of either kernel holds a partial lane-group
DIMS = [4, 12, 16, 20, 80, 252, 256]
U = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
PADDED = pytest.mark.parametrize("padded", [False, True], ids=["compact", "128B"])


def _row_bytes(D, padded):
    compact = 16 + 16 * ((D + 15) // 16)
    return -(-compact // 128) * 128 if padded else compact


def _table(D):
    """normal(0, 0.01) with the hand-placed rows: all equal, all zero, all negative, an outlier of 1e3 among 1e-3, minimum last"""
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((V, D)) * 0.01).astype(np.float32)
    x[0], x[1], x[2], x[3] = 0.37, 0.0, -np.abs(x[2]) - 1e-4, 1e-3
    x[3, D // 2], x[4, D - 1] = 1e3, -1.0
    return x, (rng.standard_normal((V, 1)) * 0.01).astype(np.float32)


def _quantize(dev, D, fused, padded):
    """(Q8Table, lo, scale, wide as fp32 vectors, codes [V, D], the bytes that must be zero)"""
    from mindrec_amd import ops
    x, w = _table(D)
    buf = torch.zeros((V, D + 12 if fused else D + 1), dtype=torch.float32, device=dev)
    buf[:, :D], buf[:, D:D + 1] = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    table, wide = (buf[:, :D], buf[:, D:D + 1]) if fused else (buf[:, :D].contiguous(), buf[:, D:D + 1].contiguous())
    out = torch.full((V, _row_bytes(D, padded)), 0xAB, dtype=torch.uint8, device=dev)       # no memset is needed in front
    q8 = ops.quantize_rows_q8(table, wide, row_bytes=_row_bytes(D, padded), out=out)
    rec = q8.records.cpu().numpy()
    f = np.ascontiguousarray(rec[:, :12]).view(np.float32)
    return q8, f[:, 0], f[:, 1], f[:, 2], rec[:, 16:16 + D], np.concatenate([rec[:, 12:16], rec[:, 16 + D:]], axis=1)


@PADDED
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("D", DIMS)
def test_quantize(dev, D, fused, padded):
    from mindrec_amd import ops
    q8, lo, scale, wide, code, zeros = _quantize(dev, D, fused, padded)
    assert (q8.V, q8.D, q8.row_bytes) == (V, D, _row_bytes(D, padded)) and ops.q8_row_bytes(D) == _row_bytes(D, False)
    x, w = _table(D)
    assert np.array_equal(lo.view(np.uint32), x.min(axis=1).view(np.uint32)), "lo is not the row minimum bit for bit"
    ref = (x.max(axis=1).astype(np.float64) - x.min(axis=1).astype(np.float64)) / 255.0
    assert np.all(np.abs(scale.astype(np.float64) - ref) <= np.spacing(ref.astype(np.float32)).astype(np.float64)), "scale"
    assert np.array_equal(wide.view(np.uint32), w[:, 0].view(np.uint32)), "wide is not copied unchanged"
    assert not zeros.any(), "bytes 12..15 or the padding are not zero"
    s64 = scale.astype(np.float64)[:, None]
    err, bound = np.abs(lo.astype(np.float64)[:, None] + code.astype(np.float64) * s64 - x.astype(np.float64)), 0.5 * s64 * (1 + 2.0 ** -12)
    print("  max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    assert scale[0] == 0 and scale[1] == 0 and not code[:2].any(), "a constant row has scale 0 and all codes 0"


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("dt", list(U), ids=["f32", "bf16", "f16"])
@PADDED
@pytest.mark.parametrize("D", DIMS)
def test_gather(dev, D, padded, dt, idt, scaled):
    from mindrec_amd import ops
    q8, lo, scale, wide, code, _ = _quantize(dev, D, False, padded)
    rng = np.random.default_rng(7)
    ids = rng.integers(0, V, size=N)
    ids[:8] = [3, 3, -1, V, 0, 66, 4, 3]                    # duplicates, both sides out of range, the first and the last row
    rs = rng.random(N).astype(np.float32) if scaled else np.ones(N, np.float32)
    rows, wprod = ops.gather_rows_q8(q8, torch.from_numpy(ids).to(dev).to(idt), torch.from_numpy(rs).to(dev) if scaled else None,
                                     out_dtype=dt)
    assert rows.dtype == dt and tuple(rows.shape) == (N, D) and tuple(wprod.shape) == (N, 2)
    got, wp = rows.double().cpu().numpy(), wprod.cpu().numpy()
    ok = (ids >= 0) & (ids < V)
    ic, rs64 = np.where(ok, ids, 0), rs.astype(np.float64)[:, None]
    ref = (lo.astype(np.float64)[ic, None] + code[ic].astype(np.float64) * scale.astype(np.float64)[ic, None]) * rs64
    bound = (U[dt] * np.abs(ref) + 2.0 ** -22 * (np.abs(lo[ic]) + 255.0 * scale[ic]).astype(np.float64)[:, None] * rs64
             + (2.0 ** -25 if dt == torch.float16 else 0.0))
    print("  max |out - ref|", float(np.abs(got - ref)[ok].max()), "worst err / bound", float((np.abs(got - ref)[ok] / bound[ok]).max()))
    assert np.all(np.abs(got - ref)[ok] <= bound[ok])
    assert not got[~ok].any() and not wp[~ok].any(), "an id outside [0, V) gives exact zeros"
    assert np.array_equal(wp[:, 0].view(np.uint32)[ok], (wide[ic] * rs).view(np.uint32)[ok]) and not wp[:, 1].any()


@pytest.mark.parametrize("D,row_bytes,code", [(6, 32, -3), (260, 288, -3), (80, 80, -1), (80, 100, -1)])
def test_refusals_leave_the_output_untouched(dev, D, row_bytes, code):
    from mindrec_amd import _lib, ops
    rec = torch.full((V, row_bytes), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.full((N, D), 7.0, dtype=torch.float16, device=dev)
    with pytest.raises(_lib.MrecError) as e:
        ops.quantize_rows_q8(torch.zeros((V, D), dtype=torch.float32, device=dev), row_bytes=row_bytes, out=rec)
    assert e.value.code == code
    with pytest.raises(_lib.MrecError) as e:
        ops.gather_rows_q8(ops.Q8Table(rec, V, D, row_bytes), torch.zeros(N, dtype=torch.int32, device=dev), out=out)
    assert e.value.code == code
    torch.cuda.synchronize()
    assert bool((rec == 0xAB).all()) and bool((out == 7.0).all())
