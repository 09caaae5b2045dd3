"""ops.gather_pool_fields_q8 (k_q8_gather_pool_fields) against float64 over the records' own fields read back from the device:
ref = sum_s m_s (lo_s + code_sd scale_s) / (L_f or 1) per field.  Bound, from include/mrec.h's arithmetic with u = 2^-24 and
S = sum_s |m_s| (|lo_s| + 255 scale_s): u on t_s = m_s scale_s, L_f u on the fma chain (one rounding a slot), L_f u on the products
u_s = m_s lo_s and the base chain (the first add to +0 is exact), u on acc + base, u on the mean's division, 2 u for higher orders:
|got - ref| <= (L_f + 5) u S / (L_f or 1) + u_out |ref|, u_out = 0, 2^-8, 2^-11 (f16 with its 2^-25 subnormal floor).  The wide sum:
Ls products, Ls adds in two levels, |w - ref| <= (Ls + 2) u sum_s |m_s wide_s|.  A dropped slot moves a bag by about S / L_f."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_q8_rows_gpu import U, V, _quantize

pytestmark = pytest.mark.gpu
B = 67                  # the last wave holds a partial set of lane-groups at every D
FIELDS = [(1,), (4,), (5,), (9,), (3, 5, 4, 3, 4, 2), (1, 1, 1)]      # a lone slot, one batch of four, a partial second, a third, seams inside a batch, single-hot


@pytest.mark.parametrize("padded", [False, True], ids=["compact", "128B"])
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("fields", FIELDS, ids=lambda f: "x".join(map(str, f)))
@pytest.mark.parametrize("D", [4, 12, 20, 64, 80, 252, 256])
def test_gather_pool_fields_q8(dev, D, fields, mode, padded):
    from mindrec_amd import ops
    q8, lo, scale, wide, code, _ = _quantize(dev, D, False, padded)
    F, Ls, rng = len(fields), sum(fields), np.random.default_rng(100 + sum(fields))
    ids, mask = rng.integers(0, V, size=(B, Ls)), rng.random((B, Ls)).astype(np.float32)
    ids[1] = [(-1, V)[k % 2] for k in range(Ls)]           # a sample with no id in range
    ids[2:6, 0], ids[B - 1, Ls - 1], mask[6, 0] = [0, 66, -1, V], 66, 0.0
    ic, m = np.where(ok := (ids >= 0) & (ids < V), ids, 0), np.where(ok, mask, 0).astype(np.float64)
    term = m[..., None] * (lo[ic].astype(np.float64)[..., None] + code[ic].astype(np.float64) * scale[ic].astype(np.float64)[..., None])
    S, gw = m * (np.abs(lo[ic]).astype(np.float64) + 255.0 * scale[ic]), m * wide[ic].astype(np.float64)
    off, den = np.concatenate([[0], np.cumsum(fields)]), [float(L) if mode == "mean" else 1.0 for L in fields]
    ref = np.concatenate([term[:, off[f]:off[f + 1]].sum(axis=1) / den[f] for f in range(F)], axis=1)
    arith = np.repeat(np.stack([(fields[f] + 5) * 2.0 ** -24 * S[:, off[f]:off[f + 1]].sum(axis=1) / den[f] for f in range(F)], axis=1), D, axis=1)
    wref, wbound = gw.sum(axis=1), (Ls + 2) * 2.0 ** -24 * np.abs(gw).sum(axis=1)
    tids, tmask, x32, wbits = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), None, None
    for dt, idt in [(k, torch.int32) for k in U] + [(torch.float32, torch.int64)] * (D == 80):
        x, w = ops.gather_pool_fields_q8(q8, tids.to(idt), fields, tmask, mode=mode, out_dtype=dt, wide=True)
        assert x.dtype == dt and tuple(x.shape) == (B, F * D) and w.dtype == torch.float32 and tuple(w.shape) == (B,)
        err, werr = np.abs(x.double().cpu().numpy() - ref), np.abs(w.double().cpu().numpy() - wref)
        bound = arith + U[dt] * np.abs(ref) + (2.0 ** -25 if dt == torch.float16 else 0.0)
        print(f"  {dt} {idt}: worst err / bound", float((err / np.maximum(bound, 1e-300)).max()), "wide", float((werr / np.maximum(wbound, 1e-300)).max()))
        assert np.all(err <= bound) and np.all(werr <= wbound)
        assert not x[1].float().any() and float(w[1]) == 0, "a sample with every id out of range: a zero row, w 0"
        x32, wbits = (x, w) if x32 is None else (x32, wbits)
        assert torch.equal(x.view(torch.uint8), x32.to(dt).view(torch.uint8)), "not the fp32 row rounded once to nearest even / depends on the id width"
        assert torch.equal(w.view(torch.int32), wbits.view(torch.int32)), "w depends on the output kind or the id width"
    ones = ops.gather_pool_fields_q8(q8, tids.int(), fields, torch.ones_like(tmask), mode=mode, wide=True)
    none = ops.gather_pool_fields_q8(q8, tids.int(), fields, None, mode=mode, wide=True)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ones, none)), "mask=None is not a mask of ones"
    big, wbig = torch.full((B, F * D + 8), 7.0, dtype=torch.float16, device=dev), torch.full((B, 3), 7.0, device=dev)
    ops.gather_pool_fields_q8(q8, tids.int(), fields, tmask, mode=mode, out=big[:, 4:4 + F * D], wide=True, wide_out=wbig[:, 1])
    assert torch.equal(big[:, 4:4 + F * D], x32.half()) and torch.equal(wbig[:, 1], wbits), "a column block (8-byte aligned only), a strided wide column"
    assert bool((big[:, :4] == 7.0).all()) and bool((big[:, 4 + F * D:] == 7.0).all()) and bool((wbig[:, ::2] == 7.0).all()), "other columns touched"


@pytest.mark.parametrize("kw,code", [(dict(D=6, rb=32), -3), (dict(D=260, rb=288), -3), (dict(rb=80), -1), (dict(rb=100), -1), (dict(fields=(0,)), -1),
                                     (dict(fields=(1,) * 65), -3), (dict(fields=(4097,)), -3), (dict(mode=2), -1)])
def test_refusals_leave_the_outputs_untouched(dev, kw, code):
    from mindrec_amd import _lib, ops
    D, rb, fields, mode = kw.get("D", 80), kw.get("rb", 96), kw.get("fields", (3, 2)), kw.get("mode", 1)
    F, Ls = len(fields), max(sum(fields), 1)
    rec, ids = torch.zeros((V + 1, rb), dtype=torch.uint8, device=dev), torch.zeros((B, Ls), dtype=torch.int32, device=dev)
    out, w = torch.full((B, F * D), 7.0, dtype=torch.float16, device=dev), torch.full((B,), 7.0, device=dev)
    rc = _lib.lib().mrec_q8_gather_pool_fields(ops._ptr(rec), V, rb, D, ops._ptr(ids), 4, B, F, (C.c_int32 * F)(*fields), None, mode, ops._ptr(out),
                                               2, 0, ops._ptr(w), 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == code and bool((out == 7.0).all()) and bool((w == 7.0).all())
