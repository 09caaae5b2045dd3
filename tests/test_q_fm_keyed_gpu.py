"""The keyed FM lookups over records (k_q8_fm_lookup_keyed, k_q4_fm_lookup_keyed) at every lane geometry: bit for bit the unkeyed lookups over
ids = dict.get(key, -1); one case a bit width against records dequantized in numpy (rows: the fp32 chain rounded once to the output kind,
exactly; lin_fm: float64, test_q8_deepfm_predict_gpu.py's bound); every refusal in its order, outputs untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N = 200                                                                   # records = keys in the index
DS, FS, BS = {8: (4, 20, 80, 256), 4: (4, 36, 80, 256)}, (1, 4, 5, 39), (1, 11, 300)
CASES = [(bits, DS[bits][i], FS[(i + j) % 4], BS[(i + 2 * j) % 3], (torch.int64, torch.int32)[(i + j) % 2],     # (a sparse cross: every D with two F)
          (torch.float16, torch.float32, torch.bfloat16)[(i + j) % 3]) for bits in (8, 4) for j in (0, 1) for i in range(4)]


def _setup(dev, bits, D, F, B, kdt):
    """records, an index over N keys (key 0 -> a row outside the table), a batch: ~1/4 absent keys, some -1, a duplicate a sample; ids: a dict's"""
    from mindrec_amd import ops
    g = torch.Generator().manual_seed(1000 * D + 10 * F + bits)
    table, wide = torch.randn((N, D), generator=g), torch.randn((N, 1), generator=g)
    q = (ops.quantize_rows_q4 if bits == 4 else ops.quantize_rows_q8)(table.to(dev), wide.to(dev))
    pool = torch.randperm(1 << 20, generator=g)[: 2 * N].to(kdt) * (3 if kdt == torch.int32 else -(1 << 33) - 7) + 5
    stored, absent = pool[:N], pool[N:]
    rows = torch.arange(N, dtype=torch.int32)
    rows[0] = N + 5
    kidx = ops.FrozenKeyIndex(stored.to(dev), rows.to(dev))
    pick = torch.randint(0, N, (B, F), generator=g)
    u = torch.rand((B, F), generator=g)
    keys = torch.where(u < 0.7, stored[pick], absent[pick])
    keys[u > 0.95] = -1
    keys[:, F // 2] = keys[:, 0]
    d = {int(k): int(r) for k, r in zip(stored, rows)}
    ids = torch.tensor([d.get(int(k), -1) for k in keys.view(-1)], dtype=torch.int32).view(B, F)
    wts = torch.rand((B, F), generator=g) + 0.5
    return q, kidx, keys.to(dev), ids, wts.to(dev)


@pytest.mark.parametrize("bits,D,F,B,kdt,odt", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_keyed_equals_unkeyed(dev, bits, D, F, B, kdt, odt):
    from mindrec_amd import ops
    q, kidx, keys, ids, wts = _setup(dev, bits, D, F, B, kdt)
    keyed, plain = (ops.fm_lookup_q4_keyed, ops.fm_lookup_q4) if bits == 4 else (ops.fm_lookup_q8_keyed, ops.fm_lookup_q8)
    rows, lin_fm = keyed(q, kidx, keys, wts, out_dtype=odt)
    want_rows, want_lin = plain(q, ids.to(dev), wts, out_dtype=odt)
    assert torch.equal(kidx.find(keys).cpu(), ids)
    assert torch.equal(rows.view(torch.uint8), want_rows.view(torch.uint8)) and torch.equal(lin_fm.view(torch.int32), want_lin.view(torch.int32))


@pytest.mark.parametrize("bits,D,odt", [(8, 20, torch.float16), (4, 36, torch.bfloat16)], ids=["q8", "q4"])
def test_keyed_against_numpy(dev, bits, D, odt):
    from mindrec_amd import ops
    F, B = 5, 11
    q, kidx, keys, ids, wts = _setup(dev, bits, D, F, B, torch.int64)
    rows, lin_fm = (ops.fm_lookup_q4_keyed if bits == 4 else ops.fm_lookup_q8_keyed)(q, kidx, keys, wts, out_dtype=odt)
    rec = q.records.cpu().numpy()
    hdr = rec[:, :12].copy().view(np.float32)
    code = rec[:, 16:]
    code = (np.stack([code & 15, code >> 4], axis=2).reshape(N, -1) if bits == 4 else code)[:, :D].astype(np.float32)
    deq = np.concatenate([hdr[:, 0:1] + code * hdr[:, 1:2], np.zeros((1, D), np.float32)])        # fp32 multiply, fp32 add; row N: absent
    lin_w = np.concatenate([hdr[:, 2], np.zeros(1, np.float32)])
    ic, w = np.where((ids.numpy() >= 0) & (ids.numpy() < N), ids.numpy(), N), wts.cpu().numpy()
    y32 = deq[ic] * w[..., None]
    assert torch.equal(rows.cpu().view(torch.uint8), torch.from_numpy(y32).to(odt).view(torch.uint8))
    y, lin = y32.astype(np.float64), (lin_w[ic] * w).astype(np.float64)
    exact = lin.sum(axis=1) + 0.5 * ((y.sum(axis=1) ** 2).sum(axis=1) - (y ** 2).sum(axis=(1, 2)))
    bound = (2 * F + D + 4) * 2.0 ** -24 * (0.5 * ((np.abs(y).sum(axis=1) ** 2).sum(axis=1) + (y ** 2).sum(axis=(1, 2))) + np.abs(lin).sum(axis=1))
    err = np.abs(lin_fm.cpu().numpy().astype(np.float64) - exact)
    print(f"  worst |lin_fm - float64| / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("bits", [8, 4])
def test_keyed_refusals_in_order(dev, bits):
    from mindrec_amd import _lib, ops
    D, F, B = 20, 5, 11
    q, kidx, keys, _, wts = _setup(dev, bits, D, F, B, torch.int64)
    rows = torch.full((B * F * D + 64,), 0x5A5A, dtype=torch.int16, device=dev)
    lin_fm = torch.full((B + 64,), -7.0, device=dev)
    unbuilt = torch.zeros(2048, dtype=torch.uint8, device=dev)
    ok = dict(D=D, rb=q.row_bytes, kidx=kidx._ptr().value, kb=8, wts=wts.data_ptr(), rows=rows.data_ptr() + 64)
    faults = [(dict(D=6), -3), (dict(rb=q.row_bytes - 16), -1), (dict(kb=3), -1), (dict(wts=None), -1), (dict(rows=ok["rows"] + 2), -3),
              (dict(kidx=None), -1), (dict(kidx=ok["kidx"] + 16), -3), (dict(kidx=unbuilt.data_ptr() + (-unbuilt.data_ptr()) % 256), -3)]
    fn = getattr(_lib.lib(), f"mrec_q{bits}_fm_lookup_keyed")
    for i, (_, code) in enumerate(faults):                               # fault i with every later fault behind it: the earlier one answers
        a = dict(ok)
        for f, _ in reversed(faults[i:]):
            a.update(f)
        got = fn(q.records.data_ptr(), q.V, a["rb"], a["D"], a["kidx"], keys.data_ptr(), a["kb"], a["wts"], B, F, a["rows"], 2,
                 lin_fm.data_ptr() + 64, ops._stream())
        assert got == code, f"fault {i}: {got}"
    torch.cuda.synchronize()
    assert bool((rows == 0x5A5A).all()) and bool((lin_fm == -7.0).all())
