"""freeze_q8 of the multi-hot classes (serving.MultiHotQ8): the frozen lookup is ops.gather_pool_fields_q8 over ops.quantize_rows_q8's records
bit for bit, and lies within the quantize bound of test_q8_rows_gpu.py carried through the bag -- 0.5 (1 + 2^-12) sum_s |m_s| scale_s /
(L_f or 1) -- plus test_q8_pool_gpu.py's arithmetic bound of the fp32 classes' own lookup; the wide sum within that file's wide bound."""
import numpy as np
import pytest
import torch

from test_q8_rows_gpu import V

pytestmark = pytest.mark.gpu
B, BAG = 67, (3, 5, 4, 3, 4, 2)


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("D", [64, 80])
def test_wide_deep_freeze_q8(dev, D, mode):
    from mindrec_amd import multi_hot, ops
    pair = multi_hot.MultiHotWideDeep(vocab=V, dim=D, bag=BAG, mode=mode, device=dev)
    rng = np.random.default_rng(D)
    ids, mask = rng.integers(0, V, size=(B, sum(BAG))).astype(np.int32), rng.random((B, sum(BAG))).astype(np.float32)
    tids, tmask, frozen = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev), pair.freeze_q8()
    (x, w), (x0, w0) = frozen.lookup(tids, tmask), pair.lookup(tids, tmask)
    assert not hasattr(frozen, "table") and not hasattr(frozen, "apply_")
    want = ops.gather_pool_fields_q8(ops.quantize_rows_q8(pair.deep.table, pair.wide.table), tids, BAG, tmask, mode=mode, wide=True)
    assert torch.equal(x.view(torch.int32), want[0].view(torch.int32)) and torch.equal(w.view(torch.int32), want[1].view(torch.int32))
    hdr = np.ascontiguousarray(frozen.q8.records.cpu().numpy()[:, :12]).view(np.float32).astype(np.float64)
    m, off = mask.astype(np.float64), np.concatenate([[0], np.cumsum(BAG)])
    wabs = np.abs(m * pair.wide.table.double().cpu().numpy()[ids, 0]).sum(axis=1)
    assert np.all(np.abs((w.double() - w0.double()).cpu().numpy()) <= (sum(BAG) + 2) * 2.0 ** -24 * wabs)
    bound = np.stack([(0.5 * (1 + 2.0 ** -12) * (m * hdr[ids, 1])[:, off[f]:off[f + 1]].sum(axis=1)
                       + (L + 5) * 2.0 ** -24 * (m * (np.abs(hdr[ids, 0]) + 255.0 * hdr[ids, 1]))[:, off[f]:off[f + 1]].sum(axis=1))
                      / (L if mode == "mean" else 1) for f, L in enumerate(BAG)], axis=1)
    err = np.abs((x.double() - x0.double()).cpu().numpy()).reshape(B, len(BAG), D).max(axis=2)
    print("  worst |x_q8 - x_fp32| / bound", float((err / bound).max()))
    assert np.all(err <= bound)


def test_embedding_freeze_q8_bags_per_sample(dev):
    from mindrec_amd.multi_hot import MultiHotEmbedding
    frozen = MultiHotEmbedding(vocab=V, dim=64, bag=4, device=dev).freeze_q8(row_bytes=128)
    ids, mask = torch.randint(0, V, (B, 3, 4), device=dev), torch.rand((B, 3, 4), device=dev)
    x = frozen.lookup(ids, mask)
    assert tuple(x.shape) == (B, 3 * 64) and torch.equal(x.view(3 * B, 64), frozen.lookup(ids.view(3 * B, 4), mask.view(3 * B, 4)))


@pytest.mark.parametrize("kw", [dict(dim=64, max_norm=1.0), dict(dim=6)])
def test_freeze_q8_refusals(dev, kw):
    from mindrec_amd.multi_hot import MultiHotEmbedding, MultiHotWideDeep
    for cls in (MultiHotEmbedding, MultiHotWideDeep):
        with pytest.raises(ValueError):
            cls(vocab=V, bag=(2, 3), device=dev, **kw).freeze_q8()
