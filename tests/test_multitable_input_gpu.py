"""ops.multitable_input / mrec_mt_input (csrc/mrec_multitable.hip) on the GPU, kernel level: every deep column bit for bit against the
host restatement (tests/_multitable_ref.py) and against the merged lookups it replaces (ops.gather_rows, ops.gather_pool_fields), the
wide sum inside the first-order bound of an fp32 sum, the same bits on every run, and NaN confined to the samples that look it up."""
import functools

import numpy as np
import pytest
import torch

import _multitable_ref as R

pytestmark = pytest.mark.gpu

KINDS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
# (D, L, pooled, mask: None / "01" / "real", wide weights?, V, columns skipped in front of the block)
MIXED = dict(C=32, pad=8, ld_extra=16, segs=[
    (64, 1, False, None, True, 16, 0), (128, 3, False, "real", True, 300, 0), (64, 7, True, "01", True, 50, 16),
    (8, 2, True, None, False, 9, 0), (256, 1, True, "real", True, 20, 0), (8, 3, False, None, True, 11, 0),
    (256, 1, False, "01", True, 12, 0), (128, 2, True, "01", True, 300, 0)])
NOCONT = dict(C=0, pad=0, ld_extra=0, segs=[(64, 3, False, None, True, 30, 0), (8, 7, True, "real", True, 5, 8), (128, 1, True, None, True, 40, 0)])
SMALLC = dict(C=8, pad=0, ld_extra=8, segs=[(8, 1, False, "01", False, 7, 0), (64, 2, True, "real", True, 33, 0)])
SIXTEEN = dict(C=8, pad=16, ld_extra=0, segs=[((8, 64, 128, 8)[i % 4], (1, 3, 2, 7)[i % 4], i % 2 == 1, (None, "01", "real")[i % 3], i != 5, 13 + i, 8 * (i == 9))
                                              for i in range(16)])
LAYOUTS = {"mixed": MIXED, "nocont": NOCONT, "smallc": SMALLC, "sixteen": SIXTEEN}


@functools.lru_cache(maxsize=None)
def case(layout, B):
    """numpy inputs of a layout at batch B and their host answers, computed once and shared (read-only) by the tests"""
    spec = LAYOUTS[layout]
    rng = np.random.default_rng(1000 + 7 * B + len(layout))
    C = spec["C"]
    cont = rng.standard_normal((B, C)).astype(np.float32) if C else None
    wc = rng.standard_normal(C).astype(np.float32) if C else None
    wb = rng.standard_normal(1).astype(np.float32)
    segs, col = [], C
    for D, L, pooled, mk, has_wide, V, skip in spec["segs"]:
        col += skip
        table = rng.standard_normal((V, D)).astype(np.float32)
        ids = rng.integers(0, V, size=(B, L)).astype(np.int32)
        bad = rng.random((B, L)) < 0.1
        ids[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, V)          # ids outside [0, V) on both sides
        ids.flat[0] = -1
        if ids.size > 1:
            ids.flat[ids.size - 1] = V
        mask = None if mk is None else ((rng.random((B, L)) < 0.6).astype(np.float32) if mk == "01" else rng.standard_normal((B, L)).astype(np.float32))
        wide = rng.standard_normal(V).astype(np.float32) if has_wide else None
        segs.append(R.Seg(table, ids, col, pooled, mask, wide))
        col += segs[-1].width
    K0 = col + spec["pad"]
    order = list(rng.permutation(len(segs)))                                  # the caller's order is not the column order
    segs = [segs[i] for i in order]
    ref = {k: R.input_row(cont, segs, K0, k, B=B) for k in KINDS}
    for a in [cont, wc, wb] + list(ref.values()) + [t for s in segs for t in (s.table, s.ids, s.mask, s.wide)]:
        if a is not None:
            a.setflags(write=False)
    return dict(B=B, C=C, cont=cont, wc=wc, wb=wb, segs=segs, K0=K0, ldx=K0 + spec["ld_extra"], ref=ref, wide=R.wide_sum(cont, wc, wb, segs, B=B))


def dev_segs(segs, dev):
    from mindrec_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    return [ops.MtSegment(t(s.table), t(s.ids), s.col, s.pooled, t(s.mask), t(s.wide)) for s in segs]


def run(c, kind, dev, segs=None):
    from mindrec_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    big = torch.full((c["B"], c["ldx"]), 7.0, dtype=KINDS[kind], device=dev)  # the sentinel: columns K0 .. ldx-1 must keep it
    segs = dev_segs(c["segs"], dev) if segs is None else segs
    x, wide = ops.multitable_input(t(c["cont"]), t(c["wc"]), t(c["wb"]), segs, K0=c["K0"], out=big[:, :c["K0"]])
    assert x.data_ptr() == big.data_ptr() and wide.shape == (c["B"],) and wide.dtype == torch.float32
    return big, wide, segs


def bits(t):
    """a tensor's values widened to float32 (exact), as their bit patterns"""
    return t.detach().float().cpu().contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("B", [1, 3, 64, 257])
@pytest.mark.parametrize("layout", ["mixed", "nocont"])
def test_deep_columns_bit_for_bit_and_wide_within_bound(dev, layout, B, kind):
    from mindrec_amd import ops
    c = case(layout, B)
    big, wide, segs = run(c, kind, dev)
    K0 = c["K0"]
    assert np.array_equal(bits(big[:, :K0]), c["ref"][kind].view(np.uint32)), "deep columns differ from the host restatement"
    covered = np.zeros(K0, bool)
    covered[:c["C"]] = True
    for s in c["segs"]:
        covered[s.col:s.col + s.width] = True
    assert (~covered).sum() == LAYOUTS[layout]["pad"] + sum(sp[6] for sp in LAYOUTS[layout]["segs"])
    assert not bits(big[:, :K0])[:, ~covered].any(), "gap / pad columns are not +0"
    assert (big[:, K0:].float() == 7.0).all(), "columns past K0 were written"
    # against the merged kernels, written for the same column block
    for s, ds in zip(c["segs"], segs):
        blk = bits(big[:, s.col:s.col + s.width])
        if s.pooled:
            old = ops.gather_pool_fields(ds.table, ds.ids, (s.ids.shape[1],), ds.mask, mode="mean", out_dtype=KINDS[kind])
        else:
            old = ops.gather_rows(ds.table, ds.ids, ds.mask, out_dtype=KINDS[kind]).reshape(B, -1)
        assert np.array_equal(blk, bits(old)), f"block at column {s.col} differs from the merged lookup"
    # the wide sum: the first-order bound of an fp32 sum of n rounded products in any order, no further slack
    w64, aw, n = c["wide"]
    err = np.abs(wide.cpu().numpy().astype(np.float64) - w64)
    bound = (n + 1) * 2.0 ** -24 * aw
    print(f"wide: max err {err.max():.3e}, min bound {bound.min():.3e}, n = {n}")
    assert (err <= bound).all(), f"wide sum off by {err.max():.3e}, bound {bound[err.argmax()]:.3e}"
    big2, wide2, _ = run(c, kind, dev, segs)
    assert torch.equal(wide, wide2) and np.array_equal(bits(big), bits(big2)), "two calls differ"


@pytest.mark.parametrize("layout,B,kind", [("smallc", 3, "f16"), ("smallc", 257, "f32"), ("sixteen", 64, "bf16"), ("sixteen", 257, "f16")])
def test_small_continuous_block_and_sixteen_segments(dev, layout, B, kind):
    c = case(layout, B)
    assert layout != "sixteen" or len(c["segs"]) == 16
    big, wide, _ = run(c, kind, dev)
    assert np.array_equal(bits(big[:, :c["K0"]]), c["ref"][kind].view(np.uint32))
    assert (big[:, c["K0"]:].float() == 7.0).all()
    w64, aw, n = c["wide"]
    assert (np.abs(wide.cpu().numpy().astype(np.float64) - w64) <= (n + 1) * 2.0 ** -24 * aw).all()


def test_fresh_outputs_strided_ids_and_tuples(dev):
    """without out= / wide_out= the wrapper allocates [B, K0]; ids and masks that are column slices of wider tensors go in by their
    row stride; segments may be plain tuples"""
    from mindrec_amd import ops
    c = case("smallc", 64)
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    segs = []
    for s in c["segs"]:
        L = s.ids.shape[1]
        wide_ids = torch.full((64, L + 3), 1 << 20, dtype=torch.int32, device=dev)
        wide_ids[:, 1:1 + L] = t(s.ids)
        mask = None
        if s.mask is not None:
            mask = torch.full((64, L + 3), float("nan"), device=dev)
            mask[:, 1:1 + L] = t(s.mask)
            mask = mask[:, 1:1 + L]
        segs.append((t(s.table), wide_ids[:, 1:1 + L], s.col, s.pooled, mask, t(s.wide)))
    x, wide = ops.multitable_input(t(c["cont"]), t(c["wc"]), t(c["wb"]), segs, out_dtype=torch.float16)
    assert tuple(x.shape) == (64, c["K0"]) and x.dtype == torch.float16 and x.is_contiguous()
    assert np.array_equal(bits(x), c["ref"]["f16"].view(np.uint32))
    w64, aw, n = c["wide"]
    assert (np.abs(wide.cpu().numpy().astype(np.float64) - w64) <= (n + 1) * 2.0 ** -24 * aw).all()
    wo = torch.empty(64, device=dev)
    x2, w2 = ops.multitable_input(t(c["cont"]), t(c["wc"]), t(c["wb"]), segs, out=torch.empty_like(x), wide_out=wo)
    assert w2.data_ptr() == wo.data_ptr() and torch.equal(w2, wide) and torch.equal(x2, x)
    with pytest.raises(TypeError):
        ops.multitable_input(t(c["cont"]), t(c["wc"]), t(c["wb"]), segs, out=torch.empty((64, c["K0"] + 8), dtype=torch.float16, device=dev))
    with pytest.raises(TypeError):
        ops.multitable_input(t(c["cont"]), t(c["wc"]), t(c["wb"]), [(segs[0][0], segs[0][1].long(), segs[0][2])])
    with pytest.raises(Exception, match="EINVAL"):                            # overlapping blocks: the entry's refusal, as MrecError
        ops.multitable_input(t(c["cont"]), t(c["wc"]), t(c["wb"]), [segs[0], segs[0]])


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_nan_row_reaches_only_the_samples_that_look_it_up(dev, kind):
    from mindrec_amd import ops
    B, V = 64, 40
    rng = np.random.default_rng(7)
    cont = rng.standard_normal((B, 8)).astype(np.float32)
    wc, wb = rng.standard_normal(8).astype(np.float32), rng.standard_normal(1).astype(np.float32)
    t1, t2 = rng.standard_normal((V, 64)).astype(np.float32), rng.standard_normal((V, 128)).astype(np.float32)
    w1, w2 = rng.standard_normal(V).astype(np.float32), rng.standard_normal(V).astype(np.float32)
    i1 = rng.integers(0, V - 1, size=(B, 3)).astype(np.int32)                 # row V - 1 belongs to the poisoned samples alone
    i2 = rng.integers(0, V - 1, size=(B, 5)).astype(np.int32)
    i1[5, 1] = V - 1                                                          # single-hot: sample 5, slot 1
    i2[20, 4] = V - 1                                                         # pooled: sample 20
    m2 = np.ones((B, 5), np.float32)
    segs = [R.Seg(t1, i1, 8, False, None, w1), R.Seg(t2, i2, 200, True, m2, w2)]
    K0 = 328
    clean_x, (clean_w, aw, n) = R.input_row(cont, segs, K0, kind), R.wide_sum(cont, wc, wb, segs)
    t1p, t2p, w1p, w2p = t1.copy(), t2.copy(), w1.copy(), w2.copy()
    t1p[V - 1], t2p[V - 1], w1p[V - 1], w2p[V - 1] = np.nan, np.nan, np.nan, np.nan
    t = lambda a: torch.from_numpy(a).to(dev)
    x, wide = ops.multitable_input(t(cont), t(wc), t(wb), [(t(t1p), t(i1), 8, False, None, t(w1p)), (t(t2p), t(i2), 200, True, t(m2), t(w2p))],
                                   K0=K0, out_dtype=KINDS[kind])
    x, wide = x.float().cpu().numpy(), wide.cpu().numpy()
    exp_nan = np.zeros((B, K0), bool)
    exp_nan[5, 8 + 64:8 + 128] = True
    exp_nan[20, 200:328] = True
    assert np.array_equal(np.isnan(x), exp_nan)
    assert np.array_equal(x[~exp_nan].view(np.uint32), clean_x[~exp_nan].view(np.uint32))
    assert np.array_equal(np.isnan(wide), np.isin(np.arange(B), [5, 20]))
    ok = ~np.isnan(wide)
    assert (np.abs(wide[ok].astype(np.float64) - clean_w[ok]) <= (n + 1) * 2.0 ** -24 * aw[ok]).all()
