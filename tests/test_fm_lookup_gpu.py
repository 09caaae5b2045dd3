"""ops.fm_lookup (csrc/mrec_fm.hip: k_fm_lookup, mrec_fm_lookup) -- the DeepFM evaluation forward's lookup, one launch -- against the three
launches it stands for: gather_rows(max_norm=...) -> wide_sum -> fm_forward(add=linear, out16=...).  The kernel keeps every expression
of that composition in its order (the build has -ffp-contract=off), so the rows and lin_fm are compared BIT FOR BIT: integer views
under torch.equal, no tolerance.  For fp32 rows the reference is gather_rows' own output.

Shapes: D in {4, 8, 20, 64, 80, 128, 132, 256} -- lanes per row 1, 2, 5, 16, 20 (idle lanes in the wave), 32, 33, 64, so 16 .. 1 samples
per wave --, F in {1, 3, 4, 5, 39} (the group of four fields and every remainder), B in {1, 3, 13, 257} (less than a wave, a partial
last wave, several workgroups), and D 4 / F 1 with B just past 2048 * 4 * 16, where the capped grid's stride loop takes a second trip."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DS = [4, 8, 20, 64, 80, 128, 132, 256]
FS = [1, 3, 4, 5, 39]
BS = [1, 3, 13, 257]
KINDS = [torch.float32, torch.bfloat16, torch.float16]
V, VW = 61, 47


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _tables(dev, D, seed, strided=False):
    g = torch.Generator().manual_seed(seed)
    if strided:                                   # a view with ld = D + 8 whose first column sits 16 bytes into the buffer's rows
        table = torch.randn((V, D + 8), generator=g).to(dev)[:, 4:4 + D]
        assert table.stride(0) == D + 8 and table.data_ptr() % 16 == 0
    else:
        table = torch.randn((V, D), generator=g).to(dev)
    return table, torch.randn((V, 1), generator=g).to(dev)


def _inputs(dev, B, F, dtype, seed, lo=-1, hi=V):
    """ids in [lo, hi] -- with the defaults -1 and V, the ids just outside the table, among them (placed where the batch has room) --,
    weights with zeros and negative values"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(lo, hi + 1, (B, F), generator=g)
    wts = torch.randn((B, F), generator=g)
    wts[torch.rand((B, F), generator=g) < 0.2] = 0.0
    if B * F >= 4:
        ids.view(-1)[0], ids.view(-1)[-1] = lo, hi
        wts.view(-1)[0], wts.view(-1)[-1], wts.view(-1)[1], wts.view(-1)[2] = -1.5, 0.75, 0.0, -0.25
    return ids.to(dtype).to(dev), wts.to(dev)


def _composition(table, wtable, ids, wts, ids_w, dt, c=None):
    from mindrec_amd import ops
    vx = ops.gather_rows(table, ids, wts, max_norm=c)
    lin = ops.wide_sum(wtable, ids if ids_w is None else ids_w, wts)
    if dt == torch.float32:
        return vx, ops.fm_forward(vx, add=lin)[0]
    rows = torch.empty(vx.shape, dtype=dt, device=vx.device)
    return rows, ops.fm_forward(vx, add=lin, out16=rows)[0]


def _check(table, wtable, ids, wts, dt, ids_w=None, c=None, what=None):
    from mindrec_amd import ops
    rows, lin_fm = ops.fm_lookup(table, wtable, ids, wts, ids_w=ids_w, out_dtype=dt, max_norm=c)
    ref_rows, ref_lin_fm = _composition(table, wtable, ids, wts, ids_w, dt, c)
    B, F = ids.shape
    assert rows.dtype == dt and tuple(rows.shape) == (B, F, table.shape[1]) and tuple(lin_fm.shape) == (B,) and lin_fm.dtype == torch.float32
    assert torch.equal(_bits(rows), _bits(ref_rows)), ("rows", what)
    assert torch.equal(_bits(lin_fm), _bits(ref_lin_fm)), ("lin_fm", what)


@pytest.mark.parametrize("D", DS)
def test_fm_lookup_is_the_three_launch_composition_bit_for_bit(dev, D):
    table, wtable = _tables(dev, D, seed=D)
    for F in FS:
        for B in BS:
            for idt in (torch.int32, torch.int64):
                ids, wts = _inputs(dev, B, F, idt, seed=1000 * F + B)
                for dt in KINDS:
                    _check(table, wtable, ids, wts, dt, what=(D, F, B, idt, dt))


@pytest.mark.parametrize("dt", KINDS, ids=["fp32", "bf16", "f16"])
def test_second_trip_of_the_grid_stride_loop(dev, dt):
    """D = 4: 16 samples a wave, 64 a workgroup; the grid stops at 2048 workgroups = 131072 samples, the rest is a second trip"""
    B = 2048 * 4 * 16 + 37
    table, wtable = _tables(dev, 4, seed=7)
    ids, wts = _inputs(dev, B, 1, torch.int32, seed=8)
    _check(table, wtable, ids, wts, dt, what=dt)


@pytest.mark.parametrize("D", [20, 80, 132])
def test_strided_table_view(dev, D):
    table, wtable = _tables(dev, D, seed=D + 1, strided=True)
    for idt in (torch.int32, torch.int64):
        ids, wts = _inputs(dev, 13, 39, idt, seed=D)
        for dt in KINDS:
            _check(table, wtable, ids, wts, dt, what=(D, idt, dt))
            _check(table, wtable, ids, wts, dt, c=0.9 * float(np.sqrt(D)), what=(D, idt, dt, "clip"))


@pytest.mark.parametrize("D", [8, 80, 256])
def test_ids_w_of_its_own_over_a_table_of_another_size(dev, D):
    """the linear weights looked up at other positions than the rows (the hash engine's two tables number their rows apart); the
    [Vw, 1] table is shorter than V, so an id valid for one table is outside the other"""
    table, _ = _tables(dev, D, seed=D + 2)
    wtable = torch.randn((VW, 1), generator=torch.Generator().manual_seed(D)).to(dev)
    for idt in (torch.int32, torch.int64):
        ids, wts = _inputs(dev, 13, 5, idt, seed=D + 3)
        ids_w, _ = _inputs(dev, 13, 5, idt, seed=D + 4, hi=VW)
        assert not torch.equal(ids, ids_w) and int(ids.max()) > VW
        for dt in KINDS:
            _check(table, wtable, ids, wts, dt, ids_w=ids_w, what=(D, idt, dt))
            _check(table, wtable, ids, wts, dt, ids_w=ids, what=(D, idt, dt, "same ids, passed twice"))


def _bound(table, ids):
    """as tests/test_engine_max_norm_gpu.py::_bound: a bound at the median norm (float64) of the looked-up rows with no row's norm within
    1e-5 (relative) of it -- here the midpoint between the two neighbouring norms of the table around that median, since a table of 61
    rows has the median ON a row's norm more often than not; and the share of looked-up rows above it"""
    n = np.linalg.norm(table.double().cpu().numpy(), axis=1)
    looked = ids.cpu().numpy().reshape(-1)
    looked = looked[(looked >= 0) & (looked < n.size)]
    ns = np.unique(n)
    i = int(np.clip(np.searchsorted(ns, np.median(n[looked]), side="right"), 1, ns.size - 1))
    c = float(0.5 * (ns[i - 1] + ns[i]))
    assert np.abs(n / c - 1.0).min() > 1e-5
    return c, float((n[looked] > c).mean())


@pytest.mark.parametrize("D", DS)
def test_fm_lookup_with_max_norm(dev, D):
    table, wtable = _tables(dev, D, seed=3 * D)
    for F, B in ((39, 13), (5, 257), (1, 3), (4, 1), (3, 13)):
        for idt in (torch.int32, torch.int64):
            ids, wts = _inputs(dev, B, F, idt, seed=F + B)
            c, share = _bound(table, ids)
            if B * F >= 40:
                assert 0.2 < share < 0.8, share                  # both branches of the clip run
            for dt in KINDS:
                _check(table, wtable, ids, wts, dt, c=c, what=(D, F, B, idt, dt))
    # ... and the clip changes the result (the bound is not vacuous)
    from mindrec_amd import ops
    ids, wts = _inputs(dev, 13, 39, torch.int32, seed=52)
    c, share = _bound(table, ids)
    assert 0.2 < share < 0.8, share
    assert not torch.equal(ops.fm_lookup(table, wtable, ids, wts, out_dtype=torch.float32, max_norm=c)[0],
                           ops.fm_lookup(table, wtable, ids, wts, out_dtype=torch.float32)[0])


def test_out_buffers_and_graph_replay(dev):
    """out=: the call fills the dict once and writes the same tensors afterwards; one call captured with them replays, after the inputs
    changed in place, to an eager call's bits"""
    from mindrec_amd import ops
    D, F, B = 80, 39, 13
    table, wtable = _tables(dev, D, seed=11)
    ids, wts = _inputs(dev, B, F, torch.int32, seed=12)
    out = {}
    rows, lin_fm = ops.fm_lookup(table, wtable, ids, wts, out=out, max_norm=8.0)
    assert out["rows"] is rows and out["lin_fm"] is lin_fm and rows.dtype == torch.float16
    ptrs = (rows.data_ptr(), lin_fm.data_ptr())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r2, l2 = ops.fm_lookup(table, wtable, ids, wts, out=out, max_norm=8.0)
    assert (r2.data_ptr(), l2.data_ptr()) == ptrs
    ids_new, wts_new = _inputs(dev, B, F, torch.int32, seed=13)
    assert not torch.equal(ids_new, ids)
    ids.copy_(ids_new)
    wts.copy_(wts_new)
    graph.replay()
    torch.cuda.synchronize()
    ref_rows, ref_lin_fm = ops.fm_lookup(table, wtable, ids_new, wts_new, max_norm=8.0)
    assert torch.equal(_bits(rows), _bits(ref_rows)) and torch.equal(_bits(lin_fm), _bits(ref_lin_fm))
    with pytest.raises(TypeError, match="out\\['rows'\\]"):
        ops.fm_lookup(table, wtable, ids, wts, out=out, out_dtype=torch.bfloat16)


def test_argument_checks(dev):
    from mindrec_amd import ops
    from mindrec_amd._lib import MrecError
    table, wtable = _tables(dev, 8, seed=1)
    ids, wts = _inputs(dev, 3, 4, torch.int32, seed=2)
    with pytest.raises(TypeError):
        ops.fm_lookup(table, wtable, ids.to(torch.int16), wts)
    with pytest.raises(ValueError):
        ops.fm_lookup(table, wtable, ids.view(-1), wts.view(-1))
    with pytest.raises(TypeError):
        ops.fm_lookup(table, wtable.view(1, -1), ids, wts)
    with pytest.raises(TypeError):
        ops.fm_lookup(table, wtable, ids, wts.double())
    with pytest.raises(TypeError):
        ops.fm_lookup(table, wtable, ids, wts, ids_w=ids.long())
    with pytest.raises(TypeError):
        ops.fm_lookup(table, wtable, ids, wts, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.fm_lookup(table, wtable, ids, wts, max_norm=-1.0)
    with pytest.raises(RuntimeError):
        ops.fm_lookup(table.cpu(), wtable, ids, wts)
    with pytest.raises(MrecError, match="EUNSUPPORTED"):
        ops.fm_lookup(torch.randn((V, 6), device=dev), wtable, ids, wts)
    rows, lin_fm = ops.fm_lookup(table, wtable, ids[:0], wts[:0])
    assert tuple(rows.shape) == (0, 4, 8) and tuple(lin_fm.shape) == (0,)
