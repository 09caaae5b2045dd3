"""The DCN-v1 cross stack (mrec_cross.hip) at every width bucket, every backward (bucket, depth bound) kernel, the batch sizes
at which its loops change shape, and depths past the backward's 8 layers -- against tests/_cross_ref.py.

Bars.  Forward: row_rel(out, float64 stack) <= 1e-5 (include/mrec.h).  Backward, each of dx0 / dw / db:
    err_gpu <= max(4 * err_closed32, 16 * 2^-24)
where err_closed32 is the error of the closed form evaluated in float32 on the host (numpy's summation order) against the
same float64 gradient: the kernel and that restatement evaluate the same expressions in the same precision and differ in
the order of their additions only, which 4x covers; the floor is a few units in the last place for cases where the
restatement happens to land exactly.

Reach of the parameter lists, counted from the dispatch in mrec_cross.hip:
  forward   k_cross_fwd<Lane1<1|2>, LDS> (one column per lane); k_cross_fwd<Lane4<4|8|12|16|20|24|32>, LDS> (four columns per lane,
            L <= 8) and <Lane4<4|8|12|16|20|24|32>, global> (L > 8; D = 2048 at L = 11 is also past the LDS-size condition): 16
            of the 18 instantiations.  k_cross_fwd<Lane1<1|2>, global> needs 2 L DP 4 > 160 KB at DP <= 128, i.e. L > 160: not
            reachable at a test's size, not run.  test_forward_bit_for_bit holds both layouts, and the global form of Lane4, to
            _cross_ref.cross_fwd_bits bit for bit.
  backward  k_cross_bwd<4|8|16|20|32, LT = 2|4|6|8>: all 20, each at L = LT and at L = LT - 1.

Largest err_gpu / err_closed32 observed on an MI355X over the 90 backward cases of this module (the bar allows 4):
    dx0 3.17 (B=70 D=65 L=3: 1.82e-6 against 5.76e-7)    dw 2.12 (B=70 D=5 L=1, under the floor)    db 1.80 (B=1 D=300 L=6, under
    the floor).  Closest to its bar: dx0 at 0.79 of it (the same case), dw 0.29, db 0.30.  Largest forward error: 2.0e-6
    (B=40 D=30 L=16).
"""
import functools

import numpy as np
import pytest
import torch

import _cross_ref as R

pytestmark = pytest.mark.gpu

FWD_BAR = 1e-5
FLOOR = 16 * 2.0 ** -24
GUARD = 64                      # sentinel floats on each side of a view
SENT = 7777.25


def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)         # a copy: the cached arrays are read-only


@functools.lru_cache(maxsize=None)
def case(B, D, L):
    """Inputs, the float64 results and the float32 restatement's distance from them: computed once per shape, read-only."""
    x0, w, b, dy = R.inputs(B, D, L)
    y, dx0, dw, db = R.cross_f64(x0, w, b, dy)
    closed = R.cross_bwd_closed_f32(x0, w, b, dy) if L <= 8 else None
    c = {"x0": x0, "w": w, "b": b, "dy": dy, "y": y, "dx0": dx0, "dw": dw, "db": db}
    if closed is not None:
        c["closed_err"] = (R.row_rel(closed[0], dx0), R.layer_rel(closed[1], dw), R.layer_rel(closed[2], db))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def poison_workspace(B, D, L, dev):
    """NaN into the cached workspace the backward is about to get: a slab word read but not written shows in dw / db."""
    from mindrec_amd import _lib, ops
    nb = _lib.query_bytes("mrec_cross_layers_bwd_workspace_bytes", L, B, D)
    ws = ops.workspace("cross", nb, dev)
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))


def check_fwd(c, out, what):
    out = out.cpu().numpy()
    assert not np.isnan(out).any(), what
    err = R.row_rel(out, c["y"])
    print(f"CROSSFWD {what} err {err:.3e}")
    assert err <= FWD_BAR, (what, err)


def check_bwd(c, dx0, dw, db, what):
    got = (dx0.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy())
    ref = (c["dx0"], c["dw"], c["db"])
    bad = []
    for name, g, r, ec, metric in zip(("dx0", "dw", "db"), got, ref, c["closed_err"], (R.row_rel, R.layer_rel, R.layer_rel)):
        assert not np.isnan(g).any(), (what, name)
        e = metric(g, r)
        bar = max(4 * ec, FLOOR)
        print(f"CROSSBWD {what} {name} err_gpu {e:.3e} err_closed32 {ec:.3e} ratio {e / max(ec, 1e-300):.2f} bar {bar:.3e}")
        if e > bar:
            bad.append((name, e, ec, bar))
    assert not bad, (what, bad)


def run_both(dev, B, D, L):
    from mindrec_amd import ops
    c = case(B, D, L)
    what = f"B={B} D={D} L={L}"
    x0, w, b, dy = (T(c[k], dev) for k in ("x0", "w", "b", "dy"))
    check_fwd(c, ops.cross_layers(x0, w, b), what)
    poison_workspace(B, D, L, dev)
    check_bwd(c, *ops.cross_layers_bwd(x0, w, b, dy), what)


# both sides of every forward bucket edge (64 x {1, 2, 4, 8, 12, 16, 20, 24}), then the ends and the residues mod 4; the depths
# 1 .. 8 all appear
WIDTHS = [(64, 6), (65, 3), (128, 8), (129, 1), (256, 2), (257, 7), (512, 4), (513, 5), (768, 6), (769, 2), (1024, 1), (1025, 8),
          (1280, 3), (1281, 4), (1536, 5), (1537, 7),
          (1, 3), (2, 8), (3, 5), (5, 1), (66, 2), (67, 4), (1170, 6), (2047, 7), (2048, 8)]


@pytest.mark.parametrize("D,L", WIDTHS)
def test_width_sweep(dev, D, L):
    """70 rows: two backward blocks, the second with rows in six of its eight waves."""
    assert sorted({l for _, l in WIDTHS}) == list(range(1, 9))
    run_both(dev, 70, D, L)


# one width per backward bucket (4, 8, 16, 20, 32 x 64 columns); the width sweep has widths off a multiple of 4 in every one
# of them (67, 257, 769, 1170, 1537)
@pytest.mark.parametrize("L", range(1, 9))
@pytest.mark.parametrize("D", [200, 300, 769, 1170, 1537])
def test_backward_instantiation_grid(dev, D, L):
    """Every k_cross_bwd<bucket, LT> at L = LT and at L = LT - 1 (the guarded layer slot of the LT-sized arrays)."""
    run_both(dev, 70, D, L)


@pytest.mark.parametrize("B", [1, 7, 8, 9, 33, 63, 64, 65, 2113, 8200])
@pytest.mark.parametrize("D,L", [(67, 3), (300, 6)])
def test_batch_edges(dev, D, L, B):
    """Fewer rows than waves, the forward's 32-row and the backward's 64-row block; 2113 rows = 34 slabs (the finish kernel's
    strided slab loop turns twice); 8200 rows: the forward's grid-stride loop takes a second pass with no second row, the
    backward walks up to eight rows per wave."""
    run_both(dev, B, D, L)


def guarded(dev, shapes, lead=0):
    """One flat NaN buffer holding a view per shape, GUARD sentinels in front of the first (then `lead` more floats, to move
    the views off 16-byte alignment), between them and directly behind the last row of each.  -> flat, views, guard slices."""
    sizes = [int(np.prod(s)) for s in shapes]
    flat = torch.full((GUARD + lead + sum(sizes) + GUARD * len(sizes),), float("nan"), dtype=torch.float32, device=dev)
    flat[: GUARD + lead] = SENT
    guards, views, off = [slice(0, GUARD + lead)], [], GUARD + lead
    for s, n in zip(shapes, sizes):
        views.append(flat[off:off + n].view(s))
        off += n
        flat[off:off + GUARD] = SENT
        guards.append(slice(off, off + GUARD))
        off += GUARD
    assert off == flat.numel() and all(v.is_contiguous() for v in views)
    return flat, views, guards


def assert_guards(flat, views, guards, what):
    for k, g in enumerate(guards):
        assert bool((flat[g] == SENT).all()), (what, "sentinel zone", k)
    for k, v in enumerate(views):
        assert not bool(torch.isnan(v).any()), (what, "unwritten element in view", k)


def offset_input(a, dev):
    """a at a one-float offset inside a NaN buffer: a read past a row's end that the range check does not zero-fill, or in
    front of the tensor, poisons the result."""
    buf = torch.full((GUARD + 1 + a.size + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    v = buf[GUARD + 1: GUARD + 1 + a.size].view(a.shape)
    v.copy_(T(a, dev))
    assert v.data_ptr() % 16 == 4
    return v


# D = 3, 67: one column per lane (4-byte accesses); 1170, 2047: four columns per lane (16-byte accesses); lead = 1: bases 4- but not 16-byte aligned
@pytest.mark.parametrize("D,L,lead", [(3, 3, 0), (67, 5, 1), (1170, 6, 0), (2047, 8, 1), (1170, 7, 3)])
def test_written_exactly_once_nowhere_else(dev, D, L, lead):
    from mindrec_amd import ops
    B = 70
    c = case(B, D, L)
    what = f"B={B} D={D} L={L} lead={lead}"
    x0, dy = offset_input(c["x0"], dev), offset_input(c["dy"], dev)
    w, b = T(c["w"], dev), T(c["b"], dev)
    # forward into a guarded out=
    flat, (out,), guards = guarded(dev, [(B, D)], lead)
    assert out.data_ptr() % 16 == (4 * lead) % 16
    assert ops.cross_layers(x0, w, b, out=out) is out
    assert_guards(flat, [out], guards, what + " fwd")
    check_fwd(c, out, what)
    # backward into guarded views of one flat buffer, its workspace poisoned
    flat, (dx0, dw, db), guards = guarded(dev, [(B, D), (L, D), (L, D)], lead)
    poison_workspace(B, D, L, dev)
    ops.cross_layers_bwd(x0, w, b, dy, dx0_out=dx0, dw_out=dw, db_out=db)
    assert_guards(flat, [dx0, dw, db], guards, what + " bwd")
    check_bwd(c, dx0, dw, db, what)
    # run to run, bit for bit
    flat2, (dx0b, dwb, dbb), guards2 = guarded(dev, [(B, D), (L, D), (L, D)], lead)
    poison_workspace(B, D, L, dev)
    ops.cross_layers_bwd(x0, w, b, dy, dx0_out=dx0b, dw_out=dwb, db_out=dbb)
    assert_guards(flat2, [dx0b, dwb, dbb], guards2, what + " bwd again")
    assert torch.equal(dx0b, dx0) and torch.equal(dwb, dw) and torch.equal(dbb, db)
    # dx0 += ...: onto another branch's gradient the same sum to the bit, dw and db identical between the two entry points
    base = np.random.default_rng([D, L, 7]).standard_normal((B, D)).astype(np.float32)
    flat3, (acc, dw3, db3), guards3 = guarded(dev, [(B, D), (L, D), (L, D)], lead)
    acc.copy_(T(base, dev))
    poison_workspace(B, D, L, dev)
    ops.cross_layers_bwd(x0, w, b, dy, dx0_out=acc, dw_out=dw3, db_out=db3, accumulate=True)
    assert_guards(flat3, [acc, dw3, db3], guards3, what + " bwd accumulate")
    assert np.array_equal(acc.cpu().numpy(), base + dx0.cpu().numpy())
    assert torch.equal(dw3, dw) and torch.equal(db3, db)


@functools.lru_cache(maxsize=None)
def bits_case(B, D, L):
    x0, w, b, _ = R.inputs(B, D, L)
    want = R.cross_fwd_bits(x0, w, b)
    for v in (x0, w, b, want):
        v.setflags(write=False)
    return x0, w, b, want


@pytest.mark.parametrize("D,L", R.BITS_DL)
@pytest.mark.parametrize("B", R.BITS_B)
def test_forward_bit_for_bit(dev, B, D, L):
    """The forward's bits: ops.cross_layers against _cross_ref.cross_fwd_bits, the kernel's order of operations restated in
    float32 -- lane ownership, slot order and, per layout, its own wave sum (the butterfly at one column per lane, the lane-order
    tree at four).  The evaluation kernel's logit is held bit for bit to a dot with THIS output (test_dcn_predict_gpu.py)."""
    from mindrec_amd import ops
    x0, w, b, want = bits_case(B, D, L)
    got = ops.cross_layers(T(x0, dev), T(w, dev), T(b, dev)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    differ = got.view(np.int32) != want.view(np.int32)
    print(f"CROSSBITS B={B} D={D} L={L} elements that differ: {int(differ.sum())} of {differ.size}")
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (B, D, L, int(differ.sum()))


def test_out_argument_is_checked(dev):
    from mindrec_amd import ops
    x0 = torch.zeros((4, 6), device=dev); w = torch.zeros((2, 6), device=dev)
    for bad in (torch.zeros((4, 5), device=dev), torch.zeros((4, 6), dtype=torch.float64, device=dev),
                torch.zeros((4, 12), device=dev)[:, ::2]):
        with pytest.raises(TypeError):
            ops.cross_layers(x0, w, w, out=bad)


# The forward takes any depth.  Past 8 layers the four-column layout (D > 128) reads w / b from global memory, layer by layer;
# D = 30, 100 stay on the one-column layout's LDS form, whose staging loop has no depth bound (its global form would need L > 160:
# not run).  The
# bias is non-zero: a stack that loses or garbles b_7, b_8 .. is far outside the bar.
@pytest.mark.parametrize("L", [9, 12, 16])
@pytest.mark.parametrize("D", [30, 100, 1170, 1537])
def test_forward_past_eight_layers(dev, D, L):
    _deep_forward(dev, 40, D, L)


@pytest.mark.parametrize("D", [129, 257, 513, 769, 1281])
def test_forward_global_form_in_the_other_buckets(dev, D):
    """k_cross_fwd<Lane4<4|8|12|16|24>, global> (1170 and 1537 above are buckets 20 and 32), each at its narrowest width."""
    _deep_forward(dev, 40, D, 9)


def test_forward_stack_too_large_for_lds(dev):
    """L = 11 at D = 2048: 2 * 11 * 2048 * 4 bytes = 176 KB of w and b, more than the 160 KB of LDS."""
    _deep_forward(dev, 40, 2048, 11)


def _deep_forward(dev, B, D, L):
    from mindrec_amd import ops
    c = case(B, D, L)
    assert np.abs(c["b"][7:]).min() > 0
    what = f"B={B} D={D} L={L}"
    flat, (out,), guards = guarded(dev, [(B, D)], 1)
    ops.cross_layers(offset_input(c["x0"], dev), T(c["w"], dev), T(c["b"], dev), out=out)
    assert_guards(flat, [out], guards, what)
    check_fwd(c, out, what)


def test_backward_past_eight_layers_is_refused(dev):
    from mindrec_amd import _lib, ops
    B, D, L = 40, 100, 9
    c = case(B, D, L)
    dx0 = torch.full((B, D), SENT, device=dev); dw = torch.full((L, D), SENT, device=dev); db = torch.full((L, D), SENT, device=dev)
    with pytest.raises(_lib.MrecError) as e:
        ops.cross_layers_bwd(T(c["x0"], dev), T(c["w"], dev), T(c["b"], dev), T(c["dy"], dev), dx0_out=dx0, dw_out=dw, db_out=db)
    assert e.value.code == -3                                   # MREC_EUNSUPPORTED
    torch.cuda.synchronize()
    for t in (dx0, dw, db):
        assert bool((t == SENT).all())
