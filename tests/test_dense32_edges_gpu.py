"""The fp32-MFMA DenseLayer (csrc/mrec_gemm_f32.hip: all 27 (form, VA, VB) instantiations of k_gemm_f32 behind mrec_dense32_fwd,
mrec_dense32_bwd_input and mrec_dense32_bwd_weight) at every load width, edge and slab split.  Cases, generators and the host
restatements: _dense32_edge_cases.py (checked without a device by test_dense32_edges.py).

  exact family     nonzero integers in [-8, 8] whose every partial sum stays below 2^24: the result IS the int64 product, bit for
                   bit, in whatever order the matrix instruction adds -- a K-tile, a row or a term dropped, doubled or read from
                   the wrong place shows
  general family   the inputs and bounds of tests/test_dense32_gpu.py, nothing wider: 1.5 red 2^-24 sum |a| |b| + 2^-23 |ref| (2^-22
                   |ref| for a slab), outputs in the ReLU's corner judged as there
  poison           every operand is a window of a wider buffer whose other columns and rows (and the floats around the bias) are
                   NaN: rows and k outside an operand are switched off through the buffer range check, and a value that leaks in
                   on one side meets the other side's zero -- 0 . NaN = NaN shows it.  Every output is a window of a buffer that
                   holds the sentinel -768; outside the window it comes back bit for bit
  column sums      per 64-row block, not in total: the integer sums on the exact family; on the general family bit-equal to the
                   epilogue's order restated in fp32 over the device's own dx
  slabs            each slab against its own batch rows, for every S the batch admits; the S it does not admit refused, output
                   untouched

Every case written for one pair of load widths asks mrec_dense32_load_widths with the tensors' real addresses and strides, and FAILS
when the launch would pick another."""
import numpy as np
import pytest
import torch

import _dense32_edge_cases as T

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -768.0
SENT_BITS = np.float32(SENT).view(np.uint32)
EINVAL = -1


# ---- windows ------------------------------------------------------------------------------------------------------------------------------
def window(a, off, pad, dev):
    """`a` [rows, ext] on the device as the [FRONT : FRONT + rows, off : off + ext] window of a NaN buffer off + ext + pad wide"""
    rows, ext = a.shape
    buf = torch.full((T.FRONT + rows + T.BACK, off + ext + pad), NAN, dtype=torch.float32, device=dev)
    win = buf[T.FRONT:T.FRONT + rows, off:off + ext]
    win.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return win


def vector(a, dev, fill=NAN):
    """`a` [n] contiguous, four floats of `fill` in front of and behind it"""
    buf = torch.full((a.size + 8,), fill, dtype=torch.float32, device=dev)
    buf[4:4 + a.size] = torch.from_numpy(a)
    return buf[4:4 + a.size]


class Held:
    """an output [*lead, rows, W]: NaN (never written shows) inside a buffer of sentinels -- `off` columns left and `pad` right of
    every row, two rows (of the leading extent: two slabs) in front and behind"""

    def __init__(self, shape, off, pad, dev):
        *lead, rows, W = shape
        self.shape, self.off = tuple(shape), off
        self.buf = torch.full((*[n + 4 for n in lead], rows + (0 if lead else 4), off + W + pad), SENT, dtype=torch.float32, device=dev)
        self.t = self.buf[2:2 + lead[0], :, off:off + W] if lead else self.buf[2:2 + rows, off:off + W]
        self.t.fill_(NAN)

    def read(self, what, written=True):
        g = self.buf.cpu().numpy()
        inside = np.zeros(g.shape, bool)
        *lead, rows, W = self.shape
        if lead:
            inside[2:2 + lead[0], :, self.off:self.off + W] = True
        else:
            inside[2:2 + rows, self.off:self.off + W] = True
        bad = g.view(np.uint32)[~inside] != SENT_BITS
        assert not bad.any(), f"{what}: {int(bad.sum())} floats outside the output's window written, first at {tuple(np.argwhere((g.view(np.uint32) != SENT_BITS) & ~inside)[0])} of {g.shape}"
        out = np.ascontiguousarray(g[inside].reshape(self.shape))
        if written:
            assert not np.isnan(out).any(), f"{what}: {int(np.isnan(out).sum())} of {out.size} elements NaN: never written, or an operand's surroundings read"
        else:
            assert np.isnan(out).all(), f"{what}: output touched"
        return out


def require_widths(form, a, b, want, what):
    """the load widths this launch picks, from the tensors as they are: the library's answer, and the restated rule on what
    ops.dense32_* passes"""
    from mindrec_amd import ops
    got = ops.dense32_load_widths(form, a, b)
    assert got == tuple(T.vec_of(t.data_ptr() % 16, t.stride(0) if t.shape[0] > 1 else t.shape[1], t.shape[1]) for t in (a, b)), what
    assert got == tuple(want), (f"{what}: operands at {a.data_ptr() % 16} / {b.data_ptr() % 16} mod 16, strides {a.stride(0)} / {b.stride(0)}, extents "
                                f"{a.shape[1]} / {b.shape[1]} are loaded (VA, VB) = {got}, this case was written for {tuple(want)}: the layout or the "
                                "allocator's alignment moved -- resize the case, do not drop it")


# ---- one launch of each form -------------------------------------------------------------------------------------------------------------
def run_fwd(dev, d, la, lb, want=None, bias=True, relu=True, out=(1, 2), what="fwd"):
    from mindrec_amd import ops
    x, w = window(d["x"], *la, dev), window(d["w"], *lb, dev)
    if want is not None:
        require_widths(0, x, w, want, what)
    y = Held((x.shape[0], w.shape[1]), *out, dev)
    ops.dense32_fwd(x, w, vector(d["bias"], dev) if bias else None, relu=relu, out=y.t)
    return y.read(what)


def run_dgrad(dev, d, la, lb, want=None, mask=True, colsum=True, out=(1, 2), hl=(2, 1), what="dgrad"):
    """-> (dx, colsum or None)"""
    from mindrec_amd import ops
    dy, w = window(d["dy"], *la, dev), window(d["w"], *lb, dev)
    if want is not None:
        require_widths(1, dy, w, want, what)
    M, K = dy.shape[0], w.shape[0]
    dx = Held((M, K), *out, dev)
    cs = Held((T.cdiv(M, 64), K), 0, 0, dev) if colsum else None
    ops.dense32_bwd_input(dy, w, h=window(d["h"], *hl, dev) if mask else None, out=dx.t, colsum=cs.t if colsum else None)
    got = dx.read(what)
    if not colsum:
        return got, None
    sums = cs.read(what + " colsum")
    assert np.isfinite(sums).all()
    return got, sums


def run_wgrad(dev, d, la, lb, S, want=None, what="wgrad"):
    """-> slabs [S, K, N]"""
    from mindrec_amd import ops
    x, dy = window(d["x"], *la, dev), window(d["dy"], *lb, dev)
    if want is not None:
        require_widths(2, x, dy, want, what)
    slabs = Held((S, x.shape[1], dy.shape[1]), 0, 0, dev)
    assert slabs.t.is_contiguous()
    ops.dense32_bwd_weight(x, dy, slabs.t)
    return slabs.read(what)


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------
def same(got, ref, what):
    """exact family: the device's fp32 result equals the integer result"""
    bad = got.astype(np.float64) != ref
    assert got.shape == ref.shape and not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ from the integer result, first at "
                                                       f"{tuple(np.argwhere(bad)[0])}: {got[bad][0]} for {ref[bad][0]}")


def block_sums(a):
    return np.stack([a[r:r + 64].sum(0) for r in range(0, a.shape[0], 64)])


def exact_fwd(dev, shape, la, lb, want=None, what=""):
    d = T.exact_inputs(0, *shape)
    prod = T.product(0, d)
    same(run_fwd(dev, d, la, lb, want, what=what + " bias relu"), np.maximum(prod + d["bias"], 0.0), what + " bias relu")
    same(run_fwd(dev, d, la, lb, want, bias=False, relu=False, out=(0, 1), what=what + " plain"), prod, what + " plain")


def exact_dgrad(dev, shape, la, lb, want=None, what=""):
    d = T.exact_inputs(1, *shape)
    prod = T.product(1, d)
    masked = np.where(d["h"] > 0, prod, 0.0)
    dx, cs = run_dgrad(dev, d, la, lb, want, what=what + " mask colsum")
    same(dx, masked, what + " mask colsum")
    same(cs, block_sums(masked), what + " column sums per 64 rows")
    dx, _ = run_dgrad(dev, d, la, lb, want, mask=False, colsum=False, out=(2, 3), what=what + " plain")
    same(dx, prod, what + " plain")


def exact_wgrad(dev, shape, la, lb, want=None, what=""):
    d = T.exact_inputs(2, *shape)
    same(run_wgrad(dev, d, la, lb, 1, want, what=what)[0], T.product(2, d), what)


EXACT = {0: exact_fwd, 1: exact_dgrad, 2: exact_wgrad}


def general_fwd(dev, shape, la, lb, want=None, what=""):
    d = T.general_inputs(0, *shape)
    pre, tol, near0 = T.forward_reference(d)
    assert near0.mean() <= T.NEAR0_CAP
    y = run_fwd(dev, d, la, lb, want, what=what + " bias relu")
    assert (np.abs(y - np.maximum(pre, 0.0)) <= tol)[~near0].all() and (np.abs(y) <= 2 * tol)[near0].all(), what + " bias relu"
    y = run_fwd(dev, d, la, lb, want, bias=False, relu=False, what=what + " plain")
    assert (np.abs(y - (pre - d["bias"])) <= tol).all(), what + " plain"


def general_dgrad(dev, shape, la, lb, want=None, what=""):
    d = T.general_inputs(1, *shape)
    full = T.product(1, d)
    tol = T.bound(1, d) + 2.0 ** -23 * np.abs(full)
    dx, cs = run_dgrad(dev, d, la, lb, want, what=what + " mask colsum")
    assert (np.abs(dx - np.where(d["h"] > 0, full, 0.0)) <= tol).all() and (dx[d["h"] <= 0] == 0).all(), what + " mask colsum"
    same_bits(cs, T.colsum_restated(dx), what)
    dx, cs = run_dgrad(dev, d, la, lb, want, mask=False, what=what + " colsum")
    assert (np.abs(dx - full) <= tol).all(), what + " colsum"
    same_bits(cs, T.colsum_restated(dx), what)


def same_bits(cs, want, what):
    bad = cs.view(np.uint32) != want.view(np.uint32)
    assert cs.shape == want.shape and not bad.any(), (f"{what}: column sums of {int(bad.sum())} (64-row block, column) pairs differ from the epilogue's "
                                                       f"order over the device's own dx, first {tuple(np.argwhere(bad)[0])}: {cs[bad][0]!r} for {want[bad][0]!r}")


def check_slabs_general(slabs, d, what):
    """each slab within the bound of the float64 product of its own batch rows"""
    S, M = slabs.shape[0], d["x"].shape[0]
    kps = T.rows_per_slab(M, S)
    for s in range(S):
        ds = dict(x=d["x"][s * kps:(s + 1) * kps], dy=d["dy"][s * kps:(s + 1) * kps])
        ref = T.product(2, ds)
        assert (np.abs(slabs[s] - ref) <= T.bound(2, ds) + 2.0 ** -22 * np.abs(ref)).all(), f"{what}: slab {s} of {S}"


def general_wgrad(dev, shape, la, lb, want=None, what=""):
    d = T.general_inputs(2, *shape)
    check_slabs_general(run_wgrad(dev, d, la, lb, 1, want, what=what), d, what)


GENERAL = {0: general_fwd, 1: general_dgrad, 2: general_wgrad}


# ---- 0. one interior tile, one K-tile -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2])
def test_simplest_exact_case(dev, form):
    EXACT[form](dev, T.SIMPLEST, (0, 4), (0, 4), (4, 4), what=f"form {form} {T.SIMPLEST}")


# ---- 1. + 2. one extent at a time around the base, exact family, every operand poisoned around its window -----------------------------------
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("extent", ["red", "p", "q"])
def test_sweep(dev, form, extent):
    p0, r0, q0 = T.BASE
    cases = {"red": [(p0, r, q0) for r in T.SWEEP_RED], "p": [(p, r0, q0) for p in T.SWEEP_P], "q": [(p0, r0, q) for q in T.SWEEP_Q]}[extent]
    for shape in cases:
        EXACT[form](dev, shape, *T.SWEEP_LAYOUT, what=f"form {form} (M, K, N) = {T.mkn(form, *shape)}")


@pytest.mark.parametrize("form", [0, 1, 2])
def test_poisoned_windows_at_every_column_offset(dev, form):
    """the base case with the operands' windows 0, 1 and 2 floats into their rows (and the output's and h's likewise)"""
    for off in (0, 1, 2):
        for pad in (1, 2):
            what = f"form {form} {T.BASE} offset {off} pad {pad}"
            if form == 0:
                d = T.exact_inputs(0, *T.BASE)
                same(run_fwd(dev, d, (off, pad), (2 - off, pad), out=(off, pad), what=what), np.maximum(T.product(0, d) + d["bias"], 0.0), what)
            elif form == 1:
                d = T.exact_inputs(1, *T.BASE)
                masked = np.where(d["h"] > 0, T.product(1, d), 0.0)
                dx, cs = run_dgrad(dev, d, (off, pad), (2 - off, pad), out=(off, pad), hl=(2 - off, 3 - pad), what=what)
                same(dx, masked, what)
                same(cs, block_sums(masked), what + " column sums")
            else:
                exact_wgrad(dev, T.BASE, (off, pad), (2 - off, pad), what=what)


# ---- 3. all 27 instantiations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2])
def test_every_load_width_pair(dev, form):
    seen = set()
    for f, shape, la, lb, want in T.width_cases():
        if f != form:
            continue
        what = f"form {form} (M, K, N) = {T.mkn(form, *shape)} A at {la} B at {lb} (VA, VB) = {want}"
        EXACT[form](dev, shape, la, lb, want, what=what)
        if want == T.GENERAL_WIDTHS[form]:
            GENERAL[form](dev, shape, la, lb, want, what=what + " general")
        seen.add(want)
    assert seen == {(a, b) for a in (4, 2, 1) for b in (4, 2, 1)} and T.GENERAL_WIDTHS[form] in seen


# ---- 4. column sums per 64-row block --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", T.COLSUM_M)
def test_column_sums_per_block(dev, M):
    shape = (M, T.BASE[1], T.BASE[2])                    # dx [M, 130]: two column tiles, the second two columns wide
    what = f"dgrad (M, K, N) = {T.mkn(1, *shape)}"
    exact_dgrad(dev, shape, (0, 2), (1, 2), what=what)
    general_dgrad(dev, shape, (0, 2), (0, 4), what=what + " general")


# ---- 5. weight-gradient slabs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", T.SLAB_M)
@pytest.mark.parametrize("K,N", T.SLAB_KN)
def test_slab_splits(dev, M, K, N):
    from mindrec_amd import _lib, ops
    ok, refused = T.slab_counts(M)
    assert ok[0] == 1 and len(ok) + len(refused) == T.cdiv(M, 32)
    la, lb = (0, 2), (1, 3)
    d = T.exact_inputs(2, K, M, N)
    for S in ok:
        what = f"wgrad (M, K, N) = ({M}, {K}, {N}) S = {S}"
        slabs = run_wgrad(dev, d, la, lb, S, what=what)
        kps = T.rows_per_slab(M, S)
        for s in range(S):
            rows = slice(s * kps, (s + 1) * kps)
            same(slabs[s], T.product(2, dict(x=d["x"][rows], dy=d["dy"][rows])), f"{what} slab {s} (batch rows {s * kps} .. {min(M, (s + 1) * kps) - 1})")
    for S in refused + [T.cdiv(M, 32) + 1]:
        x, dy = window(d["x"], *la, dev), window(d["dy"], *lb, dev)
        slabs = Held((S, K, N), 0, 0, dev)
        with pytest.raises(_lib.MrecError) as e:
            ops.dense32_bwd_weight(x, dy, slabs.t)
        assert e.value.code == EINVAL
        slabs.read(f"refused S = {S}", written=False)
    # general inputs at the proposed count and at the finest split the batch admits
    g = T.general_inputs(2, K, M, N)
    proposed = ops.dense32_bwd_weight_slabs(M, K, N)
    assert proposed == T.proposed_slabs(M, K, N) and proposed in ok
    for S in sorted({proposed, ok[-1]}):
        what = f"wgrad (M, K, N) = ({M}, {K}, {N}) S = {S} general"
        check_slabs_general(run_wgrad(dev, g, la, lb, S, what=what), g, what)


def test_empty_batch_zero_fills_the_slabs(dev):
    from mindrec_amd import ops
    K, N = T.SLAB_KN[0]
    for S in (1, 3):
        slabs = Held((S, K, N), 0, 0, dev)
        ops.dense32_bwd_weight(torch.empty((0, K), dtype=torch.float32, device=dev), torch.empty((0, N), dtype=torch.float32, device=dev), slabs.t)
        out = slabs.read(f"M = 0, S = {S}")
        assert (out.view(np.uint32) == 0).all()


# ---- 6. the same launch twice ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2])
def test_repeatable(dev, form):
    from mindrec_amd import ops
    d = {k: torch.from_numpy(v).to(dev) for k, v in T.general_inputs(form, *T.BASE).items()}
    outs = []
    for _ in range(2):
        if form == 0:
            outs.append([ops.dense32_fwd(d["x"], d["w"], d["bias"], relu=True)])
        elif form == 1:
            cs = torch.empty((T.cdiv(T.BASE[0], 64), T.BASE[2]), dtype=torch.float32, device=dev)
            outs.append([ops.dense32_bwd_input(d["dy"], d["w"], h=d["h"], colsum=cs), cs])
        else:
            outs.append([ops.dense32_bwd_weight(d["x"], d["dy"], torch.empty((1, T.BASE[0], T.BASE[2]), dtype=torch.float32, device=dev))])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    GENERAL[form](dev, T.BASE, (0, 2), (0, 2), what=f"form {form} {T.BASE} general")
