"""The FM term's kernels (csrc/mrec_fm.hip: k_fm_fwd4, k_fm_fwd, k_fm_bwd, k_fm_bwd4, k_fm_bwd4_mix) through mindrec_amd.ops at every
lane geometry, BIT FOR BIT against the host restatements of _fm_cases.py (checked without a device by test_fm_ref.py, which also
shows that a tree without its guard, a tree in place, dropped remainder fields or a dropped last lane cannot equal them) and within the
derived float64 bound stated there.  Nothing here is compared with allclose.

Every tensor a kernel writes (fm, the column sums, the gradient, the 16-bit copy) is a view between sentinel values that must come
back untouched; a refused call must leave the views themselves untouched too."""
import numpy as np
import pytest
import torch

import _fm_cases as T

pytestmark = pytest.mark.gpu

SENT = -768.0                                       # (exact in bf16 and f16)
EUNSUPPORTED = -3
DT16 = {"bf16": torch.bfloat16, "f16": torch.float16}


class Held:
    """`a` on the device as a view into a larger buffer: 16 bytes of sentinels (+ `off` elements: the view is then not 16-byte aligned)
    in front, 16 bytes behind"""

    def __init__(self, a, dev, off=0, dtype=torch.float32):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        pad = 16 // t.element_size()
        self.lo, self.n = pad + off, t.numel()
        self.buf = torch.full((self.lo + self.n + pad,), SENT, dtype=dtype, device=dev)
        self.t = self.buf[self.lo:self.lo + self.n].view(t.shape)
        self.t.copy_(t)
        assert self.t.is_contiguous() and (self.t.data_ptr() % 16 == 0) == (off == 0)

    def bits(self):
        """the view's bits, after checking the sentinels around it"""
        b = self.buf.cpu()
        assert bool((b[:self.lo] == SENT).all()) and bool((b[self.lo + self.n:] == SENT).all()), "wrote outside the view"
        v = b[self.lo:self.lo + self.n]
        return v.view(torch.int32 if v.element_size() == 4 else torch.int16).numpy().copy().reshape(self.t.shape)

    def untouched(self):
        return bool((self.buf == SENT).all())


def blank(shape, dev, dtype=torch.float32, off=0):
    return Held(np.full(shape, SENT, np.float32), dev, off, dtype)


def forward(vx, add, dev, off=0, dt16=None):
    """ops.fm_forward into held outputs: (fm bits, colsum bits, out16 bits or None); off: vx starts `off` floats into its buffer"""
    from mindrec_amd import ops
    B, F, D = vx.shape
    hx = Held(vx, dev, off)
    ha = Held(add, dev) if add is not None else None
    hf, hc = blank((B,), dev), blank((B, D), dev)
    h16 = blank((B, F, D), dev, dt16) if dt16 is not None else None
    fm, cs = ops.fm_forward(hx.t, add=ha.t if ha else None, out16=h16.t if h16 else None, out=dict(fm=hf.t, colsum=hc.t))
    assert fm.data_ptr() == hf.t.data_ptr() and cs.data_ptr() == hc.t.data_ptr()
    assert np.array_equal(hx.bits(), T.bits(vx)) and (ha is None or np.array_equal(ha.bits(), T.bits(add)))      # inputs are read only
    return hf.bits(), hc.bits(), (h16.bits() if h16 else None)


def hold_to(restate, vx, add, got_fm, got_cs, what):
    """the device's fm and column sums equal the restatement's bits and meet the float64 bound; returns the worst error / bound"""
    fm, cs = restate(vx, add)
    assert np.array_equal(got_cs, T.bits(cs)), what
    assert np.array_equal(got_fm, T.bits(fm)), (what, int((got_fm != T.bits(fm)).sum()))
    err, bnd = np.abs(got_fm.view(np.float32).astype(np.float64) - T.fm64(vx, add)), T.bound(vx, add)
    ratio = float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0
    assert (err <= bnd).all(), (what, ratio)
    return ratio


def backward(x, cs, dev, off=0):
    """ops.fm_backward_ on a held g: the updated g's bits"""
    from mindrec_amd import ops
    hg, hx, hc, hd = Held(x["g"], dev), Held(x["vx"], dev, off), Held(cs, dev), Held(x["dout"], dev)
    assert ops.fm_backward_(hg.t, hx.t, hc.t, hd.t) is hg.t
    for h, a in ((hx, x["vx"]), (hc, cs), (hd, x["dout"])):
        assert np.array_equal(h.bits(), T.bits(a))
    return hg.bits()


def backward_mix(x, cs, dev, dt):
    """ops.fm_backward_mix into a held output: (its bits, the 16-bit gradient widened to fp32)"""
    from mindrec_amd import ops
    g16 = torch.from_numpy(x["g"]).to(DT16[dt])
    hg, ho = Held(g16.float().numpy(), dev, dtype=DT16[dt]), blank(x["vx"].shape, dev)
    out = ops.fm_backward_mix(hg.t, Held(x["vx"], dev).t, Held(cs, dev).t, Held(x["dout"], dev).t, out=ho.t)
    assert out is ho.t and np.array_equal(hg.bits(), g16.view(torch.int16).numpy())
    return ho.bits(), g16.float().numpy()


def whole_case(case, dev, off=0, restate=None):
    restate = restate or T.restate(case)
    x = T.inputs(case.B, case.F, case.D)
    worst = 0.0
    for add in (None, x["add"]):
        fm, cs, _ = forward(x["vx"], add, dev, off)
        worst = max(worst, hold_to(restate, x["vx"], add, fm, cs, (tuple(case), off, add is not None)))
    cs = T.col_sums(x["vx"])[0]
    assert np.array_equal(backward(x, cs, dev, off), T.bits(T.backward(x["g"], x["vx"], cs, x["dout"]))), case
    if case.D % 4 == 0 and off == 0:
        for dt in DT16:
            got, g = backward_mix(x, cs, dev, dt)
            assert np.array_equal(got, T.bits(T.backward(g, x["vx"], cs, x["dout"]))), (case, dt)
    return worst


@pytest.mark.parametrize("D", T.VEC_D)
def test_vector_path_at_every_lane_group_width(dev, D):
    """k_fm_fwd4, k_fm_bwd4 and k_fm_bwd4_mix: lpr from 1 to 64, spare lanes, G = 1; B on both sides of a workgroup's 4 G samples; the
    field remainder 0, 1 and 3; with and without add"""
    worst = max(whole_case(c, dev) for c in T.vec_cases(D))
    print(f"fm4 D={D}: worst |err| / bound over the cases = {worst:.4f}")


@pytest.mark.parametrize("D", T.SCALAR_D)
def test_scalar_path_by_width(dev, D):
    """k_fm_fwd and k_fm_bwd where D % 4 != 0: one to four guarded columns per lane"""
    worst = max(whole_case(c, dev) for c in T.scalar_cases(D))
    print(f"fm1 D={D}: worst |err| / bound over the cases = {worst:.4f}")


@pytest.mark.parametrize("D", T.MISALIGNED_D)
def test_scalar_path_by_alignment(dev, D):
    """vx a contiguous view one float into its buffer: the scalar kernels run (the result is fm1's sum order, not fm4's), and the column
    sums equal the aligned run's bit for bit"""
    differ = False
    for case in T.scalar_cases(D):
        whole_case(case, dev, off=1, restate=T.fm1)
        x = T.inputs(case.B, case.F, D)
        fm_a, cs_a, _ = forward(x["vx"], x["add"], dev)
        fm_m, cs_m, _ = forward(x["vx"], x["add"], dev, off=1)
        assert np.array_equal(cs_a, cs_m), case
        assert np.array_equal(fm_a, T.bits(T.fm4(x["vx"], x["add"])[0])), case
        differ |= not np.array_equal(fm_a, fm_m)
    assert differ                                   # (the two orders do differ on these inputs: the check above can tell them apart)


@pytest.mark.parametrize("kernel", sorted(T.SECOND_TRIPS))
def test_second_trip_of_every_grid_stride_loop(dev, kernel):
    B, F, D = T.SECOND_TRIPS[kernel]
    x = T.inputs(B, F, D)
    cs = T.col_sums(x["vx"])[0]
    if kernel in ("fwd4", "fwd1"):
        fm, got_cs, _ = forward(x["vx"], x["add"], dev)
        worst = hold_to(T.fm4 if kernel == "fwd4" else T.fm1, x["vx"], x["add"], fm, got_cs, (kernel, B, F, D))
        print(f"{kernel} {B, F, D}: worst |err| / bound = {worst:.4f}")
    elif kernel == "bwd4_mix":
        for dt in DT16:                             # (one instantiation of the kernel per 16-bit type)
            got, g = backward_mix(x, cs, dev, dt)
            assert np.array_equal(got, T.bits(T.backward(g, x["vx"], cs, x["dout"]))), dt
    else:
        assert np.array_equal(backward(x, cs, dev), T.bits(T.backward(x["g"], x["vx"], cs, x["dout"])))


@pytest.mark.parametrize("D", T.COPY_D)
@pytest.mark.parametrize("dt", sorted(DT16))
def test_16bit_copy_is_the_rounded_input(dev, dt, D):
    """out16's bits equal vx.to(dtype) -- on rounding ties, and for f16 above 65504 and below its smallest subnormal --; fm and the
    column sums equal the run without out16 bit for bit"""
    G = T.lanes(D)[1]
    for F in T.COPY_F:
        for B in (1, 4 * G + 1):
            x = T.inputs(B, F, D)
            vx = T.plant(x["vx"], T.BF16_PLANTS if dt == "bf16" else T.F16_PLANTS, seed=F)
            fm0, cs0, _ = forward(vx, x["add"], dev)
            fm1, cs1, got = forward(vx, x["add"], dev, dt16=DT16[dt])
            assert np.array_equal(fm0, fm1) and np.array_equal(cs0, cs1), (B, F, D)
            assert np.array_equal(fm0, T.bits(T.fm4(vx, x["add"])[0])), (B, F, D)
            want = torch.from_numpy(vx).to(DT16[dt]).view(torch.int16).numpy()
            assert np.array_equal(got, want), (B, F, D, int((got != want).sum()))


def _raises_unsupported(fn):
    from mindrec_amd import _lib
    with pytest.raises(_lib.MrecError) as e:
        fn()
    assert e.value.code == EUNSUPPORTED


def test_refusals_raise_and_write_nothing(dev):
    from mindrec_amd import ops
    for D in T.REFUSED_D:                                                                   # wider than 4 columns per lane
        hf, hc = blank((5,), dev), blank((5, D), dev)
        _raises_unsupported(lambda: ops.fm_forward(Held(T.inputs(5, 3, D)["vx"], dev).t, out=dict(fm=hf.t, colsum=hc.t)))
        assert hf.untouched() and hc.untouched()
    # the 16-bit copy rides the vector kernel alone
    for D, off in ((30, 0), (80, 1)):
        x = T.inputs(5, 3, D)
        hf, hc, h16 = blank((5,), dev), blank((5, D), dev), blank((5, 3, D), dev, torch.bfloat16)
        call = lambda: ops.fm_forward(Held(x["vx"], dev, off).t, out16=h16.t, out=dict(fm=hf.t, colsum=hc.t))
        if D % 4:
            with pytest.raises(TypeError):
                call()
        else:
            _raises_unsupported(call)
        assert hf.untouched() and hc.untouched() and h16.untouched()
    # the mixed backward has no scalar kernel: a misaligned operand is refused
    x = T.inputs(5, 3, 80)
    cs = T.col_sums(x["vx"])[0]
    g16 = torch.from_numpy(x["g"]).to(torch.bfloat16).float().numpy()
    for which in ("vx", "colsum", "out", "g16"):
        off = {w: int(w == which) for w in ("vx", "colsum", "out", "g16")}
        ho = blank(x["vx"].shape, dev, off=off["out"])
        hg = Held(g16, dev, 4 * off["g16"] + off["g16"], torch.bfloat16)      # (5 bf16: not 8-byte aligned)
        _raises_unsupported(lambda: ops.fm_backward_mix(hg.t, Held(x["vx"], dev, off["vx"]).t, Held(cs, dev, off["colsum"]).t,
                                                        Held(x["dout"], dev).t, out=ho.t))
        assert ho.untouched(), which


def test_wrappers_refuse_operands_the_flat_index_would_misread(dev):
    """fm_backward_ walks g and colsum by their flat index: a non-contiguous or non-fp32 one would be updated at the wrong elements"""
    from mindrec_amd import ops
    B, F, D = 5, 3, 20
    x = T.inputs(B, F, D)
    cs = T.col_sums(x["vx"])[0]
    t = lambda a, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)
    vx, c, w = t(x["vx"]), t(cs), t(x["dout"])
    wide_g = torch.full((B, F, D + 4), SENT, dtype=torch.float32, device=dev)
    wide_c = torch.full((B, D + 4), SENT, dtype=torch.float32, device=dev)
    g = t(x["g"])
    bad = [
        dict(g=wide_g[:, :, :D]), dict(g=t(x["g"], torch.float16)), dict(g=t(x["g"], torch.float64)), dict(g=g.view(B, F * D)),
        dict(g=t(x["g"][:4])), dict(g=g.permute(1, 0, 2)),
        dict(colsum=wide_c[:, :D]), dict(colsum=t(cs, torch.float64)), dict(colsum=c.view(-1)), dict(colsum=t(cs[:, :16])),
        dict(dout=t(x["dout"], torch.float64)), dict(dout=t(x["dout"][:4])),
        dict(vx=t(x["vx"], torch.float64)), dict(vx=vx.view(B, F * D)),
    ]
    for kw in bad:
        args = dict(g=g, vx=vx, colsum=c, dout=w)
        args.update(kw)
        with pytest.raises(TypeError):
            ops.fm_backward_(**args)
    assert torch.equal(g, t(x["g"])) and bool((wide_g == SENT).all()) and bool((wide_c == SENT).all())
    g16 = t(x["g"], torch.bfloat16)
    for kw in bad[6:]:
        args = dict(g16=g16, vx=vx, colsum=c, dout=w)
        args.update(kw)
        with pytest.raises(TypeError):
            ops.fm_backward_mix(**args)
    for out in (wide_g[:, :, :D], t(x["g"], torch.float64), g.view(B, F * D)):
        with pytest.raises(TypeError):
            ops.fm_backward_mix(g16, vx, c, w, out=out)
    for bad_vx in (t(x["vx"], torch.float64), t(x["vx"], torch.float16), vx.view(B, F * D), vx.view(1, B, F, D)):
        with pytest.raises(TypeError):
            ops.fm_forward(bad_vx)
    for out in (dict(fm=w.double()), dict(colsum=wide_c[:, :D]), dict(fm=t(x["dout"][:4])), dict(colsum=c.view(-1))):
        with pytest.raises(TypeError):
            ops.fm_forward(vx, out=out)
    assert bool((wide_g == SENT).all()) and bool((wide_c == SENT).all())
    # a [B, 1] dout is B values all the same, and a well-formed call still goes through
    ops.fm_backward_(g, vx, c, w.view(B, 1))
    assert np.array_equal(T.bits(g.cpu().numpy()), T.bits(T.backward(x["g"], x["vx"], cs, x["dout"])))


def test_empty_batch(dev):
    from mindrec_amd import ops
    for D in (80, 30):
        vx = torch.empty((0, 3, D), dtype=torch.float32, device=dev)
        fm, cs = ops.fm_forward(vx, add=torch.empty(0, dtype=torch.float32, device=dev))
        assert tuple(fm.shape) == (0,) and tuple(cs.shape) == (0, D) and fm.dtype == cs.dtype == torch.float32
        g = torch.empty_like(vx)
        assert ops.fm_backward_(g, vx, cs, fm) is g
        if D % 4 == 0:
            assert tuple(ops.fm_backward_mix(g.to(torch.bfloat16), vx, cs, fm).shape) == (0, 3, D)
