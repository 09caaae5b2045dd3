"""The dense Adam launch's dispatch, every path of it: the float4 kernels with their scalar remainder (16-byte aligned buffers) and the
scalar kernel alone (views one element into a larger buffer), fp32 and bf16 gradients, with and without the bf16 shadow, the one
element that belongs to FTRL on either side of the vector / remainder seam -- bit for bit against the oracle -- and the entries that
are faces of one launch against each other.  Every view sits between sentinel floats that must come back untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_dense_optim_abi as abi  # noqa: E402

SENT = -768.0                                       # (exact in bf16 too)
KW = dict(lr=1e-4, beta1_power=0.81, beta2_power=0.998, grad_scale=1e-3)
OKW = dict(lr=1e-4, b1_pow=0.81, b2_pow=0.998, grad_scale=1e-3)
FTRL = dict(lr=5e-2, l1=1e-8, l2=1e-8, lr_power=-0.5)
EINVAL = -1


class Held:
    """`a` on the device as a view into a larger buffer: 16 bytes of sentinels (+ `off` elements: the view is then NOT 16-byte, for
    a 16-bit dtype not even 4-byte, aligned) in front, 16 bytes behind."""

    def __init__(self, a, dev, off=0, dtype=torch.float32):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        pad = 16 // t.element_size()
        self.lo, self.n = pad + off, t.numel()
        self.buf = torch.full((self.lo + self.n + pad,), SENT, dtype=dtype, device=dev)
        self.t = self.buf[self.lo:self.lo + self.n]
        self.t.copy_(t)
        assert (self.t.data_ptr() % 16 == 0) == (off == 0)

    def bits(self):
        """the view's bits, after checking the sentinels around it"""
        b = self.buf.cpu()
        assert bool((b[:self.lo] == SENT).all()) and bool((b[self.lo + self.n:] == SENT).all()), "wrote outside the view"
        v = b[self.lo:self.lo + self.n]
        return v.view(torch.int32 if v.element_size() == 4 else torch.int16).numpy().copy()


def f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def state(rng, n):
    p = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.random(n) * 0.01).astype(np.float32)
    g = (rng.standard_normal(n) * 1000).astype(np.float32)
    return p, m, v, g


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("off", [0, 1])
def test_dense_adam_every_path_against_the_oracle(dev, oracle, off, gdt, shadow):
    from mindrec_amd import ops
    rng = np.random.default_rng(21)
    for n in (1, 3, 4, 5, 1027):
        p, m, v, g = state(rng, n)
        g = torch.from_numpy(g).to(gdt).float().numpy()                     # (the values the device widens a bf16 gradient to)
        hp, hm, hv = (Held(x, dev, off) for x in (p, m, v))
        hg = Held(g, dev, off, gdt)
        hs = Held(np.zeros(n, np.float32), dev, off, torch.bfloat16) if shadow else None
        ops.dense_adam_(hp.t, hm.t, hv.t, hg.t, shadow_bf16=hs.t if shadow else None, **KW)
        oracle.dense_adam(p, m, v, g, **OKW)
        for h, want in ((hp, p), (hm, m), (hv, v)):
            assert np.array_equal(h.bits(), f32bits(want)), (n, off)
        assert np.array_equal(hg.bits(), Held(g, dev, off, gdt).bits())
        if shadow:
            assert np.array_equal(hs.bits(), torch.from_numpy(p).to(torch.bfloat16).view(torch.int16).numpy()), (n, off)


@pytest.mark.parametrize("off", [0, 1])
def test_one_ftrl_element_on_both_sides_of_the_vector_seam(dev, oracle, off):
    """n = 1027: 256 float4 vectors and a remainder of 3 where the buffers are aligned, 1027 scalar elements where they are not"""
    from mindrec_amd import ops
    n = 1027
    rng = np.random.default_rng(22)
    p0, m0, v0, g = state(rng, n)
    m0 = np.abs(m0) + np.float32(0.1)                                       # (FTRL's accum where the element is FTRL's)

    def run(ftrl1):
        hs = [Held(x, dev, off) for x in (p0, m0, v0, g)]
        ops.dense_adam_(*(h.t for h in hs), ftrl1=ftrl1, **KW)
        out = [h.bits() for h in hs]
        assert np.array_equal(out[3], f32bits(g))
        return out[:3]

    plain = run(None)
    for a, b in zip(plain, run((-1, *FTRL.values()))):
        assert np.array_equal(a, b)
    adam = [x.copy() for x in (p0, m0, v0)]
    oracle.dense_adam(*adam, g, **OKW)
    for a, b in zip(plain, adam):
        assert np.array_equal(a, f32bits(b))
    for idx in (0, 5, 1023, 1024, 1026):
        want = [x.copy() for x in adam]
        one = [x[idx:idx + 1].copy() for x in (p0, m0, v0)]
        oracle.dense_ftrl(*one, g[idx:idx + 1], grad_scale=KW["grad_scale"], **FTRL)
        for w, o in zip(want, one):
            w[idx] = o[0]
        assert f32bits(want[0])[idx] != f32bits(adam[0])[idx]
        for a, b in zip(run((idx, *FTRL.values())), want):
            assert np.array_equal(a, f32bits(b)), (idx, off)
    with pytest.raises(TypeError):                                          # no FTRL element under a bf16 gradient
        ops.dense_adam_(*(Held(x, dev).t for x in (p0, m0, v0)), Held(g, dev, 0, torch.bfloat16).t, ftrl1=(0, *FTRL.values()), **KW)


HYPER = (1e-4, 0.9, 0.999, 1e-8, 0.81, 0.998, 1e-3, 0)                      # lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov


def test_three_faces_of_the_dense_adam_launch(dev):
    from mindrec_amd import _lib, ops
    n = 1027
    x = state(np.random.default_rng(23), n)
    outs = []
    for face in ("mrec_dense_adam_f32", "mrec_dense_adam_ex_f32", "mrec_dense_adam_one_ftrl_f32"):
        hs = [Held(a, dev) for a in x]
        p, m, v, g = (ops._ptr(h.t) for h in hs)
        if face == "mrec_dense_adam_f32":
            _lib.call(face, p, m, v, g, n, *HYPER, ops._stream())
        elif face == "mrec_dense_adam_ex_f32":
            _lib.call(face, p, m, v, g, 0, None, n, *HYPER, ops._stream())
        else:
            _lib.call(face, p, m, v, g, n, *HYPER, None, ops._stream())
        outs.append([h.bits() for h in hs])
    assert not np.array_equal(outs[0][0], f32bits(x[0]))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


def slab_args(dev, starts, parts):
    k = len(parts)
    ptrs, st, ln, sp = (C.c_void_p * k)(), (C.c_int64 * k)(), (C.c_int64 * k)(), (C.c_int32 * k)()
    for q, (s, part) in enumerate(zip(starts, parts)):
        ptrs[q], st[q], ln[q], sp[q] = part.data_ptr(), s, part[0].numel(), part.shape[0]
    return [C.cast(a, C.c_void_p) for a in (ptrs, st, ln, sp)]


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_two_faces_of_the_slabs_launch(dev, kind):
    from mindrec_amd import _lib, ops
    n = 1028
    rng = np.random.default_rng(24)
    x = state(rng, n)
    slabs = torch.from_numpy(rng.standard_normal((3, 64)).astype(np.float32)).to(dev)
    outs = []
    for face in ("mrec_dense_adam_slabs_f32", "mrec_dense_adam_slabs_one_ftrl_f32"):
        hs = [Held(a, dev) for a in x]
        sh = Held(np.zeros(n, np.float32), dev, 0, (None, torch.bfloat16, torch.float16)[kind]) if kind else None
        args = (*(ops._ptr(h.t) for h in hs), ops._ptr(sh.t) if kind else None, kind, n, 1, *slab_args(dev, [512], [slabs]), *HYPER, None)
        if face.endswith("one_ftrl_f32"):
            args += (None,)
        _lib.call(face, *args, ops._stream())
        outs.append([h.bits() for h in hs] + ([sh.bits()] if kind else []))
    assert not np.array_equal(outs[0][0][512:576], f32bits(x[0])[512:576])
    if kind:
        assert outs[0][4].any()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_slabs_finish_refuses_what_the_slabs_entry_refuses(dev):
    """mrec_dense_adam_slabs_finish_f32 with a real finish record: the bad-segment rows of test_dense_optim_abi.py and a bad
    one-FTRL record are MREC_EINVAL before anything runs; then the record is spent by a valid call."""
    from mindrec_amd import _lib, ops
    rng = np.random.default_rng(3)
    V, D, B, F, ld = 5000, 80, 512, 39, 256
    ids = np.minimum(rng.zipf(1.1, size=(B, F)) + 12, V - 1)
    ids[:, :13] = np.arange(13)
    tid = torch.from_numpy(ids).to(dev, torch.int32)
    wts = torch.from_numpy(rng.random((B, F)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((B * F, D)).astype(np.float32)).to(dev, torch.bfloat16)
    gw = torch.from_numpy(rng.standard_normal(B).astype(np.float32)).to(dev)
    st = torch.from_numpy(rng.standard_normal((V, ld)).astype(np.float32) * 0.01).to(dev)
    st[:, D + 1] = 1.0
    st[:, 2 * D + 4:3 * D + 4] = st[:, 2 * D + 4:3 * D + 4].abs()
    kw = dict(lr=3.5e-4, beta1_power=0.9, beta2_power=0.999, grad_scale=1 / 1024)
    plan = ops.sparse_plan(tid)
    fin = ops.sparse_lazy_adam_wide_(st[:, :D], st[:, D + 4:2 * D + 4], st[:, 2 * D + 4:3 * D + 4], plan, g, wts, gw, F, D, defer=True, **kw)
    n = abi.N
    hs = [Held(a, dev) for a in state(rng, n)]
    hs[2].t.abs_()
    slab = torch.zeros((3, 8), device=dev)
    finp = C.cast(C.pointer(fin), C.c_void_p)
    l = _lib.lib()

    def finish(nseg, slab_ptr, start, length, split, gp, one=None):
        s = [C.cast(a, C.c_void_p) for a in abi.seg_arrays(nseg, slab_ptr, start, length, split)]
        return l.mrec_dense_adam_slabs_finish_f32(ops._ptr(hs[0].t), ops._ptr(hs[1].t), ops._ptr(hs[2].t), gp, None, 0, n, nseg, *s,
                                                  *abi.HYPER, None, C.cast(C.pointer(one), C.c_void_p) if one is not None else None, finp,
                                                  ops._stream())

    good = slab.data_ptr()
    before = [h.bits() for h in hs]
    for row, (args, code) in sorted(abi.SEGMENT_ROWS.items()):
        if code != EINVAL:
            continue
        nseg, slab_ptr, start, length, split, _ = args
        bad = {abi.A: good, abi.A + 8: good + 8, None: None}[slab_ptr]
        assert finish(nseg, bad, start, length, split, hs[3].t.data_ptr()) == EINVAL, row
    assert finish(1, good, 0, 8, 3, hs[3].t.data_ptr(), abi.Ftrl1(n, 5e-2, 1e-8, 1e-8, -0.5)) == EINVAL          # index = n
    assert finish(1, good, 0, 8, 3, hs[3].t.data_ptr() + 4) == -3                  # g not 16-byte aligned: MREC_EUNSUPPORTED
    # ... and judged before the record is (the slabs entry without a finish judges the record first)
    assert finish(1, good, 0, 8, 3, hs[3].t.data_ptr() + 4, abi.Ftrl1(n, 5e-2, 1e-8, 1e-8, -0.5)) == -3
    torch.cuda.synchronize()
    for h, b in zip(hs, before):
        assert np.array_equal(h.bits(), b)                                  # nothing ran
    ops.dense_adam_slabs_(*(h.t for h in hs), [(0, slab)], finish=fin, **kw)
    torch.cuda.synchronize()
    assert not np.array_equal(hs[0].bits(), before[0])
