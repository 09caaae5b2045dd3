"""The fused tail launch (mrec_tail_fwd_bwd: csrc/mrec_tail.hip k_tail + k_tail_finish), its weight pack and the output head
(csrc/mrec_mlp.hip) against float64 restatements -- cases and input families from _tail_cases.py (checked without a device by
test_tail_oracle.py), EPS16 / TINY and the elementwise bounds from tests/test_dense_gpu.py.

The tail writes y2, logit, dlogit, dz4, dz3, dz2.  Every stage is compared with the oracle fed the GPU's OWN output of the stage
before, so a rounding flip cannot travel and each stage has a bound that is derived:

  y2      |y2 - round16(relu(x . w2 + b2))| <= delta2 = ulp16 + TINY + 2 K 2^-24 (|x| . |w2| + |b2|)         (test_dense_gpu.py)
          With Dropout the kernel rounds, scales, rounds again, zeroes (oracle.dropout of the rounded value).  Scale-and-round is
          monotone, so the value lies between the oracle's Dropout of (ref - delta2, not below 0) and of (ref + delta2): the same
          bound taken through the Dropout, with nothing added.  > 98 % of the elements are the reference's value exactly.
  logit   y3 never leaves LDS: y3_ref = the same restatement on y2_gpu (layer + 2 mask), delta3_k its bound as above.  The kernel's z =
          fl(sum_k y3_k w5_k) + b5 + wv, wv the fp32 field-order sum + wide_b (restated exactly on the host).  Against z_ref = y3_ref . w5
          + b5 + wv in float64: replacing y3 by y3_ref moves the dot product by at most sum_k |w5_k| delta3_k; the N3 products and N3 +
          2 adds of the kernel, in any order, each round once: (N3 + 3) 2^-24 times the sum of the magnitudes; the F field adds are
          restated in their order, and F 2^-24 more covers any other.  Hence
              |z_gpu - z_ref| <= sum_k |w5_k| delta3_k + (N3 + F + 3) 2^-24 (sum_k |y3_ref_k w5_k| + |b5| + sum_f |prod_f| + |wide_b|)
          The field order itself is pinned exactly: the launch given the host's fp32 field-order sum as a per-sample wide value must
          return the same logit bits.
  dlogit  the oracle's value at z_gpu, rtol 1e-4 / atol 1e-7 (test_head_fwd_bwd).
  dw5     the one visible handle on y3: against y3_ref^T . dlogit_gpu within sum_b |dl_b| delta3_b + B 2^-24 (|y3_ref|^T . |dl|).
  dz4     the kernel's fp32 arithmetic restated in np.float32: round16((dl_gpu * w5) * dh_scale); every element is exactly that or
          exactly 0, and it is nonzero exactly where y3_ref > 0 -- except where |y2 . w3 + b3| <= delta3: there the kernel's ReLU may
          fall on either side (at most 0.5 % of a case: asserted for the inputs by test_tail_oracle.py, and here).
  dz3 dz2 oracle.dense_bwd_input(dz4_gpu, w3, y2_gpu) and (dz3_gpu, w2, x) within ulp16 + TINY + 2 N 2^-24 (|dy| . |w|^T) [/ keep]
          (test_dense_bwd_input_matches_oracle); exactly +0 wherever the activation is not positive (negative values and -0.0 in x).
  sums    db3, db2 (of the rounded dz3, dz2), db4 (of the UNROUNDED fp32 values, restated), db5 (of dlogit), loss (mean of the
          per-sample loss at z_gpu): against the float64 sum of the GPU's own rows within the any-order bound B 2^-24 sum |terms|
          (loss: relative 1e-5); dwide_bias_out == db5 bit for bit.

Every output is an interior window of a sentinel-filled flat buffer with a guard row on either side; x is a view of a NaN-filled
buffer."""
import ctypes as C

import numpy as np
import pytest
import torch

import _tail_cases as T
from _tail_cases import K2, N2, N3, PW, U
from test_dense_gpu import DT, EPS16, TINY

pytestmark = pytest.mark.gpu

FILL = 7.0
NAN = float("nan")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _t16(a, dt, dev):
    return _t(a, dev).to(DT[dt])


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def _from_bits(p, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(p)).to(dev).view(DT[dt])


# ---- guarded windows ----------------------------------------------------------------------------------------------------------------
def _win(shape, dtype, dev, fill):
    """(flat buffer, interior window of `shape`, guard length): one guard row before and after"""
    n, g = int(np.prod(shape)), int(shape[-1]) if len(shape) > 1 else 64
    buf = torch.full((n + 2 * g,), fill, dtype=dtype, device=dev)
    return buf, buf[g:g + n].view(shape), g


def _read(buf, win, g, what):
    a = buf.float().cpu().numpy()
    guard = np.concatenate([a[:g], a[g + win.numel():]])
    assert (np.isnan(guard).all() if np.isnan(a[0]) else (guard == FILL).all()), f"{what}: written outside its window"
    out = a[g:g + win.numel()].reshape(tuple(win.shape))
    assert not np.isnan(out).any(), f"{what}: elements never written"
    return out


def _x_view(x, dt, pad, dev):
    buf = torch.full((x.shape[0] + 1, K2 + pad), NAN, dtype=DT[dt], device=dev)
    buf[:-1, :K2] = _t16(x, dt, dev)
    return buf[:-1, :K2]


def _drop(ops, case):
    if not case.drop:
        return None
    keep, row0, layer = case.drop
    return ops.Dropout(keep, T.SEED, layer, step=T.STEP, row0=row0)


def _run(ops, dev, dt, case, inp, wide=None, wb=None):
    """the launch through ops.tail_fwd_bwd with every output a guarded window; dict of numpy arrays (16-bit ones widened to fp32)"""
    B = case.B
    wide = inp["wide"] if wide is None else wide
    wb = inp["wb"] if wide is inp["wide"] else wb
    packed = ops.tail_pack_weights(_t16(inp["w2"], dt, dev), _t16(inp["w3"], dt, dev))
    wins = {n: _win(s, DT[dt], dev, FILL) for n, s in (("y2", (B, N2)), ("dz4", (B, N3)), ("dz3", (B, N2)), ("dz2", (B, K2)))}
    wins.update({n: _win(s, torch.float32, dev, NAN) for n, s in (("logit", (B,)), ("dlogit", (B,)), ("dw5", (N3,)), ("db4", (N3,)),
                                                                   ("db5", (1,)), ("db3", (N2,)), ("db2", (K2,)), ("dwb", (1,)), ("loss", (1,)))})
    w = {n: v[1] for n, v in wins.items()}
    out = {n: w[n] for n in ("y2", "dz4", "dz3", "dz2", "logit", "dlogit", "loss")}
    x = _x_view(inp["x"], dt, case.pad, dev)
    assert x.stride(0) == K2 + case.pad
    ops.tail_fwd_bwd(x, packed, _t(inp["b2"], dev), _t(inp["b3"], dev), _t(inp["w5"], dev), _t(inp["b5"], dev), _t(wide, dev),
                     None if wb is None else _t(np.float32([wb]), dev), _t(inp["label"], dev), inp["dscale"], w["dw5"], w["db4"], w["db5"],
                     w["db3"], w["db2"], dwide_bias_out=w["dwb"] if wb is not None else None, drop_in=_drop(ops, case), out=out)
    torch.cuda.synchronize()
    res = {n: _read(b, v, g, n) for n, (b, v, g) in wins.items() if n != "dwb" or wb is not None}
    res["zero_bits"] = {n: _bits(w[n]) == 0 for n in ("dz4", "dz3", "dz2")}
    return res


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def _restated_o(inp, case, g, dt, oracle):
    """the head's fp32 arithmetic on the GPU's dlogit: (o32 unrounded, o16 = round16(o32))"""
    o32 = (g["dlogit"].astype(np.float32)[:, None] * inp["w5"][None, :]) * np.float32(T.drop_scale(case))
    assert o32.dtype == np.float32
    return o32, oracle.round16(o32, dt)


def _check_rows(oracle, case, dt, inp, g, sl, stats):
    """every per-row output of the rows sl, stage by stage"""
    what = (case.name, dt, sl.start)
    exact = case.family == "int"
    x, y2, dz4, dz3, dz2 = inp["x"][sl], g["y2"][sl], g["dz4"][sl], g["dz3"][sl], g["dz2"][sl]
    scale = T.drop_scale(case)
    # y2
    s2 = T.stage(oracle, x, inp["w2"], inp["b2"], dt, T.masks(oracle, case, sl, 1), EPS16[dt], TINY[dt])
    assert np.all((y2 >= s2["lo"]) & (y2 <= s2["hi"])), (what, "y2", float(np.abs(y2 - s2["ref"]).max()))
    assert np.mean(y2 == s2["ref"]) > 0.98, (what, "y2 exactly rounded share")
    if case.drop:
        m1 = T.masks(oracle, case, sl, 1)
        assert not y2[m1 == 0].any() and (y2[m1 > 0] > 0).mean() > 0.2
    # y3 (in LDS) from the GPU's y2, and the logit
    s3 = T.stage(oracle, y2, inp["w3"], inp["b3"], dt, T.masks(oracle, case, sl, 2), EPS16[dt], TINY[dt])
    y3 = s3["ref"].astype(np.float64)
    w5 = inp["w5"].astype(np.float64)
    F = case.F
    if F:
        wv = T.wide_sum_f32(inp["wide"][sl], inp["wb"]).astype(np.float64)
        wmag = np.abs(inp["wide"][sl][:, :, 0]).astype(np.float64).sum(1) + abs(float(inp["wb"]))
    else:
        wv = inp["wide"][sl].astype(np.float64)
        wmag = np.abs(wv)
    z_ref = y3 @ w5 + float(inp["b5"][0]) + wv
    z_bound = s3["dev"] @ np.abs(w5) + (N3 + F + 3) * U * (np.abs(y3 * w5[None, :]).sum(1) + abs(float(inp["b5"][0])) + wmag)
    z = g["logit"][sl].astype(np.float64)
    assert np.all(np.abs(z - z_ref) <= z_bound), (what, "logit", float((np.abs(z - z_ref) / z_bound).max()))
    # dlogit at the GPU's logit
    y = inp["label"][sl].astype(np.float64)
    dl_ref = (1.0 / (1.0 + np.exp(-z)) - y) * inp["dscale"]
    assert np.allclose(g["dlogit"][sl], dl_ref, rtol=1e-4, atol=1e-7), (what, "dlogit")
    # dz4: exactly the restated value or exactly 0; the zeros where y3_ref is not positive
    o32, o16 = _restated_o(inp, case, {"dlogit": g["dlogit"][sl]}, dt, oracle)
    assert np.all((dz4 == o16) | g["zero_bits"]["dz4"][sl]), (what, "dz4 values")
    open_ = np.zeros_like(o16, bool) if exact else T.undecidable(s3)
    stats["open"] += int(open_.sum()); stats["n"] += open_.size
    look = ~open_ & (o16 != 0)
    assert np.array_equal((dz4 != 0)[look], (y3 > 0)[look]), (what, "dz4 zero pattern", int(((dz4 != 0) != (y3 > 0))[look].sum()))
    assert (y3 > 0)[look].any() and not (y3 > 0)[look].all()
    # dz3, dz2
    for name, dx, dy, w, h in (("dz3", dz3, dz4, inp["w3"], y2), ("dz2", dz2, dz3, inp["w2"], x)):
        ref, _ = oracle.dense_bwd_input(dy, w, h, dt, scale)
        bound = EPS16[dt] * np.abs(ref) + TINY[dt] + 2 * w.shape[1] * U * scale * (np.abs(dy).astype(np.float64) @ np.abs(w).T)
        assert np.all(np.abs(dx.astype(np.float64) - ref) <= bound), (what, name, float((np.abs(dx - ref) / bound).max()))
        assert g["zero_bits"][name][sl][~(h > 0)].all(), (what, name, "not +0 where the activation is not positive")
        nz = np.abs(ref) > bound
        assert np.array_equal((dx != 0)[nz], (h > 0)[nz]) and (dx != 0).any(), (what, name, "zero pattern")
    if exact:
        assert np.array_equal(y2, s2["ref"]), (what, "y2 bit for bit")
        assert np.array_equal(g["logit"][sl], z_ref.astype(np.float32)), (what, "logit bit for bit")
    return s3


def _check_sums(oracle, case, dt, inp, g):
    what = (case.name, dt)
    B = case.B

    def close(name, terms, slack=0.0):
        terms = terms.astype(np.float64)
        tol = B * U * np.abs(terms).sum(0) + slack + 1e-30
        assert np.all(np.abs(g[name].astype(np.float64) - terms.sum(0)) <= tol), (what, name, float((np.abs(g[name] - terms.sum(0)) / tol).max()))
    close("db3", g["dz3"])
    close("db2", g["dz2"])
    # db4 adds the unrounded values where the mask is open, and dz4 shows the mask wherever the rounded value is not 0 itself (a
    # saturated sigmoid makes dlogit, and with it a whole row of dz4, exactly 0: such terms may or may not have been added)
    o32, o16 = _restated_o(inp, case, g, dt, oracle)
    assert (o16 != 0).mean() > 0.9
    close("db4", np.where(g["dz4"] != 0, o32, np.float32(0)), slack=np.where(o16 == 0, np.abs(o32), 0).astype(np.float64).sum(0))
    close("db5", g["dlogit"][:, None])
    z, y = g["logit"].astype(np.float64), inp["label"].astype(np.float64)
    loss = (np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))).mean()
    assert abs(float(g["loss"][0]) - loss) <= 1e-5 * abs(loss), (what, "loss")
    if case.F:
        assert g["dwb"].view(np.int32)[0] == g["db5"].view(np.int32)[0], (what, "dwide_bias_out")
    # dw5 against y3_ref of ALL rows (from the GPU's y2)
    sl = slice(0, B)
    s3 = T.stage(oracle, g["y2"], inp["w3"], inp["b3"], dt, T.masks(oracle, case, sl, 2), EPS16[dt], TINY[dt])
    dl = g["dlogit"].astype(np.float64)
    ref = s3["ref"].astype(np.float64).T @ dl
    bound = s3["dev"].T @ np.abs(dl) + B * U * (np.abs(s3["ref"]).astype(np.float64).T @ np.abs(dl)) + 1e-30
    assert np.all(np.abs(g["dw5"] - ref) <= bound), (what, "dw5", float((np.abs(g["dw5"] - ref) / bound).max()))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_tail_stage_by_stage(dev, oracle, name, dt):
    from mindrec_amd import ops
    case = T.BY_NAME[name]
    inp = T.inputs(oracle, case, dt)
    g = _run(ops, dev, dt, case, inp)
    stats = {"open": 0, "n": 0}
    for sl in T.tiles(case.B):
        _check_rows(oracle, case, dt, inp, g, sl, stats)
    assert stats["open"] <= T.UNDECIDABLE_CAP * stats["n"], (name, dt, stats)
    _check_sums(oracle, case, dt, inp, g)
    if case.F and case.B <= T.FULL_ORACLE_B:
        # the field order, exactly: the same launch on the host's fp32 field-order sum as a per-sample wide value
        h = _run(ops, dev, dt, case, inp, wide=T.wide_sum_f32(inp["wide"], inp["wb"]))
        for n in ("logit", "dlogit", "dz4", "dz3", "dz2", "y2"):
            assert np.array_equal(g[n].view(np.int32), h[n].view(np.int32)), (name, dt, n, "products in field order")


# ---- the pack -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_pack_layout_equals_the_host_restatement(dev, dt):
    from mindrec_amd import ops
    p2, p3 = T.index_patterns(K2, N2), T.index_patterns(N2, N3, first=40009)
    ref = T.pack_ref(p2, p3)
    w2, w3 = _from_bits(p2, dt, dev), _from_bits(p3, dt, dev)
    assert np.array_equal(_bits(ops.tail_pack_weights(w2, w3)), ref)
    for n_t in (0, 3, 4):               # the transposes' first_block selection sees q = 2 and 3
        srcs = [_from_bits(T.index_patterns(r, c, first=977 * k), dt, dev) for k, (r, c) in enumerate(T.TRANSPOSE_SHAPES[:n_t])]
        dsts = [torch.full((s.shape[1] + 1, s.shape[0]), FILL, dtype=DT[dt], device=dev) for s in srcs]
        buf, packed, gd = _win((ref.size,), DT[dt], dev, FILL)
        ops.operand_copies([(s, d[:-1]) for s, d in zip(srcs, dsts)], tail=(w2, w3, packed))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(packed), ref), n_t
        a = buf.float().cpu().numpy()
        assert (a[:gd] == FILL).all() and (a[gd + ref.size:] == FILL).all()
        for s, d in zip(srcs, dsts):
            assert np.array_equal(_bits(d[:-1]), _bits(s.t().contiguous())), (n_t, tuple(s.shape))
            assert (d[-1].float() == FILL).all()
    # the transposes alone, four of them
    srcs = [_from_bits(T.index_patterns(r, c, first=31 * k), dt, dev) for k, (r, c) in enumerate(T.TRANSPOSE_SHAPES)]
    dsts = [torch.empty((s.shape[1], s.shape[0]), dtype=DT[dt], device=dev) for s in srcs]
    ops.operand_copies(list(zip(srcs, dsts)))
    for s, d in zip(srcs, dsts):
        assert np.array_equal(_bits(d), _bits(s.t().contiguous()))


# ---- the C ABI: workspace window, refusals -----------------------------------------------------------------------------------------
class _Abi:
    """the arguments of mrec_tail_fwd_bwd over buffers large enough for EVERY batch used below (a refusal that failed to refuse would
    still stay inside them), outputs sentinel-filled"""
    ROWS = 64 * 513

    def __init__(self, dev, oracle, dt="bf16"):
        from mindrec_amd import ops
        self.dev, self.dt = dev, dt
        case = T.Case("abi", 64, 0, 0, None, "rand")
        self.inp = inp = T.inputs(oracle, case, dt)
        R = self.ROWS
        self.x = torch.zeros((R + 1) * K2 + 8, dtype=DT[dt], device=dev)
        self.x[:64 * K2] = _t16(inp["x"], dt, dev).reshape(-1)
        self.packed = ops.tail_pack_weights(_t16(inp["w2"], dt, dev), _t16(inp["w3"], dt, dev))
        self.b2, self.b3, self.b5 = _t(inp["b2"], dev), _t(inp["b3"], dev), _t(inp["b5"], dev)
        self.w5 = torch.zeros(N3 + 4, device=dev)
        self.w5[:N3] = _t(inp["w5"], dev)
        self.wide = torch.zeros(R, device=dev)
        self.wprod = torch.zeros((R, 65, 2), device=dev)
        self.wb = torch.zeros(1, device=dev)
        self.label = torch.zeros(R, device=dev)
        self.out16 = {n: torch.full((R, w), FILL, dtype=DT[dt], device=dev) for n, w in (("y2", N2), ("dz4", N3), ("dz3", N2), ("dz2", K2))}
        self.out32 = {n: torch.full((k,), FILL, device=dev) for n, k in (("logit", R), ("dlogit", R), ("dw5", N3), ("db4", N3), ("db5", 1),
                                                                         ("dwb", 1), ("loss", 1), ("db3", N2), ("db2", K2))}
        self.ws = torch.full((R // 64 * PW + 2 * PW,), FILL, device=dev)

    def untouched(self):
        return all(bool((t == FILL).all()) for t in list(self.out16.values()) + list(self.out32.values()) + [self.ws])

    def call(self, B=64, K=(K2, N2, N3), ldx=K2, F=0, prod=False, bias=True, w5_off=0, x_off=0, ws_bytes=None, ws_off=PW, drop=None):
        from mindrec_amd import _lib, ops
        p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
        o16, o32 = self.out16, self.out32
        if ws_bytes is None:
            ws_bytes = max(B, 64) // 64 * PW * 4
        d = ops._drop_ref(drop) if drop is not None else None
        return _lib.lib().mrec_tail_fwd_bwd(int(self.dt == "f16"), p(self.x, 2 * x_off), ldx, p(self.packed), p(self.b2), p(self.b3), p(self.w5, 4 * w5_off),
                                            p(self.b5), None if prod else p(self.wide), p(self.wprod) if prod else None, F, p(self.wb) if bias else None,
                                            p(self.label), B, K[0], K[1], K[2], 16.0, p(o16["y2"]), p(o16["dz4"]), p(o16["dz3"]), p(o16["dz2"]),
                                            p(o32["logit"]), p(o32["dlogit"]), p(o32["dw5"]), p(o32["db4"]), p(o32["db5"]), p(o32["dwb"]), p(o32["loss"]),
                                            p(o32["db3"]), p(o32["db2"]), p(self.ws, 4 * ws_off), ws_bytes, d, None)


def test_refusals_over_the_c_abi(dev, oracle):
    from mindrec_amd import _lib, ops
    a = _Abi(dev, oracle)
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
    refused = [
        ("B = 0", dict(B=0), (EINVAL,)),
        ("B = 100", dict(B=100), (EUNSUPPORTED,)),
        ("B = 64 * 513", dict(B=64 * 513), (EUNSUPPORTED,)),
        ("K2", dict(K=(256, N2, N3)), (EUNSUPPORTED,)),
        ("N2", dict(K=(K2, 128, N3)), (EUNSUPPORTED,)),
        ("N3", dict(K=(K2, N2, 64)), (EUNSUPPORTED,)),
        ("F = 65", dict(F=65, prod=True), (EUNSUPPORTED,)),
        ("F = 0 with products", dict(F=0, prod=True), (EINVAL,)),
        ("products without a bias", dict(F=26, prod=True, bias=False), (EINVAL,)),
        ("w5 offset by one float", dict(w5_off=1), (EUNSUPPORTED,)),
        ("x offset by one element", dict(x_off=1), (EUNSUPPORTED,)),
        ("ldx = K2 + 4", dict(ldx=K2 + 4), (EUNSUPPORTED,)),
        ("ldx < K2", dict(ldx=K2 - 8), (EINVAL,)),
        ("workspace not 16-byte aligned", dict(ws_off=PW + 1), (EUNSUPPORTED,)),
        ("workspace one byte short", dict(ws_bytes=PW * 4 - 1), (EWORKSPACE,)),
        ("workspace one byte short, B = 128", dict(B=128, ws_bytes=2 * PW * 4 - 1), (EWORKSPACE,)),
        ("dropout layer 14", dict(drop=ops.Dropout(0.5, T.SEED, 14, step=T.STEP)), (EINVAL,)),
    ]
    for what, kw, codes in refused:
        rc = a.call(**kw)
        assert rc in codes, (what, rc)
    torch.cuda.synchronize()
    assert a.untouched(), "a refused call wrote an output"
    # through the Python layer: a view whose row stride is no multiple of 8 elements
    big = torch.zeros((64, K2 + 4), dtype=torch.bfloat16, device=dev)
    z = lambda n: torch.zeros(n, device=dev)
    with pytest.raises(_lib.MrecError) as e:
        ops.tail_fwd_bwd(big[:, :K2], a.packed, a.b2, a.b3, a.w5[:N3], a.b5, a.wide[:64], None, a.label[:64], 1.0, z(N3), z(N3), z(1), z(N2), z(K2))
    assert e.value.code == EUNSUPPORTED


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_workspace_window_and_highest_dropout_layer(dev, oracle, dt):
    """over the C ABI: the partial rows are a window of a sentinel-filled buffer, exactly B / 64 rows are written, the two pad columns
    hold 0; the finishing pass's sums are the partial rows added in workgroup order; Dropout layer 13 is accepted"""
    from mindrec_amd import ops
    a = _Abi(dev, oracle, dt)
    for B, drop in ((64, None), (128, ops.Dropout(0.5, T.SEED, 13, step=T.STEP))):
        a.ws.fill_(FILL)
        assert a.call(B=B, drop=drop) == 0
        torch.cuda.synchronize()
        ws = a.ws.cpu().numpy()
        nb = B // 64
        assert (ws[:PW] == FILL).all() and (ws[PW * (1 + nb):] == FILL).all(), "workspace written outside its window"
        rows = ws[PW:PW * (1 + nb)].reshape(nb, PW)
        assert np.isfinite(rows).all() and not (rows[:, 2 * N3 + 2:2 * N3 + 4] != 0).any()
        assert (rows[:, :2 * N3 + 2] != FILL).all()
        for n, t in a.out16.items():
            assert bool((t[B:] == FILL).all()) and bool(torch.isfinite(t[:B].float()).all()), n
        for n in ("logit", "dlogit"):
            assert bool((a.out32[n][B:] == FILL).all()), n
        # the finishing pass adds the partial rows in workgroup order: the same bits as the host's sequential fp32 sum
        acc = rows[0].copy()
        for r in rows[1:]:
            acc = acc + r
        assert np.array_equal(a.out32["dw5"].cpu().numpy(), acc[:N3]) and np.array_equal(a.out32["db4"].cpu().numpy(), acc[N3:2 * N3])
        assert a.out32["db5"].cpu().numpy()[0] == acc[2 * N3] and a.out32["loss"].cpu().numpy()[0] == np.float32(acc[2 * N3 + 1] * np.float32(1.0 / B))
        assert np.array_equal(a.out32["db3"].cpu().numpy(), acc[2 * N3 + 4:2 * N3 + 4 + N2]) and np.array_equal(a.out32["db2"].cpu().numpy(), acc[2 * N3 + 4 + N2:])


# ---- the head at every lane-group size ---------------------------------------------------------------------------------------------
HEAD_K5 = [8, 16, 32, 64, 128, 256, 512]
HEAD_B = [1, 2, 63, 65, 257, 1000]


def _head_inputs(rng, B, K5, kind, oracle):
    h4 = np.maximum(rng.standard_normal((B, K5)), 0).astype(np.float32)
    if kind != "f32":
        h4 = oracle.round16(h4, kind)
    # |w5| bounded away from 0 (no f16 underflow of dh4 to 0) and scaled so that the logit stays of order 1 at every K5
    w5 = (rng.choice([-1.0, 1.0], K5) * (0.02 + 0.1 * np.abs(rng.standard_normal(K5))) * min(1.0, (128.0 / K5) ** 0.5)).astype(np.float32)
    return h4, w5, np.float32([0.05]), (rng.standard_normal(B) * 0.3).astype(np.float32), (rng.random(B) < 0.3).astype(np.float32)


def _head_dev(h4, kind, dev):
    return _t(h4, dev) if kind == "f32" else _t16(h4, kind, dev)


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5", HEAD_K5)
def test_head_matches_oracle_at_every_lane_group(dev, oracle, K5, kind):
    """tolerances: exactly those of test_head_fwd_bwd (16-bit) and test_head_fwd_bwd_fp32"""
    from mindrec_amd import ops
    assert ops.head_supported(K5)
    for B in HEAD_B:
        for dhs in (1.0, 2.0):
            rng = np.random.default_rng([K5, B, int(dhs)])
            h4, w5, b5, wide, label = _head_inputs(rng, B, K5, kind, oracle)
            dscale = 1.0 / B if kind == "f32" else 1024.0 / B
            dw5 = torch.empty(K5, device=dev); db4 = torch.empty(K5, device=dev); db5 = torch.empty(1, device=dev)
            loss, logit, dlogit, dh4 = ops.head_fwd_bwd(_head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), _t(wide, dev), _t(label, dev), dscale,
                                                        dw5, db4, db5, dh_scale=dhs)
            r = oracle.head_fwd_bwd(h4, w5, b5[0], wide, label, dscale, dh_scale=dhs)
            what = (K5, kind, B, dhs)
            assert abs(float(loss) - r["loss"]) <= 1e-5 * abs(r["loss"]), what
            assert np.allclose(logit.cpu().numpy(), r["logit"], rtol=1e-5, atol=1e-5), what
            got = dh4.float().cpu().numpy()
            assert np.array_equal(got == 0, r["dh4"] == 0), what
            if kind == "f32":
                assert dh4.dtype == torch.float32
                assert np.allclose(dlogit.cpu().numpy(), r["dlogit"], rtol=1e-4, atol=1e-9), what
                assert np.allclose(got, r["dh4"], rtol=1e-4, atol=1e-10), what
                assert np.abs(db4.cpu().numpy() - r["db4"]).max() <= 1e-4 * np.abs(r["db4"]).max(), what
                assert abs(float(db5) - r["db5"]) <= 1e-4 * max(abs(r["db5"]), 1e-6), what
            else:
                assert np.allclose(dlogit.cpu().numpy(), r["dlogit"], rtol=1e-4, atol=1e-7), what
                assert np.allclose(got, r["dh4"], rtol=1e-2, atol=1e-6), what
                assert np.abs(db4.cpu().numpy() - r["db4"]).max() <= 1e-2 * np.abs(r["db4"]).max(), what
                assert abs(float(db5) - r["db5"]) <= 1e-4 * max(abs(r["db5"]), 1e-3), what
            assert np.abs(dw5.cpu().numpy() - r["dw5"]).max() <= 1e-4 * np.abs(r["dw5"]).max(), what


def test_head_refuses_other_widths(dev):
    from mindrec_amd import _lib, ops
    for K5 in (24, 520):
        assert not ops.head_supported(K5)
        z = lambda *s: torch.zeros(s, device=dev)
        dh_before = torch.zeros((4, K5), dtype=torch.bfloat16, device=dev)
        with pytest.raises(_lib.MrecError) as e:
            ops.head_fwd_bwd(dh_before, z(K5), z(1), z(4), z(4), 1.0, z(K5), z(K5), z(1))
        assert e.value.code == -3


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("K5", HEAD_K5)
def test_head_wide_equals_head_on_the_field_order_sum(dev, oracle, K5, dt):
    from mindrec_amd import ops
    CG = K5 // 8
    for F in sorted({f for f in (1, CG - 1, CG, CG + 1, 2 * CG + 1, 64, 100) if f > 0}):
        for B in (1, 65, 257):
            rng = np.random.default_rng([K5, F, B])
            h4, w5, b5, _, label = _head_inputs(rng, B, K5, dt, oracle)
            prod = np.zeros((B, F, 2), np.float32)
            prod[:, :, 0] = (rng.standard_normal((B, F)) * 10.0 ** rng.uniform(-4, 0, (B, F))).astype(np.float32)
            wb = np.float32(-0.2)
            outs = []
            for mode in ("prod", "sum"):
                dw5 = torch.zeros(K5, device=dev); db4 = torch.zeros(K5, device=dev); db5 = torch.zeros(1, device=dev)
                dwb = torch.full((1,), NAN, device=dev)
                args = (_t(label, dev), 1024.0 / B, dw5, db4, db5)
                if mode == "prod":
                    r = ops.head_fwd_bwd_wide(_t16(h4, dt, dev), _t(w5, dev), _t(b5, dev), _t(prod, dev), _t(np.float32([wb]), dev), *args,
                                              dwide_bias_out=dwb, dh_scale=2.0)
                    assert torch.equal(dwb, db5), (K5, F, B)
                else:
                    r = ops.head_fwd_bwd(_t16(h4, dt, dev), _t(w5, dev), _t(b5, dev), _t(T.wide_sum_f32(prod, wb), dev), *args, dh_scale=2.0)
                outs.append([t.clone() for t in r[1:]] + [db5])
            for n, x, y in zip(("logit", "dlogit", "dh4", "db5"), *outs):
                assert torch.equal(x, y), (K5, dt, F, B, n)
