"""The output head for any last hidden width (csrc/mrec_mlp.hip: k_head_any + k_head_finish, mrec_head_fwd_bwd_any) against the
float64 restatement oracle.head_fwd_bwd, on the input recipe of test_tail_oracle_gpu.py's _head_inputs (restated below).

Widths: non-power-of-two lane groups (24, 40, 72, 136: groups of 4, 8, 16, 32 lanes with lanes that own nothing), 63 / 64 / 65
chunks of 8 values a row (504, 512, 520), every number of chunks a lane (1: <= 512, 2: <= 1024, 3: <= 1536, 4: <= 2048) and the last
chunk of a lane absent (520, 1000, 1032, 2040).

Tolerances: those of test_head_matches_oracle_at_every_lane_group, unchanged.  They bound batch reductions over the same B, and a
K5-term fp32 dot whose inputs the recipe scales so that the logit stays of order 1.  The logit bound (rtol = atol = 1e-5) was checked
on the CPU at every (K5, B, kind) below before it was relied on: numpy's float32 dot of the same inputs, and a strictly sequential
float32 sum (the worst order), both + b5 + wide in float32, against the float64 oracle -- the largest deviation is 0.22 of the bound
(at K5 = 2040), so the bound stands at every width."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
KIND = {"bf16": 0, "f16": 1, "f32": 2}
HEAD_K5 = [8, 24, 40, 72, 136, 400, 504, 512, 520, 1000, 1024, 1032, 1536, 2040, 2048]
HEAD_B = [1, 2, 63, 65, 257, 1000]
FILL = 7.0


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _head_inputs(rng, B, K5, kind, oracle):
    h4 = np.maximum(rng.standard_normal((B, K5)), 0).astype(np.float32)
    if kind != "f32":
        h4 = oracle.round16(h4, kind)
    # |w5| bounded away from 0 (no f16 underflow of dh4 to 0) and scaled so that the logit stays of order 1 at every K5
    w5 = (rng.choice([-1.0, 1.0], K5) * (0.02 + 0.1 * np.abs(rng.standard_normal(K5))) * min(1.0, (128.0 / K5) ** 0.5)).astype(np.float32)
    return h4, w5, np.float32([0.05]), (rng.standard_normal(B) * 0.3).astype(np.float32), (rng.random(B) < 0.3).astype(np.float32)


def _head_dev(h4, kind, dev):
    return _t(h4, dev).to(DT[kind])


def _wide_sum_f32(prod, wb):
    """(((0 + p0) + p1) + ...) + wide_b in fp32: the head's adds, and mrec_wide_sum's"""
    acc = np.zeros(prod.shape[0], np.float32)
    for f in range(prod.shape[1]):
        acc = acc + prod[:, f, 0]
    return acc + np.float32(wb)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _call(ops, dev, h4, w5, b5, wide, label, dscale, kind, dhs=1.0, prod=None, wb=None):
    """through ops.head_fwd_bwd_any; every output as a tensor: [loss, logit, dlogit, dh4, dw5, db4, db5, dwb]"""
    K5 = h4.shape[1]
    dw5 = torch.full((K5,), FILL, device=dev); db4 = torch.full((K5,), FILL, device=dev); db5 = torch.full((1,), FILL, device=dev)
    dwb = torch.full((1,), FILL, device=dev)
    if prod is None:
        r = ops.head_fwd_bwd_any(_head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), _t(wide, dev), _t(label, dev), dscale, dw5, db4, db5, dh_scale=dhs)
    else:
        r = ops.head_fwd_bwd_any(_head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), None, _t(label, dev), dscale, dw5, db4, db5, dh_scale=dhs,
                                 wide_prod=_t(prod, dev), wide_bias=_t(np.float32([wb]), dev), dwide_bias_out=dwb)
    return [t.clone() for t in r] + [dw5, db4, db5, dwb]


NAMES = ("loss", "logit", "dlogit", "dh4", "dw5", "db4", "db5")


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5", HEAD_K5)
def test_head_any_matches_oracle(dev, oracle, K5, kind):
    """every output against the float64 oracle, the zero pattern of dh4 exactly; two calls give the same bits.
    Tolerances: exactly those of test_head_matches_oracle_at_every_lane_group (see the module docstring for the logit's)."""
    from mindrec_amd import ops
    assert ops.head_any_supported(K5)
    for B in HEAD_B:
        for dhs in (1.0, 2.0):
            rng = np.random.default_rng([K5, B, int(dhs)])
            h4, w5, b5, wide, label = _head_inputs(rng, B, K5, kind, oracle)
            dscale = 1.0 / B if kind == "f32" else 1024.0 / B
            out = _call(ops, dev, h4, w5, b5, wide, label, dscale, kind, dhs)
            loss, logit, dlogit, dh4, dw5, db4, db5, _ = out
            r = oracle.head_fwd_bwd(h4, w5, b5[0], wide, label, dscale, dh_scale=dhs)
            what = (K5, kind, B, dhs)
            assert dh4.dtype == DT[kind] and tuple(dh4.shape) == (B, K5), what
            assert abs(float(loss) - r["loss"]) <= 1e-5 * abs(r["loss"]), what
            assert np.allclose(logit.cpu().numpy(), r["logit"], rtol=1e-5, atol=1e-5), what
            got = dh4.float().cpu().numpy()
            assert np.array_equal(got == 0, r["dh4"] == 0), what
            if kind == "f32":
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
            if dhs == 2.0:
                again = _call(ops, dev, h4, w5, b5, wide, label, dscale, kind, dhs)
                for n, x, y in zip(NAMES, out, again):
                    assert torch.equal(_bits(x), _bits(y)), (what, n, "two runs differ")


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5", [24, 520, 2048])
def test_head_any_products_equal_the_field_order_sum(dev, oracle, K5, kind):
    """the products form == the per-sample form fed the host's field-order fp32 sum + bias, bit for bit in every output"""
    from mindrec_amd import ops
    for F in (1, 3, 63, 64, 65, 100):
        for B in (1, 65, 257):
            rng = np.random.default_rng([K5, F, B])
            h4, w5, b5, _, label = _head_inputs(rng, B, K5, kind, oracle)
            prod = np.zeros((B, F, 2), np.float32)
            prod[:, :, 0] = (rng.standard_normal((B, F)) * 10.0 ** rng.uniform(-4, 0, (B, F))).astype(np.float32)
            prod[:, :, 1] = np.float32("nan")          # the pad word is not part of the sum
            wb = np.float32(-0.2)
            a = _call(ops, dev, h4, w5, b5, None, label, 1024.0 / B, kind, 2.0, prod=prod, wb=wb)
            b = _call(ops, dev, h4, w5, b5, _wide_sum_f32(prod, wb), label, 1024.0 / B, kind, 2.0)
            for n, x, y in zip(NAMES, a, b):
                assert torch.equal(_bits(x), _bits(y)), (K5, kind, F, B, n)
            assert torch.equal(a[7], a[6]) and float(b[7]) == FILL, (K5, kind, F, B, "dwide_bias")


@pytest.mark.parametrize("kind", ["bf16", "f32"])
@pytest.mark.parametrize("K5", [24, 520, 2048])
def test_head_any_rows_do_not_depend_on_the_partition(dev, oracle, K5, kind):
    """a row's logit, dlogit and dh4 are the same bits whatever the batch around it: the first rows of a batch of 1000 (32 workgroups
    at K5 >= 512) against the same rows as batches of 63, 5 and 1 (one workgroup, other row groups), dscale held"""
    from mindrec_amd import ops
    rng = np.random.default_rng([K5, 77])
    h4, w5, b5, wide, label = _head_inputs(rng, 1000, K5, kind, oracle)
    full = _call(ops, dev, h4, w5, b5, wide, label, 0.25, kind, 2.0)
    for n0, n1 in ((0, 63), (0, 5), (4, 5), (937, 1000), (999, 1000)):
        part = _call(ops, dev, h4[n0:n1], w5, b5, wide[n0:n1], label[n0:n1], 0.25, kind, 2.0)
        for i in (1, 2, 3):
            assert torch.equal(_bits(full[i][n0:n1]), _bits(part[i])), (K5, kind, n0, n1, NAMES[i])


def _geometry(B, K5):
    """the launch's workgroups, restated from mrec_head_fwd_bwd_any: G lanes a row, 256 / G rows a pass, at most 256 workgroups of
    at least 4 passes (fewer rows: fewer workgroups)"""
    return _launch(B, K5)[0]


def _launch(B, K5):
    """(workgroups, rows a workgroup, rows a pass) of that launch"""
    Cn = K5 // 8
    G = 1
    while G < Cn and G < 64:
        G *= 2
    RP = 256 // G
    nblk = 256
    while nblk > 1 and B // nblk < 4 * RP:
        nblk //= 2
    per = -(-(-(-B // nblk)) // RP) * RP
    return -(-B // per), per, RP


def _finish_sum(rows):
    """k_head_finish's order in fp32: the partial rows in workgroup order -- eight runs of ceil(nb / 8) consecutive rows, each added
    up in order from 0, then the eight run sums in order.  Up to 8 rows that is the plain sequential sum."""
    nb = rows.shape[0]
    chunk = (nb + 7) // 8
    tot = np.zeros(rows.shape[1], np.float32)
    for g in range(8):
        s = np.zeros(rows.shape[1], np.float32)
        for r in rows[g * chunk:(g + 1) * chunk]:
            s = s + r
        tot = tot + s
    return tot


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5,B,nb", [(24, 65, 1), (520, 65, 4), (2048, 128, 8), (2048, 130, 7), (520, 1000, 32), (2040, 257, 13), (1032, 1000, 32)])
def test_head_any_workspace_window_and_guard_rows(dev, oracle, K5, B, nb, kind):
    """over the C ABI, with buffers longer than B rows: the rows past B hold NaN in h4 and a sentinel in dh4, logit, dlogit -- the
    outputs are finite and the sentinel untouched; the partial rows written are a prefix of the sentinel-filled workspace, nb of them;
    dw5, db4, db5 and the loss are the partial rows added in workgroup order (up to 8 rows: the host's sequential fp32 sum)."""
    from mindrec_amd import _lib
    assert _geometry(B, K5) == nb
    R = B + 70
    rng = np.random.default_rng([K5, B, 5])
    h4, w5, b5, wide, label = _head_inputs(rng, B, K5, kind, oracle)
    h4_buf = torch.full((R, K5), float("nan"), dtype=DT[kind], device=dev)
    h4_buf[:B] = _head_dev(h4, kind, dev)
    dh4 = torch.full((R, K5), FILL, dtype=DT[kind], device=dev)
    logit, dlogit = torch.full((R,), FILL, device=dev), torch.full((R,), FILL, device=dev)
    wide_buf, label_buf = torch.full((R,), float("nan"), device=dev), torch.full((R,), float("nan"), device=dev)
    wide_buf[:B], label_buf[:B] = _t(wide, dev), _t(label, dev)
    W = 2 * K5 + 2
    ws_bytes = _lib.query_bytes("mrec_head_workspace_bytes", B, K5)
    assert ws_bytes >= 256 * W * 4
    ws = torch.full((ws_bytes // 4 + W,), FILL, device=dev)
    o = {n: torch.full((k,), FILL, device=dev) for n, k in (("dw5", K5), ("db4", K5), ("db5", 1), ("dwb", 1), ("loss", 1))}
    w5d, b5d = _t(w5, dev), _t(b5, dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    rc = _lib.lib().mrec_head_fwd_bwd_any(KIND[kind], p(h4_buf), p(w5d), p(b5d), p(wide_buf), None, 0, None, p(label_buf), B, K5, 1024.0 / B, 2.0,
                                          p(logit), p(dlogit), p(dh4), p(o["dw5"]), p(o["db4"]), p(o["db5"]), p(o["dwb"]), p(o["loss"]),
                                          p(ws, 4 * W), ws_bytes, None)
    assert rc == 0
    torch.cuda.synchronize()
    for n, t in (("dh4", dh4), ("logit", logit), ("dlogit", dlogit)):
        assert bool((t[B:] == FILL).all()), (n, "written past row B")
        assert bool(torch.isfinite(t[:B].float()).all()), n
    a = ws.cpu().numpy()
    assert (a[:W] == FILL).all() and (a[W * (1 + nb):] == FILL).all(), "workspace written outside its first nb partial rows"
    rows = a[W:W * (1 + nb)].reshape(nb, W)
    assert np.isfinite(rows).all() and (rows != FILL).all()
    acc = _finish_sum(rows)
    if nb <= 8:
        seq = rows[0].copy()
        for r in rows[1:]:
            seq = seq + r
        assert np.array_equal(acc, seq)
    got = {n: t.cpu().numpy() for n, t in o.items()}
    assert np.array_equal(got["dw5"], acc[:K5]) and np.array_equal(got["db4"], acc[K5:2 * K5])
    assert got["db5"][0] == acc[2 * K5] and got["dwb"][0] == acc[2 * K5]
    assert got["loss"][0] == np.float32(acc[2 * K5 + 1] * np.float32(1.0 / B))
    # and the per-row outputs are what the Python layer returns for the same rows
    from mindrec_amd import ops
    r = _call(ops, dev, h4, w5, b5, wide, label, 1024.0 / B, kind, 2.0)
    assert torch.equal(_bits(r[3]), _bits(dh4[:B])) and torch.equal(r[1], logit[:B]) and torch.equal(r[2], dlogit[:B])
    assert torch.equal(r[4], o["dw5"]) and torch.equal(r[5], o["db4"]) and torch.equal(r[6], o["db5"]) and torch.equal(r[0], o["loss"])


# (K5, batch of at least two workgroups whose last one ends in a partly filled pass); B = 3 is one partly filled pass at each
FIXED_K5_B = [(8, 2100), (64, 301), (512, 301)]


def _call_fixed(ops, dev, h4, w5, b5, wide, label, dscale, kind, dhs, prod=None, wb=None):
    """_call through ops.head_fwd_bwd / ops.head_fwd_bwd_wide, the head of the power-of-two widths up to 512"""
    K5 = h4.shape[1]
    dw5 = torch.full((K5,), FILL, device=dev); db4 = torch.full((K5,), FILL, device=dev); db5 = torch.full((1,), FILL, device=dev)
    dwb = torch.full((1,), FILL, device=dev)
    if prod is None:
        r = ops.head_fwd_bwd(_head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), _t(wide, dev), _t(label, dev), dscale, dw5, db4, db5, dh_scale=dhs)
    else:
        r = ops.head_fwd_bwd_wide(_head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), _t(prod, dev), _t(np.float32([wb]), dev), _t(label, dev),
                                  dscale, dw5, db4, db5, dwide_bias_out=dwb, dh_scale=dhs)
    return [t.clone() for t in r] + [dw5, db4, db5, dwb]


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5,Bbig", FIXED_K5_B)
def test_fixed_width_heads_equal_head_any_bit_for_bit(dev, oracle, K5, Bbig, kind):
    """ops.head_fwd_bwd and ops.head_fwd_bwd_wide == ops.head_fwd_bwd_any in every bit of every output (loss, logit, dlogit, dh4, dw5,
    db4, db5, dwide_bias) at widths both serve: the two training heads share one launch geometry, one row arithmetic and one order
    of partial sums.  Batches: several workgroups with a ragged last one, and a single partly filled pass."""
    from mindrec_amd import ops
    assert ops.head_supported(K5) and ops.head_any_supported(K5)
    nb, per, RP = _launch(Bbig, K5)
    assert nb >= 2 and (Bbig - (nb - 1) * per) % RP != 0, "the last workgroup must end in a partly filled pass"
    assert _launch(3, K5)[0] == 1 and 3 % RP != 0
    for B in (Bbig, 3):
        for dhs in (1.0, 2.0):
            rng = np.random.default_rng([K5, B, int(dhs), 11])
            h4, w5, b5, wide, label = _head_inputs(rng, B, K5, kind, oracle)
            dscale = 1.0 / B if kind == "f32" else 1024.0 / B
            a = _call_fixed(ops, dev, h4, w5, b5, wide, label, dscale, kind, dhs)
            b = _call(ops, dev, h4, w5, b5, wide, label, dscale, kind, dhs)
            for n, x, y in zip(NAMES, a, b):
                assert torch.equal(_bits(x), _bits(y)), (K5, kind, B, dhs, n)
            if kind == "f32":
                continue                      # head_fwd_bwd_wide: the two 16-bit kinds
            for F in (1, 39, 70):
                prod = np.zeros((B, F, 2), np.float32)
                prod[:, :, 0] = (rng.standard_normal((B, F)) * 10.0 ** rng.uniform(-4, 0, (B, F))).astype(np.float32)
                prod[:, :, 1] = np.float32("nan")          # the pad word is not part of the sum
                wb = np.float32(-0.2)
                a = _call_fixed(ops, dev, h4, w5, b5, None, label, dscale, kind, dhs, prod=prod, wb=wb)
                b = _call(ops, dev, h4, w5, b5, None, label, dscale, kind, dhs, prod=prod, wb=wb)
                for n, x, y in zip(NAMES + ("dwide_bias",), a, b):
                    assert torch.equal(_bits(x), _bits(y)), (K5, kind, B, dhs, F, n)
                assert torch.equal(a[7], a[6]), (K5, kind, B, dhs, F, "dwide_bias is db5")


def test_head_any_refuses_through_the_python_layer(dev):
    from mindrec_amd import _lib, ops
    z = lambda *s: torch.zeros(s, device=dev)
    for K5, code in ((12, -3), (2056, -3)):
        assert not ops.head_any_supported(K5)
        with pytest.raises(_lib.MrecError) as e:
            ops.head_fwd_bwd_any(torch.zeros((4, K5), dtype=torch.bfloat16, device=dev), z(K5), z(1), z(4), z(4), 1.0, z(K5), z(K5), z(1))
        assert e.value.code == code
    with pytest.raises(_lib.MrecError) as e:          # neither form of the wide branch
        ops.head_fwd_bwd_any(torch.zeros((4, 24), dtype=torch.bfloat16, device=dev), z(24), z(1), None, z(4), 1.0, z(24), z(24), z(1))
    assert e.value.code == -1
