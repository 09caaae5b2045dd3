"""The evaluation forward of the output head (csrc/mrec_mlp.hip: k_head_predict + k_head_predict_finish, mrec_head_predict) against
the float64 restatement oracle.head_fwd_bwd and, bit for bit, against the training head it is the forward half of
(ops.head_fwd_bwd_any), on the input recipe of test_head_any_gpu.py (_head_inputs, restated below).

Widths: every lane-group size with lanes that own nothing (8, 24, 72, 136: groups of 1, 4, 16, 32 lanes), 63 / 64 / 65 chunks of 8
values a row (504, 512, 520), every number of chunks a lane (1: <= 512, 2: <= 1024, 3: <= 1536, 4: <= 2048) and the last chunk of a
lane absent (520, 1000, 1032, 2040).

Tolerances: the project's, none new.  logit rtol = atol = 1e-5 (test_head_any_gpu.py's docstring: checked on the CPU at these widths
against the worst summation order); prob rtol 1e-4, atol 1e-7 (that file's dlogit bound for the 16-bit kinds, at dscale 1: the oracle
called with label 0 and dscale 1 returns the sigmoid as its dlogit); loss 1e-5 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
KIND = {"bf16": 0, "f16": 1, "f32": 2}
HEAD_K5 = [8, 24, 72, 136, 504, 512, 520, 1000, 1032, 1536, 2040, 2048]
HEAD_B = [1, 2, 63, 65, 257, 1000]
FILL = 7.0


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _head_inputs(rng, B, K5, kind, oracle):
    h4 = np.maximum(rng.standard_normal((B, K5)), 0).astype(np.float32)
    if kind != "f32":
        h4 = oracle.round16(h4, kind)
    # |w5| bounded away from 0 and scaled so that the logit stays of order 1 at every K5
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
    return t.contiguous().view(torch.int32)


def _predict(ops, dev, h4, w5, b5, wide, label, kind, prod=None, wb=None):
    """through ops.head_predict: (logit, prob[, loss]) as clones"""
    if prod is None:
        r = ops.head_predict(_head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), wide=_t(wide, dev), label=None if label is None else _t(label, dev))
    else:
        r = ops.head_predict(_head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), wide_prod=_t(prod, dev), wide_bias=_t(np.float32([wb]), dev),
                             label=None if label is None else _t(label, dev))
    return [t.clone() for t in r]


def _train_head(ops, dev, h4, w5, b5, wide, label, dscale, kind, prod=None, wb=None):
    """through ops.head_fwd_bwd_any: (logit, dlogit)"""
    K5 = h4.shape[1]
    z = lambda n: torch.full((n,), FILL, device=dev)      # noqa: E731
    if prod is None:
        r = ops.head_fwd_bwd_any(_head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), _t(wide, dev), _t(label, dev), dscale, z(K5), z(K5), z(1))
    else:
        r = ops.head_fwd_bwd_any(_head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), None, _t(label, dev), dscale, z(K5), z(K5), z(1),
                                 wide_prod=_t(prod, dev), wide_bias=_t(np.float32([wb]), dev))
    return r[1].clone(), r[2].clone()


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5", HEAD_K5)
def test_head_predict_matches_oracle_and_the_training_head(dev, oracle, K5, kind):
    """logit, prob and loss against the float64 oracle; logit bit for bit the training head's logit, prob bit for bit its dlogit at
    label 0 and dscale 1 ((sg - 0) * 1 is exact)."""
    from mindrec_amd import ops
    assert ops.head_predict_supported(K5)
    for B in HEAD_B:
        rng = np.random.default_rng([K5, B, 3])
        h4, w5, b5, wide, label = _head_inputs(rng, B, K5, kind, oracle)
        logit, prob, loss = _predict(ops, dev, h4, w5, b5, wide, label, kind)
        what = (K5, kind, B)
        assert tuple(logit.shape) == (B,) and tuple(prob.shape) == (B,) and tuple(loss.shape) == (1,), what
        r = oracle.head_fwd_bwd(h4, w5, b5[0], wide, label, 1.0 / B)
        sg = oracle.head_fwd_bwd(h4, w5, b5[0], wide, np.zeros(B, np.float32), 1.0)["dlogit"]
        assert np.allclose(logit.cpu().numpy(), r["logit"], rtol=1e-5, atol=1e-5), what
        assert np.allclose(prob.cpu().numpy(), sg, rtol=1e-4, atol=1e-7), what
        assert abs(float(loss) - r["loss"]) <= 1e-5 * abs(r["loss"]), what
        t_logit, _ = _train_head(ops, dev, h4, w5, b5, wide, label, 1024.0 / B, kind)
        assert torch.equal(_bits(t_logit), _bits(logit)), (what, "logit differs from the training head's")
        t_logit0, t_dl = _train_head(ops, dev, h4, w5, b5, wide, np.zeros(B, np.float32), 1.0, kind)
        assert torch.equal(_bits(t_logit0), _bits(logit)) and torch.equal(_bits(t_dl), _bits(prob)), (what, "prob differs from the training head's sigmoid")


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5", [24, 512, 1032])
def test_head_predict_products_form(dev, oracle, K5, kind):
    """the per-field products form (F below, at and above the lane group): bit for bit the training head's on the same products, and
    the per-sample form's fed the host's field-order fp32 sum + bias"""
    from mindrec_amd import ops
    for F in (1, 26, 39, 64, 65):
        for B in (1, 65, 257):
            rng = np.random.default_rng([K5, F, B])
            h4, w5, b5, _, label = _head_inputs(rng, B, K5, kind, oracle)
            prod = np.zeros((B, F, 2), np.float32)
            prod[:, :, 0] = (rng.standard_normal((B, F)) * 10.0 ** rng.uniform(-4, 0, (B, F))).astype(np.float32)
            prod[:, :, 1] = np.float32("nan")          # the pad word is not part of the sum
            wb = np.float32(-0.2)
            what = (K5, kind, F, B)
            a = _predict(ops, dev, h4, w5, b5, None, label, kind, prod=prod, wb=wb)
            b = _predict(ops, dev, h4, w5, b5, _wide_sum_f32(prod, wb), label, kind)
            for n, x, y in zip(("logit", "prob", "loss"), a, b):
                assert torch.equal(_bits(x), _bits(y)), (what, n, "products form != field-order sum")
            t_logit, t_dl = _train_head(ops, dev, h4, w5, b5, None, np.zeros(B, np.float32), 1.0, kind, prod=prod, wb=wb)
            assert torch.equal(_bits(t_logit), _bits(a[0])) and torch.equal(_bits(t_dl), _bits(a[1])), (what, "differs from the training head")


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5", [72, 1032])
def test_head_predict_rows_do_not_depend_on_the_batch(dev, oracle, K5, kind):
    """rows 0, 63, 64, 999 of a batch of 1000 are the same bits as the same rows run as four batches of 1, in both wide forms"""
    from mindrec_amd import ops
    rng = np.random.default_rng([K5, 78])
    B, F = 1000, 39
    h4, w5, b5, wide, label = _head_inputs(rng, B, K5, kind, oracle)
    prod = np.zeros((B, F, 2), np.float32)
    prod[:, :, 0] = (rng.standard_normal((B, F)) * 0.05).astype(np.float32)
    full = _predict(ops, dev, h4, w5, b5, wide, label, kind)
    full_p = _predict(ops, dev, h4, w5, b5, None, None, kind, prod=prod, wb=0.1)
    for r in (0, 63, 64, 999):
        one = _predict(ops, dev, h4[r:r + 1], w5, b5, wide[r:r + 1], label[r:r + 1], kind)
        one_p = _predict(ops, dev, h4[r:r + 1], w5, b5, None, None, kind, prod=prod[r:r + 1], wb=0.1)
        for i, n in enumerate(("logit", "prob")):
            assert torch.equal(_bits(full[i][r:r + 1]), _bits(one[i])), (K5, kind, r, n)
            assert torch.equal(_bits(full_p[i][r:r + 1]), _bits(one_p[i])), (K5, kind, r, n, "products")


def _geometry(B, K5):
    """the launch's workgroups, restated from mrec_head_predict (mrec_head_fwd_bwd_any's): G lanes a row, 256 / G rows a pass, at most
    256 workgroups of at least 4 passes"""
    Cn = K5 // 8
    G = 1
    while G < Cn and G < 64:
        G *= 2
    RP = 256 // G
    nblk = 256
    while nblk > 1 and B // nblk < 4 * RP:
        nblk //= 2
    per = -(-(-(-B // nblk)) // RP) * RP
    return -(-B // per)


def _abi(dev, kind, h4_view, w5d, b5d, wide_d, label_d, B, K5, logit, prob, loss, ws, ws_bytes):
    from mindrec_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    rc = _lib.lib().mrec_head_predict(KIND[kind], p(h4_view), p(w5d), p(b5d), p(wide_d), None, 0, None, p(label_d), B, K5, p(logit), p(prob),
                                      p(loss), p(ws), ws_bytes, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5,B,nb", [(24, 65, 1), (520, 257, 13), (2040, 257, 13), (1032, 1000, 32), (72, 1000, 8)])
def test_head_predict_windows(dev, oracle, K5, B, nb, kind):
    """over the C ABI: h4 is a view into a taller NaN-filled buffer, logit / prob / loss are windows of sentinel-filled buffers and
    the workspace is sentinel-filled -- the outputs are finite, every neighbour keeps its sentinel, the workspace is written in its first
    nb words only (one partial a workgroup), and the windows hold what the Python layer returns."""
    from mindrec_amd import _lib, ops
    assert _geometry(B, K5) == nb
    top, R = 3, B + 70
    rng = np.random.default_rng([K5, B, 6])
    h4, w5, b5, wide, label = _head_inputs(rng, B, K5, kind, oracle)
    h4_buf = torch.full((R, K5), float("nan"), dtype=DT[kind], device=dev)
    h4_buf[top:top + B] = _head_dev(h4, kind, dev)
    wide_buf, label_buf = torch.full((R,), float("nan"), device=dev), torch.full((R,), float("nan"), device=dev)
    wide_buf[top:top + B], label_buf[top:top + B] = _t(wide, dev), _t(label, dev)
    logit, prob, loss = torch.full((R,), FILL, device=dev), torch.full((R,), FILL, device=dev), torch.full((3,), FILL, device=dev)
    ws_bytes = _lib.query_bytes("mrec_head_predict_workspace_bytes", B)
    ws = torch.full((ws_bytes // 4 + 8,), FILL, device=dev)
    rc = _abi(dev, kind, h4_buf[top:], _t(w5, dev), _t(b5, dev), wide_buf[top:], label_buf[top:], B, K5, logit[top:], prob[top:], loss[1:],
              ws[4:], ws_bytes)
    assert rc == 0
    for n, t in (("logit", logit), ("prob", prob)):
        assert bool((t[:top] == FILL).all()) and bool((t[top + B:] == FILL).all()), (n, "written outside its window")
        assert bool(torch.isfinite(t[top:top + B]).all()), n
    assert float(loss[0]) == FILL and float(loss[2]) == FILL and np.isfinite(float(loss[1])) and float(loss[1]) != FILL
    a = ws.cpu().numpy()
    assert (a[:4] == FILL).all() and (a[4 + nb:] == FILL).all(), "workspace written outside its first nb partials"
    assert np.isfinite(a[4:4 + nb]).all() and (a[4:4 + nb] != FILL).all()
    r = _predict(ops, dev, h4, w5, b5, wide, label, kind)
    assert torch.equal(r[0], logit[top:top + B]) and torch.equal(r[1], prob[top:top + B]) and torch.equal(r[2], loss[1:2])


@pytest.mark.parametrize("kind", ["bf16", "f32"])
@pytest.mark.parametrize("K5", [72, 1032, 2048])
def test_head_predict_two_runs_give_the_same_bits(dev, oracle, K5, kind):
    from mindrec_amd import ops
    rng = np.random.default_rng([K5, 79])
    h4, w5, b5, wide, label = _head_inputs(rng, 1000, K5, kind, oracle)
    a = _predict(ops, dev, h4, w5, b5, wide, label, kind)
    b = _predict(ops, dev, h4, w5, b5, wide, label, kind)
    for n, x, y in zip(("logit", "prob", "loss"), a, b):
        assert torch.equal(_bits(x), _bits(y)), (K5, kind, n, "two runs differ")


@pytest.mark.parametrize("kind", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("K5,B", [(24, 65), (1032, 1000)])
def test_unlabelled_call_needs_no_workspace(dev, oracle, K5, B, kind):
    """without a label: one launch that leaves a sentinel-filled workspace untouched, is accepted with ws = NULL and zero bytes, and
    returns the labelled call's logit and prob bits"""
    from mindrec_amd import _lib, ops
    rng = np.random.default_rng([K5, B, 7])
    h4, w5, b5, wide, label = _head_inputs(rng, B, K5, kind, oracle)
    h4d, w5d, b5d, wide_d = _head_dev(h4, kind, dev), _t(w5, dev), _t(b5, dev), _t(wide, dev)
    ref = _predict(ops, dev, h4, w5, b5, wide, label, kind)
    ws_bytes = _lib.query_bytes("mrec_head_predict_workspace_bytes", B)
    ws = torch.full((ws_bytes // 4,), FILL, device=dev)
    for w, nbytes in ((ws, ws_bytes), (None, 0)):
        logit, prob = torch.full((B,), FILL, device=dev), torch.full((B,), FILL, device=dev)
        assert _abi(dev, kind, h4d, w5d, b5d, wide_d, None, B, K5, logit, prob, None, w, nbytes) == 0
        assert torch.equal(_bits(logit), _bits(ref[0])) and torch.equal(_bits(prob), _bits(ref[1]))
    assert bool((ws == FILL).all()), "an unlabelled call wrote its workspace"
    r = _predict(ops, dev, h4, w5, b5, wide, None, kind)
    assert len(r) == 2 and torch.equal(_bits(r[0]), _bits(ref[0])) and torch.equal(_bits(r[1]), _bits(ref[1]))


def test_head_predict_out_and_refusals_through_the_python_layer(dev):
    from mindrec_amd import _lib, ops
    z = lambda *s: torch.zeros(s, device=dev)      # noqa: E731
    h = torch.zeros((4, 24), dtype=torch.bfloat16, device=dev)
    out = {}
    a = ops.head_predict(h, z(24), z(1), wide=z(4), label=z(4), out=out)
    assert set(out) == {"logit", "prob", "loss"} and all(a[i] is out[n] for i, n in enumerate(("logit", "prob", "loss")))
    ptrs = [t.data_ptr() for t in a]
    b = ops.head_predict(h, z(24), z(1), wide=z(4), label=z(4), out=out)
    assert [t.data_ptr() for t in b] == ptrs                     # persistent outputs: the addresses a captured graph replays into
    assert float(a[0][0]) == 0.0 and float(a[1][0]) == 0.5
    for K5, code in ((12, -3), (2056, -3)):
        assert not ops.head_predict_supported(K5)
        with pytest.raises(_lib.MrecError) as e:
            ops.head_predict(torch.zeros((4, K5), dtype=torch.bfloat16, device=dev), z(K5), z(1), wide=z(4))
        assert e.value.code == code
    with pytest.raises(_lib.MrecError) as e:          # neither form of the wide branch
        ops.head_predict(h, z(24), z(1))
    assert e.value.code == -1
