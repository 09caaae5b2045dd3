"""ops.dcn_predict (csrc/mrec_cross.hip: k_dcn_predict, both lane layouts) on the device against the references of
_dcn_predict_cases.py.  c of the references is the device's own ops.cross_layers(x0, cw, cb) -- the kernel runs the same device code
on a row and never writes it.  Per case: the logit equals the fp32 restatement bit for bit and lies within the derived bound of
float64; prob within 0.25 bound + 2^-23 of the float64 sigmoid of the float64 logit; the loss within (B + 8) u T / B of float64 BCE of
the device's own logit; the unlabelled call gives the same logit and prob bits with no workspace; two calls give the same loss
bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dcn_predict_cases as T

pytestmark = pytest.mark.gpu

CASES = T.all_cases()


def _dev(x, dev):
    return {k: torch.from_numpy(v).to(dev) for k, v in x.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check(case, x, c, logit, prob, loss):
    """the assertions on one labelled result (numpy arrays; c: the device's cross_layers output)"""
    d2, w3, b3, label = x["d2"], x["w3"], x["b3"], x["label"]
    z32, z64, bound = T.logit32(d2, c, w3, b3), T.logit64(d2, c, w3, b3), T.logit_bound(d2, c, w3, b3)
    err = np.abs(logit.astype(np.float64) - z64)
    p64 = T.sigmoid64(z64)
    perr = np.abs(prob.astype(np.float64) - p64)
    l64, lbound = T.loss64(logit, label)
    print(f"  {T.name(case)}: logit bits differ in {int((_bits(logit) != _bits(z32)).sum())} rows, max err/bound {float((err / bound).max()):.3f}, "
          f"prob max err {float(perr.max()):.3e}, loss {float(loss[0])!r} float64 {l64!r} bound {lbound:.3e}")
    assert np.array_equal(_bits(logit), _bits(z32)), "the logit is not the restatement's, bit for bit"
    assert (err <= bound).all()
    assert np.isfinite(prob).all() and (perr <= 0.25 * bound + 2.0 ** -23).all()
    assert np.isfinite(loss).all() and abs(float(loss[0]) - l64) <= lbound


@pytest.mark.parametrize("case", CASES, ids=[T.name(c) for c in CASES])
def test_case_against_the_restatement_and_float64(dev, case):
    from mindrec_amd import ops
    x = T.inputs(case)
    t = _dev(x, dev)
    c = ops.cross_layers(t["x0"], t["cw"], t["cb"]).cpu().numpy()
    logit, prob, loss = ops.dcn_predict(t["x0"], t["cw"], t["cb"], t["d2"], t["w3"], t["b3"], t["label"])
    logit, prob, loss = logit.cpu().numpy(), prob.cpu().numpy(), loss.cpu().numpy()
    _check(case, x, c, logit, prob, loss)
    if case.kind == "values":
        for tgt in T.VALUE_LOGITS:
            assert (np.abs(logit - tgt) <= 0.02).sum() >= len(T.VALUE_LABELS), tgt
    # the unlabelled call: the same bits, no workspace (the entry is handed ws = NULL)
    lu, pu = ops.dcn_predict(t["x0"], t["cw"], t["cb"], t["d2"], t["w3"], t["b3"])
    assert np.array_equal(_bits(lu.cpu().numpy()), _bits(logit)) and np.array_equal(_bits(pu.cpu().numpy()), _bits(prob))
    # the same loss bits on a second run
    loss2 = ops.dcn_predict(t["x0"], t["cw"], t["cb"], t["d2"], t["w3"], t["b3"], t["label"])[2].cpu().numpy()
    assert np.array_equal(_bits(loss2), _bits(loss))


def test_unlabelled_call_needs_no_workspace(dev):
    """straight over the ABI: ws = NULL, 0 bytes"""
    from mindrec_amd import _lib, ops
    case = T.ROW_CASES[3]
    x = T.inputs(case)
    t = _dev(x, dev)
    logit, prob = torch.full((case.B,), 7.0, device=dev), torch.full((case.B,), 7.0, device=dev)
    p = lambda a: C.c_void_p(a.data_ptr())      # noqa: E731
    rc = _lib.lib().mrec_dcn_predict(p(t["x0"]), p(t["cw"]), p(t["cb"]), case.L, p(t["d2"]), case.H, p(t["w3"]), p(t["b3"]), None, case.B, case.H,
                                     case.X, p(logit), p(prob), None, None, 0, ops._stream())
    assert rc == 0
    ref = ops.dcn_predict(t["x0"], t["cw"], t["cb"], t["d2"], t["w3"], t["b3"])
    assert torch.equal(logit, ref[0]) and torch.equal(prob, ref[1])


def test_strided_d2_and_output_views_keep_their_neighbours(dev):
    """d2 a column view of a wider buffer (ldd > H); out= views with sentinel floats on both sides that must be unchanged"""
    from mindrec_amd import ops
    case = T.STRIDE_CASE
    x = T.inputs(case)
    t = _dev(x, dev)
    B, H = case.B, case.H
    wide = torch.full((B, H + 24), 9.5, device=dev)
    wide[:, 8:8 + H] = t["d2"]
    d2v = wide[:, 8:8 + H]
    assert d2v.stride(0) == H + 24 and d2v.data_ptr() % 16 == 0
    S = 1234.5
    bufs = {n: torch.full((k + 16,), S, device=dev) for n, k in (("logit", B), ("prob", B), ("loss", 1))}
    out = {n: b[8:-8] for n, b in bufs.items()}
    logit, prob, loss = ops.dcn_predict(t["x0"], t["cw"], t["cb"], d2v, t["w3"], t["b3"], t["label"], out=out)
    assert logit.data_ptr() == out["logit"].data_ptr() and prob.data_ptr() == out["prob"].data_ptr() and loss.data_ptr() == out["loss"].data_ptr()
    for n, b in bufs.items():
        assert bool((b[:8] == S).all()) and bool((b[-8:] == S).all()), n
    c = ops.cross_layers(t["x0"], t["cw"], t["cb"]).cpu().numpy()
    _check(case, x, c, logit.cpu().numpy(), prob.cpu().numpy(), loss.cpu().numpy())
    ref = ops.dcn_predict(t["x0"], t["cw"], t["cb"], t["d2"], t["w3"], t["b3"], t["label"])
    assert all(torch.equal(a, b) for a, b in zip((logit, prob, loss), ref))            # the stride changes no bit
    assert bool((wide[:, :8] == 9.5).all()) and bool((wide[:, 8 + H:] == 9.5).all())


@pytest.mark.parametrize("how", T.REFUSED, ids=[str(sorted(h.items())) for h in T.REFUSED])
def test_refused_shapes_raise_before_any_launch(dev, how):
    from mindrec_amd import _lib, ops
    H, X, B, L = how.get("H", 64), how.get("X", 30), 8, 2
    f = lambda *s: torch.ones(s, device=dev)      # noqa: E731
    d2 = f(B, H)
    if "offset" in how:
        d2 = f(B * H + 4)[how["offset"]:how["offset"] + B * H].view(B, H)
        assert d2.data_ptr() % 16 == 4
    assert ops.dcn_predict_supported(H, X, L) == ("offset" in how)
    out = {"logit": f(B) * 7, "prob": f(B) * 7, "loss": f(1) * 7}
    for label in (f(B), None):
        with pytest.raises(_lib.MrecError, match="EUNSUPPORTED"):
            ops.dcn_predict(f(B, X), f(L, X), f(L, X), d2, f(H + X), f(1), label, out=out)
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in out.values())


def test_an_empty_batch_touches_nothing(dev):
    from mindrec_amd import ops
    f = lambda *s: torch.ones(s, device=dev)      # noqa: E731
    out = {"loss": f(1) * 7}
    logit, prob, loss = ops.dcn_predict(f(0, 30), f(2, 30), f(2, 30), f(0, 64), f(94), f(1), f(0), out=out)
    assert logit.numel() == 0 and prob.numel() == 0 and float(loss) == 7.0
