"""mrec_head_predict (the evaluation forward of the output head: logit, sigmoid and, with a label, the mean loss, for any last hidden
width K5 % 8 == 0 up to 2048) over the C ABI, without a device: the symbols, their binding, and the order in which the entry refuses
-- EINVAL, then the width, then the alignment, then (with a label only) the workspace -- all of it decided before any launch.  Every
call here is refused: the labelled ones at the latest by a workspace too small for their shape, the unlabelled ones (which need no
workspace, so nothing stands between them and a launch) by an earlier check.  That an unlabelled call is ACCEPTED with ws = NULL is
therefore shown where it may launch: tests/test_head_predict_gpu.py::test_unlabelled_call_needs_no_workspace.
(The file fails where the entry point does not exist.)"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3


def _buf():
    """a host buffer and a 16-byte aligned address inside it: a stand-in for a device pointer that is never dereferenced"""
    raw = (C.c_char * 128)()
    return raw, (C.addressof(raw) + 15) & ~15


def _call(kind=0, K5=24, B=4, F=0, wide=True, prod=False, bias=False, ws_bytes=0, h4_off=0, null=()):
    """a labelled call (label, loss and ws set) unless `null` takes them away"""
    from mindrec_amd import _lib
    raw, a = _buf()
    p = {n: C.c_void_p(a) for n in ("h4", "w5", "b5", "wide", "prod", "bias", "label", "logit", "prob", "loss", "ws")}
    p["h4"] = C.c_void_p(a + h4_off)
    if not wide:
        p["wide"] = None
    if not prod:
        p["prod"] = None
    if not bias:
        p["bias"] = None
    for n in null:
        p[n] = None
    return _lib.lib().mrec_head_predict(kind, p["h4"], p["w5"], p["b5"], p["wide"], p["prod"], F, p["bias"], p["label"], B, K5, p["logit"],
                                        p["prob"], p["loss"], p["ws"], ws_bytes, None)


def test_symbols_declared_bound_and_exported():
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    decl = re.search(r"\bint mrec_head_predict\(([^;]*)\);", text)
    assert decl, "mrec_head_predict is not declared in include/mrec.h"
    assert re.search(r"\bint mrec_head_predict_workspace_bytes\(int64_t B, size_t\* out\);", text)
    assert "mrec_head_predict" in _lib.EXPORTED and "mrec_head_predict_workspace_bytes" in _lib.EXPORTED
    f = _lib.lib().mrec_head_predict
    assert len(f.argtypes) == decl.group(1).count(",") + 1 == 17
    assert len(_lib.lib().mrec_head_predict_workspace_bytes.argtypes) == 2
    assert _lib.lib().mrec_version() >= 103


def test_width_check():
    for K5 in (12, 2056, 4, 2052):
        assert _call(K5=K5) == EUNSUPPORTED, K5
        assert _call(K5=K5, null=("label", "loss", "ws")) == EUNSUPPORTED, K5          # the unlabelled form refuses the same widths
    for K5 in (8, 24, 520, 1024, 2048):            # past the width check: the next refusal is the workspace's
        for kind in (0, 1, 2):
            assert _call(K5=K5, kind=kind) == EWORKSPACE, (K5, kind)


def test_einval_comes_first():
    assert _call(wide=True, prod=True, F=3, bias=True) == EINVAL          # both forms of the wide branch
    assert _call(wide=False, prod=False) == EINVAL                         # neither
    assert _call(wide=False, prod=True, F=0, bias=True) == EINVAL          # products without a field count
    assert _call(wide=False, prod=True, F=3, bias=False) == EINVAL         # products without the bias
    assert _call(wide=False, prod=True, F=3, bias=True) == EWORKSPACE      # the products form itself is accepted
    assert _call(kind=3) == EINVAL and _call(kind=-1) == EINVAL
    assert _call(B=0) == EINVAL and _call(B=-1) == EINVAL and _call(K5=0) == EINVAL and _call(K5=-8) == EINVAL
    for n in ("h4", "w5", "b5", "logit", "prob"):
        assert _call(null=(n,)) == EINVAL, n
        assert _call(null=(n, "label", "loss", "ws")) == EINVAL, n          # ... in the unlabelled form too
    # label and loss: both or neither
    assert _call(null=("label",)) == EINVAL and _call(null=("loss",)) == EINVAL
    # ... before the width: a bad argument AND a bad width is EINVAL; a bad width AND a misaligned row is EUNSUPPORTED
    assert _call(K5=12, null=("w5",)) == EINVAL and _call(K5=12, null=("label",)) == EINVAL
    assert _call(K5=12, h4_off=8) == EUNSUPPORTED
    assert _call(K5=24, h4_off=8) == EINVAL and _call(K5=24, h4_off=4) == EINVAL
    # the alignment comes before the workspace, and without a label it is the last check: refused with ws = NULL and with one
    assert _call(K5=24, h4_off=8, null=("label", "loss", "ws")) == EINVAL
    assert _call(K5=24, h4_off=8, null=("label", "loss")) == EINVAL


def test_workspace_check():
    from mindrec_amd import _lib
    for K5 in (24, 520, 2048):
        # B = 1: one workgroup, one partial (4 bytes); with a label a missing workspace is a workspace too small
        assert _call(K5=K5, B=1, ws_bytes=3) == EWORKSPACE
        assert _call(K5=K5, B=1, ws_bytes=1 << 20, null=("ws",)) == EWORKSPACE
        # a batch that fills the launch: 256 workgroups
        assert _call(K5=K5, B=1 << 20, ws_bytes=256 * 4 - 1) == EWORKSPACE
    for B in (0, 1, 1000, 1 << 20):
        assert _lib.query_bytes("mrec_head_predict_workspace_bytes", B) >= 256 * 4      # the launch never has more than 256 workgroups
    out = C.c_size_t(0)
    assert _lib.lib().mrec_head_predict_workspace_bytes(-1, C.byref(out)) == EINVAL
    assert _lib.lib().mrec_head_predict_workspace_bytes(4, None) == EINVAL


def test_width_predicate():
    from mindrec_amd import ops
    assert [K5 for K5 in range(0, 2100) if ops.head_predict_supported(K5)] == list(range(8, 2049, 8))
    assert all(ops.head_predict_supported(K5) == ops.head_any_supported(K5) for K5 in range(0, 2100))
