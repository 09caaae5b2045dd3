"""mrec_dcn_predict (the evaluation forward of Deep&Cross behind the hidden layers in one launch: cross stack, output layer over
[d2 | x_L], sigmoid and, with a label, the mean loss) over the C ABI, without a device: the symbols, their binding, and the order in
which the entry refuses -- EINVAL, B == 0 (MREC_OK, nothing touched), EINVAL for null pointers, then the shapes and alignments, then
(with a label only) the workspace -- all of it decided before any launch.  Every call here with B > 0 is refused: the labelled ones
at the latest by a workspace too small for their shape, the unlabelled ones (which need no workspace, so nothing stands between them
and a launch) by an earlier check.  That an unlabelled call is ACCEPTED with ws = NULL is shown where it may launch:
tests/test_dcn_predict_gpu.py.
(The file fails where the entry point does not exist.)"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3
PTRS = ("x0", "cw", "cb", "d2", "w3", "b3", "label", "logit", "prob", "loss", "ws")


def _buf():
    """a host buffer and a 16-byte aligned address inside it: a stand-in for a device pointer that is never dereferenced"""
    raw = (C.c_char * 128)()
    return raw, (C.addressof(raw) + 15) & ~15


def _call(H=64, X=30, L=6, B=4, ldd=None, ws_bytes=0, off=None, null=()):
    """a labelled call (label, loss and ws set) unless `null` takes them away.  off: {pointer name: bytes added to it}"""
    from mindrec_amd import _lib
    raw, a = _buf()
    p = {n: C.c_void_p(a + (off or {}).get(n, 0)) for n in PTRS}
    for n in null:
        p[n] = None
    return _lib.lib().mrec_dcn_predict(p["x0"], p["cw"], p["cb"], L, p["d2"], H if ldd is None else ldd, p["w3"], p["b3"], p["label"], B, H,
                                       X, p["logit"], p["prob"], p["loss"], p["ws"], ws_bytes, None)


UNLABELLED = ("label", "loss", "ws")


def test_symbols_declared_bound_and_exported():
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    decl = re.search(r"\bint mrec_dcn_predict\(([^;]*)\);", text)
    assert decl, "mrec_dcn_predict is not declared in include/mrec.h"
    assert re.search(r"\bint mrec_dcn_predict_workspace_bytes\(int64_t B, size_t\* out\);", text)
    assert "mrec_dcn_predict" in _lib.EXPORTED and "mrec_dcn_predict_workspace_bytes" in _lib.EXPORTED
    f = _lib.lib().mrec_dcn_predict
    assert len(f.argtypes) == decl.group(1).count(",") + 1 == 18
    assert len(_lib.lib().mrec_dcn_predict_workspace_bytes.argtypes) == 2
    assert _lib.lib().mrec_version() >= 105


def test_einval_comes_first():
    assert _call(B=-1) == EINVAL and _call(H=0) == EINVAL and _call(H=-4) == EINVAL and _call(X=0) == EINVAL and _call(L=-1) == EINVAL
    assert _call(H=64, ldd=60) == EINVAL
    for n in ("x0", "d2", "w3", "b3", "logit", "prob", "cw", "cb"):
        assert _call(null=(n,)) == EINVAL, n
        assert _call(null=(n,) + UNLABELLED) == EINVAL, n          # ... in the unlabelled form too
    # label and loss: both or neither
    assert _call(null=("label",)) == EINVAL and _call(null=("loss",)) == EINVAL
    # without layers the stack's weights may be null
    assert _call(L=0, null=("cw", "cb")) == EWORKSPACE
    # ... before the shapes: a bad argument AND a bad shape is EINVAL
    assert _call(H=6, null=("w3",)) == EINVAL and _call(X=2049, null=("label",)) == EINVAL and _call(H=6, B=-1) == EINVAL


def test_an_empty_batch_is_ok_and_touches_nothing():
    assert _call(B=0) == OK and _call(B=0, null=UNLABELLED) == OK
    assert _call(B=0, H=6) == OK and _call(B=0, null=PTRS) == OK      # (decided before the pointers and the shapes are looked at)
    assert _call(B=0, H=0) == EINVAL


def test_shape_and_alignment_checks():
    for kw in (dict(H=6), dict(H=1028), dict(H=2), dict(X=2049), dict(H=64, ldd=66), dict(off={"d2": 4}), dict(off={"d2": 8}),
               dict(off={"w3": 4})):
        assert _call(ws_bytes=1 << 20, **kw) == EUNSUPPORTED, kw
        assert _call(null=UNLABELLED, **kw) == EUNSUPPORTED, kw                        # the unlabelled form refuses the same
    # past them: the next refusal is the workspace's -- every width bucket and path, any depth, a row stride
    for X in (1, 2, 64, 65, 128, 129, 256, 257, 1170, 1280, 2048):
        for L in (0, 1, 8, 9, 40):
            assert _call(X=X, L=L) == EWORKSPACE, (X, L)
    for H in (4, 252, 1020, 1024):
        assert _call(H=H) == EWORKSPACE and _call(H=H, ldd=H + 4) == EWORKSPACE, H
    assert _call(off={"x0": 4, "label": 4, "logit": 4}) == EWORKSPACE                # only d2 and w3 are read 16 bytes at a time


def test_workspace_check():
    from mindrec_amd import _lib
    assert _call(B=1, ws_bytes=3) == EWORKSPACE
    assert _call(B=1, ws_bytes=1 << 20, null=("ws",)) == EWORKSPACE
    assert _call(B=1 << 20, ws_bytes=256 * 4 - 1) == EWORKSPACE
    for B in (0, 1, 1000, 1 << 20):
        assert _lib.query_bytes("mrec_dcn_predict_workspace_bytes", B) >= 256 * 4      # the launch never has more than 256 workgroups
    out = C.c_size_t(0)
    assert _lib.lib().mrec_dcn_predict_workspace_bytes(-1, C.byref(out)) == EINVAL
    assert _lib.lib().mrec_dcn_predict_workspace_bytes(4, None) == EINVAL


def test_shape_predicate_agrees_with_the_abi():
    from mindrec_amd import ops
    for H in (0, 2, 4, 6, 8, 64, 252, 1020, 1024, 1028, 2048):
        for X in (0, 1, 2, 30, 128, 129, 1170, 2048, 2049, 4096):
            for L in (0, 1, 6, 8, 9):
                if H <= 0 or X <= 0:
                    assert not ops.dcn_predict_supported(H, X, L) and _call(H=H, X=X, L=L) == EINVAL
                else:
                    assert ops.dcn_predict_supported(H, X, L) == (_call(H=H, X=X, L=L) == EWORKSPACE), (H, X, L)
