"""mrec_tail_predict (the evaluation forward of the fused tail: 512 -> 256 -> 128 -> 1 in one launch, any 1 <= B <= 32768) over the C
ABI, without a device: the symbols, their binding, and the order in which the entry refuses -- EINVAL, then the shape, the field
count, the row stride and the alignment, then (with a label only) the workspace -- all of it decided before any launch.  Every call
here is refused: the labelled ones at the latest by a workspace too small for their batch, the unlabelled ones (which need no
workspace, so nothing stands between them and a launch) by an earlier check.  That an unlabelled call is ACCEPTED with ws = NULL is
therefore shown where it may launch: tests/test_tail_predict_gpu.py (the unlabelled call of every case goes through ops.tail_predict,
which passes no workspace).
(The file fails where the entry point does not exist.)"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
K2, N2, N3 = 512, 256, 128
PTRS = ("x", "packed", "b2", "b3", "w5", "b5", "wide", "prod", "bias", "label", "logit", "prob", "loss", "ws")


def _buf():
    """a host buffer and a 16-byte aligned address inside it: a stand-in for a device pointer that is never dereferenced"""
    raw = (C.c_char * 128)()
    return raw, (C.addressof(raw) + 15) & ~15


def _call(f16=0, B=4, ldx=K2, dims=(K2, N2, N3), F=0, wide=True, prod=False, bias=False, ws_bytes=0, off=None, null=()):
    """a labelled call (label, loss and ws set, ws_bytes = 0: refused by the workspace check at the latest) unless `null` takes them
    away; off: {pointer name: byte offset from the aligned address}"""
    from mindrec_amd import _lib
    raw, a = _buf()
    p = {n: C.c_void_p(a + (off or {}).get(n, 0)) for n in PTRS}
    if not wide:
        p["wide"] = None
    if not prod:
        p["prod"] = None
    if not bias:
        p["bias"] = None
    for n in null:
        p[n] = None
    return _lib.lib().mrec_tail_predict(f16, p["x"], ldx, p["packed"], p["b2"], p["b3"], p["w5"], p["b5"], p["wide"], p["prod"], F, p["bias"],
                                        p["label"], B, dims[0], dims[1], dims[2], p["logit"], p["prob"], p["loss"], p["ws"], ws_bytes, None)


UNLABELLED = ("label", "loss", "ws")
OTHER_WIDTHS = [(256, 256, 128), (512, 128, 128), (512, 256, 64), (512, 256, 256), (504, 256, 128), (0, 0, 0)]


def test_symbols_declared_bound_and_exported():
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    decl = re.search(r"\bint mrec_tail_predict\(([^;]*)\);", text)
    assert decl, "mrec_tail_predict is not declared in include/mrec.h"
    assert re.search(r"\bint mrec_tail_predict_supported\(int64_t B, int32_t K2, int32_t N2, int32_t N3\);", text)
    assert re.search(r"\bint mrec_tail_predict_workspace_bytes\(int64_t B, size_t\* out\);", text)
    for name in ("mrec_tail_predict", "mrec_tail_predict_supported", "mrec_tail_predict_workspace_bytes"):
        assert name in _lib.EXPORTED, name
    f = _lib.lib().mrec_tail_predict
    assert len(f.argtypes) == decl.group(1).count(",") + 1 == 23
    assert len(_lib.lib().mrec_tail_predict_supported.argtypes) == 4
    assert len(_lib.lib().mrec_tail_predict_workspace_bytes.argtypes) == 2
    assert _lib.lib().mrec_version() >= 107


def test_einval_comes_first():
    assert _call() == EWORKSPACE                                             # the well-formed labelled call: past every earlier check
    assert _call(f16=1) == EWORKSPACE
    assert _call(B=0) == EINVAL and _call(B=-64) == EINVAL
    assert _call(ldx=K2 - 8) == EINVAL and _call(ldx=0) == EINVAL
    for n in ("x", "packed", "b2", "b3", "w5", "b5", "logit", "prob"):
        assert _call(null=(n,)) == EINVAL, n
        assert _call(null=(n,) + UNLABELLED) == EINVAL, n                    # ... in the unlabelled form too
    assert _call(wide=True, prod=True, F=3, bias=True) == EINVAL             # both forms of the wide branch
    assert _call(wide=False, prod=False) == EINVAL                           # neither
    assert _call(wide=False, prod=True, F=0, bias=True) == EINVAL            # products without a field count
    assert _call(wide=False, prod=True, F=-1, bias=True) == EINVAL
    assert _call(wide=False, prod=True, F=3, bias=False) == EINVAL           # products without the bias
    assert _call(wide=False, prod=True, F=3, bias=True) == EWORKSPACE        # the products form itself is accepted
    assert _call(wide=False, prod=True, F=64, bias=True) == EWORKSPACE
    # label and loss: both or neither
    assert _call(null=("label",)) == EINVAL and _call(null=("loss",)) == EINVAL
    assert _call(null=("label", "ws")) == EINVAL and _call(null=("loss", "ws")) == EINVAL
    # a bad argument AND a bad shape is EINVAL
    for dims in OTHER_WIDTHS:
        assert _call(dims=dims, null=("w5",)) == EINVAL, dims
        assert _call(dims=dims, null=("label",)) == EINVAL, dims
        assert _call(dims=dims, wide=False) == EINVAL, dims
    assert _call(B=32769, null=("prob",)) == EINVAL
    assert _call(B=32769, wide=False, prod=True, F=65, bias=False) == EINVAL
    # ... and so is a bad argument with a misaligned pointer or too many fields
    assert _call(off={"x": 8}, null=("loss",)) == EINVAL
    assert _call(wide=False, prod=True, F=65, bias=False) == EINVAL


def test_unsupported_comes_second():
    for dims in OTHER_WIDTHS:
        assert _call(dims=dims, ldx=1024) == EUNSUPPORTED, dims
        assert _call(dims=dims, ldx=1024, null=UNLABELLED) == EUNSUPPORTED, dims      # the unlabelled form refuses the same shapes
    assert _call(B=32769) == EUNSUPPORTED and _call(B=1 << 40) == EUNSUPPORTED
    assert _call(B=32768) == EWORKSPACE and _call(B=1) == EWORKSPACE and _call(B=209) == EWORKSPACE
    assert _call(wide=False, prod=True, F=65, bias=True) == EUNSUPPORTED
    assert _call(wide=False, prod=True, F=65, bias=True, null=UNLABELLED) == EUNSUPPORTED
    for ldx in (K2 + 1, K2 + 4, K2 + 12):
        assert _call(ldx=ldx) == EUNSUPPORTED, ldx
    assert _call(ldx=K2 + 8) == EWORKSPACE and _call(ldx=K2 + 24) == EWORKSPACE
    # the pointers the kernel reads 16 bytes at a time
    for n in ("x", "packed", "b2", "b3", "w5"):
        for o in (2, 4, 8):
            if o == 2 and n not in ("x", "packed"):
                continue
            assert _call(off={n: o}) == EUNSUPPORTED, (n, o)
            assert _call(off={n: o}, null=UNLABELLED) == EUNSUPPORTED, (n, o)        # without a label it is the last check, ws or not
            assert _call(off={n: o}, null=("label", "loss")) == EUNSUPPORTED, (n, o)
    # ... and the ones it reads a float at a time may sit anywhere a float may
    for n in ("b5", "wide", "label", "logit", "prob", "loss", "ws"):
        assert _call(off={n: 4}) == EWORKSPACE, n
    assert _call(wide=False, prod=True, F=3, bias=True, off={"prod": 8, "bias": 4}) == EWORKSPACE
    # a bad shape AND a misaligned pointer is EUNSUPPORTED; all of it before the workspace
    assert _call(dims=(256, 256, 128), off={"x": 8}) == EUNSUPPORTED
    assert _call(B=32769, off={"w5": 4}, ws_bytes=1 << 20) == EUNSUPPORTED
    assert _call(off={"b2": 8}, ws_bytes=1 << 20) == EUNSUPPORTED


def test_workspace_check():
    from mindrec_amd import _lib
    # one float per workgroup of 64 rows
    for B, nbytes in ((1, 4), (64, 4), (65, 8), (32768, 2048)):
        assert _lib.query_bytes("mrec_tail_predict_workspace_bytes", B) == nbytes, B
        assert _call(B=B, ws_bytes=nbytes - 1) == EWORKSPACE, B
        assert _call(B=B, ws_bytes=0) == EWORKSPACE, B
        assert _call(B=B, ws_bytes=1 << 20, null=("ws",)) == EWORKSPACE, B          # with a label a missing workspace is one too small
    out = C.c_size_t(0)
    assert _lib.lib().mrec_tail_predict_workspace_bytes(-1, C.byref(out)) == EINVAL
    assert _lib.lib().mrec_tail_predict_workspace_bytes(4, None) == EINVAL


def test_shape_predicate():
    from mindrec_amd import ops
    f = lambda B, dims=(K2, N2, N3): ops.tail_predict_supported(B, *dims)
    assert all(f(B) for B in range(1, 32769))
    assert not f(0) and not f(-1) and not f(32769) and not f(32832) and not f(1 << 40)
    for dims in OTHER_WIDTHS + [(128, 256, 512), (1024, 512, 256)]:
        assert not f(64, dims) and not f(1, dims), dims
    # every batch the training launch takes, the evaluation launch takes
    assert all(f(B) for B in range(64, 32769, 64) if ops.tail_supported(B, K2, N2, N3))
