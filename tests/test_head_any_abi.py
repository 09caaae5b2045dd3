"""mrec_head_fwd_bwd_any (the output head for any last hidden width K5 % 8 == 0 up to 2048) over the C ABI, without a device: the
symbol, its binding, and the order in which it refuses -- EINVAL, then the width, then the alignment, then the workspace -- all of
it decided before any launch.  Every call here carries a workspace too small for its shape, so none of them can reach a launch.
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


def _call(kind=0, K5=24, B=4, F=0, wide=True, prod=False, bias=False, dh_scale=1.0, ws_bytes=0, h4_off=0, dh4_off=0, null=()):
    from mindrec_amd import _lib
    raw, a = _buf()
    p = {n: C.c_void_p(a) for n in ("h4", "w5", "b5", "wide", "prod", "bias", "label", "logit", "dlogit", "dh4", "dw5", "db4", "db5", "dwb",
                                    "loss", "ws")}
    p["h4"], p["dh4"] = C.c_void_p(a + h4_off), C.c_void_p(a + dh4_off)
    if not wide:
        p["wide"] = None
    if not prod:
        p["prod"] = None
    if not bias:
        p["bias"] = None
    for n in null:
        p[n] = None
    return _lib.lib().mrec_head_fwd_bwd_any(kind, p["h4"], p["w5"], p["b5"], p["wide"], p["prod"], F, p["bias"], p["label"], B, K5, 1.0, dh_scale,
                                            p["logit"], p["dlogit"], p["dh4"], p["dw5"], p["db4"], p["db5"], p["dwb"], p["loss"], p["ws"],
                                            ws_bytes, None)


def test_symbol_declared_bound_and_exported():
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    decl = re.search(r"\bint mrec_head_fwd_bwd_any\(([^;]*)\);", text)
    assert decl, "mrec_head_fwd_bwd_any is not declared in include/mrec.h"
    assert "mrec_head_fwd_bwd_any" in _lib.EXPORTED
    f = _lib.lib().mrec_head_fwd_bwd_any
    assert len(f.argtypes) == decl.group(1).count(",") + 1 == 24
    assert _lib.lib().mrec_version() >= 102


def test_width_check():
    for K5 in (12, 2056, 4, 2052):
        assert _call(K5=K5) == EUNSUPPORTED, K5
    for K5 in (8, 24, 520, 1024, 2048):            # past the width check: the next refusal is the workspace's
        for kind in (0, 1, 2):
            assert _call(K5=K5, kind=kind) == EWORKSPACE, (K5, kind)
    # the entries of the first head kernel refuse what they refused
    from mindrec_amd import _lib
    raw, a = _buf()
    p = C.c_void_p(a)
    for name in ("bf16", "f16", "f32"):
        for K5 in (24, 520, 1024):
            assert getattr(_lib.lib(), "mrec_head_fwd_bwd_" + name)(p, p, p, p, p, 4, K5, 1.0, 1.0, p, p, p, p, p, p, p, p, 0, None) == EUNSUPPORTED


def test_einval_comes_first():
    assert _call(wide=True, prod=True, F=3, bias=True) == EINVAL          # both forms of the wide branch
    assert _call(wide=False, prod=False) == EINVAL                         # neither
    assert _call(wide=False, prod=True, F=0, bias=True) == EINVAL          # products without a field count
    assert _call(wide=False, prod=True, F=3, bias=False) == EINVAL         # products without the bias
    assert _call(wide=False, prod=True, F=3, bias=True) == EWORKSPACE      # the products form itself is accepted
    assert _call(kind=3) == EINVAL and _call(kind=-1) == EINVAL
    assert _call(B=0) == EINVAL and _call(K5=0) == EINVAL and _call(K5=-8) == EINVAL
    assert _call(dh_scale=0.5) == EINVAL and _call(dh_scale=float("nan")) == EINVAL
    for n in ("h4", "w5", "b5", "label", "logit", "dlogit", "dh4", "dw5", "db4", "db5", "loss", "ws"):
        assert _call(null=(n,)) == EINVAL, n
    assert _call(null=("dwb",)) == EWORKSPACE                               # dwide_bias may be NULL
    # ... before the width: a bad argument AND a bad width is EINVAL; a bad width AND a misaligned row is EUNSUPPORTED
    assert _call(K5=12, null=("w5",)) == EINVAL
    assert _call(K5=12, h4_off=8) == EUNSUPPORTED
    assert _call(K5=24, h4_off=8) == EINVAL and _call(K5=24, dh4_off=4) == EINVAL


def test_workspace_check():
    from mindrec_amd import _lib
    for K5 in (24, 520, 2048):
        need = (2 * K5 + 2) * 4                    # B = 1: one workgroup, one partial row
        assert _call(K5=K5, B=1, ws_bytes=need - 1) == EWORKSPACE
        for B in (1, 1000, 1 << 20):
            assert _lib.query_bytes("mrec_head_workspace_bytes", B, K5) >= 256 * need      # the launch never has more than 256 workgroups


def test_width_predicates():
    from mindrec_amd import ops
    assert [K5 for K5 in range(0, 2100) if ops.head_any_supported(K5)] == list(range(8, 2049, 8))
    assert [K5 for K5 in range(1, 2100) if ops.head_supported(K5)] == [8, 16, 32, 64, 128, 256, 512]
