"""mrec_mt_optim (the table optimizers of the multitable Wide&Deep's step, one launch chain) on a machine without a GPU: both entries
declared, exported and bound, the records mirrored member for member; the workspace query; every refusal comes back with its code
before any HIP call, in the documented order (include/mrec.h) -- no call here gets as far as a launch: each holds a defect, or null
pointers, or nothing to do."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
P = 0x10000          # a non-null, 16-byte aligned address that nothing dereferences: every call below is refused before a launch


def _header():
    return open(os.path.join(ROOT, "include", "mrec.h")).read()


def test_symbols_declared_exported_and_bound():
    from mindrec_amd import _lib, ops
    text = _header()
    decl = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", decl))
    for name, nargs in (("mrec_mt_optim", 10), ("mrec_mt_optim_workspace_bytes", 3), ("mrec_dense_adam_step_f32", 17)):
        assert name in declared and name in _lib.EXPORTED and len(getattr(_lib.lib(), name).argtypes) == nargs
    assert f"MREC_MT_OPT_MAX_VECS {ops.MT_OPT_MAX_VECS}" in text and f"MREC_MT_BWD_MAX_GROUPS {ops.MT_BWD_MAX_GROUPS}" in text
    for cls, cname, size in ((ops.MtOptTab, "mrec_mt_opt_tab_t", 104), (ops.MtOptVec, "mrec_mt_opt_vec_t", 40),
                             (ops.MtOptAdam, "mrec_mt_opt_adam_t", 36), (ops.MtOptFtrl, "mrec_mt_opt_ftrl_t", 20)):
        body = re.search(r"typedef struct \{([^}]*?)\} " + cname + ";", decl, flags=re.S).group(1)
        members = [n for part in body.split(";") for n in re.findall(r"[ *]([A-Za-z_0-9]+)\s*(?:,|$)", part.strip())]
        assert C.sizeof(cls) == size and [n for n, _ in cls._fields_] == members, cname


def _tab(V=40, D=64, U=8, ptr=None, wide="same", **over):
    w = ptr if wide == "same" else wide
    rec = dict(p=ptr, m=ptr, v=ptr, V=V, D=D, w=w, accum=w, linear=w, uniq=ptr, U=U, n_uniq_dev=ptr, sums=ptr, wsums=ptr)
    rec.update(over)
    return rec


def _vec(n=32, ptr=None, **over):
    rec = dict(w=ptr, accum=ptr, linear=ptr, g=ptr, n=n)
    rec.update(over)
    return rec


def _call(tabs, vecs=(), ws=None, ws_bytes=0, n_tabs=None, n_vecs=None, null_tabs=False, null_vecs=False, adam=True, ftrl=True,
          query=False):
    from mindrec_amd import _lib, ops
    ta = (ops.MtOptTab * max(len(tabs), 1))(*[ops.MtOptTab(**t) for t in tabs])
    va = (ops.MtOptVec * max(len(vecs), 1))(*[ops.MtOptVec(**q) for q in vecs])
    tp = None if null_tabs else C.cast(ta, C.c_void_p)
    nt = len(tabs) if n_tabs is None else n_tabs
    if query:
        out = C.c_size_t(0)
        return _lib.lib().mrec_mt_optim_workspace_bytes(tp, nt, C.byref(out)), out.value
    ah = ops.MtOptAdam(0.003, 0.9, 0.999, 1e-6, 0.9, 0.999, 1.0, 0.0, 0)
    fh = ops.MtOptFtrl(0.1, 5e-4, 5e-4, -0.5, 1.0)
    return _lib.lib().mrec_mt_optim(tp, nt, None if null_vecs else C.cast(va, C.c_void_p), len(vecs) if n_vecs is None else n_vecs,
                                    C.cast(C.pointer(ah), C.c_void_p) if adam else None, C.cast(C.pointer(fh), C.c_void_p) if ftrl else None,
                                    None, ws, ws_bytes, None)


def test_workspace_query():
    rc, nbytes = _call([_tab(V=40), _tab(V=16), _tab(V=1)], query=True)
    assert rc == 0 and 57 * 4 <= nbytes <= 57 * 4 + 256              # ONE map of sum(V) ints, not one per table
    ref = [_tab(V=16, D=64), _tab(V=650000, D=128), _tab(V=17300, D=64), _tab(V=20900, D=64)]
    rc, nbytes = _call(ref, query=True)
    assert rc == 0 and (16 + 650000 + 17300 + 20900) * 4 <= nbytes < 3 << 20
    assert _call([], query=True) == (0, 0)
    assert _call([_tab(V=0)], query=True) == (0, 0)
    from mindrec_amd import _lib
    assert _lib.lib().mrec_mt_optim_workspace_bytes(None, 0, None) == EINVAL
    assert _call([_tab()], query=True, null_tabs=True)[0] == EINVAL
    assert _call([_tab()] * 9, query=True)[0] == EINVAL
    assert _call([_tab(V=-1)], query=True)[0] == EINVAL
    assert _call([_tab(D=0)], query=True)[0] == EINVAL
    assert _call([_tab(V=1 << 31)], query=True)[0] == EUNSUPPORTED


def test_einval_before_any_hip_call():
    rc, nbytes = _call([_tab()], query=True)
    full = dict(ws=P, ws_bytes=nbytes)
    assert _call([_tab()]) == EINVAL                                  # null pointers: the baseline
    assert _call([_tab(ptr=P)], n_tabs=-1, **full) == EINVAL
    assert _call([_tab(ptr=P)] * 9, **full) == EINVAL                 # counts over the limits
    assert _call([_tab(ptr=P)], [_vec(ptr=P)] * 5, **full) == EINVAL
    assert _call([_tab(ptr=P)], [_vec(ptr=P)], n_vecs=-1, **full) == EINVAL
    assert _call([_tab(ptr=P)], null_tabs=True, **full) == EINVAL
    assert _call([_tab(ptr=P)], [_vec(ptr=P)], null_vecs=True, **full) == EINVAL
    assert _call([_tab(ptr=P, V=-1)], **full) == EINVAL
    assert _call([_tab(ptr=P, D=0)], **full) == EINVAL
    assert _call([_tab(ptr=P, D=-4)], **full) == EINVAL
    assert _call([_tab(ptr=P, U=-1)], **full) == EINVAL
    assert _call([_tab(ptr=P)], [_vec(ptr=P, n=-1)], **full) == EINVAL
    assert _call([_tab(ptr=P)], adam=False, **full) == EINVAL
    assert _call([_tab(ptr=P)], ftrl=False, **full) == EINVAL
    for hole in ("p", "m", "v", "uniq", "sums", "wsums"):
        assert _call([_tab(ptr=P, **{hole: None})], **full) == EINVAL, hole
    for hole in ("w", "accum", "linear"):                             # a wide vector comes whole
        assert _call([_tab(ptr=P, **{hole: None})], **full) == EINVAL, hole
    for hole in ("w", "accum", "linear", "g"):
        assert _call([_tab(ptr=P)], [_vec(ptr=P, **{hole: None})], **full) == EINVAL, hole
    # what may be null: the device count, the whole wide side (then wsums too), everything of an empty table or vector
    assert _call([_tab(ptr=P, n_uniq_dev=None)]) == EWORKSPACE
    assert _call([_tab(ptr=P, wide=None, wsums=None)]) == EWORKSPACE
    assert _call([_tab(ptr=P, U=0, uniq=None, sums=None, wsums=None)]) == EWORKSPACE
    assert _call([_tab(V=0)], [_vec(n=0)]) == 0                       # nothing to do, nothing touched, no launch
    assert _call([]) == 0


def test_eunsupported_eworkspace_and_the_order_of_refusals():
    rc, nbytes = _call([_tab()], query=True)
    full = dict(ws=P, ws_bytes=nbytes)
    for field in ("p", "m", "v", "sums"):                             # D % 4 == 0: the float4 path wants 16-byte rows
        assert _call([_tab(ptr=P, **{field: P + 8})], **full) == EUNSUPPORTED, field
        assert _call([_tab(ptr=P, D=6, **{field: P + 8})]) == EWORKSPACE, field          # the scalar path takes any address
    assert _call([_tab(ptr=P, V=1 << 31)], **full) == EUNSUPPORTED
    assert _call([_tab(ptr=P, U=1 << 31)], **full) == EUNSUPPORTED
    assert _call([_tab(ptr=P, V=1 << 30, D=1024)], **full) == EUNSUPPORTED               # V * D >= 2^40
    # a short workspace
    assert _call([_tab(ptr=P)]) == EWORKSPACE
    assert _call([_tab(ptr=P)], ws=P, ws_bytes=nbytes - 1) == EWORKSPACE
    assert _call([_tab(ptr=P)], ws=None, ws_bytes=nbytes) == EWORKSPACE
    assert nbytes == 256                                              # (40 ints, rounded up to the arena's 256-byte blocks)
    assert _call([_tab(ptr=P), _tab(ptr=P, V=64)], ws=P, ws_bytes=nbytes) == EWORKSPACE  # sized for one table, called with two: 416 bytes
    # the record wins over the shapes, the shapes over the pointers, the pointers over the alignment, all of them over the workspace
    assert _call([_tab(V=1 << 31, D=0)]) == EINVAL
    assert _call([_tab(V=1 << 31)]) == EUNSUPPORTED
    assert _call([_tab(ptr=P, p=P + 8, m=None)]) == EINVAL
    assert _call([_tab(ptr=P, p=P + 8)]) == EUNSUPPORTED


def test_python_wrapper_refuses_before_a_launch():
    import pytest
    import torch
    from mindrec_amd import ops
    f = lambda *s: torch.zeros(s)
    plan = ops.Dedup(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), None, torch.zeros(1, dtype=torch.int64))
    tab = ops.MtOptTable(f(8, 4), f(8, 4), f(8, 4), plan, f(4, 4))
    adam, ftrl = dict(lr=1e-3), dict(lr=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.multitable_optim_([tab], adam=adam, ftrl=ftrl)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.multitable_optim_([], [ops.MtOptVector(f(4), f(4), f(4), f(4))], adam=adam, ftrl=ftrl)
    with pytest.raises(ValueError, match="at most 8"):
        ops.multitable_optim_([tab] * 9, adam=adam, ftrl=ftrl)
    with pytest.raises(ValueError, match="at most 4"):
        ops.multitable_optim_([], [(f(4),) * 4] * 5, adam=adam, ftrl=ftrl)
    with pytest.raises(TypeError, match="come together"):
        ops.multitable_optim_([tab._replace(w=f(8))], adam=adam, ftrl=ftrl)
    with pytest.raises(TypeError, match="unknown optimizer scalars"):
        ops.multitable_optim_([tab], adam=dict(learning_rate=1.0), ftrl=ftrl)
    ops.multitable_optim_([], adam=adam, ftrl=ftrl)                    # nothing to do
