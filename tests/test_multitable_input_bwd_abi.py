"""mrec_mt_input_bwd (the backward of the multitable Wide&Deep's input stage) on a machine without a GPU: both entries declared, exported
and bound; every refusal comes back with its code before any HIP call, in the documented order (include/mrec.h) -- no call here gets
as far as a launch: each holds a defect, or null pointers, or B == 0; the workspace query; the host restatement the GPU tests compare
with (tests/_multitable_bwd_ref.py) on one hand-computed case."""
import ctypes as C
import os
import re

import numpy as np

import _multitable_bwd_cases as K
import _multitable_bwd_ref as BR
import _multitable_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
P = 0x10000          # a non-null, 16-byte aligned address that nothing dereferences: every call below is refused before a launch


def test_symbols_declared_exported_and_bound():
    from mindrec_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", text))
    for name, nargs in (("mrec_mt_input_bwd", 17), ("mrec_mt_input_bwd_workspace_bytes", 5)):
        assert name in declared and name in _lib.EXPORTED and len(getattr(_lib.lib(), name).argtypes) == nargs
    assert f"MREC_MT_BWD_MAX_GROUPS {ops.MT_BWD_MAX_GROUPS}" in text and "} mrec_mt_grp_t;" in text
    assert K.chunk_len() == ops.MT_BWD_CHUNK >= 64
    assert C.sizeof(ops.MtGrp) == 72 and [n for n, _ in ops.MtGrp._fields_] == re.findall(
        r"[ *]([a-z_]+);", re.search(r"typedef struct \{([^}]*?)\} mrec_mt_grp_t;", text, flags=re.S).group(1))


def _seg(D=64, L=2, pooled=0, col=8, ld_ids=None, mask=None):
    return dict(table=None, V=0, ld=D, D=D, wide=None, ids=None, ld_ids=L if ld_ids is None else ld_ids, mask=mask, L=L, pooled=pooled, col=col)


def _call(groups, B=5, C_=8, K0=None, ldg=None, kind=2, g=None, gw=None, cont=None, dc=None, db=None, ws=None, ws_bytes=0, ld_cont=None,
          gs=1.0, n_groups=None, null_groups=False, query=False, **grp):
    """groups: [[seg dict, ..], ..]; grp: per-call overrides of every group's record (n=, ptr= for the five index / output pointers)"""
    from mindrec_amd import _lib, ops
    keep, arr = [], (ops.MtGrp * max(len(groups), 1))()
    end = C_
    for i, segs in enumerate(groups):
        sa = (ops.MtSeg * max(len(segs), 1))(*[ops.MtSeg(**s) for s in segs])
        keep.append(sa)
        Ls = sum(max(s["L"], 0) for s in segs)
        end = max([end] + [s["col"] + s["D"] * (1 if s["pooled"] == 1 else max(s["L"], 1)) for s in segs])
        ptr = grp.get("ptr")
        arr[i] = ops.MtGrp(None if grp.get("null_segs") else C.cast(sa, C.c_void_p), grp.get("n_segs", len(segs)), ptr, ptr, ptr, ptr,
                           grp.get("n", B * Ls), grp.get("sums", ptr), grp.get("wsums", ptr))
    K0 = end if K0 is None else K0
    gp = None if null_groups else C.cast(arr, C.c_void_p)
    ng = len(groups) if n_groups is None else n_groups
    if query:
        out = C.c_size_t(0)
        return _lib.lib().mrec_mt_input_bwd_workspace_bytes(gp, ng, B, C_, C.byref(out)), out.value
    return _lib.lib().mrec_mt_input_bwd(g, kind, K0 if ldg is None else ldg, K0, gw, cont, C_ if ld_cont is None else ld_cont, C_, gp, ng, B,
                                        gs, dc, db, ws, ws_bytes, None)


ALL = dict(g=P, gw=P, cont=P, dc=P, db=P, ptr=P)      # every pointer non-null and aligned; the callers add one defect each


def test_einval_before_any_hip_call():
    one = [[_seg()]]
    assert _call(one) == EINVAL                                      # null pointers: the baseline
    assert _call(one, n_groups=-1) == EINVAL
    assert _call(one * 9, n_groups=9) == EINVAL
    assert _call(one, null_groups=True) == EINVAL
    assert _call(one, B=-1, n=0) == EINVAL
    assert _call(one, kind=3) == EINVAL
    assert _call(one, K0=200, ldg=192) == EINVAL                     # ldg < K0
    assert _call(one, ld_cont=4) == EINVAL
    assert _call(one, gs=float("inf")) == EINVAL
    assert _call(one, gs=float("nan")) == EINVAL
    assert _call(one, n_segs=0) == EINVAL
    assert _call(one, null_segs=True) == EINVAL
    assert _call(one, n=-2) == EINVAL
    assert _call([[_seg(D=8, L=1, col=8)] * 9, [_seg(D=8, L=1, col=8)] * 8]) == EINVAL          # 17 segments in all
    for bad in (_seg(L=0), _seg(pooled=2), _seg(D=0), _seg(ld_ids=1), _seg(col=-8)):
        assert _call([[bad]], **ALL) == EINVAL
    assert _call([[_seg(D=64), _seg(D=128, col=136)]], **ALL) == EINVAL                          # one table, one width
    assert _call(one, n=11, **ALL) == EINVAL                         # Ls = 2 does not divide n
    assert _call(one, n=12, **ALL) == EINVAL                         # n / Ls != B
    assert _call(one, K0=128, ldg=128, **ALL) == EINVAL              # the block ends at 136 > K0
    assert _call([[_seg(pooled=1, col=72)]], K0=128, ldg=128, **ALL) == EINVAL
    for hole in ("g", "gw", "cont", "dc", "db", "ptr"):
        assert _call(one, **{**ALL, hole: None}) == EINVAL, hole
    assert _call(one, C_=0, **{**ALL, "gw": None, "cont": None, "dc": None, "db": None}) == EINVAL      # g_wide: the group has wsums
    # a group that can be long needs the workspace
    rc, nbytes = _call(one, B=1000, query=True)
    assert rc == 0 and nbytes >= 8 * 2 * (64 + 4) * 4 + 4 * 9 * 4
    assert _call(one, B=1000, **ALL) == EWORKSPACE
    assert _call(one, B=1000, ws=P, ws_bytes=nbytes - 1, **ALL) == EWORKSPACE


def test_eunsupported_and_the_order_of_refusals():
    assert _call([[_seg(D=12)]]) == EUNSUPPORTED
    assert _call([[_seg(D=264)]]) == EUNSUPPORTED
    assert _call([[_seg(col=12)]]) == EUNSUPPORTED
    assert _call([[_seg()]], K0=140, ldg=144) == EUNSUPPORTED
    assert _call([[_seg()]], ldg=140) == EUNSUPPORTED
    assert _call([[_seg(L=1)]], B=1 << 31, C_=0) == EUNSUPPORTED     # n >= 2^31
    one = [[_seg()]]
    assert _call(one, **{**ALL, "g": P + 8}) == EUNSUPPORTED
    assert _call(one, **{**ALL, "sums": P + 8}) == EUNSUPPORTED
    rc, nbytes = _call(one, B=1000, query=True)
    assert _call(one, B=1000, ws=P + 8, ws_bytes=nbytes + 8, **ALL) == EUNSUPPORTED
    # an argument error wins over a shape refusal, a shape refusal over the column blocks, all of them over B == 0 and the pointers
    assert _call([[_seg(D=12, L=0)]]) == EINVAL
    assert _call([[_seg(D=12)]], K0=16, ldg=16, **ALL) == EUNSUPPORTED
    assert _call([[_seg(D=12)]], B=0) == EUNSUPPORTED
    assert _call(one, B=0, K0=128, ldg=128) == EINVAL


def test_the_reference_layout_passes_and_b0_returns_ok():
    ref = [[_seg(D=64, L=2, col=32)], [_seg(D=128, L=3, col=160)], [_seg(D=64, L=2, col=544)],
           [_seg(D=64, L=L, pooled=1, col=672 + 64 * f) for f, L in enumerate((3, 5, 4, 3, 4, 2))]]
    assert _call(ref, C_=32) == EINVAL                               # K0 = 1056: nothing but the null pointers is refused
    assert _call(ref, C_=32, B=0) == 0                               # nothing to do, nothing touched, no launch
    assert _call([], C_=0, B=0, K0=0) == 0
    rc, nbytes = _call(ref, C_=32, B=16384, query=True)
    assert rc == 0 and 0 < nbytes < 8 << 20
    assert _call(ref, C_=32, B=64, query=True)[0] == 0
    assert _call(ref[:1], C_=0, B=64, query=True) == (0, 0)          # 128 positions, no continuous values: one launch, no workspace


def test_host_restatement_against_hand_computed_answers():
    """B = 2, D = 8: a single-hot group (L = 2, ids [[1, 1], [0, 1]]) and a pooled group of two bags (L = 2 and 1; masks [[1, 0], [2, 1]] and
    none) sharing id 4; every value a small dyadic number, so the expected sums are exact by hand."""
    g = np.zeros((2, 40), np.float32)
    g[0, 8:16], g[0, 16:24], g[1, 8:16], g[1, 16:24] = 1, 2, 4, 8
    g[0, 24:32], g[0, 32:40], g[1, 24:32], g[1, 32:40] = 16, 32, 64, 128
    gw = np.array([0.5, 0.25], np.float32)
    t = np.zeros((5, 8), np.float32)
    s1 = R.Seg(t, np.array([[1, 1], [0, 1]], np.int32), 8, False, None, None)
    u, s, b, w, wb = BR.group_sums(g, gw, [s1], 0.5)
    assert list(u) == [1, 0] and np.array_equal(s[:, 0], [(1 + 2 + 8) * 0.5, 4 * 0.5]) and np.array_equal(w, [(0.5 + 0.5 + 0.25) * 0.5, 0.125])
    assert (b > 0).all() and (b < 1e-5).all()
    p1 = R.Seg(t, np.array([[4, 2], [2, 4]], np.int32), 24, True, np.array([[1, 0], [2, 1]], np.float32), None)
    p2 = R.Seg(t, np.array([[4], [3]], np.int32), 32, True, None, None)
    u, s, b, w, wb = BR.group_sums(g, gw, [p1, p2])
    assert list(u) == [4, 2, 3]
    # id 4: bag 1 of sample 0 (16 * 1 / 2), bag 2 of sample 0 (32 * 1 / 1), bag 1 slot 1 of sample 1 (64 * 1 / 2); id 2: a masked slot, 64 * 2 / 2
    assert np.array_equal(s[:, 3], [8 + 32 + 32, 0 + 64, 128]) and np.array_equal(w, [0.5 + 0.5 + 0.25, 0.5, 0.25])
    d, bd, db, bb = BR.cont_grads(gw, np.array([[1, 2], [4, 8]], np.float32), 2.0)
    assert np.array_equal(d, [3.0, 6.0]) and db == 1.5 and (bd > 0).all() and bb > 0
