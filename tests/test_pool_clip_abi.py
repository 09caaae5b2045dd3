"""max_norm over multi-hot fields (mrec_gather_pool_fields_clip, mrec_gather_pool_fields_keyed_clip, max_norm beside the fields form in
mrec_apply_opts_t) on a machine without a GPU: declared, exported and bound; argument errors and the float4 limits come back before any
HIP call (null device pointers everywhere); a refused or invalid record changes nothing for the call after it; the pooled clip is
refused by everything that is not a plain LazyAdam apply; the Python wrappers and the three classes check max_norm on the host."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
NEW = ("mrec_gather_pool_fields_clip", "mrec_gather_pool_fields_keyed_clip")
MAX_FIELDS, MAX_BAG = 64, 4096
BAD_NORMS = (0.0, -1.0, float("inf"), float("nan"))


def _i32(xs):
    return (C.c_int32 * max(len(xs), 1))(*xs)


def _f32(xs):
    return (C.c_float * max(len(xs), 1))(*xs)


def test_new_symbols_declared_exported_and_bound():
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", text))
    l = _lib.lib()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/mrec.h"
        assert name in _lib.EXPORTED, f"{name} is not in the binding table"
        assert getattr(l, name).argtypes is not None
    # the existing argument lists plus `float max_norm` before `stream`
    for name in NEW:
        plain = getattr(l, name[: -len("_clip")]).argtypes
        assert list(getattr(l, name).argtypes) == list(plain[:-1]) + [C.c_float] + list(plain[-1:])
    assert "float max_norm;" in text and "} mrec_apply_opts_t;" in text      # the apply's clip: a member of the options record


def _poolc(l, V=10, ld=8, D=8, id_bytes=4, B=5, lens=(3, 5, 4), F=None, mode=1, out_kind=0, ldo=0, c=0.5):
    return l.mrec_gather_pool_fields_clip(None, V, ld, D, None, id_bytes, B, len(lens) if F is None else F, _i32(lens), None, mode, None,
                                          out_kind, ldo, c, None)


def _poolkc(l, V=10, ld=8, D=8, key_bytes=8, B=5, lens=(3, 5, 4), F=None, mode=1, out_kind=0, ldo=0, sigma=0.01, fill=0.0, c=0.5):
    return l.mrec_gather_pool_fields_keyed_clip(None, V, ld, D, None, None, key_bytes, B, len(lens) if F is None else F, _i32(lens), None,
                                                mode, 7, sigma, fill, None, out_kind, ldo, c, None)


@pytest.mark.parametrize("call", [_poolc, _poolkc])
def test_clip_lookups_argument_errors_before_any_hip_call(call):
    from mindrec_amd import _lib
    l = _lib.lib()
    for c in BAD_NORMS:
        assert call(l, c=c) == EINVAL
        assert call(l, c=c, B=0) == EINVAL                            # ... whatever else the call holds
    assert call(l, D=6, ld=8) == EUNSUPPORTED                         # float4 rows only
    assert call(l, D=260, ld=260) == EUNSUPPORTED                     # one column block: a row's norm is one lane-group's
    assert call(l, D=8, ld=10) == EUNSUPPORTED                        # rows that are not 16-byte aligned
    assert call(l, D=8, ldo=26) == EUNSUPPORTED                       # output rows that are not
    assert call(l, D=256, ld=256) == EINVAL                           # the widest row is supported: what is refused is the null table
    assert call(l, D=4, ld=4) == EINVAL
    assert call(l, F=0) == EINVAL
    assert call(l, lens=(3, 0, 4)) == EINVAL                          # an empty bag
    assert call(l, lens=(MAX_BAG, 1)) == EUNSUPPORTED                 # Ls over the bag limit
    assert call(l, lens=(1,) * (MAX_FIELDS + 1)) == EUNSUPPORTED      # F over the field limit
    assert call(l, ldo=23) == EINVAL                                  # ldo < F * D = 24
    assert call(l, ld=4) == EINVAL                                    # ld < D
    assert call(l, B=-1) == EINVAL
    assert call(l, D=0) == EINVAL
    assert call(l, out_kind=3) == EINVAL
    assert call(l, mode=2) == EINVAL
    assert call(l, V=0) == EINVAL                                     # no row to read
    assert call(l, B=1 << 30) == EUNSUPPORTED                         # B * F bags are numbered in 32 bits
    assert call(l, B=0) == 0                                          # nothing to do, nothing touched
    assert call(l) == EINVAL                                          # null pointers
    if call is _poolc:
        assert call(l, id_bytes=2) == EINVAL
    else:
        assert call(l, key_bytes=2) == EINVAL
        assert call(l, sigma=float("nan")) == EINVAL and call(l, fill=float("inf")) == EINVAL


LENS, SC = (1, 2, 1), (1.0, 0.5, 1.0)                                 # Ls = 4: n = 2^30 positions are n * Ls = 2^32


def _rec(c=0.5, F=3, lens=LENS, sc=SC, **members):
    """the record of a pooled apply under the clip, by reference"""
    from mindrec_amd import ops
    return C.byref(ops.ApplyOpts(n_fields=F, field_len=_i32(lens) if lens is not None else None,
                                 field_scale=_f32(sc) if sc is not None else None, max_norm=c, **members))


def _seg(l, opts=None, n=1 << 30, gs=1.0):
    return l.mrec_segment_sum_f32(None, None, None, n, None, 4, None, gs, 4, None, None, 0, opts, None)


def _adam(l, opts=None, D=4, n=16, gs=1.0):      # (ld = ldg = D)
    return l.mrec_sparse_lazy_adam_f32_i32(None, None, None, 10, D, D, None, None, None, None, n, None, D, None, 1e-3, 0.9, 0.999, 1e-8,
                                           0.9, 0.999, gs, 0, None, 0, opts, None)


def _ftrl(l, opts=None, n=16):
    return l.mrec_sparse_ftrl_f32_i32(None, None, None, 10, 4, 4, None, None, None, None, n, None, 4, None, 5e-2, 1e-8, 1e-8, -0.5, 1.0,
                                      None, 0, opts, None)


def test_clip_arm_is_for_one_call():
    """What the pooled clip means is visible without a GPU: a segment sum refuses it as unsupported before it looks at its (null)
    pointers (a pooled segment sum over n * Ls >= 2^32 positions is refused either way); a plain one gets as far as the pointers."""
    from mindrec_amd import _lib
    l = _lib.lib()
    assert _seg(l) == EINVAL                                          # plain: null pointers
    assert _seg(l, _rec()) == EUNSUPPORTED                            # with the record
    assert _seg(l, _rec(), n=0) == EUNSUPPORTED and _seg(l, n=0) == 0
    assert _seg(l) == EINVAL                                          # ... for that one call
    assert _adam(l, _rec()) == EINVAL                                 # a LazyAdam apply takes it (and stops at its null pointers)
    assert _adam(l, _rec(), n=0) == 0
    assert _seg(l) == EINVAL
    assert _adam(l, _rec(), gs=0.5) == EINVAL and _adam(l, _rec(), gs=0.5, n=0) == EINVAL      # grad_scale must be 1
    assert _adam(l, n=0, gs=0.5) == 0 and _seg(l) == EINVAL           # ... and the plain call after it
    one = dict(F=1, lens=(4,), sc=(0.25,))                            # F = 1 with field_scale = {grad_scale}: the equal-length case
    assert _adam(l, _rec(**one), n=0) == 0
    assert _seg(l, _rec(**one)) == EUNSUPPORTED and _seg(l) == EINVAL


def test_clip_arm_errors_leave_nothing_armed():
    from mindrec_amd import _lib
    l = _lib.lib()
    # (max_norm = 0.0, an error of the old arming entry, is the record's "none": the fields form without a clip -- last lines)
    bad = [dict(c=c) for c in BAD_NORMS if c != 0.0] + [dict(F=0), dict(F=-2), dict(lens=None), dict(sc=None), dict(lens=(1, 0, 1)),
                                                        dict(sc=(1.0, float("nan"), 1.0)), dict(sc=(1.0, float("inf"), 1.0))]
    for kw in bad:
        assert _adam(l, _rec(**kw), n=0) == EINVAL, kw                # answered first, whatever else the call holds
        assert _seg(l, _rec(**kw), n=0) == EINVAL, kw                 # ... before the entry is asked whether it takes a clip at all
        assert _seg(l) == EINVAL and _adam(l, n=0) == 0, kw           # the plain calls after it
        assert _seg(l, _rec(**dict(kw, c=kw.get("c", 0.0))), n=0) == EINVAL, kw      # ... and the same error without the clip
    assert _adam(l, _rec(F=2, lens=(MAX_BAG, 1), sc=(1.0, 1.0)), n=0) == EUNSUPPORTED
    assert _adam(l, n=0) == 0
    assert _adam(l, _rec(F=MAX_FIELDS + 1, lens=(1,) * (MAX_FIELDS + 1), sc=(1.0,) * (MAX_FIELDS + 1)), n=0) == EUNSUPPORTED
    assert _adam(l, n=0) == 0
    # the plain max_norm of a LazyAdam apply: the same four bounds
    from mindrec_amd import ops
    for c in BAD_NORMS:
        rc = _adam(l, C.byref(ops.ApplyOpts(max_norm=c)), n=0)
        assert rc == (0 if c == 0.0 else EINVAL), c
    assert _ftrl(l, _rec(c=0.0), n=0) == 0 and _ftrl(l, _rec(c=0.5), n=0) == EUNSUPPORTED      # 0.0: no clip, FTRL takes the fields form


def test_the_pooled_arms_replace_each_other():
    """one record, one form: the clip is a member beside the fields form, so a record without it is the plain pooled apply (FTRL
    refuses the pooled clip, and runs into its null pointers under a plain pooled form), and pool = L takes no clip"""
    from mindrec_amd import _lib, ops
    l = _lib.lib()
    assert _ftrl(l, _rec()) == EUNSUPPORTED
    assert _ftrl(l, _rec(c=0.0)) == EINVAL and _ftrl(l, _rec(c=0.0), n=0) == 0
    assert _ftrl(l, C.byref(ops.ApplyOpts(pool=4))) == EINVAL and _ftrl(l, C.byref(ops.ApplyOpts(pool=4)), n=0) == 0
    assert _ftrl(l, C.byref(ops.ApplyOpts(pool=4, max_norm=0.5)), n=0) == EUNSUPPORTED
    assert _adam(l, C.byref(ops.ApplyOpts(pool=4, max_norm=0.5)), n=0) == EUNSUPPORTED
    assert _ftrl(l, _rec(pool=4), n=0) == EINVAL                      # pool = L and the fields form in one record
    assert _seg(l, C.byref(ops.ApplyOpts(pool=1))) == EINVAL          # pool = 1: the plain apply
    assert _ftrl(l) == EINVAL and _ftrl(l, n=0) == 0


def test_clip_arm_refused_by_everything_but_the_plain_lazy_adam_apply():
    from mindrec_amd import _lib, ops
    l = _lib.lib()
    wargs = (None, None, None, 10, 8, 4, None, 4, None, None, None, 16, None, 0, 4, None, 1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999, 1.0, 0,
             None, 1, 2, 4, 5e-2, 1e-8, 1e-8, -0.5, None, 0, None, None)
    fin = (C.c_ubyte * 448)()

    def wide(opts=None):
        return l.mrec_sparse_lazy_adam_wide(*wargs, opts, None)

    def defer(opts=None):
        return l.mrec_sparse_lazy_adam_wide_defer(*wargs, C.cast(fin, C.c_void_p), opts, None)

    def seg(opts=None):
        return _seg(l, opts, n=16)

    def ftrl(opts=None):
        return _ftrl(l, opts)

    def adam(opts=None):
        return _adam(l, opts)

    calls = (wide, defer, seg, ftrl, adam)
    plain = tuple(f() for f in calls)
    assert EUNSUPPORTED not in plain
    for f in (wide, defer, seg, ftrl):                                # the folded wide forms, a segment sum, an FTRL apply
        assert f(_rec()) == EUNSUPPORTED, f.__name__
        assert tuple(g() for g in calls) == plain, f.__name__         # every call after the refusal is plain
    # widths the clip cannot run at: refused before the call looks at its pointers
    for D in (6, 260):
        assert _adam(l, D=D) == EINVAL                                # plain: null pointers
        assert _adam(l, _rec(), D=D) == EUNSUPPORTED
        assert _adam(l, D=D) == EINVAL and tuple(g() for g in calls) == plain
    assert _adam(l, _rec(), D=256) == EINVAL                          # the widest row is supported
    # the plain max_norm: LazyAdam entries only, and not beside pool = L
    for f in (seg, ftrl):
        assert f(C.byref(ops.ApplyOpts(max_norm=1.0))) == EUNSUPPORTED, f.__name__
    assert adam(C.byref(ops.ApplyOpts(max_norm=1.0, pool=4))) == EUNSUPPORTED
    assert _seg(l) == EINVAL and tuple(g() for g in calls) == plain


def test_python_wrappers_check_max_norm_on_the_host():
    import torch
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotEmbedding, MultiHotHashEmbedding, MultiHotWideDeep
    ids = torch.zeros((2, 12), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_pool_fields(torch.zeros(4, 4), ids, (3, 5, 4), max_norm=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_pool(torch.zeros(4, 4), ids, max_norm=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_pool_fields_keyed(torch.zeros(4, 4), ids, ids, (3, 5, 4), max_norm=0.5, default=(0.01, None, 0))

    class Plan:
        n = 24

    for c in BAD_NORMS:
        with pytest.raises(ValueError):
            ops._pooled(Plan, None, (3, 5, 4), None, 1.0, c)
    with pytest.raises(ValueError):
        ops._pooled(Plan, None, None, None, 1.0, 0.5)                 # pool_max_norm goes with pool= or fields=
    rec, rows, gs = ops._pooled(Plan, None, (3, 5, 4), (1.0, 0.5, 0.25), 1.0, 0.5)
    assert (rec.struct_bytes, rec.pool, rec.n_fields, rec.max_norm) == (C.sizeof(ops.ApplyOpts), 1, 3, 0.5) and rows[0] == 6 and gs == 1.0
    assert rec.field_len[:3] == [3, 5, 4] and rec.field_scale[:3] == [1.0, 0.5, 0.25] and not rec.const_state and not rec.const_ids
    rec, rows, gs = ops._pooled(Plan, 4, None, None, 0.25, 0.5)       # pool=L: F = 1, field_scale = {grad_scale}
    assert (rec.pool, rec.n_fields, rec.max_norm) == (1, 1, 0.5) and rec.field_len[:1] == [4] and rec.field_scale[:1] == [0.25]
    assert rows[0] == 6 and gs == 1.0
    rec, rows, gs = ops._pooled(Plan, 4, None, None, 0.25)            # without it: pool = L, scaled by the call's grad_scale
    assert (rec.pool, rec.n_fields, rec.max_norm, bool(rec.field_len), bool(rec.field_scale)) == (4, 0, 0.0, False, False)
    assert rows[0] == 6 and gs == 0.25
    rec, rows, gs = ops._pooled(Plan, None, (3, 5, 4), None, 1.0)
    assert (rec.pool, rec.n_fields, rec.max_norm) == (1, 3, 0.0) and rec.field_len[:3] == [3, 5, 4] and rec.field_scale[:3] == [1.0] * 3
    assert ops._pooled(Plan, None, None, None, 0.5) == (None, None, 0.5)      # the plain apply: no record
    # the classes: everything about max_norm is checked before the device
    for opt in ("ftrl", "adam"):
        with pytest.raises(ValueError, match="max_norm"):
            MultiHotEmbedding(100, 8, (3, 5, 4), optimizer=opt, device="cpu", max_norm=0.5)
        with pytest.raises(ValueError, match="max_norm"):
            MultiHotWideDeep(100, 8, (3, 5, 4), optimizer=opt, device="cpu", max_norm=0.5)
    for dim in (6, 260):
        with pytest.raises(ValueError, match="max_norm"):
            MultiHotEmbedding(100, dim, (3, 5, 4), device="cpu", max_norm=0.5)
    for c in BAD_NORMS:
        with pytest.raises(ValueError, match="max_norm"):
            MultiHotEmbedding(100, 8, (3, 5, 4), device="cpu", max_norm=c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MultiHotEmbedding(100, 8, (3, 5, 4), device="cpu", max_norm=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MultiHotWideDeep(100, 8, (3, 5, 4), device="cpu", max_norm=0.5)      # (ftrl on the wide half: never clipped, not refused)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MultiHotHashEmbedding(dict(key_dtype=torch.int64, value_shape=8, capacity=64, device="cpu"), bag=(3, 5), max_norm=0.5)
