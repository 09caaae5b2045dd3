"""max_norm over multi-hot fields (mrec_gather_pool_fields_clip, mrec_gather_pool_fields_keyed_clip,
mrec_sparse_apply_next_pool_fields_clip) on a machine without a GPU: declared, exported and bound; argument errors and the float4
limits come back before any HIP call (null device pointers everywhere); a refused or invalid arm leaves nothing armed; the clip arm is
refused by everything that is not a plain LazyAdam apply; the Python wrappers and the three classes check max_norm on the host."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
NEW = ("mrec_gather_pool_fields_clip", "mrec_gather_pool_fields_keyed_clip", "mrec_sparse_apply_next_pool_fields_clip")
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
    for name in NEW[:2]:
        plain = getattr(l, name[: -len("_clip")]).argtypes
        assert list(getattr(l, name).argtypes) == list(plain[:-1]) + [C.c_float] + list(plain[-1:])
    assert list(getattr(l, NEW[2]).argtypes) == list(l.mrec_sparse_apply_next_pool_fields.argtypes) + [C.c_float]


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


def _seg(l, n=1 << 30, gs=1.0):
    return l.mrec_segment_sum_f32(None, None, None, n, None, 4, None, gs, 4, None, None, 0, None)


def _adam(l, D=4, n=16, gs=1.0):      # (ld = ldg = D)
    return l.mrec_sparse_lazy_adam_f32_i32(None, None, None, 10, D, D, None, None, None, None, n, None, D, None, 1e-3, 0.9, 0.999, 1e-8,
                                           0.9, 0.999, gs, 0, None, 0, None)


def _ftrl(l):
    return l.mrec_sparse_ftrl_f32_i32(None, None, None, 10, 4, 4, None, None, None, None, 16, None, 4, None, 5e-2, 1e-8, 1e-8, -0.5, 1.0,
                                      None, 0, None)


LENS, SC = (1, 2, 1), (1.0, 0.5, 1.0)                                 # Ls = 4: n = 2^30 positions are n * Ls = 2^32


def _arm(l, c=0.5, F=3, lens=LENS, sc=SC):
    return l.mrec_sparse_apply_next_pool_fields_clip(F, _i32(lens) if lens is not None else None, _f32(sc) if sc is not None else None, c)


def test_clip_arm_is_for_one_call():
    """What 'armed' means is visible without a GPU: a segment sum refuses the clip arm as unsupported before it looks at its (null)
    pointers (an armed segment sum over n * Ls >= 2^32 positions is refused either way); a plain one gets as far as the pointers."""
    from mindrec_amd import _lib
    l = _lib.lib()
    assert _seg(l) == EINVAL                                          # plain: null pointers
    assert _arm(l) == 0
    assert _seg(l) == EUNSUPPORTED                                    # armed
    assert _seg(l) == EINVAL                                          # ... for that one call
    assert _arm(l) == 0
    assert _adam(l) == EINVAL                                         # a LazyAdam apply takes the arm (and stops at its null pointers)
    assert _seg(l) == EINVAL
    assert _arm(l) == 0
    assert _adam(l, gs=0.5) == EINVAL and _seg(l) == EINVAL           # grad_scale must be 1: refused, and disarmed
    assert _arm(l, F=1, lens=(4,), sc=(0.25,)) == 0                   # F = 1 with field_scale = {grad_scale}: the equal-length case
    assert _seg(l) == EUNSUPPORTED and _seg(l) == EINVAL


def test_clip_arm_errors_leave_nothing_armed():
    from mindrec_amd import _lib
    l = _lib.lib()
    bad = [dict(c=c) for c in BAD_NORMS] + [dict(F=0), dict(F=-2), dict(lens=None), dict(sc=None), dict(lens=(1, 0, 1)),
                                            dict(sc=(1.0, float("nan"), 1.0)), dict(sc=(1.0, float("inf"), 1.0))]
    for kw in bad:
        assert _arm(l) == 0
        assert _arm(l, **kw) == EINVAL, kw
        assert _seg(l) == EINVAL, kw                                  # nothing armed: the earlier arm is gone too
        assert l.mrec_sparse_apply_next_pool_fields(3, _i32(LENS), _f32(SC)) == 0
        assert _arm(l, **kw) == EINVAL, kw                            # ... and so is an earlier arm of the plain fields form
        assert _seg(l) == EINVAL, kw
    assert _arm(l) == 0
    assert _arm(l, F=2, lens=(MAX_BAG, 1), sc=(1.0, 1.0)) == EUNSUPPORTED
    assert _seg(l) == EINVAL
    assert _arm(l) == 0
    assert _arm(l, F=MAX_FIELDS + 1, lens=(1,) * (MAX_FIELDS + 1), sc=(1.0,) * (MAX_FIELDS + 1)) == EUNSUPPORTED
    assert _seg(l) == EINVAL


def test_the_pooled_arms_replace_each_other():
    from mindrec_amd import _lib
    l = _lib.lib()
    # the clip arm, then a plain pooled arm: the clip is gone (FTRL refuses a clip arm, and runs into its null pointers under a plain one)
    assert _arm(l) == 0
    assert l.mrec_sparse_apply_next_pool_fields(3, _i32(LENS), _f32(SC)) == 0
    assert _ftrl(l) == EINVAL
    assert _arm(l) == 0
    assert l.mrec_sparse_apply_next_pool(4) == 0
    assert _ftrl(l) == EINVAL
    assert _arm(l) == 0
    assert l.mrec_sparse_apply_next_pool(1) == 0                      # the plain apply: disarms
    assert _seg(l) == EINVAL
    # a plain pooled arm, then the clip arm: the clip arm holds
    assert l.mrec_sparse_apply_next_pool(4) == 0
    assert _arm(l) == 0
    assert _ftrl(l) == EUNSUPPORTED
    assert _ftrl(l) == EINVAL


def test_clip_arm_refused_by_everything_but_the_plain_lazy_adam_apply():
    from mindrec_amd import _lib
    l = _lib.lib()
    wargs = (None, None, None, 10, 8, 4, None, 4, None, None, None, 16, None, 0, 4, None, 1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999, 1.0, 0,
             None, 1, 2, 4, 5e-2, 1e-8, 1e-8, -0.5, None, 0, None, None)
    fin = (C.c_ubyte * 448)()

    def wide():
        return l.mrec_sparse_lazy_adam_wide(*wargs, None)

    def defer():
        return l.mrec_sparse_lazy_adam_wide_defer(*wargs, C.cast(fin, C.c_void_p), None)

    def seg():
        return _seg(l, n=16)

    def ftrl():
        return _ftrl(l)

    def adam():
        return _adam(l)

    calls = (wide, defer, seg, ftrl, adam)
    plain = tuple(f() for f in calls)
    assert EUNSUPPORTED not in plain
    for f in (wide, defer, seg, ftrl):                                # the folded wide forms, a segment sum, an FTRL apply
        assert _arm(l) == 0
        assert f() == EUNSUPPORTED, f.__name__
        assert tuple(g() for g in calls) == plain, f.__name__         # disarmed by the refusal: every call after it is plain
    # widths the clip cannot run at: refused by the armed call, before it looks at its pointers
    for D in (6, 260):
        assert _adam(l, D=D) == EINVAL                                # plain: null pointers
        assert _arm(l) == 0
        assert _adam(l, D=D) == EUNSUPPORTED
        assert _adam(l, D=D) == EINVAL and tuple(g() for g in calls) == plain
    assert _arm(l) == 0 and _adam(l, D=256) == EINVAL                 # the widest row is supported
    # a separately armed max_norm on top of it: refused like today, and both are disarmed
    assert _arm(l) == 0
    assert l.mrec_sparse_apply_next_max_norm(1.0) == 0
    assert adam() == EUNSUPPORTED
    assert _seg(l) == EINVAL and tuple(g() for g in calls) == plain
    # ... and the old combination is what it was
    assert l.mrec_sparse_apply_next_pool_fields(3, _i32(LENS), _f32(SC)) == 0
    assert l.mrec_sparse_apply_next_max_norm(1.0) == 0
    assert adam() == EUNSUPPORTED
    assert tuple(g() for g in calls) == plain


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
    arm, rows, gs = ops._pooled(Plan, None, (3, 5, 4), (1.0, 0.5, 0.25), 1.0, 0.5)
    assert arm[0] == "mrec_sparse_apply_next_pool_fields_clip" and arm[1] == 3 and arm[4] == 0.5 and rows[0] == 6 and gs == 1.0
    arm, rows, gs = ops._pooled(Plan, 4, None, None, 0.25, 0.5)       # pool=L: F = 1, field_scale = {grad_scale}
    assert arm[0] == "mrec_sparse_apply_next_pool_fields_clip" and arm[1] == 1 and list(arm[2]) == [4] and list(arm[3]) == [0.25]
    assert rows[0] == 6 and gs == 1.0
    assert ops._pooled(Plan, 4, None, None, 0.25)[0] == ("mrec_sparse_apply_next_pool", 4)      # without it: today's arms
    assert ops._pooled(Plan, None, (3, 5, 4), None, 1.0)[0][0] == "mrec_sparse_apply_next_pool_fields"
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
