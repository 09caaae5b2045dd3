"""The fields form of the multi-hot entry points (mrec_gather_pool_fields, the n_fields / field_len / field_scale members of
mrec_apply_opts_t) on a machine without a GPU: declared, exported and bound; argument errors come back before any HIP call (null device
pointers everywhere); a refused or invalid record changes nothing for the call after it (nothing is armed: there is no state); the
Python wrappers check the tuple of bag lengths on the host and refuse CPU tensors."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
NEW = ("mrec_gather_pool_fields",)
MAX_FIELDS, MAX_BAG = 64, 4096


def _i32(xs):
    return (C.c_int32 * max(len(xs), 1))(*xs)


def _f32(xs):
    return (C.c_float * max(len(xs), 1))(*xs)


def test_new_symbols_declared_exported_and_bound():
    from mindrec_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", text))
    l = _lib.lib()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/mrec.h"
        assert name in _lib.EXPORTED, f"{name} is not in the binding table"
        assert getattr(l, name).argtypes is not None
    assert f"MREC_POOL_MAX_FIELDS {MAX_FIELDS}" in text and f"MREC_POOL_MAX_BAG {MAX_BAG}" in text
    for member in ("int32_t n_fields;", "const int32_t* field_len;", "const float* field_scale;", "} mrec_apply_opts_t;"):
        assert member in text
    assert (ops.MAX_FIELDS, ops.MAX_BAG) == (MAX_FIELDS, MAX_BAG)


def _poolf(l, V=10, ld=8, D=8, id_bytes=4, B=5, lens=(3, 5, 4), F=None, mode=1, out_kind=0, ldo=0):
    return l.mrec_gather_pool_fields(None, V, ld, D, None, id_bytes, B, len(lens) if F is None else F, _i32(lens), None, mode, None,
                                     out_kind, ldo, None)


def test_gather_pool_fields_argument_errors_before_any_hip_call():
    from mindrec_amd import _lib
    l = _lib.lib()
    assert _poolf(l, F=0) == EINVAL
    assert _poolf(l, F=-1) == EINVAL
    assert _poolf(l, lens=(3, 0, 4)) == EINVAL                       # an empty bag
    assert _poolf(l, lens=(3, 5, -1)) == EINVAL
    assert _poolf(l, lens=(MAX_BAG, 1)) == EUNSUPPORTED              # Ls over the bag limit
    assert _poolf(l, lens=(1,) * (MAX_FIELDS + 1)) == EUNSUPPORTED   # F over the field limit
    assert _poolf(l, lens=(MAX_BAG - 1, 1)) == EINVAL                # the longest sample is supported: what is refused is the null table
    assert _poolf(l, lens=(1,) * MAX_FIELDS) == EINVAL               # ... and so is the largest number of fields
    assert _poolf(l, ldo=23) == EINVAL                               # ldo < F * D = 24
    assert _poolf(l, ldo=24, B=0) == 0
    assert _poolf(l, ld=4) == EINVAL                                 # ld < D
    assert _poolf(l, B=-1) == EINVAL
    assert _poolf(l, D=0) == EINVAL
    assert _poolf(l, id_bytes=2) == EINVAL
    assert _poolf(l, out_kind=3) == EINVAL
    assert _poolf(l, mode=2) == EINVAL
    assert _poolf(l, V=0) == EINVAL                                  # no row to read
    assert _poolf(l, B=1 << 30) == EUNSUPPORTED                      # B * F bags are numbered in 32 bits
    assert _poolf(l, B=0) == 0                                       # nothing to do, nothing touched
    assert _poolf(l) == EINVAL                                       # null pointers
    assert l.mrec_gather_pool_fields(None, 10, 8, 8, None, 4, 5, 3, None, None, 1, None, 0, 0, None) == EINVAL      # no lengths


def _rec(F, lens, sc, **members):
    """the record of a fields apply (lens / sc: ctypes arrays or None), by reference"""
    from mindrec_amd import ops
    return C.byref(ops.ApplyOpts(n_fields=F, field_len=lens, field_scale=sc, **members))


def _seg(l, opts=None, n=1 << 30, gs=1.0):
    return l.mrec_segment_sum_f32(None, None, None, n, None, 4, None, gs, 4, None, None, 0, opts, None)


def test_next_pool_fields_refuses_and_leaves_nothing_armed():
    """What the fields form means is visible without a GPU: a segment sum with it over n * Ls >= 2^32 positions is refused as
    unsupported before it looks at its (null) pointers, a plain one gets as far as the pointers; and the call with opts = NULL right
    after any of them is the plain call."""
    from mindrec_amd import _lib
    l = _lib.lib()
    lens, sc = _i32((1, 2, 1)), _f32((1.0, 0.5, 1.0))                # Ls = 4: n * Ls = 2^32
    assert _seg(l) == EINVAL                                         # plain: null pointers
    assert _seg(l, _rec(3, lens, sc)) == EUNSUPPORTED                # the fields form
    assert _seg(l) == EINVAL                                         # ... for that one call
    assert _seg(l, n=0) == 0                                         # (nothing to do: a call that only a bad record can fail)
    bad = [(0, lens, sc, EINVAL), (-2, lens, sc, EINVAL), (3, None, sc, EINVAL), (3, lens, None, EINVAL),
           (3, _i32((1, 0, 1)), sc, EINVAL), (3, lens, _f32((1.0, float("nan"), 1.0)), EINVAL),
           (3, lens, _f32((1.0, float("inf"), 1.0)), EINVAL), (2, _i32((MAX_BAG, 1)), sc, EUNSUPPORTED),
           (MAX_FIELDS + 1, _i32((1,) * (MAX_FIELDS + 1)), _f32((1.0,) * (MAX_FIELDS + 1)), EUNSUPPORTED)]
    for F, a, b, code in bad:
        assert _seg(l, _rec(F, a, b), n=0) == code                   # the record is answered first, whatever else the call holds
        assert _seg(l, _rec(F, a, b)) == code
        assert _seg(l) == EINVAL and _seg(l, n=0) == 0               # the plain call after it
    big = _rec(MAX_FIELDS, _i32((1,) * MAX_FIELDS), _f32((1.0,) * MAX_FIELDS))
    assert _seg(l, big, n=1 << 26) == EUNSUPPORTED and _seg(l, n=1 << 26) == EINVAL      # Ls = 64: 2^26 * 64 = 2^32


def test_armed_call_takes_grad_scale_one_only():
    """the fields form has one scale per contribution, the field's: the call's own grad_scale must be 1"""
    from mindrec_amd import _lib
    l = _lib.lib()
    lens, sc = _i32((1, 2, 1)), _f32((1.0, 0.5, 1.0))
    assert _seg(l, n=0, gs=0.5) == 0
    assert _seg(l, _rec(3, lens, sc), n=0, gs=0.5) == EINVAL         # refused for its grad_scale, whatever else the call holds
    assert _seg(l, _rec(3, lens, sc), n=16, gs=0.5) == EINVAL
    assert _seg(l) == EINVAL
    assert _seg(l, _rec(3, lens, sc), gs=0.5) == EINVAL              # refused for its grad_scale BEFORE the range check ...
    assert _seg(l, _rec(3, lens, sc)) == EUNSUPPORTED                # ... which is what the same record meets at grad_scale 1
    assert _seg(l) == EINVAL and _seg(l, n=0, gs=0.5) == 0           # the plain call after it


def test_the_two_pooled_arms_replace_each_other():
    """pool = L and the fields form are two forms of the same thing: a record holds one of them"""
    from mindrec_amd import _lib
    l = _lib.lib()
    lens, sc = _i32((1, 2, 1)), _f32((1.0, 0.5, 1.0))
    assert _seg(l, _rec(3, lens, sc, pool=4), n=0) == EINVAL         # both
    assert _seg(l, _rec(3, lens, sc, pool=1), n=0) == 0              # pool = 1 is no pool: the fields form alone
    assert _seg(l, _rec(0, None, None, pool=1)) == EINVAL            # neither: the plain apply (null pointers)
    assert _seg(l, _rec(0, None, None, pool=1), n=0) == 0
    assert _seg(l, _rec(0, None, None, pool=4)) == EUNSUPPORTED      # pool = 4: out of range at n = 2^30 ...
    assert _seg(l, _rec(1, _i32((1,)), _f32((1.0,)))) == EINVAL      # ... where Ls = 1 is in range (null pointers)
    assert _seg(l) == EINVAL and _seg(l) == EINVAL


def test_next_pool_fields_refused_for_the_folded_wide_apply_and_max_norm():
    from mindrec_amd import _lib
    l = _lib.lib()
    wargs = (None, None, None, 10, 8, 4, None, 4, None, None, None, 16, None, 0, 4, None, 1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999, 1.0, 0,
             None, 1, 2, 4, 5e-2, 1e-8, 1e-8, -0.5, None, 0, None, None)
    fin = (C.c_ubyte * 448)()
    lens, sc = _i32((1, 2, 1)), _f32((1.0, 0.5, 1.0))

    def wide(opts=None):
        return l.mrec_sparse_lazy_adam_wide(*wargs, opts, None)

    def defer(opts=None):
        return l.mrec_sparse_lazy_adam_wide_defer(*wargs, C.cast(fin, C.c_void_p), opts, None)

    def adam(opts=None, D=4):
        return l.mrec_sparse_lazy_adam_f32_i32(None, None, None, 10, D, D, None, None, None, None, 16, None, D, None, 1e-3, 0.9, 0.999, 1e-8,
                                               0.9, 0.999, 1.0, 0, None, 0, opts, None)

    plain = (wide(), defer(), adam())
    assert EUNSUPPORTED not in plain
    for call in (wide, defer):
        assert call(_rec(3, lens, sc)) == EUNSUPPORTED
        assert _seg(l) == EINVAL                                     # the call after the refusal is plain
        assert call() == plain[0 if call is wide else 1]
    # max_norm beside the fields form is the pooled clip (tests/test_pool_clip_abi.py): a LazyAdam apply takes it, at a width the clip
    # can run at; max_norm beside pool = L is refused
    assert adam(_rec(3, lens, sc, max_norm=1.0)) == EINVAL           # (null pointers)
    assert adam(_rec(3, lens, sc, max_norm=1.0), D=6) == EUNSUPPORTED
    assert adam(_rec(0, None, None, pool=4, max_norm=1.0)) == EUNSUPPORTED
    assert _seg(l) == EINVAL and (wide(), defer(), adam()) == plain  # ... and plain calls after them


def test_fields_tuple_is_checked_on_the_host():
    from mindrec_amd import ops
    for bad in ((), (3, 0), (3, -1), (2.5, 1), (1,) * (MAX_FIELDS + 1), (MAX_BAG, 1), 7, "34", (True, 2)):
        with pytest.raises(ValueError):
            ops._fields(bad)
    assert ops._fields([3, 5, 4]) == (3, 5, 4)
    assert ops._fields((1,) * MAX_FIELDS) == (1,) * MAX_FIELDS
    assert ops._field_scales((3, 5), None, 0.25) == (0.25, 0.25)
    assert ops._field_scales((3, 5), (0.5, 2.0), 1.0) == (0.5, 2.0)
    for lens, fs, gs in (((3, 5), (0.5,), 1.0), ((3, 5), (0.5, float("nan")), 1.0), ((3, 5), (0.5, 2.0), 0.5)):
        with pytest.raises(ValueError):
            ops._field_scales(lens, fs, gs)
    with pytest.raises(ValueError):
        ops._fields_arm(None, (1.0,), 1.0)                           # field_scale without fields=


def test_cpu_tensors_refused_and_the_tuple_bag_validated():
    import torch
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotEmbedding
    ids = torch.zeros((2, 12), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_pool_fields(torch.zeros(4, 4), ids, (3, 5, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_pool_fields(torch.zeros(4, 4), ids, (3, 5, 4), torch.ones(2, 12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MultiHotEmbedding(100, 8, (3, 5, 4), device="cpu")
    for bad in ((), (3, 0, 4), (3, 2.5), (1,) * (MAX_FIELDS + 1), (MAX_BAG, 1)):
        with pytest.raises(ValueError):
            MultiHotEmbedding(100, 8, bad, device="cpu")             # the tuple is checked before the device
