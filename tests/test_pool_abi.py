"""The multi-hot entry points (mrec_gather_pool, the pool member of mrec_apply_opts_t) on a machine without a GPU: declared, exported
and bound; argument errors come back before any HIP call (null pointers everywhere); a refused record changes nothing for the call
after it; the Python wrappers refuse CPU tensors."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
NEW = ("mrec_gather_pool",)


def test_new_symbols_declared_exported_and_bound():
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", text))
    l = _lib.lib()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/mrec.h"
        assert name in _lib.EXPORTED, f"{name} is not in the binding table"
        assert getattr(l, name).argtypes is not None
    assert "MREC_POOL_MAX_BAG 4096" in text and "int32_t pool;" in text and "} mrec_apply_opts_t;" in text


def _pool(l, V=10, ld=8, D=8, id_bytes=4, B=5, L=3, mode=1, out_kind=0, ldo=0):
    return l.mrec_gather_pool(None, V, ld, D, None, id_bytes, B, L, None, mode, None, out_kind, ldo, None)


def test_gather_pool_argument_errors_before_any_hip_call():
    from mindrec_amd import _lib
    l = _lib.lib()
    assert _pool(l, L=0) == EINVAL
    assert _pool(l, L=-2) == EINVAL
    assert _pool(l, L=4097) == EUNSUPPORTED
    assert _pool(l, L=4096) == EINVAL            # the longest bag is supported: what is refused here is the null table
    assert _pool(l, ld=4) == EINVAL              # ld < D
    assert _pool(l, B=-1) == EINVAL
    assert _pool(l, D=0) == EINVAL
    assert _pool(l, ldo=4) == EINVAL             # ldo < D
    assert _pool(l, id_bytes=2) == EINVAL
    assert _pool(l, out_kind=3) == EINVAL
    assert _pool(l, mode=2) == EINVAL
    assert _pool(l, V=0) == EINVAL               # no row to read
    assert _pool(l, B=0) == 0                    # nothing to do, nothing touched
    assert _pool(l) == EINVAL                    # null pointers


def _rec(**members):
    from mindrec_amd import ops
    return C.byref(ops.ApplyOpts(**members))


def test_next_pool_refuses_and_leaves_nothing_armed():
    """pool = 0 and -1 are MREC_EINVAL; what the pooled form means is visible without a GPU: a pooled segment sum over n * L >= 2^32
    positions is refused as unsupported before it looks at its (null) pointers, a plain one gets as far as the pointers -- and the
    same call with opts = NULL right afterwards is the plain call: nothing travels from one call to the next."""
    from mindrec_amd import _lib, ops
    l = _lib.lib()

    def seg(opts=None, n=1 << 30):
        return l.mrec_segment_sum_f32(None, None, None, n, None, 4, None, 1.0, 4, None, None, 0, opts, None)

    assert seg() == EINVAL                                         # plain: null pointers
    assert seg(_rec(pool=4)) == EUNSUPPORTED                       # pooled: n * L = 2^32
    assert seg() == EINVAL                                         # ... for that one call
    assert seg(n=0) == 0                                           # (nothing to do: a call that only a bad record can fail)
    for bad in (0, -1):
        assert seg(_rec(pool=bad), n=0) == EINVAL
        assert seg(_rec(pool=bad)) == EINVAL
        assert seg() == EINVAL and seg(n=0) == 0                   # the plain call after it
    assert seg(_rec(pool=1)) == EINVAL and seg(_rec(pool=1), n=0) == 0      # L = 1 is the plain apply
    rec = ops.ApplyOpts(pool=4)
    for wrong in (0, 4, C.sizeof(ops.ApplyOpts) - 8, C.sizeof(ops.ApplyOpts) + 8):
        rec.struct_bytes = wrong
        assert seg(C.byref(rec), n=0) == EINVAL, wrong             # a record of another size is not read at all
    assert seg() == EINVAL and seg(n=0) == 0


def test_next_pool_refused_for_the_folded_wide_apply_and_max_norm():
    from mindrec_amd import _lib
    l = _lib.lib()
    n = 1 << 30
    wargs = (None, None, None, 10, 8, 4, None, 4, None, None, None, 16, None, 0, 4, None, 1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999, 1.0, 0,
             None, 1, 2, 4, 5e-2, 1e-8, 1e-8, -0.5, None, 0, None, None)
    fin = (C.c_ubyte * 448)()

    def wide(opts=None):
        return l.mrec_sparse_lazy_adam_wide(*wargs, opts, None)

    def defer(opts=None):
        return l.mrec_sparse_lazy_adam_wide_defer(*wargs, C.cast(fin, C.c_void_p), opts, None)

    def adam(opts=None):
        return l.mrec_sparse_lazy_adam_f32_i32(None, None, None, 10, 4, 4, None, None, None, None, 16, None, 4, None, 1e-3, 0.9, 0.999, 1e-8,
                                               0.9, 0.999, 1.0, 0, None, 0, opts, None)

    def seg():
        return l.mrec_segment_sum_f32(None, None, None, n, None, 4, None, 1.0, 4, None, None, 0, None, None)

    plain = (wide(), defer(), adam())
    assert EUNSUPPORTED not in plain
    for call in (wide, defer):
        assert call(_rec(pool=2)) == EUNSUPPORTED
        assert seg() == EINVAL                                     # the call after the refusal is plain
    assert adam(_rec(pool=2, max_norm=1.0)) == EUNSUPPORTED        # max_norm and pool together
    assert seg() == EINVAL and (wide(), defer(), adam()) == plain  # ... and plain calls after it


def test_cpu_tensors_refused():
    import torch
    from mindrec_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_pool(torch.zeros(4, 4), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_pool(torch.zeros(4, 4), torch.zeros((2, 3), dtype=torch.int32), torch.ones(2, 3))


def test_pool_keyword_is_checked_on_the_host():
    from mindrec_amd import ops
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            ops._pool(bad)
    assert ops._pool(7) == 7
