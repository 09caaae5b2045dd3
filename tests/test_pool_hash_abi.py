"""The keyed pooled lookup (mrec_gather_pool_fields_keyed) and MultiHotHashEmbedding on a machine without a GPU: the entry is declared,
exported and bound; every argument error comes back with its documented code before any HIP call (null device pointers everywhere);
the class refuses the dense optimizer and a CPU device, and the wrapper CPU tensors."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
NAME = "mrec_gather_pool_fields_keyed"
MAX_FIELDS, MAX_BAG = 64, 4096


def _i32(xs):
    return (C.c_int32 * max(len(xs), 1))(*xs)


def _keyed(l, V=10, ld=8, D=8, key_bytes=8, B=5, lens=(3, 5, 4), F=None, mode=1, seed=7, sigma=0.01, fill=0.0, out_kind=0, ldo=0):
    return getattr(l, NAME)(None, V, ld, D, None, None, key_bytes, B, len(lens) if F is None else F, _i32(lens), None, mode, seed, sigma,
                            fill, None, out_kind, ldo, None)


def test_symbol_declared_exported_and_bound():
    from mindrec_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", text))
    assert NAME in declared, f"{NAME} is not declared in include/mrec.h"
    assert NAME in _lib.EXPORTED, f"{NAME} is not in the binding table"
    assert len(getattr(_lib.lib(), NAME).argtypes) == 19
    assert callable(ops.gather_pool_fields_keyed)


def test_argument_errors_before_any_hip_call():
    from mindrec_amd import _lib
    l = _lib.lib()
    for kb in (0, 2, 3, 16, -4):
        assert _keyed(l, key_bytes=kb) == EINVAL
    assert _keyed(l, F=0) == EINVAL
    assert _keyed(l, F=-1) == EINVAL
    assert _keyed(l, lens=(1,) * (MAX_FIELDS + 1)) == EUNSUPPORTED   # F > 64
    assert _keyed(l, lens=(MAX_BAG, 1)) == EUNSUPPORTED              # Ls > 4096
    assert _keyed(l, lens=(MAX_BAG + 1,)) == EUNSUPPORTED
    assert _keyed(l, lens=(3, 0, 4)) == EINVAL                       # an L_f < 1
    assert _keyed(l, lens=(3, 5, -1)) == EINVAL
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert _keyed(l, sigma=bad) == EINVAL
        assert _keyed(l, sigma=-1.0, fill=bad) == EINVAL
        assert _keyed(l, fill=bad) == EINVAL                         # (refused whichever of the two the default row uses)
    # the limits themselves are supported: what is refused then is the null table
    assert _keyed(l, lens=(MAX_BAG - 1, 1)) == EINVAL
    assert _keyed(l, lens=(1,) * MAX_FIELDS) == EINVAL
    assert _keyed(l, key_bytes=4) == EINVAL and _keyed(l, key_bytes=8) == EINVAL
    assert _keyed(l, sigma=-1.0, fill=0.5) == EINVAL
    # ... and what mrec_gather_pool_fields checks
    assert _keyed(l, ldo=23) == EINVAL                               # ldo < F * D = 24
    assert _keyed(l, ld=4) == EINVAL
    assert _keyed(l, B=-1) == EINVAL
    assert _keyed(l, D=0) == EINVAL
    assert _keyed(l, out_kind=3) == EINVAL
    assert _keyed(l, mode=2) == EINVAL
    assert _keyed(l, V=0) == EINVAL
    assert _keyed(l, B=1 << 30) == EUNSUPPORTED                      # B * F bags are numbered in 32 bits
    assert _keyed(l, B=0) == 0                                       # nothing to do, nothing touched
    assert getattr(l, NAME)(None, 10, 8, 8, None, None, 8, 5, 3, None, None, 1, 7, 0.01, 0.0, None, 0, 0, None) == EINVAL      # no lengths


def test_adam_is_refused():
    from mindrec_amd.multi_hot import MultiHotHashEmbedding
    with pytest.raises(ValueError, match="every row"):
        MultiHotHashEmbedding(dict(value_shape=8), bag=(3, 5), optimizer="adam")
    with pytest.raises(ValueError):
        MultiHotHashEmbedding(dict(value_shape=8), bag=(3, 5), optimizer="sgd")
    with pytest.raises(ValueError):
        MultiHotHashEmbedding(dict(value_shape=8), bag=(3, 5), mode="max")
    for bad in ((), (3, 0, 4), (1,) * (MAX_FIELDS + 1), (MAX_BAG, 1), 0):
        with pytest.raises(ValueError):
            MultiHotHashEmbedding(dict(value_shape=8, device="cpu"), bag=bad)      # the bag is checked before the device


def test_cpu_device_and_cpu_tensors_refused():
    import torch
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotHashEmbedding
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MultiHotHashEmbedding(dict(value_shape=8, device="cpu"), bag=(3, 5, 4))
    rows = torch.zeros((2, 12), dtype=torch.int32)
    keys = torch.zeros((2, 12), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_pool_fields_keyed(torch.zeros(4, 4), rows, keys, (3, 5, 4), default=(0.01, None, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_pool_fields_keyed(torch.zeros(4, 4), rows, keys, (3, 5, 4), torch.ones(2, 12), default=(None, 0.5, 7))
