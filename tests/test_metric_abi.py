"""The evaluation-metric entry points (mrec_auc_counts, mrec_group_rank_hist and their workspace queries) on a machine without a GPU:
declared, exported and bound; the workspace queries grow with n; argument errors come back before any HIP call; the Python wrappers
refuse what they cannot run on the host."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
NEW = ("mrec_auc_ws_bytes", "mrec_auc_counts", "mrec_group_rank_ws_bytes", "mrec_group_rank_hist")


def test_new_symbols_declared_exported_and_bound():
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", text))
    l = _lib.lib()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/mrec.h"
        assert name in _lib.EXPORTED, f"{name} is not in the binding table"
        assert hasattr(l, name), f"{name} is not exported"


@pytest.mark.parametrize("query", ["mrec_auc_ws_bytes", "mrec_group_rank_ws_bytes"])
def test_workspace_queries_are_monotone(query):
    from mindrec_amd import _lib
    sizes = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 1 << 16, (1 << 20) + 1, 1 << 22, (1 << 30) - 1]
    got = [_lib.query_bytes(query, n) for n in sizes]
    assert all(b >= a for a, b in zip(got, got[1:])), got
    assert got[0] > 0 and got[-1] > got[0]
    n = 1 << 22
    if query == "mrec_auc_ws_bytes":
        assert got[sizes.index(n)] >= 4 * 4 * n + 8 * (n + 1)          # two (key, class) buffers + the compacted boundaries
    else:
        assert got[sizes.index(n)] >= 16 * n                           # clicked row, rows and rows above it per group
    l = _lib.lib()
    out = C.c_size_t()
    assert getattr(l, query)(-1, C.byref(out)) == EINVAL
    assert getattr(l, query)(4, None) == EINVAL
    assert getattr(l, query)(1 << 31, C.byref(out)) == EUNSUPPORTED


def test_argument_errors_before_any_hip_call():
    from mindrec_amd import _lib
    l = _lib.lib()
    p = C.c_void_p(256)                                                 # a non-null pointer nothing dereferences
    assert l.mrec_auc_counts(None, None, 8, None, None, 0, None) == EINVAL
    assert l.mrec_auc_counts(p, p, 0, p, p, 1 << 20, None) == EINVAL                      # n == 0
    assert l.mrec_auc_counts(p, p, 1 << 31, p, p, 1 << 20, None) == EUNSUPPORTED
    assert l.mrec_auc_counts(p, p, 4097, p, p, 64, None) == EWORKSPACE
    assert l.mrec_group_rank_hist(None, None, None, None, 8, 12, 30, None, None, 0, None) == EINVAL
    for topk in (0, -1, 65):
        assert l.mrec_group_rank_hist(p, p, p, p, 8, topk, 30, p, p, 1 << 20, None) == EINVAL
    assert l.mrec_group_rank_hist(p, p, p, p, 8, 12, -1, p, p, 1 << 20, None) == EINVAL
    assert l.mrec_group_rank_hist(p, p, p, p, 0, 12, 30, p, p, 1 << 20, None) == EINVAL
    assert l.mrec_group_rank_hist(p, p, p, p, 1 << 30, 12, 30, p, p, 1 << 20, None) == EUNSUPPORTED
    assert l.mrec_group_rank_hist(p, p, p, p, 4097, 12, 30, p, p, 64, None) == EWORKSPACE


def test_python_wrappers_refuse_on_the_host():
    import torch
    from mindrec_amd import ops
    from mindrec_amd.metrics import DeviceAUCMAPMetric, DeviceAUCMetric
    f, g = torch.zeros(8), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(TypeError, match="no CPU fallback"):
        ops.auc_counts(f, f)
    with pytest.raises(TypeError, match="no CPU fallback"):
        ops.group_rank_hist(f, f, g)
    for bad in (f.double(), f.half(), g):
        with pytest.raises(TypeError, match="float32"):
            ops.auc_counts(bad, f)
        with pytest.raises(TypeError, match="float32"):
            ops.auc_counts(f, bad)
        with pytest.raises(TypeError, match="float32"):
            ops.group_rank_hist(f, bad, g)
    with pytest.raises(TypeError, match="int32"):
        ops.group_rank_hist(f, f, f)
    with pytest.raises(TypeError, match="int32"):
        ops.group_rank_hist(f, f, g.to(torch.int16))
    with pytest.raises(ValueError, match="rows"):
        ops.auc_counts(f, torch.zeros(7))
    with pytest.raises(ValueError, match="rows"):
        ops.group_rank_hist(f, f, g[:5])
    with pytest.raises(ValueError, match="contiguous"):
        ops.auc_counts(torch.zeros(16)[::2], f)
    with pytest.raises(ValueError, match="contiguous"):
        ops.auc_counts(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="no rows"):
        ops.auc_counts(f[:0], f[:0])
    for topk in (0, 65, 2.0):
        with pytest.raises(ValueError, match="topk"):
            ops.group_rank_hist(f, f, g, topk=topk)
        with pytest.raises(ValueError, match="topk"):
            DeviceAUCMAPMetric(topk=topk)
    with pytest.raises(ValueError, match="pad_to"):
        ops.group_rank_hist(f, f, g, pad_to=-1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        DeviceAUCMetric(device="cpu")
    with pytest.raises(ValueError, match="capacity"):
        DeviceAUCMetric(capacity=0)
    m = DeviceAUCMetric(capacity=64)                                    # building one touches no device
    with pytest.raises(ValueError, match="no rows"):
        m.eval()
