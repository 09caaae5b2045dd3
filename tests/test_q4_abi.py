"""Row-wise 4-bit serving records without a GPU: the three entries are declared in include/mrec.h and bound in _lib._SIGS with the 8-bit
entries' arguments, and a Q8Table built from four values is an 8-bit one."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["mrec_q4_row_bytes", "mrec_q4_quantize_rows", "mrec_q4_gather_rows"])
def test_entry_declared_and_bound(name):
    from mindrec_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", text)
    assert m, f"{name} is not declared in include/mrec.h"
    assert name in _lib._SIGS and name in _lib.EXPORTED, f"{name} is not in the binding table"
    assert len(_lib._SIGS[name]) == len(m.group(1).split(",")), "the binding's argument count differs from the declaration's"
    assert getattr(_lib.lib(), name).argtypes == _lib._SIGS[name] == _lib._SIGS[name.replace("_q4_", "_q8_")]
    assert [_lib.lib().mrec_q4_row_bytes(D) for D in (4, 20, 36, 80, 256, 6, 260)] == [32, 32, 48, 64, 144, -3, -3]
    assert ops.Q8Table(None, 67, 80, 96).bits == 8 and ops.Q8Table(None, 67, 80, 64, 4).bits == 4
