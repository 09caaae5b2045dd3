"""The pooled lookup over 8-bit records without a GPU: its entry is declared in include/mrec.h and bound in _lib._SIGS."""
import os
import re


def test_entry_declared_and_bound(name="mrec_q8_gather_pool_fields"):
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mrec.h")).read(), flags=re.S)
    m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", text)
    assert m, f"{name} is not declared in include/mrec.h"
    assert name in _lib._SIGS and name in _lib.EXPORTED, f"{name} is not in the binding table"
    assert len(_lib._SIGS[name]) == len(m.group(1).split(",")) == 17, "the binding's argument count differs from the declaration's"
    assert getattr(_lib.lib(), name).argtypes == _lib._SIGS[name]
