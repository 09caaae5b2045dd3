"""The frozen key index's and the keyed FM lookups' entries without a GPU: declared in include/mrec.h, bound with its argument count."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mrec_kidx_bytes", "mrec_kidx_build", "mrec_kidx_release", "mrec_kidx_find", "mrec_q8_fm_lookup_keyed", "mrec_q4_fm_lookup_keyed"]


@pytest.mark.parametrize("name", NAMES)
def test_entry_declared_and_bound(name):
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)", text)
    assert m, f"{name} is not declared in include/mrec.h"
    assert name in _lib._SIGS and name in _lib.EXPORTED, f"{name} is not in the binding table"
    assert len(_lib._SIGS[name]) == len(m.group(1).split(",")), "the binding's argument count differs from the declaration's"
    assert getattr(_lib.lib(), name).argtypes == _lib._SIGS[name]
