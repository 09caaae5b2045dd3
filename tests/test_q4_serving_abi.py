"""The 4-bit FM and pooled lookups without a GPU: test_q4_abi.py's check (declared in include/mrec.h, bound with the 8-bit arguments)."""
import pytest

from test_q4_abi import test_entry_declared_and_bound as _declared_and_bound


@pytest.mark.parametrize("name", ["mrec_q4_fm_lookup", "mrec_q4_gather_pool_fields"])
def test_entry_declared_and_bound(name):
    _declared_and_bound(name)
