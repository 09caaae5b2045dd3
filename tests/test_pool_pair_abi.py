"""MultiHotWideDeep and MultiHotEmbedding.apply_(plan=) on a machine without a GPU: the class refuses a CPU device and a malformed
`bag`, `mode` or `wide_optimizer` on the host, the bag before the device; apply_ takes a plan."""
import pytest

MAX_FIELDS, MAX_BAG = 64, 4096


def test_pair_class_checks_on_the_host():
    from mindrec_amd.multi_hot import MultiHotEmbedding, MultiHotWideDeep
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MultiHotWideDeep(100, 8, (3, 5, 4), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MultiHotWideDeep(100, 8, 7, device="cpu")                   # an int: one field
    for bad in ((), (3, 0, 4), (3, 2.5), (1,) * (MAX_FIELDS + 1), (MAX_BAG, 1), 0, -3):
        with pytest.raises(ValueError):
            MultiHotWideDeep(100, 8, bad, device="cpu")              # the bag is checked before the device
    with pytest.raises(ValueError):
        MultiHotWideDeep(100, 8, (3, 5), wide_optimizer="sgd", device="cpu")
    with pytest.raises(ValueError):
        MultiHotWideDeep(100, 8, (3, 5), mode="max", device="cpu")
    import inspect
    assert "plan" in inspect.signature(MultiHotEmbedding.apply_).parameters
    assert inspect.signature(MultiHotEmbedding.apply_).parameters["plan"].default is None
