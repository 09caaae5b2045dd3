"""max_norm in front of a dense optimizer (mrec_clip_group_sums_f32, DeepFMConfig.max_norm, DeepCrossConfig.max_norm,
DeepFMHashEngine(max_norm=)) on a machine without a GPU: the entry is declared, exported and bound; its argument errors and the float4
limits come back before any HIP call (the pointers it is given are host words it never gets to read); the engines refuse at construction
what the kernels would refuse."""
import ctypes as C
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
NAME = "mrec_clip_group_sums_f32"
BAD_NORMS = (0.0, -1.0, float("inf"), float("nan"))


def _call(l, p=True, uniq=True, sums=True, n_dev=True, V=10, ld=None, D=8, U=5, c=0.5):
    """never-read, 16-byte aligned host words stand in for the device pointers (every case here returns before a launch)"""
    buf = (C.c_char * 64)()
    a = C.c_void_p((C.addressof(buf) + 15) & ~15)
    pick = lambda on: a if on else None  # noqa: E731
    rc = getattr(l, NAME)(pick(p), V, D if ld is None else ld, D, pick(uniq), U, pick(n_dev), pick(sums), c, None)
    del buf
    return rc


def test_entry_declared_exported_and_bound():
    from mindrec_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", text))
    l = _lib.lib()
    assert NAME in declared, f"{NAME} is not declared in include/mrec.h"
    assert NAME in _lib.EXPORTED, f"{NAME} is not in the binding table"
    # p, V, ld, D, uniq_rows, U, n_uniq_dev, sums, max_norm, stream
    assert list(getattr(l, NAME).argtypes) == [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.c_float, C.c_void_p]
    m = re.search(NAME + r"\s*\(([^)]*)\)", text)
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["const float* p", "int64_t V", "int64_t ld", "int32_t D", "const int32_t* uniq_rows", "int64_t U",
                    "const int64_t* n_uniq_dev", "float* sums", "float max_norm", "void* stream"]


def test_argument_errors_before_any_hip_call():
    from mindrec_amd import _lib
    l = _lib.lib()
    for c in BAD_NORMS:
        assert _call(l, c=c) == EINVAL
        assert _call(l, c=c, U=0) == EINVAL                      # ... whatever else the call holds
    for which in ("p", "uniq", "sums"):
        assert _call(l, **{which: False}) == EINVAL              # null pointers
        assert _call(l, **{which: False}, U=0) == EINVAL
    assert _call(l, U=-1) == EINVAL
    assert _call(l, V=-1) == EINVAL
    assert _call(l, D=0, ld=8) == EINVAL
    assert _call(l, D=8, ld=4) == EINVAL                         # ld < D
    for D in (6, 30, 260):
        assert _call(l, D=D) == EUNSUPPORTED                     # float4 rows, one lane-group per row
        assert _call(l, D=D, U=0) == EUNSUPPORTED
    assert _call(l, D=8, ld=10) == EUNSUPPORTED                  # rows that are not 16-byte aligned
    for D in (4, 8, 252, 256):
        assert _call(l, D=D, U=0) == 0                           # nothing to do: no launch
        assert _call(l, D=D, U=0, n_dev=False) == 0              # (the device count is optional)
    assert _call(l, V=0) == 0                                    # an empty table has no row to clip by


@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan"), "0.5", True])
def test_configs_refuse_values(bad):
    from _oracle_engine import OracleDeepCrossEngine, OracleDeepFMEngine
    from mindrec_amd.deep_cross import DeepCrossConfig
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMHashEngine
    fm = dict(data_vocab_size=100, data_emb_dim=16, data_field_size=4, batch_size=8, deep_layer_dims=[8], mlp_dtype="fp32")
    with pytest.raises(ValueError, match="max_norm"):
        OracleDeepFMEngine(DeepFMConfig(max_norm=bad, **fm), "cpu")
    with pytest.raises(ValueError, match="max_norm"):
        OracleDeepCrossEngine(DeepCrossConfig(vocab_size=100, emb_dim=16, field_size=4, batch_size=8, deep_layer_dim=[8, 8], max_norm=bad), "cpu")
    with pytest.raises(ValueError, match="max_norm"):
        DeepFMHashEngine(DeepFMConfig(**fm), "cpu", max_norm=bad)
    with pytest.raises(ValueError, match="max_norm"):
        DeepFMHashEngine(DeepFMConfig(max_norm=bad, **fm), "cpu")


@pytest.mark.parametrize("D", [6, 30, 260])
def test_configs_refuse_widths(D):
    from _oracle_engine import OracleDeepCrossEngine, OracleDeepFMEngine
    from mindrec_amd.deep_cross import DeepCrossConfig
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMHashEngine
    fm = dict(data_vocab_size=100, data_emb_dim=D, data_field_size=4, batch_size=8, deep_layer_dims=[8], mlp_dtype="fp32")
    with pytest.raises(ValueError, match=r"max_norm.*emb_dim"):
        OracleDeepFMEngine(DeepFMConfig(max_norm=0.5, **fm), "cpu")
    with pytest.raises(ValueError, match=r"max_norm.*emb_dim"):
        OracleDeepCrossEngine(DeepCrossConfig(vocab_size=100, emb_dim=D, field_size=4, batch_size=8, deep_layer_dim=[8, 8], max_norm=0.5), "cpu")
    with pytest.raises(ValueError, match=r"max_norm.*emb_dim"):
        DeepFMHashEngine(DeepFMConfig(**fm), "cpu", max_norm=0.5)


def test_deep_cross_default_width_is_refused_with_a_hint():
    from _oracle_engine import OracleDeepCrossEngine
    from mindrec_amd.deep_cross import DeepCrossConfig
    cfg = DeepCrossConfig(vocab_size=100, field_size=4, batch_size=8, deep_layer_dim=[8, 8], max_norm=0.5)
    assert cfg.emb_dim == 30
    with pytest.raises(ValueError, match=r"max_norm.*default emb_dim = 30"):
        OracleDeepCrossEngine(cfg, "cpu")


def test_engines_without_max_norm_construct_as_before():
    """None is not a refusal: the oracle-side engines build on the CPU, and the hash engine gets as far as its no-CPU refusal"""
    from _oracle_engine import OracleDeepCrossEngine, OracleDeepFMEngine
    from mindrec_amd.deep_cross import DeepCrossConfig
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMHashEngine
    fm = dict(data_vocab_size=100, data_emb_dim=30, data_field_size=4, batch_size=8, deep_layer_dims=[8], mlp_dtype="fp32")
    assert OracleDeepFMEngine(DeepFMConfig(**fm), "cpu")._max_norm is None
    assert OracleDeepCrossEngine(DeepCrossConfig(vocab_size=100, field_size=4, batch_size=8, deep_layer_dim=[8, 8]), "cpu")._max_norm is None
    e = OracleDeepFMEngine(DeepFMConfig(**{**fm, "data_emb_dim": 16}, max_norm=0.5), "cpu")
    assert e._max_norm == 0.5 and e._clip_kw() == {"max_norm": 0.5}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeepFMHashEngine(DeepFMConfig(**fm), "cpu")


def test_hash_engine_refuses_max_norm_on_key_shards():
    from mindrec_amd.deepfm import DeepFMConfig, DeepFMHashEngine
    cfg = DeepFMConfig(data_vocab_size=100, data_emb_dim=16, data_field_size=4, batch_size=8, deep_layer_dims=[8], mlp_dtype="fp32")
    with pytest.raises(ValueError, match=r"max_norm.*shards \(world > 1\)"):
        DeepFMHashEngine(cfg, "cpu", rank=0, world=2, max_norm=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # world = 2 without max_norm is not refused for its shards
        DeepFMHashEngine(cfg, "cpu", rank=0, world=2)
