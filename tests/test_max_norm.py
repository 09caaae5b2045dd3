"""max_norm without a GPU: the C entry points validate their arguments before any launch, the engine refuses the modes it has no
clip for, and the clip-aware oracle of the GPU tests agrees with the compat layer's ClipByNorm."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

EINVAL, EUNSUPPORTED = -1, -3


def test_clip_entry_points_validate_before_any_launch():
    from mindrec_amd import _lib
    l = _lib.lib()
    for name in ("mrec_gather_rows_clip_f32_i32", "mrec_gather_rows_clip_f32_i64", "mrec_gather_rows_clip_bf16_i32",
                 "mrec_gather_rows_clip_bf16_i64", "mrec_gather_rows_clip_f16_i32", "mrec_gather_rows_clip_f16_i64"):
        f = getattr(l, name)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert f(None, 10, 80, 80, None, 5, None, None, bad, None) == EINVAL, (name, bad)
        assert f(None, 10, 80, 78, None, 5, None, None, 1.0, None) == EUNSUPPORTED        # D % 4 != 0
        assert f(None, 10, 300, 260, None, 5, None, None, 1.0, None) == EUNSUPPORTED      # D > 256
        assert f(None, 10, 80, 80, None, -1, None, None, 1.0, None) == EINVAL             # the plain checks still apply
    w = l.mrec_gather_rows_wide_clip
    args = lambda D, c: (None, 10, 260, D, None, 4, 1, 4, None, 1, None, 1, D, D, None, 2, None, 0, 0, None, c, None)  # noqa: E731
    assert w(*args(80, 0.0)) == EINVAL
    assert w(*args(80, float("nan"))) == EINVAL
    assert w(*args(256, 1.0)) == EUNSUPPORTED                                                # > 252 with the wide word
    assert w(*args(82, 1.0)) == EUNSUPPORTED
    # the apply takes the bound in its options record: a bad bound is refused first, an unsupported width before any launch
    from mindrec_amd import ops
    rec = lambda c: C.byref(ops.ApplyOpts(max_norm=c))  # noqa: E731
    f = l.mrec_sparse_lazy_adam_f32_i32
    out = C.c_size_t()
    # (n == 0: the plain call returns before any launch; under max_norm, the width is checked first)
    plain = (None, None, None, 10, 80, 78, None, None, None, None, 0, None, 80, None, 1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999, 1.0, 0, None, 0)
    ok = (None, None, None, 10, 80, 80) + plain[6:]
    for bad in (-2.0, float("inf"), float("nan")):
        assert f(*ok, rec(bad), None) == EINVAL
    assert f(*ok, rec(0.0), None) == 0 and f(*plain, rec(0.0), None) == 0      # 0: none
    assert f(*ok, rec(1.0), None) == 0
    assert f(*plain, None, None) == 0
    assert f(*plain, rec(1.0), None) == EUNSUPPORTED
    assert f(*plain, None, None) == 0                      # the same call without the record: plain
    wide = l.mrec_sparse_lazy_adam_wide
    wargs = (None, None, None, 10, 260, 256, None, 4, None, None, None, 0, None, 0, 256, None, 1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999, 1.0, 0,
             None, 1, 1, 256, 5e-2, 1e-8, 1e-8, -0.5, None, 0, None, None)
    assert wide(*wargs, rec(1.0), None) == EUNSUPPORTED    # 256 + the wide record
    assert wide(*wargs, None, None) == 0
    assert l.mrec_sparse_apply_workspace_bytes(10, 80, C.byref(out)) == 0


def test_an_apply_that_never_ran_leaves_nothing_armed():
    """max_norm travels in the refused call's own arguments: when a call is refused before it reaches the library -- here ctypes
    rejects its arguments -- or by the library, the next apply of the thread is not clipped."""
    from mindrec_amd import _lib, ops
    l = _lib.lib()
    plain = (None, None, None, 10, 80, 78, None, None, None, None, 0, None, 80, None, 1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999, 1.0, 0, None, 0)
    rec = C.byref(ops.ApplyOpts(max_norm=0.5))
    with pytest.raises(C.ArgumentError):
        _lib.call("mrec_sparse_lazy_adam_f32_i32", *plain, rec, object())
    assert l.mrec_sparse_lazy_adam_f32_i32(*plain, None, None) == 0      # D = 78 is fine without max_norm (with it: EUNSUPPORTED)
    with pytest.raises(_lib.MrecError) as e:
        _lib.call("mrec_sparse_lazy_adam_f32_i32", *plain, rec, None)     # refused by the library
    assert e.value.code == EUNSUPPORTED
    assert l.mrec_sparse_lazy_adam_f32_i32(*plain, None, None) == 0


@pytest.mark.parametrize("over,what", [(dict(host_cache_rows=1000), "host_cache_rows"), (dict(sparse=False), "sparse=False"),
                                       (dict(emb_dim=78), "emb_dim"), (dict(emb_dim=256), "emb_dim"),
                                       (dict(max_norm=0.0), "max_norm"), (dict(max_norm=float("inf")), "max_norm")])
def test_engine_refuses_max_norm_modes_it_cannot_run(over, what):
    from _oracle_engine import OracleWideDeepEngine
    from mindrec_amd.wide_deep import WideDeepConfig
    kw = dict(vocab_size=1000, emb_dim=16, field_size=4, batch_size=32, deep_layer_dim=[8], mlp_dtype="fp32", max_norm=0.5)
    kw.update(over)
    with pytest.raises(ValueError, match=r"max_norm") as e:
        OracleWideDeepEngine(WideDeepConfig(**kw), "cpu")
    assert what.split("=")[0] in str(e.value) or what == "max_norm"


def test_engine_refuses_max_norm_on_row_shards():
    from _oracle_engine import OracleWideDeepEngine
    from mindrec_amd.wide_deep import WideDeepConfig
    cfg = WideDeepConfig(vocab_size=1000, emb_dim=16, field_size=4, batch_size=32, deep_layer_dim=[8], mlp_dtype="fp32", max_norm=0.5)
    with pytest.raises(ValueError, match=r"max_norm.*row shards"):
        OracleWideDeepEngine(cfg, "cpu", rank=0, world=2)


def test_clip_oracle_matches_compat_clip_by_norm():
    """tests/_oracle_clip_ops.py's float64 clip against the compat layer's ClipByNorm (the eager path of nn.EmbeddingLookup)"""
    compat = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "compat"))
    if compat not in sys.path:
        sys.path.insert(0, compat)
    from mindspore.nn.layer.basic import ClipByNorm
    import _oracle_clip_ops as OC
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((200, 3, 16)) * rng.choice([0.01, 1.0, 0.0], size=(200, 3, 1))).astype(np.float32)
    got = ClipByNorm((2,))(torch.from_numpy(x), torch.tensor(0.5))
    got = got.numpy() if isinstance(got, torch.Tensor) else got.asnumpy()
    ref, _ = OC.clip_rows64(x, 0.5)
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-9)


def test_jacobian_restatement():
    """J(x) G of the oracle is the derivative of the clip: a finite-difference check in float64"""
    import _oracle_clip_ops as OC
    rng = np.random.default_rng(1)
    x = rng.standard_normal((5, 12))
    G = rng.standard_normal((5, 12))
    c = 0.5 * np.linalg.norm(x, axis=1).min()
    JG = OC.jacobian_apply64(x, G, c)
    eps = 1e-6
    for i in range(12):
        e = np.zeros(12); e[i] = eps
        fd = (OC.clip_rows64(x + e, c)[0] - OC.clip_rows64(x - e, c)[0]) / (2 * eps)        # column i of J
        assert np.allclose((fd * G).sum(axis=1), JG[:, i], rtol=1e-6, atol=1e-8)             # J symmetric: (J G)_i = sum_j J_ji G_j
    big = 10 * np.linalg.norm(x, axis=1).max()
    assert np.array_equal(OC.jacobian_apply64(x, G, big), G)
