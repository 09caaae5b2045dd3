"""mrec_mt_input (the multitable Wide&Deep's input stage) on a machine without a GPU: declared, exported and bound; every refusal comes
back with its code before any HIP call -- no call here gets as far as a launch: each holds a defect, or null pointers, or B == 0 --
and the host restatement the GPU tests compare with (tests/_multitable_ref.py) gives hand-computed answers on one tiny case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _multitable_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
MAX_SEGS, MAX_BAG = 16, 4096
P = 0x10000          # a non-null, 16-byte aligned address that nothing dereferences: every call below is refused before a launch


def test_symbol_declared_exported_and_bound():
    from mindrec_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrec.h")).read(), flags=re.S)
    assert "mrec_mt_input" in set(re.findall(r"\b(mrec_[a-z0-9_]+)\s*\(", text))
    assert "mrec_mt_input" in _lib.EXPORTED and len(_lib.lib().mrec_mt_input.argtypes) == 14
    assert f"MREC_MT_MAX_SEGS {MAX_SEGS}" in text and "} mrec_mt_seg_t;" in text
    assert ops.MT_MAX_SEGS == MAX_SEGS
    # ops.MtSeg is mrec_mt_seg_t member for member
    body = re.search(r"typedef struct \{([^}]*?)\} mrec_mt_seg_t;", text, flags=re.S).group(1)
    members = [(t.strip(), n) for t, n in re.findall(r"([A-Za-z0-9_ ]+?[ *]+)([a-z_A-Z0-9]+);", body)]
    ctype = {"const float*": C.c_void_p, "const int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in members] == list(ops.MtSeg._fields_)
    assert C.sizeof(ops.MtSeg) == 80


def _seg(D=64, L=3, pooled=0, col=8, V=100, ld=None, ld_ids=None, table=None, ids=None, wide=None, mask=None):
    return dict(table=table, V=V, ld=D if ld is None else ld, D=D, wide=wide, ids=ids, ld_ids=L if ld_ids is None else ld_ids,
                mask=mask, L=L, pooled=pooled, col=col)


def _call(segs=(), C_=8, B=5, K0=None, ldx=None, out_kind=2, x=None, wide_out=None, cont=None, wc=None, wb=None, ld_cont=None, n_segs=None,
          null_segs=False):
    from mindrec_amd import _lib, ops
    arr = (ops.MtSeg * max(len(segs), 1))(*[ops.MtSeg(**s) for s in segs])
    end = max([C_] + [s["col"] + s["D"] * (1 if s["pooled"] == 1 else max(s["L"], 1)) for s in segs])
    K0 = end if K0 is None else K0
    return _lib.lib().mrec_mt_input(cont, C_ if ld_cont is None else ld_cont, C_, wc, wb, None if null_segs else C.cast(arr, C.c_void_p),
                                    len(segs) if n_segs is None else n_segs, B, x, out_kind, K0 if ldx is None else ldx, K0, wide_out, None)


def _all(**kw):
    """every pointer non-null and aligned (never dereferenced: the callers add one defect each)"""
    return dict(x=P, wide_out=P, cont=P, wc=P, wb=P, **kw)


def _full(**kw):
    return _seg(table=P, ids=P, wide=P, mask=P, **kw)


def test_einval_before_any_hip_call():
    s = _seg()
    assert _call([s]) == EINVAL                                      # null pointers: the baseline every case below differs from by one thing
    assert _call([s], n_segs=-1) == EINVAL
    assert _call([s], n_segs=MAX_SEGS + 1) == EINVAL
    assert _call([s], null_segs=True) == EINVAL
    assert _call([_seg(L=0)]) == EINVAL
    assert _call([_seg(L=-2)]) == EINVAL
    assert _call([_seg(pooled=2)]) == EINVAL
    assert _call([_seg(pooled=-1)]) == EINVAL
    assert _call([s], B=-1) == EINVAL
    assert _call([s], out_kind=3) == EINVAL
    assert _call([_seg(ld=32)]) == EINVAL                            # ld < D
    assert _call([_seg(ld_ids=2)]) == EINVAL                         # ld_ids < L
    assert _call([s], K0=200, ldx=192) == EINVAL                     # K0 <= ldx
    # the layout: overlapping blocks, blocks outside [0, K0) -- with every pointer set, so that nothing else can be what is refused
    full = _full()
    assert _call([full, _full(col=8 + 64)], **_all()) == EINVAL      # the second starts inside the first (3 rows of 64)
    assert _call([_full(col=0)], **_all()) == EINVAL                 # on top of the continuous block
    assert _call([full], **_all(K0=192)) == EINVAL                   # ends at 200 > K0
    assert _call([_full(pooled=1, col=64), _full(pooled=1, col=120)], **_all()) == EINVAL
    # null pointers, one at a time
    for hole in ("x", "wide_out", "cont", "wc", "wb"):
        assert _call([full], **{**_all(), hole: None}) == EINVAL, hole
    assert _call([{**full, "table": None}], **_all()) == EINVAL
    assert _call([{**full, "ids": None}], **_all()) == EINVAL
    assert _call([{**full, "V": 0}], **_all()) == EINVAL             # no row to read
    assert _call([{**full, "V": -1}], **_all()) == EINVAL


def test_eunsupported_before_any_hip_call():
    full = _full()
    assert _call([_seg(col=8)], C_=4) == EUNSUPPORTED                # C % 8
    assert _call([_seg(D=12)]) == EUNSUPPORTED
    assert _call([_seg(D=4)]) == EUNSUPPORTED
    assert _call([_seg(D=264)]) == EUNSUPPORTED                      # D > 256
    assert _call([_seg(col=12)]) == EUNSUPPORTED
    assert _call([_seg()], K0=204) == EUNSUPPORTED
    assert _call([_seg()], ldx=204) == EUNSUPPORTED
    assert _call([_seg(ld=66)]) == EUNSUPPORTED                      # rows not 16-byte aligned
    assert _call([_seg()], ld_cont=10) == EUNSUPPORTED
    assert _call([_seg(D=8, L=MAX_BAG, pooled=1), _seg(D=8, L=1, pooled=1, col=16)]) == EUNSUPPORTED      # sum L over the limit
    assert _call([_seg(D=8, L=MAX_BAG - 1, pooled=1), _seg(D=8, L=1, pooled=1, col=16)]) == EINVAL        # the limit itself: null pointers
    assert _call([_seg(pooled=1), _seg(pooled=1, col=72)], B=1 << 30) == EUNSUPPORTED                       # B * n_segs >= 2^31
    assert _call([_seg(pooled=1)], B=(1 << 31) - 1) == EINVAL                                             # below it: null pointers
    # alignment: every pointer set, one of them 8 bytes off
    assert _call([full], **{**_all(), "x": P + 8}) == EUNSUPPORTED
    assert _call([full], **{**_all(), "cont": P + 8}) == EUNSUPPORTED
    assert _call([{**full, "table": P + 8}], **_all()) == EUNSUPPORTED
    # an argument error wins over a shape refusal, a shape refusal over the layout, all of them over B == 0 and the pointers
    assert _call([_seg(D=12, L=0)]) == EINVAL
    assert _call([_full(D=12, col=0)], **_all()) == EUNSUPPORTED
    assert _call([_seg(D=12)], B=0) == EUNSUPPORTED


def test_the_reference_widths_pass_and_b0_returns_ok():
    ref = [_seg(D=64, L=2, col=32), _seg(D=128, L=3, col=160), _seg(D=64, L=2, col=544)] + \
          [_seg(D=64, L=L, pooled=1, col=672 + 64 * f) for f, L in enumerate((3, 5, 4, 3, 4, 2))]
    assert _call(ref, C_=32) == EINVAL                               # K0 = 1056: nothing but the null pointers is refused
    assert _call(ref, C_=32, B=0) == 0                               # nothing to do, nothing touched, no launch
    assert _call([], C_=0, B=0, K0=0) == 0                           # C == 0 with cont NULL, no segments
    assert _call([_seg(col=0)], C_=0, B=0) == 0
    assert _call([_seg(D=8, L=1, col=8 * i + 8) for i in range(MAX_SEGS)], B=0) == 0
    assert _call([_seg(col=64)], B=0, ldx=512) == 0                  # a gap in front of the block, ldx > K0


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from mindrec_amd import ops
    from mindrec_amd.multitable import MultiTableConfig, MultiTableWideDeep
    t, ids = torch.zeros(4, 8), torch.zeros((2, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.multitable_input(torch.zeros(2, 8), torch.zeros(8), torch.zeros(1), [(t, ids, 8)])
    with pytest.raises(ValueError):
        ops.multitable_input(None, None, torch.zeros(1), [(t, ids, 8 * i) for i in range(MAX_SEGS + 1)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MultiTableWideDeep(MultiTableConfig(device="cpu"))
    cfg = MultiTableConfig()
    assert cfg.input_emb_dim == 32 + 2 * 64 + 3 * 128 + 2 * 64 + 6 * 64      # src/datasets.py:310-314
    assert (cfg.emb128_vocab, cfg.emb64_single_vocab, cfg.emb64_multi_vocab, cfg.indicator_vocab) == (650000, 17300, 20900, 16)
    assert cfg.deep_dims == (1024,) * 5 and cfg.mlp_dtype == "fp16" and cfg.n_continue == 32
    with pytest.raises(ValueError):
        MultiTableWideDeep(MultiTableConfig(multi_bags=(3, 5, 4), device="cpu"))
    with pytest.raises(ValueError):
        MultiTableWideDeep(MultiTableConfig(mlp_dtype="fp8", device="cpu"))


def test_host_restatement_against_hand_computed_answers():
    """2 samples; C = 8; one single-hot segment (D = 8, L = 1) and one pooled segment (D = 8, L = 3) with a masked slot (sample 0, slot 1)
    and an id out of range (sample 1, slot 2).  Every value is a small dyadic number, so the expected answers are exact by hand."""
    cont = np.array([[1, 2, 3, 4, 5, 6, 7, 8], [0.5, 0, 0, 0, 0, 0, 0, -1]], np.float32)
    wc = np.array([1, 0, 0, 0, 0, 0, 0, 0.5], np.float32)
    t1 = (np.arange(4)[:, None] * 10 + np.arange(8)[None, :]).astype(np.float32)           # row v = 10 v + (0 .. 7)
    w1 = np.array([0.25, 0.5, 1.0, 2.0], np.float32)
    t2 = (np.arange(5)[:, None] * 3 + np.zeros(8)[None, :]).astype(np.float32)             # row v = 3 v in every column
    w2 = np.array([1, 2, 4, 8, 16], np.float32)
    s1 = R.Seg(t1, np.array([[2], [0]], np.int32), 8, False, None, w1)
    s2 = R.Seg(t2, np.array([[1, 4, 2], [3, 0, 5]], np.int32), 24, True, np.array([[1, 0, 0.5], [2, 1, 1]], np.float32), w2)
    x = R.input_row(cont, [s1, s2], 32)
    exp = np.zeros((2, 32), np.float32)
    exp[:, :8] = cont
    exp[0, 8:16] = 20 + np.arange(8)
    exp[1, 8:16] = np.arange(8)
    exp[:, 16:24] = 0                                                                      # the gap
    exp[0, 24:32] = (3 * 1 + 12 * 0 + 6 * 0.5) / 3                                         # = 2
    exp[1, 24:32] = (9 * 2 + 0 * 1 + 0) / 3                                                # id 5 is out of range: a zero row; = 6
    assert x.dtype == np.float32 and np.array_equal(x, exp)
    wide, aw, n = R.wide_sum(cont, wc, np.array([0.125], np.float32), [s1, s2])
    # sample 0: 1 * 1 + 8 * 0.5 = 5; w1[2] = 1; 2 * 1 + 16 * 0 + 4 * 0.5 = 4; bias 0.125
    # sample 1: 0.5 * 1 - 1 * 0.5 = 0; w1[0] = 0.25; 8 * 2 + 1 * 1 + (out of range: 0) = 17
    assert np.array_equal(wide, [10.125, 17.375]) and np.array_equal(aw, [10.125, 18.375]) and n == 1 + 8 + 1 + 3
    # the mean divides by L = 3 whatever the mask holds, and rounds once: 1 / 3 in fp32, then in fp16 / bf16
    s3 = R.Seg(np.ones((1, 8), np.float32), np.array([[0, 0, 0]], np.int32), 0, True, np.array([[1, 0, 0]], np.float32), None)
    third = np.float32(1.0) / np.float32(3.0)
    assert np.array_equal(R.input_row(None, [s3], 8), np.full((1, 8), third, np.float32))
    assert np.array_equal(R.input_row(None, [s3], 8, "f16"), np.full((1, 8), np.float32(np.float16(third)), np.float32))
    assert R.input_row(None, [s3], 8, "bf16")[0, 0] == np.float32(0.333984375)                # 0x3EAB
    assert R.wide_sum(None, None, np.array([2.0], np.float32), [s3])[0][0] == 2.0             # no wide weights: the bias alone
    # round16's bf16 ties go to even, and NaN stays NaN
    tie = np.array([1.00390625, 1.01171875, np.nan], np.float32)                              # 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    r = R.round16(tie, "bf16")
    assert r[0] == 1.0 and r[1] == 1.015625 and np.isnan(r[2])
