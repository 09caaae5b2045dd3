"""TEST INFRASTRUCTURE ONLY: the multitable Wide&Deep's input stage (mindrec_amd/csrc/mrec_multitable.hip, mrec_mt_input) and the model
behind it (models/wide_and_deep_multitable/src/wide_and_deep.py:271-427 WideDeepModel.construct, :617-650 PredictWithSigmoid)
restated on the host in numpy.

  input_row: the deep columns in np.float32 with the kernel's exact operation order, so every column can be required to match bit
    for bit (the library is built with -ffp-contract=off): columns 0 .. C-1 the continuous values; a single-hot segment's L rows side
    by side, each the row (a +0.0 row for an id outside [0, V)) times its mask value (no product where mask is None); a pooled
    segment slot by slot in ascending order -- slot 0's product starts the sum, every later one is added -- then ONE division by
    np.float32(L); columns nobody covers +0; 16-bit outputs rounded ONCE (round16: to nearest even).
  wide_sum: float64 -- sum_c cont * wide_cont + sum over segments with wide weights, over slots, of wide[id] * mask (mask None: 1; an id
    out of range: 0) + bias -- with sum |term| and the number of terms per sample, for the first-order bound of an fp32 sum.
  model_forward: WideDeepModel.construct + sigmoid in float64 over given parameters, the DenseLayers' operands, biases and outputs
    rounded to the net's 16-bit type as the reference's casts do (wide_and_deep.py:129-137)."""
from typing import NamedTuple, Optional

import numpy as np


class Seg(NamedTuple):
    table: np.ndarray                    # [V, D] float32
    ids: np.ndarray                      # [B, L] int32
    col: int
    pooled: bool = False
    mask: Optional[np.ndarray] = None    # [B, L] float32
    wide: Optional[np.ndarray] = None    # [V] float32

    @property
    def width(self):
        return self.table.shape[1] * (1 if self.pooled else self.ids.shape[1])


def round16(x, dtype):
    """float32 values rounded to nearest even into 'f16' / 'bf16' (or left alone: 'f32'), returned as float32"""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f32":
        return x
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    assert dtype == "bf16"
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    r = np.where(np.isnan(x), np.uint32(0x7FC00000) | (x.view(np.uint32) & np.uint32(0x80000000)), r).astype(np.uint32)
    return r.view(np.float32)


def _rows(seg, s):
    t = np.asarray(seg.table, np.float32)
    r = np.asarray(seg.ids)[:, s].astype(np.int64)
    ok = (r >= 0) & (r < t.shape[0])
    x = np.where(ok[:, None], t[np.where(ok, r, 0)], np.float32(0.0)).astype(np.float32)
    return x if seg.mask is None else (x * np.asarray(seg.mask, np.float32)[:, s:s + 1]).astype(np.float32)


def input_row(cont, segs, K0, out_dtype="f32", B=None):
    """-> [B, K0] float32 holding the values of out_dtype"""
    B = cont.shape[0] if cont is not None else (segs[0].ids.shape[0] if B is None else B)
    x = np.zeros((B, K0), np.float32)
    if cont is not None:
        x[:, :cont.shape[1]] = np.asarray(cont, np.float32)
    for seg in segs:
        D, L = seg.table.shape[1], seg.ids.shape[1]
        if seg.pooled:
            acc = None
            for s in range(L):
                p = _rows(seg, s)
                acc = p if s == 0 else (acc + p).astype(np.float32)
            x[:, seg.col:seg.col + D] = (acc / np.float32(L)).astype(np.float32)
        else:
            for s in range(L):
                x[:, seg.col + s * D:seg.col + (s + 1) * D] = _rows(seg, s)
    return round16(x, out_dtype)


def wide_sum(cont, wide_cont, wide_bias, segs, B=None):
    """-> (sum [B] float64, sum of |term| [B] float64, number of terms n)"""
    B = cont.shape[0] if cont is not None else (segs[0].ids.shape[0] if B is None else B)
    terms = [np.full((B, 1), np.float64(np.asarray(wide_bias).reshape(-1)[0]))]
    if cont is not None:
        terms.append(np.asarray(cont, np.float64) * np.asarray(wide_cont, np.float64)[None, :])
    for seg in segs:
        if seg.wide is None:
            continue
        w = np.asarray(seg.wide, np.float64)
        r = np.asarray(seg.ids).astype(np.int64)
        ok = (r >= 0) & (r < w.shape[0])
        t = np.where(ok, w[np.where(ok, r, 0)], 0.0)
        if seg.mask is not None:
            t = np.where(ok, t * np.asarray(seg.mask, np.float64), 0.0)
        terms.append(t)
    t = np.concatenate(terms, axis=1)
    return t.sum(axis=1), np.abs(t).sum(axis=1), t.shape[1]


# the six multi-hot fields in the order of the reference's Concat (wide_and_deep.py:301-349)
MULTI_KEYS = ("multi_doc_ad_category_id", "multi_doc_event_entity_id", "multi_doc_ad_entity_id", "multi_doc_event_topic_id",
              "multi_doc_event_category_id", "multi_doc_ad_topic_id")


def ref_param_sigma(name, shape):
    """sigma of parameter `name` in tests/golden/ref_multitable_fwd.npz (made by tests/golden/make_ref_multitable_fwd.py): large enough
    that activations stay O(1) through the five layers and the logits spread over the sigmoid, so that a wrong column or field order
    moves the probabilities far beyond the replay tolerance"""
    if name.endswith(".weight"):
        return float(np.sqrt(2.0 / shape[0]))
    if name.endswith(".bias") or name == "wide_bias" or name == "wide_continue_w":
        return 0.1
    return 0.3 if name.startswith("wide_") else 0.5


def ref_params(shapes):
    """{name: value} for {name: shape}: tests/_ref_fixtures.cfgsize_param (the oracle's counter-based normal stream keyed by the name)
    at ref_param_sigma -- what the generator put into the reference's model, derived again instead of stored (the tables alone are 340 MB)"""
    import _ref_fixtures as RF
    return {k: RF.cfgsize_param(k, tuple(s), ref_param_sigma(k, tuple(s))) for k, s in shapes.items()}


_fixture = {}


def load_fixture():
    """tests/golden/ref_multitable_fwd.npz, once: (batch by the reference's input names, the reference's logits [256], its probabilities
    [256], the parameters derived again by name) -- shared by the tests that replay it, read-only"""
    if not _fixture:
        import json
        import os
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_multitable_fwd.npz"))
        comp = json.loads(str(z["composition"]))
        batch = {k[3:]: z[k] for k in z.files if k.startswith("in/")}
        params = ref_params(comp["shapes"])
        for a in list(batch.values()) + list(params.values()):
            a.setflags(write=False)
        _fixture.update(batch=batch, logits=z["logits"], probs=z["probs"], params=params, comp=comp)
    return _fixture["batch"], _fixture["logits"], _fixture["probs"], _fixture["params"]


def model_segments(params, batch):
    """the ten id tensors of a batch (numpy, by the reference's input names) over the parameters (numpy, by the reference's names),
    columns in the order of the reference's Concat (:351-352); returns (segs, K0)"""
    col = batch["continue_val"].shape[1]
    segs = []
    for key, table, wide in (("indicator_id", "emb64_indicator", "wide_indicator_w"), ("emb_128_id", "emb128_embedding", "wide_emb128_w"),
                             ("emb_64_single_id", "emb64_single", "wide_emb64_single_w")):
        segs.append(Seg(params[table], batch[key], col, False, None, params[wide]))
        col += segs[-1].width
    for key in MULTI_KEYS:
        segs.append(Seg(params["emb64_multi"], batch[key], col, True, batch[key + "_mask"], params["wide_emb64_multi_w"]))
        col += segs[-1].width
    return segs, col


def model_forward(params, batch, mlp_dtype="f16"):
    """float64 (logit [B], prob [B]) of WideDeepModel.construct + sigmoid; mlp_dtype 'f16' / 'bf16': the DenseLayers cast their input,
    weight and bias to that type and their output back (convert_dtype=True), 'f32': no casts"""
    def q(a):
        return round16(np.asarray(a, np.float32), mlp_dtype).astype(np.float64)
    segs, K0 = model_segments(params, batch)
    h = input_row(batch["continue_val"], segs, K0, "f32").astype(np.float64)
    n = 1
    while f"dense_layer_{n}.weight" in params:
        n += 1
    names = [f"dense_layer_{i}" for i in range(1, n)] + ["deep_predict"]
    for i, name in enumerate(names):
        y = q(h) @ q(params[name + ".weight"]) + q(params[name + ".bias"])[None, :]
        if i < len(names) - 1:
            y = np.maximum(y, 0.0)
        h = q(y)
    wide, _, _ = wide_sum(batch["continue_val"], params["wide_continue_w"], params["wide_bias"], segs)
    logit = wide + h[:, 0]
    return logit, 1.0 / (1.0 + np.exp(-logit))
