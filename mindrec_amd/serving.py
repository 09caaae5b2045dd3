"""Serving a trained Wide&Deep model from row-wise 8-bit records (csrc/mrec_q8.hip): the evaluation forward of
WideDeepEngine.predict_fused with the dequantizing lookup in front, holding neither the fp32 table nor any optimizer slot of it.
Made by WideDeepEngine.q8_predictor().  DeepFMQ8Predictor: the same for DeepFMEngine.predict_fused, with the FM lookup over records
(ops.fm_lookup_q8 / ops.fm_lookup_q4) in front.  MultiHotQ8: the multi-hot lookups of multi_hot.py (MultiHotEmbedding, MultiHotWideDeep)
over records, one pooled launch (ops.gather_pool_fields_q8 / ops.gather_pool_fields_q4).  DeepFMKeyedQ8Predictor: DeepFMHashEngine's
model -- hash tables keyed by raw ids -- served from records behind a frozen key index (ops.FrozenKeyIndex).  Every class takes 8-bit or 4-bit records: the
table's `bits` picks the lookup."""
import torch

from . import ops
from .wide_deep_mlp import DenseNetMixin, _WideProd


class _ServeNet(DenseNetMixin):
    """The dense net of a predictor: DenseNetMixin as multitable._TrainNet hosts it -- its own fp32 parameters, the 16-bit operand shadow,
    the transposes and the tail launch's fragment order --, evaluation only (no Dropout, no step, no graphs of its own)."""
    k = ops

    def __init__(self, dims, amp, mfma, device, fused_tail, fused_tail_eval):
        self.cfg, self.device, self._gpu, self._amp, self._mfma = None, device, True, amp, mfma
        self._graph_level, self.rank, self.step_count, self._step_state = 0, 0, 0, None
        self._dropout = self._training = self._emb_dropped = False
        self._init_dense_net(dims, 0, 0.01, 1.0, fused_tail=fused_tail, fused_tail_eval=fused_tail_eval)
        self.wide_b = self.extra_p                  # what mlp_predict adds to the summed wide products
        self.dense_m = self.dense_v = None          # a predictor has no optimizer


class WideDeepQ8Predictor:
    """A Q8Table (the deep rows as 8-bit or 4-bit codes, the wide weight in each record's header) + a copy of the dense parameters and
    the wide bias.  predict_fused is WideDeepEngine.predict_fused's contract over the dequantized table; the launches are issued eagerly.
    The table's `bits` picks the lookup (ops.gather_rows_q8 / ops.gather_rows_q4); everything behind it is the same."""

    def __init__(self, q8, dims, weights, biases, wide_b, mlp_dtype=None, mfma=None, fused_tail=True, fused_tail_eval=True):
        """q8: ops.Q8Table on the GPU; dims: [F * D, hidden .., 1]; weights[i] [in_i, out_i], biases[i] [out_i] and wide_b as
        load_dense_parameters takes them; mlp_dtype: torch.float16 / torch.bfloat16, None for an fp32 net."""
        self.q8 = q8
        self.device = q8.records.device
        if self.device.type != "cuda":
            raise RuntimeError("WideDeepQ8Predictor runs on an MI355X (no CPU fallback)")
        if q8.bits not in (4, 8):
            raise TypeError(f"WideDeepQ8Predictor reads 8-bit or 4-bit records, got bits={q8.bits}")
        if dims[0] % q8.D:
            raise ValueError(f"the net's input width {dims[0]} is no multiple of the table's emb_dim {q8.D}")
        mfma = (mlp_dtype is not None and DenseNetMixin.mfma_net_ok(dims)) if mfma is None else bool(mfma)
        with torch.cuda.device(self.device):
            self.net = _ServeNet(list(dims), mlp_dtype, mfma, self.device, fused_tail, fused_tail_eval)
            self.net.load_dense_parameters(weights, biases, extra=wide_b)
        self._row_dtype = mlp_dtype if mfma else torch.float32

    def _chain(self, ids, wts, label):
        B, F = ids.shape
        lookup = ops.gather_rows_q4 if self.q8.bits == 4 else ops.gather_rows_q8
        rows, wprod = lookup(self.q8, ids, wts, out_dtype=self._row_dtype)
        return self.net.mlp_predict(rows.view(B, F * self.q8.D), _WideProd(wprod), label)

    def predict_fused(self, ids, wts, label=None):
        """ids, wts [B, F] -> (logit [B, 1], prob [B, 1]) and, with `label`, the batch's mean sigmoid cross-entropy (0-d) as a third value:
        the dequantizing lookup, then the hidden-layer, tail and head launches of the engine's evaluation forward."""
        if ids.dim() != 2 or ids.shape[1] * self.q8.D != self.net.dims[0]:
            raise ValueError(f"ids must be [B, {self.net.dims[0] // self.q8.D}], got {tuple(ids.shape)}")
        with torch.cuda.device(self.device):
            return self.net._predict_run(self._chain, ids, wts, label, capture=False)


class MultiHotQ8:
    """Multi-hot fields served from a Q8Table: MultiHotEmbedding.lookup -- and, with wide=True, MultiHotWideDeep.lookup, whose wide
    weights sit in the record headers -- as ONE pooled launch over records (ops.gather_pool_fields_q8, or ops.gather_pool_fields_q4
    for a table of 4-bit records).  It holds the records only: no fp32 table, no optimizer state, no apply_.  Made by MultiHotEmbedding.freeze_q8() / MultiHotWideDeep.freeze_q8()."""

    def __init__(self, q8, bag, mode="mean", out_dtype=torch.float32, wide=False):
        """q8: ops.Q8Table on the GPU; bag: an int (one field) or a tuple of bag lengths, as MultiHotEmbedding takes it."""
        if mode not in ("sum", "mean"):
            raise ValueError(f"mode must be 'sum' or 'mean', got {mode!r}")
        if q8.records.device.type != "cuda":
            raise RuntimeError("MultiHotQ8 runs on an MI355X (no CPU fallback)")
        if q8.bits not in (4, 8):
            raise TypeError(f"MultiHotQ8 reads 8-bit or 4-bit records, got bits={q8.bits}")
        self.q8, self.device = q8, q8.records.device
        self.fields = ops._fields(bag if isinstance(bag, (tuple, list)) else (bag,))
        self.bag, self.dim, self.vocab = sum(self.fields), q8.D, q8.V
        self.mode, self.out_dtype, self.wide = mode, out_dtype, bool(wide)

    def lookup(self, ids, mask=None, out=None, wide_out=None):
        """ids, mask [B, Ls] -> x [B, F * dim], or (x, w [B] float32) with wide=True; one field also takes ids [B, G, L] -> [B, G * dim]
        (G bags of its length per sample; not with wide=True).  mask, out, wide_out: as MultiHotEmbedding.lookup and
        MultiHotWideDeep.lookup take them."""
        if ids.dim() not in ((2, 3) if len(self.fields) == 1 and not self.wide else (2,)) or ids.shape[-1] != self.bag:
            raise TypeError(f"ids must be [B, {self.bag}] (the bags of lengths {self.fields} back to back), or [B, G, {self.bag}] for one "
                            "length without the wide side")
        if mask is not None and (mask.dtype != torch.float32 or tuple(mask.shape) != tuple(ids.shape)):
            raise TypeError("mask must be float32 of the shape of ids")
        B, G = ids.shape[0], (ids.shape[1] if ids.dim() == 3 else 1)
        W = len(self.fields) * self.dim
        if out is None:
            out = torch.empty((B, G * W), dtype=self.out_dtype, device=self.device)
        elif tuple(out.shape) != (B, G * W) or (G > 1 and not out.is_contiguous()):
            raise TypeError("out must be [B, F * dim] (contiguous when ids hold more than one bag per sample)")
        with torch.cuda.device(self.device):
            pool = ops.gather_pool_fields_q4 if self.q8.bits == 4 else ops.gather_pool_fields_q8
            res = pool(self.q8, ids.reshape(B * G, self.bag), self.fields, mask.reshape(B * G, self.bag) if mask is not None else None,
                       mode=self.mode, out=out if G == 1 else out.view(B * G, W), wide=self.wide, wide_out=wide_out)
        return (out, res[1]) if self.wide else out


class DeepFMQ8Predictor:
    """DeepFM served from a Q8Table (the [V, D] rows as 8-bit or 4-bit codes, the [V, 1] first-order weight in each record's header) + a
    copy of the dense parameters.  predict_fused is DeepFMEngine.predict_fused's contract over the dequantized tables; the launches are
    issued eagerly.  The table's `bits` picks the lookup (ops.fm_lookup_q8 / ops.fm_lookup_q4).  Made by DeepFMEngine.q8_predictor()."""

    def __init__(self, q8, dims, weights, biases, mlp_dtype=None, mfma=None, fused_tail_eval=True):
        """q8: ops.Q8Table on the GPU; dims: [F * D, hidden .., 1]; weights[i] [in_i, out_i] and biases[i] [out_i] as
        load_dense_parameters takes them; mlp_dtype: torch.float16 / torch.bfloat16, None for an fp32 net."""
        self.q8 = q8
        self.device = q8.records.device
        if self.device.type != "cuda":
            raise RuntimeError("DeepFMQ8Predictor runs on an MI355X (no CPU fallback)")
        if q8.bits not in (4, 8):
            raise TypeError(f"DeepFMQ8Predictor reads 8-bit or 4-bit records, got bits={q8.bits}")
        if dims[0] % q8.D:
            raise ValueError(f"the net's input width {dims[0]} is no multiple of the table's emb_dim {q8.D}")
        mfma = (mlp_dtype is not None and DenseNetMixin.mfma_net_ok(dims)) if mfma is None else bool(mfma)
        with torch.cuda.device(self.device):
            self.net = _ServeNet(list(dims), mlp_dtype, mfma, self.device, True, fused_tail_eval)
            self.net.load_dense_parameters(weights, biases)
        self._row_dtype = mlp_dtype if mfma else torch.float32

    def _lookup(self, ids, wts):
        """(rows [B, F, D] in the net's input type, lin_fm [B]) of one batch: the one thing the keyed predictor does differently"""
        lookup = ops.fm_lookup_q4 if self.q8.bits == 4 else ops.fm_lookup_q8
        return lookup(self.q8, ids, wts, out_dtype=self._row_dtype)

    def _chain(self, ids, wts, label):
        B, F = ids.shape
        rows, lin_fm = self._lookup(ids, wts)
        return self.net.mlp_predict(rows.view(B, F * self.q8.D), lin_fm, label)

    def predict_fused(self, ids, wts, label=None):
        """ids, wts [B, F] -> (logit [B, 1], prob [B, 1]) and, with `label`, the batch's mean sigmoid cross-entropy (0-d) as a third value:
        one lookup launch for the rows, the linear and the FM term, then the hidden-layer, tail and head launches of the engine's
        evaluation forward."""
        if ids.dim() != 2 or ids.shape[1] * self.q8.D != self.net.dims[0]:
            raise ValueError(f"ids must be [B, {self.net.dims[0] // self.q8.D}], got {tuple(ids.shape)}")
        with torch.cuda.device(self.device):
            return self.net._predict_run(self._chain, ids, wts, label, capture=False)


class DeepFMKeyedQ8Predictor(DeepFMQ8Predictor):
    """DeepFM over MapParameter hash tables, frozen for serving: DeepFMQ8Predictor with raw keys in the place of ids.  It holds the
    records (record i: the [D] row and the first-order weight of the i-th frozen key), an ops.FrozenKeyIndex over those keys and a copy
    of the dense parameters -- no fp32 table, no optimizer slot, no live index.  predict_fused(keys, wts, label=None) resolves the keys
    and dequantizes their records in ONE launch (ops.fm_lookup_q8_keyed / ops.fm_lookup_q4_keyed); a key the model was not frozen with
    reads as a zero row and a zero weight and is NOT inserted -- where DeepFMHashEngine.predict_fused would give it a default row.
    Made by DeepFMHashEngine.q8_predictor()."""

    def __init__(self, q8, kidx, dims, weights, biases, mlp_dtype=None, mfma=None, fused_tail_eval=True):
        super().__init__(q8, dims, weights, biases, mlp_dtype=mlp_dtype, mfma=mfma, fused_tail_eval=fused_tail_eval)
        if not isinstance(kidx, ops.FrozenKeyIndex) or kidx.device != self.device:
            raise TypeError("kidx must be an ops.FrozenKeyIndex on the records' device")
        self.kidx = kidx

    def _lookup(self, keys, wts):
        lookup = ops.fm_lookup_q4_keyed if self.q8.bits == 4 else ops.fm_lookup_q8_keyed
        return lookup(self.q8, self.kidx, keys, wts, out_dtype=self._row_dtype)
