"""Serving a trained Wide&Deep model from row-wise 8-bit records (csrc/mrec_q8.hip): the evaluation forward of
WideDeepEngine.predict_fused with the dequantizing lookup in front, holding neither the fp32 table nor any optimizer slot of it.
Made by WideDeepEngine.q8_predictor().  DeepFMQ8Predictor: the same for DeepFMEngine.predict_fused, with the FM lookup over records
(ops.fm_lookup_q8 / ops.fm_lookup_q4) in front.  MultiHotQ8: the multi-hot lookups of multi_hot.py (MultiHotEmbedding, MultiHotWideDeep)
over records, one pooled launch (ops.gather_pool_fields_q8 / ops.gather_pool_fields_q4).  DeepFMKeyedQ8Predictor: DeepFMHashEngine's
model -- hash tables keyed by raw ids -- served from records behind a frozen key index (ops.FrozenKeyIndex).  Every class takes 8-bit or 4-bit records: the
table's `bits` picks the lookup.  The Wide&Deep and DeepFM predictors take dense_fp8= / calib=: the hidden layers in front of the fused tail on the
8-bit-float matrix kernel (ops.dense_fwd_fp8, csrc/mrec_gemm_fp8.hip), off by default."""
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
        self._fp8 = {}                              # hidden layer -> (codes [out, in] e4m3, scale [out], sa): freeze_fp8

    def fp8_layers(self, dense_fp8):
        """The hidden layers `dense_fp8` names: True = every layer in front of the fused tail (all of them where the net has none),
        or a tuple of layer indices among those."""
        n = len(self.dims) - 1
        ok = range(n - 3 if self._tail_eval else n - 1)
        if dense_fp8 is True:
            return tuple(ok)
        layers = tuple(sorted(set(int(i) for i in dense_fp8)))
        if not layers or any(i not in ok for i in layers):
            raise ValueError(f"dense_fp8 names hidden layers {layers}; this net runs layers {tuple(ok)} as GEMM launches of their own")
        return layers

    @torch.no_grad()
    def freeze_fp8(self, x, layers, headroom):
        """Moves the hidden layers `layers` to ops.dense_fwd_fp8 (cold path).  x [B, dims[0]]: the calibration batch's looked-up rows;
        it runs through the 16-bit layers once and the amax of every chosen layer's input gives that layer's static activation scale
        sa = amax * headroom / 448 (values past amax * headroom saturate).  The chosen layers' weights are kept as e4m3 codes with
        per-channel scales; their 16-bit transposes and the flat 16-bit shadow are dropped."""
        h, sa = x, {}
        for i in range(max(layers) + 1):
            if i in layers:
                amax = float(h.float().abs().max())
                sa[i] = (amax if amax > 0.0 else 1.0) * float(headroom) / 448.0
            if i < max(layers):
                h = ops.dense_fwd(h, self.dense16[2 * i], self.dense[2 * i + 1].detach(), relu=True, wt=self._dense16_t.get(i))
        for i in layers:
            codes, scale = ops.quantize_rows_fp8(self.dense16[2 * i].t().contiguous())
            self._fp8[i] = (codes, scale, sa[i])
            self._dense16_t.pop(i, None)
        self.dense16 = [None if (j % 2 == 0 and j // 2 in self._fp8) else t.clone() for j, t in enumerate(self.dense16)]
        self.dense16_flat = None

    @torch.no_grad()
    def mlp_predict(self, emb, wide, label=None):
        """DenseNetMixin.mlp_predict with the frozen layers on ops.dense_fwd_fp8; the tail launch and the head as there.  Without fp8
        layers it IS that method (wide_deep_mlp.py is untouched: the engines' evaluation forward runs the code it ran before)."""
        if not self._fp8:
            return super().mlp_predict(emb, wide, label)
        if emb.dtype != self._amp:
            raise TypeError(f"mlp_predict: the looked-up rows arrive in the net's dtype, got {emb.dtype}")
        n = len(self.dims) - 1
        prod = isinstance(wide, _WideProd)
        W5, b5 = self.dense[2 * (n - 1)].detach().view(-1), self.dense[2 * (n - 1) + 1].detach()
        tail = self._tail_eval and ops.tail_predict_supported(emb.shape[0], *self.dims[n - 3:n])
        h = self._predict_hidden(emb, n - 3 if tail else n - 1)
        lab = label.view(-1) if label is not None else None
        if tail:
            return ops.tail_predict(h, self._tail_packed, self.dense[2 * (n - 3) + 1].detach(), self.dense[2 * (n - 2) + 1].detach(), W5, b5,
                                    wide.prod if prod else wide.view(-1), wide_bias=self.wide_b if prod else None, label=lab)
        return ops.head_predict(h, W5, b5, wide=None if prod else wide.view(-1), wide_prod=wide.prod if prod else None,
                                wide_bias=self.wide_b if prod else None, label=lab)

    def _predict_hidden(self, h, count):
        for i in range(count):
            bias = self.dense[2 * i + 1].detach()
            if i in self._fp8:
                codes, scale, sa = self._fp8[i]
                nxt = self._fp8.get(i + 1) if i + 1 < count else None          # an fp8 successor reads codes, anything else 16 bits
                h = ops.dense_fwd_fp8(h, codes, scale, bias, sa, relu=True, out_scale=nxt[2] if nxt else None, out_dtype=self._amp)
            else:
                h = ops.dense_fwd(h, self.dense16[2 * i], bias, relu=True, wt=self._dense16_t.get(i))
        return h


def _freeze_dense_fp8(pred, dense_fp8, calib, fp8_headroom, mlp_dtype, mfma):
    """dense_fp8 / calib of the predictors' constructors: refusals, the calibration lookup, _ServeNet.freeze_fp8"""
    if dense_fp8 is False or dense_fp8 is None:
        return
    if mlp_dtype is None or not mfma:
        raise ValueError("dense_fp8 needs a 16-bit net on the matrix kernels (mlp_dtype float16 / bfloat16, every width a multiple of 8)")
    if calib is None or len(calib) != 2:
        raise ValueError("dense_fp8 needs calib=(ids_or_keys, wts): a batch whose activations set the static fp8 scales")
    if not fp8_headroom >= 1.0:
        raise ValueError(f"fp8_headroom must be >= 1, got {fp8_headroom!r}")
    layers = pred.net.fp8_layers(dense_fp8)
    with torch.cuda.device(pred.device):
        rows = pred._calib_rows(*calib)
        pred.net.freeze_fp8(rows, layers, fp8_headroom)


class WideDeepQ8Predictor:
    """A Q8Table (the deep rows as 8-bit or 4-bit codes, the wide weight in each record's header) + a copy of the dense parameters and
    the wide bias.  predict_fused is WideDeepEngine.predict_fused's contract over the dequantized table; the launches are issued eagerly.
    The table's `bits` picks the lookup (ops.gather_rows_q8 / ops.gather_rows_q4); everything behind it is the same."""

    def __init__(self, q8, dims, weights, biases, wide_b, mlp_dtype=None, mfma=None, fused_tail=True, fused_tail_eval=True,
                 dense_fp8=False, calib=None, fp8_headroom=2.0):
        """q8: ops.Q8Table on the GPU; dims: [F * D, hidden .., 1]; weights[i] [in_i, out_i], biases[i] [out_i] and wide_b as
        load_dense_parameters takes them; mlp_dtype: torch.float16 / torch.bfloat16, None for an fp32 net.  dense_fp8: True, or a tuple
        of hidden-layer indices -- those layers in front of the fused tail run on ops.dense_fwd_fp8 (e4m3 weights with per-channel
        scales, static per-tensor activation scales from the batch calib=(ids, wts): sa = amax * fp8_headroom / 448); False: the
        16-bit path, launch for launch."""
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
        _freeze_dense_fp8(self, dense_fp8, calib, fp8_headroom, mlp_dtype, mfma)

    def _calib_rows(self, ids, wts):
        lookup = ops.gather_rows_q4 if self.q8.bits == 4 else ops.gather_rows_q8
        return lookup(self.q8, ids, wts, out_dtype=self._row_dtype)[0].view(ids.shape[0], -1)

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

    def __init__(self, q8, dims, weights, biases, mlp_dtype=None, mfma=None, fused_tail_eval=True, dense_fp8=False, calib=None,
                 fp8_headroom=2.0):
        """q8: ops.Q8Table on the GPU; dims: [F * D, hidden .., 1]; weights[i] [in_i, out_i] and biases[i] [out_i] as
        load_dense_parameters takes them; mlp_dtype: torch.float16 / torch.bfloat16, None for an fp32 net.  dense_fp8, calib,
        fp8_headroom: as WideDeepQ8Predictor takes them (calib = (ids or keys, wts))."""
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
        self._fp8_args = (dense_fp8, calib, fp8_headroom, mlp_dtype, mfma)
        if type(self)._lookup is DeepFMQ8Predictor._lookup:          # (the keyed predictor calibrates once its key index stands)
            _freeze_dense_fp8(self, *self._fp8_args)

    def _calib_rows(self, ids, wts):
        return self._lookup(ids, wts)[0].view(ids.shape[0], -1)

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

    def __init__(self, q8, kidx, dims, weights, biases, mlp_dtype=None, mfma=None, fused_tail_eval=True, dense_fp8=False, calib=None,
                 fp8_headroom=2.0):
        super().__init__(q8, dims, weights, biases, mlp_dtype=mlp_dtype, mfma=mfma, fused_tail_eval=fused_tail_eval,
                         dense_fp8=dense_fp8, calib=calib, fp8_headroom=fp8_headroom)
        if not isinstance(kidx, ops.FrozenKeyIndex) or kidx.device != self.device:
            raise TypeError("kidx must be an ops.FrozenKeyIndex on the records' device")
        self.kidx = kidx
        _freeze_dense_fp8(self, *self._fp8_args)

    def _lookup(self, keys, wts):
        lookup = ops.fm_lookup_q4_keyed if self.q8.bits == 4 else ops.fm_lookup_q8_keyed
        return lookup(self.q8, self.kidx, keys, wts, out_dtype=self._row_dtype)
