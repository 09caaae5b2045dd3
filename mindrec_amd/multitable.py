"""MultiTableWideDeep: the evaluation forward of the reference's four-table Wide&Deep (models/wide_and_deep_multitable/src/
wide_and_deep.py:146-427 WideDeepModel, :617-650 PredictWithSigmoid; eval.py) on the hand-written kernels.

    net = MultiTableWideDeep(MultiTableConfig(n_indicator=2, n_emb128=3, n_emb64_single=2))
    net.load_parameters(named)                      # the reference's parameter names -> this model (optional: it is initialised by seed)
    logit, prob = net.predict_fused(batch)          # batch: a mapping by the reference's input names
    auc = net.evaluate(batches)                     # DeviceAUCMAPMetric over predict_fused; the metric's .map is MAP@12

The model: four fp32 tables (650 000 x 128, 17 300 x 64, 20 900 x 64, 16 x 64), a [V] wide weight vector per table, wide_continue_w
[32] and wide_bias [1]; the deep input row is Concat((continue_val, indicator rows, emb128 rows, emb64_single rows, six masked
mean-pooled multi-hot fields of emb64_multi)) (:351-352), input_emb_dim columns (src/datasets.py:310-314); five DenseLayers of 1024
with ReLU in fp16 and deep_predict (1024 -> 1); out = wide_out + deep_out (:426), prob = sigmoid(out).

predict_fused is three kinds of launch and nothing else:
  1. ops.multitable_input -- ONE launch writes the 16-bit [B, input_emb_dim] input row of dense_layer_1 and the wide term [B]; the ten
     id tensors and six masks of the batch stay separate, each a descriptor of that launch: no [B, F, D] lookup result, no concat, no cast;
  2. ops.dense_fwd x5 on the K-contiguous weight copies (mlp_dtype "fp32": ops.dense32_fwd x5, exact fp32);
  3. ops.head_predict -- deep_predict, the wide/deep add, the sigmoid and, with a label, the mean sigmoid cross-entropy.
No torch arithmetic runs on that path and nothing synchronises with the host.  (Off it, when the parameters are initialised or loaded,
the 16-bit copies of the hidden weights are made by a torch cast, as the engines make theirs, and transposed by ops.operand_copies.)  Eager only: a HIP-graph replay of the chain, the
backward and the optimizers of this model are not here.  Evaluation has no Dropout (and the reference's keep_prob is 1.0)."""
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from . import ops
from .metrics import DeviceAUCMAPMetric
from .wide_deep_mlp import UnsupportedNet

# the six multi-hot fields in the order of the reference's Concat (wide_and_deep.py:301-349): mult_emb_1 .. mult_emb_6
MULTI_KEYS = ("multi_doc_ad_category_id", "multi_doc_event_entity_id", "multi_doc_ad_entity_id", "multi_doc_event_topic_id",
              "multi_doc_event_category_id", "multi_doc_ad_topic_id")
_DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


@dataclass
class MultiTableConfig:
    """Table sizes and dims: the reference's (wide_and_deep.py:154-157,188-193).  The field counts and the bag lengths are the data
    set's (dataformat/input_shape_dict.pkl: the second dimension of indicator_id, emb_128_id, emb_64_single_id and of the six
    multi_doc_*_id tensors, in MULTI_KEYS order)."""
    emb128_vocab: int = 650000
    emb128_dim: int = 128
    emb64_single_vocab: int = 17300
    emb64_single_dim: int = 64
    emb64_multi_vocab: int = 20900
    emb64_multi_dim: int = 64
    indicator_vocab: int = 16
    indicator_dim: int = 64
    n_indicator: int = 2
    n_emb128: int = 3
    n_emb64_single: int = 2
    multi_bags: Tuple[int, ...] = (3, 5, 4, 3, 4, 2)
    n_continue: int = 32
    deep_dims: Tuple[int, ...] = (1024,) * 5
    mlp_dtype: str = "fp16"
    seed: int = 0
    emb_sigma: float = 0.01
    dense_sigma: float = 0.01
    device: str = "cuda:0"

    @property
    def input_emb_dim(self):
        """src/datasets.py:310-314"""
        return (self.n_continue + self.n_indicator * self.indicator_dim + self.n_emb128 * self.emb128_dim
                + self.n_emb64_single * self.emb64_single_dim + len(self.multi_bags) * self.emb64_multi_dim)


class MultiTableWideDeep:
    def __init__(self, cfg=None):
        cfg = cfg if cfg is not None else MultiTableConfig()
        if len(cfg.multi_bags) != len(MULTI_KEYS) or any(int(L) != L or L < 1 for L in cfg.multi_bags):
            raise ValueError(f"multi_bags must hold {len(MULTI_KEYS)} bag lengths >= 1 (MULTI_KEYS order), got {cfg.multi_bags!r}")
        if cfg.mlp_dtype not in _DTYPES:
            raise ValueError(f"mlp_dtype must be one of {tuple(_DTYPES)}, got {cfg.mlp_dtype!r}")
        if len(cfg.deep_dims) < 1 or min(cfg.n_indicator, cfg.n_emb128, cfg.n_emb64_single) < 1 or cfg.n_continue < 0:
            raise ValueError("deep_dims needs a layer, every field count must be >= 1 and n_continue >= 0")
        self.cfg, self.device = cfg, torch.device(cfg.device)
        if self.device.type != "cuda":
            raise RuntimeError("mindrec_amd ops run on the GPU only (no CPU fallback)")
        self._dt = _DTYPES[cfg.mlp_dtype]
        self.dims = [cfg.input_emb_dim] + [int(d) for d in cfg.deep_dims] + [1]
        dev, f32 = self.device, torch.float32
        seed = iter(range(int(cfg.seed), int(cfg.seed) + 64))

        def normal(shape, sigma):
            t = torch.empty(shape, dtype=f32, device=dev)
            ops.fill_normal_(t.view(-1, shape[-1]) if len(shape) == 2 else t.view(-1, 1), seed=next(seed), sigma=float(sigma))
            return t

        # parameters, by the reference's names (wide_and_deep.py:188-253); initialised on the device by seed
        self.params = {}
        for name, V, D in (("emb128_embedding", cfg.emb128_vocab, cfg.emb128_dim), ("emb64_single", cfg.emb64_single_vocab, cfg.emb64_single_dim),
                           ("emb64_multi", cfg.emb64_multi_vocab, cfg.emb64_multi_dim), ("emb64_indicator", cfg.indicator_vocab, cfg.indicator_dim)):
            self.params[name] = normal((V, D), cfg.emb_sigma)
        for name, n in (("wide_continue_w", cfg.n_continue), ("wide_emb128_w", cfg.emb128_vocab), ("wide_emb64_single_w", cfg.emb64_single_vocab),
                        ("wide_emb64_multi_w", cfg.emb64_multi_vocab), ("wide_indicator_w", cfg.indicator_vocab), ("wide_bias", 1)):
            self.params[name] = normal((max(n, 1),), cfg.emb_sigma)[:n]
        nl = len(self.dims) - 1
        for i in range(nl):
            name = f"dense_layer_{i + 1}" if i < nl - 1 else "deep_predict"
            self.params[name + ".weight"] = normal((self.dims[i], self.dims[i + 1]), cfg.dense_sigma)
            self.params[name + ".bias"] = normal((self.dims[i + 1],), cfg.dense_sigma)
        self._w16 = self._wt16 = None
        if self._dt != f32:          # the hidden layers' GEMM operands: 16-bit copies [in, out] and their K-contiguous transposes [out, in]
            self._w16 = [torch.empty((self.dims[i], self.dims[i + 1]), dtype=self._dt, device=dev) for i in range(nl - 1)]
            self._wt16 = [torch.empty((self.dims[i + 1], self.dims[i]), dtype=self._dt, device=dev) for i in range(nl - 1)]
        # 16-bit nets: the MFMA DenseLayer's widths (multiples of 8); the fp32 net's dense32_fwd takes any width
        hidden = self._dt == f32 or all(ops.dense_supported(1, self.dims[i], self.dims[i + 1]) for i in range(nl - 1))
        self._net_ok = bool(hidden and ops.head_predict_supported(self.dims[nl - 1]))
        self._refresh()

    def _refresh(self):
        """the 16-bit copies of the hidden weights and their transposes, from the fp32 parameters"""
        if self._w16 is None or not self._net_ok:
            return
        for i, w16 in enumerate(self._w16):
            w16.copy_(self.params[f"dense_layer_{i + 1}.weight"])
        tr = list(zip(self._w16, self._wt16))
        for k in range(0, len(tr), 4):                      # (at most 4 transposes per launch)
            ops.operand_copies(tr[k:k + 4])

    def load_parameters(self, named):
        """named: a mapping by the reference's parameter names -- emb128_embedding, emb64_single, emb64_multi, emb64_indicator,
        wide_continue_w, wide_emb128_w, wide_emb64_single_w, wide_emb64_multi_w, wide_indicator_w, wide_bias, dense_layer_{1..n}.weight
        / .bias, deep_predict.weight / .bias -- to arrays or tensors of this model's shapes (self.params holds them); any subset.
        ValueError on an unknown name or a shape mismatch, before anything is written.  The 16-bit copies are refreshed."""
        srcs = {}
        for name, val in named.items():
            dst = self.params.get(name)
            if dst is None:
                raise ValueError(f"load_parameters: unknown parameter {name!r} (known: {sorted(self.params)})")
            src = val if isinstance(val, torch.Tensor) else torch.from_numpy(np.array(val))      # (a copy: the caller's array may be read-only)
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"load_parameters: {name} has shape {tuple(src.shape)}, the model's is {tuple(dst.shape)}")
            srcs[name] = src
        for name, src in srcs.items():
            self.params[name].copy_(src.to(torch.float32))
        self._refresh()

    def _segments(self, batch):
        """the ten id tensors of a batch as the input launch's segments, columns in the order of the reference's Concat"""
        p, cfg = self.params, self.cfg
        segs, col = [], cfg.n_continue
        single = (("indicator_id", "emb64_indicator", "wide_indicator_w", cfg.n_indicator),
                  ("emb_128_id", "emb128_embedding", "wide_emb128_w", cfg.n_emb128),
                  ("emb_64_single_id", "emb64_single", "wide_emb64_single_w", cfg.n_emb64_single))
        for key, table, wide, n in single:
            ids = self._ids(batch, key, n)
            segs.append(ops.MtSegment(p[table], ids, col, False, None, p[wide]))
            col += n * p[table].shape[1]
        for key, L in zip(MULTI_KEYS, cfg.multi_bags):
            ids = self._ids(batch, key, L)
            mask = batch[key + "_mask"]
            if not isinstance(mask, torch.Tensor) or mask.dtype != torch.float32 or tuple(mask.shape) != tuple(ids.shape):
                raise TypeError(f"{key}_mask must be a float32 tensor of the shape of {key}, {tuple(ids.shape)}")
            segs.append(ops.MtSegment(p["emb64_multi"], ids, col, True, mask, p["wide_emb64_multi_w"]))
            col += p["emb64_multi"].shape[1]
        return segs

    @staticmethod
    def _ids(batch, key, n):
        ids = batch[key]
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 2 or ids.shape[1] != n:
            raise TypeError(f"{key} must be an int32 [B, {n}] tensor")
        return ids

    def input_row(self, batch, out=None, wide_out=None):
        """(x [B, input_emb_dim] in the net's type, wide [B] float32): ops.multitable_input over the batch, one launch"""
        cfg = self.cfg
        cont = batch["continue_val"] if cfg.n_continue else None
        if cont is not None and (not isinstance(cont, torch.Tensor) or cont.dtype != torch.float32 or cont.dim() != 2
                                 or cont.shape[1] != cfg.n_continue):
            raise TypeError(f"continue_val must be a float32 [B, {cfg.n_continue}] tensor")
        return ops.multitable_input(cont, self.params["wide_continue_w"] if cont is not None else None, self.params["wide_bias"],
                                    self._segments(batch), K0=cfg.input_emb_dim, out=out, wide_out=wide_out, out_dtype=self._dt)

    @torch.no_grad()
    def predict_fused(self, batch, label=None):
        """batch: a mapping by the reference's input names (PredictWithSigmoid.construct, wide_and_deep.py:627-635) to device
        tensors: continue_val float32 [B, 32]; indicator_id, emb_128_id, emb_64_single_id and the six multi_doc_*_id int32 [B, n];
        the six multi_doc_*_id_mask float32 of their ids' shapes.  Other keys (label, display_id, ad_id, ..) are ignored.
        Returns (logit [B, 1], prob [B, 1]) and, with `label` (float32 [B] or [B, 1]), the batch's mean sigmoid cross-entropy (0-d) as a
        third value -- the meaning of WideDeepEngine.predict_fused."""
        if not self._net_ok:
            raise UnsupportedNet(f"MREC_EUNSUPPORTED: evaluation forward: no hand-written HIP path for the {self.cfg.mlp_dtype} dense net "
                                 f"{self.dims} (16-bit nets: every width a multiple of 8; the layer in front of the output: a multiple of 8 up to 2048)")
        p = self.params
        h, wide = self.input_row(batch)
        nl = len(self.dims) - 1
        for i in range(nl - 1):
            b = p[f"dense_layer_{i + 1}.bias"]
            if self._w16 is not None:
                h = ops.dense_fwd(h, self._w16[i], b, relu=True, wt=self._wt16[i])
            else:
                h = ops.dense32_fwd(h, p[f"dense_layer_{i + 1}.weight"], b, relu=True)
        out = ops.head_predict(h, p["deep_predict.weight"].view(-1), p["deep_predict.bias"], wide=wide,
                               label=label.view(-1) if label is not None else None)
        B = h.shape[0]
        return (out[0].view(B, 1), out[1].view(B, 1)) + ((out[2].view(()),) if label is not None else ())

    def evaluate(self, batches, metric=None):
        """eval.py's loop: predict_fused over `batches` (mappings as above that also hold label and display_id) into a
        DeviceAUCMAPMetric -- update(logit, prob, label, display_id), PredictWithSigmoid's four outputs -- and its eval(): the AUC; the
        metric's .map holds MAP@12.  Nothing synchronises with the host before eval()."""
        metric = metric if metric is not None else DeviceAUCMAPMetric(device=str(self.device))
        for batch in batches:
            logit, prob = self.predict_fused(batch)
            metric.update(logit, prob, batch["label"], batch["display_id"])
        return metric.eval()
