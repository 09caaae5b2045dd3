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
the 16-bit copies of the hidden weights are made by a torch cast, as the engines make theirs, and transposed by ops.operand_copies.)
Evaluation has no Dropout (and the reference's keep_prob is 1.0).

train_step(batch, label) is TrainStepWrap.construct (wide_and_deep.py:510-612) on one GPU: FTRL over every parameter whose name holds
"wide" (lr ftrl_lr, l1 = l2 = 5e-4, initial accum 0.1), Adam over the rest (lr adam_lr, eps 1e-6), both with loss_scale sens = 1000;
the loss is the mean sigmoid cross-entropy, no L2 term.  The tables are dense Parameters under P.Gather, so both optimizers are DENSE:
Adam moves untouched rows on their momentum, FTRL recomputes every weight from linear and accum.  Its launches, in order:
  1. ops.multitable_input                          the input row and the wide term (one launch)
  2. the dense net's forward, head and backward    DenseNetMixin's chain (wide_deep_mlp.py: ops.dense_fwd, the output head with
                                                   dscale = sens / B, ops.dense_bwd; the fp32 net: ops.dense32_* / ops.x3_*): the loss, the
                                                   16-bit (fp32 net: fp32) gradient g_x of the input row, g_wide [B]
  3. ops.sparse_plan x4                            one per table; the multi-hot table's ids are the six id tensors torch.cat'ed
  4. ops.multitable_input_bwd                      g_x, g_wide -> the four tables' row-gradient sums, the wide vectors' gradient sums,
                                                   d wide_continue_w, d wide_bias, times 1 / sens (two launches; its sum order: include/mrec.h)
  5. ops.dense_adam_rows_l2_ x4                    Adam over each whole table from its groups' sums (l2_scaled = 0)
  6. per wide vector: ops.scatter_unique_rows_ into a [V] gradient kept zero between steps, ops.dense_ftrl_, the touched entries
     cleared again; ops.dense_ftrl_ on wide_continue_w and wide_bias
  7. the dense net's Adam (ops.dense_adam_slabs_, which also writes the 16-bit weights; the fp32 net: ops.dense_adam_)
  8. ops.operand_copies: the K-contiguous weight copies predict_fused reads
That list is cfg.graphs == "none" (the default).  With cfg.graphs == "step" the step is one linear chain with constant arguments -- no
side stream, no parallel branch -- that replays as ONE captured HIP graph from the third step at a batch shape (the first two run it
eagerly; a new shape captures again; release_graphs() / close() / `with` drop the graph):
  ops.StepState.advance (the Adam powers live in device memory), 1 - 4 as above, then
  5 + 6. ops.multitable_optim_ -- Adam over the four tables, FTRL over the four wide vectors, wide_continue_w and wide_bias: one memset
     of a shared row -> group map, one kernel that fills it, ONE update kernel (three graph nodes where the list above has some 26 launches),
  7, 8 with the step size read from the step state.
Both forms give the same bits.  One GPU, no Dropout; predict_fused is not captured.  Ids must lie in [0, V) when training with
graphs="none" -- the contract of the scatter; it is not checked on the device (ops.multitable_optim_ gives a row outside [0, V) no entry)."""
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from . import ops
from .metrics import DeviceAUCMAPMetric
from .wide_deep_mlp import DenseNetMixin, UnsupportedNet

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
    # training (TrainStepWrap, wide_and_deep.py:510-535; src/config.py:31-32)
    adam_lr: float = 0.003
    adam_eps: float = 1e-6
    ftrl_lr: float = 0.1
    ftrl_l1: float = 5e-4
    ftrl_l2: float = 5e-4
    ftrl_initial_accum: float = 0.1
    sens: float = 1000.0
    # "none": train_step issues its launches one by one; "step": from the third step at a batch shape the whole step -- optimizers
    # included -- replays as ONE captured HIP graph (the reference trains with dataset_sink_mode=True, train_and_eval.py:101)
    graphs: str = "none"

    @property
    def input_emb_dim(self):
        """src/datasets.py:310-314"""
        return (self.n_continue + self.n_indicator * self.indicator_dim + self.n_emb128 * self.emb128_dim
                + self.n_emb64_single * self.emb64_single_dim + len(self.multi_bags) * self.emb64_multi_dim)


class _TrainNet(DenseNetMixin):
    """The dense net's training state and step of MultiTableWideDeep: DenseNetMixin as the DeepFM engines host it -- fp32 master weights,
    gradients and Adam moments in flat buffers, the 16-bit operand shadow and its transposes, no graphs of its own (the model captures
    the whole step: MultiTableWideDeep._train_step_graph), no Dropout, every
    hidden layer a launch of its own (no fused tail: the transposes then cover every layer and are the copies predict_fused reads)."""
    k = ops

    def __init__(self, cfg, dims, dtype, device, seed):
        self.cfg, self.device, self._gpu, self._amp = cfg, device, True, (None if dtype == torch.float32 else dtype)
        self._mfma = self._amp is not None
        self._graph_level, self.rank, self.step_count, self._step_state = 0, 0, 0, None
        self._dropout = self._training = self._emb_dropped = False
        self._init_dense_net(dims, seed, 0.01, cfg.sens, fused_tail=False)


# the four tables with their wide vectors and the keys of their id tensors, in the order of the input launch's segments
_TABLES = (("emb64_indicator", "wide_indicator_w"), ("emb128_embedding", "wide_emb128_w"), ("emb64_single", "wide_emb64_single_w"),
           ("emb64_multi", "wide_emb64_multi_w"))
_WIDE = tuple(w for _, w in _TABLES) + ("wide_continue_w", "wide_bias")


class MultiTableWideDeep:
    def __init__(self, cfg=None):
        cfg = cfg if cfg is not None else MultiTableConfig()
        if len(cfg.multi_bags) != len(MULTI_KEYS) or any(int(L) != L or L < 1 for L in cfg.multi_bags):
            raise ValueError(f"multi_bags must hold {len(MULTI_KEYS)} bag lengths >= 1 (MULTI_KEYS order), got {cfg.multi_bags!r}")
        if cfg.mlp_dtype not in _DTYPES:
            raise ValueError(f"mlp_dtype must be one of {tuple(_DTYPES)}, got {cfg.mlp_dtype!r}")
        if len(cfg.deep_dims) < 1 or min(cfg.n_indicator, cfg.n_emb128, cfg.n_emb64_single) < 1 or cfg.n_continue < 0:
            raise ValueError("deep_dims needs a layer, every field count must be >= 1 and n_continue >= 0")
        if cfg.graphs not in ("none", "step"):
            raise ValueError(f"graphs must be 'none' or 'step', got {cfg.graphs!r}")
        self._graph, self._graph_key, self._graph_eager = None, None, 0      # the captured step, its batch shape, eager steps at that shape
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
        self._net = self._opt = None      # training state: made by the first train_step
        self._refresh()

    def _refresh(self):
        """the 16-bit copies of the hidden weights and their transposes, from the fp32 parameters"""
        if self._net is not None:          # they are the training net's shadow and its transposes
            if self._net._mfma:
                self._net.dense16_flat.copy_(self._net.dense_flat.detach())
                self._net._refresh_tail()
            return
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

    # ---- training ---------------------------------------------------------------------------------------------------------------
    def _train_refusal(self):
        """None where train_step runs, else what DenseNetMixin has no hand-written step for"""
        d, nl = self.dims, len(self.dims) - 1
        K5 = d[nl - 1]
        if nl < 2:
            return "a net without a hidden layer"
        if self.cfg.n_continue == 0:       # wide_bias's gradient comes out of the backward launch's continuous block (C > 0)
            return "a model without continuous values (n_continue = 0): the backward launch gives wide_bias its gradient with them"
        if self._dt == torch.float32:
            ok = ops.head_supported(K5) or ops.dcn_head_supported(K5, 2) or ops.head_any_supported(K5)
        else:
            ok = (DenseNetMixin.mfma_net_ok(d) and all(ops.dense_supported(1, d[i], d[i + 1]) for i in range(nl - 1))
                  and (ops.head_supported(K5) or ops.head_any_supported(K5)))
        return None if ok and self._net_ok else f"the {self.cfg.mlp_dtype} dense net {d}"

    def _train_state(self):
        """The training state, made on first use: the dense net as a DenseNetMixin host (_TrainNet) holding the CURRENT dense parameters
        -- self.params' dense entries become views of its flat buffer, the 16-bit copies predict_fused reads its shadow and transposes --
        Adam m, v per table, FTRL accum (ftrl_initial_accum), linear (0) and a zero [V] gradient buffer per wide vector."""
        if self._net is not None:
            return self._net
        why = self._train_refusal()
        if why is not None:
            raise UnsupportedNet(f"MREC_EUNSUPPORTED: training step: no hand-written HIP path for {why}")
        cfg, p, nl = self.cfg, self.params, len(self.dims) - 1
        names = [f"dense_layer_{i + 1}" for i in range(nl - 1)] + ["deep_predict"]
        with torch.enable_grad():          # (the mixin ties each parameter view to its gradient view)
            net = _TrainNet(cfg, self.dims, self._dt, self.device, int(cfg.seed) + 64)
        net.load_dense_parameters([p[n + ".weight"] for n in names], [p[n + ".bias"] for n in names])
        for i, n in enumerate(names):
            p[n + ".weight"], p[n + ".bias"] = net.dense[2 * i].detach(), net.dense[2 * i + 1].detach()
        if net._mfma:
            self._w16 = [net.dense16[2 * i] for i in range(nl - 1)]
            self._wt16 = [net._dense16_t[i] for i in range(nl - 1)]
        opt = {"adam": {t: (torch.zeros_like(p[t]), torch.zeros_like(p[t])) for t, _ in _TABLES}, "ftrl": {}, "gbuf": {}, "zeros": {},
               "b1": np.float32(0.9), "b2": np.float32(0.999), "b1p": np.float32(1.0), "b2p": np.float32(1.0)}
        for w in _WIDE:
            opt["ftrl"][w] = (torch.full_like(p[w], float(cfg.ftrl_initial_accum)), torch.zeros_like(p[w]))
        for _, w in _TABLES:
            opt["gbuf"][w] = torch.zeros_like(p[w])
        self._net, self._opt = net, opt
        return net

    def _groups(self, batch, segs):
        """the four tables' MtGroups over a batch: a plan per table; the multi-hot table's ids are its six id tensors side by side"""
        cfg = self.cfg
        ids = [batch["indicator_id"], batch["emb_128_id"], batch["emb_64_single_id"], torch.cat([batch[k] for k in MULTI_KEYS], dim=1)]
        parts = [segs[0:1], segs[1:2], segs[2:3], segs[3:3 + len(cfg.multi_bags)]]
        return [ops.MtGroup(tuple(sg), ops.sparse_plan(i), True) for sg, i in zip(parts, ids)]

    @torch.no_grad()
    def _backward(self, batch, label):
        """Steps 1 - 4 of train_step: the gradient of the batch's mean sigmoid cross-entropy with respect to every parameter, nothing
        updated.  Returns {"loss": 0-d, "g_x": [B, input_emb_dim] and "g_wide": [B] TIMES sens (what the net's backward leaves),
        "groups": [(table name, wide name, plan, sums [n, D], wsums [n])] -- row u < plan.U is the gradient of table row plan.uniq[u] --
        "d_wide_cont": [C] or None, "d_wide_bias": [1] or None}, all but g_x / g_wide unscaled (1 / sens applied); the dense net's
        gradients stay, times sens, in the net's slabs / flat buffer (dense_gradients() reads them)."""
        net, cfg = self._train_state(), self.cfg
        if not isinstance(label, torch.Tensor) or label.dtype != torch.float32:
            raise TypeError("label must be a float32 [B] or [B, 1] tensor")
        segs = self._segments(batch)
        x, wide = self.input_row(batch)
        if net._mfma:
            loss, g_x, g_wide = net._mlp_step_eager(x, wide, label)
        else:
            loss, g_x, g_wide = net._mlp_step_f32(x, wide, label)
        groups = self._groups(batch, segs)
        outs, (d_cont, d_bias) = ops.multitable_input_bwd(g_x, g_wide, groups, cont=batch["continue_val"],
                                                          grad_scale=1.0 / cfg.sens)
        return {"loss": loss, "g_x": g_x, "g_wide": g_wide, "d_wide_cont": d_cont, "d_wide_bias": d_bias,
                "groups": [(t, w, q.plan, s, ws) for (t, w), q, (s, ws) in zip(_TABLES, groups, outs)]}

    @torch.no_grad()
    def dense_gradients(self):
        """{parameter name: gradient} of the dense net after _backward, unscaled (a copy; the 16-bit net's slabs are summed first)"""
        net, nl = self._train_state(), len(self.dims) - 1
        if net._mfma:
            net._sum_dw_slabs()
        names = [f"dense_layer_{i + 1}" for i in range(nl - 1)] + ["deep_predict"]
        out = {}
        for i, n in enumerate(names):
            out[n + ".weight"] = net.dense_grad[2 * i] / self.cfg.sens
            out[n + ".bias"] = net.dense_grad[2 * i + 1] / self.cfg.sens
        return out

    @torch.no_grad()
    def train_step(self, batch, label):
        """One step of TrainStepWrap (module docstring: the launch list) on `batch` (predict_fused's mapping) and `label` (float32 [B] or
        [B, 1]).  The dense net runs on DenseNetMixin (its forward, head, backward and dense Adam, as the DeepFM engines use it) -- not on
        a copy of that chain.  Returns the step's loss (before the update) as a 0-d device tensor; nothing synchronises with the host.
        Ids must lie in [0, V): not checked.  UnsupportedNet, before any state exists or changes, where the net has no hand-written step
        -- and for n_continue = 0, which is refused and not trained without its wide_bias (the reference always trains it).
        predict_fused after it sees the new parameters.
        With cfg.graphs == "step" the step is the fused chain (module docstring) and, from the third step at a batch shape, ONE replayed
        HIP graph: THE RETURNED LOSS IS THEN A STATIC BUFFER WHICH THE NEXT CALL OVERWRITES -- clone what must outlive it."""
        if self.cfg.graphs == "step":
            return self._train_step_graph(batch, label)
        net = self._train_state()
        cfg, p, o = self.cfg, self.params, self._opt
        g = self._backward(batch, label)
        o["b1p"], o["b2p"] = np.float32(o["b1p"] * o["b1"]), np.float32(o["b2p"] * o["b2"])
        net.step_count += 1
        adam = dict(lr=cfg.adam_lr, beta1=float(o["b1"]), beta2=float(o["b2"]), eps=cfg.adam_eps, beta1_power=float(o["b1p"]),
                    beta2_power=float(o["b2p"]))
        ftrl = dict(lr=cfg.ftrl_lr, l1=cfg.ftrl_l1, l2=cfg.ftrl_l2, lr_power=-0.5, grad_scale=1.0)
        for table, w, plan, sums, wsums in g["groups"]:
            m, v = o["adam"][table]
            ops.dense_adam_rows_l2_(p[table], m, v, plan, sums, 0.0, grad_scale=1.0, **adam)
            gb, zeros = o["gbuf"][w], o["zeros"].get(plan.n)
            if zeros is None:
                zeros = o["zeros"][plan.n] = torch.zeros((max(plan.n, 1), 1), dtype=torch.float32, device=self.device)
            ops.scatter_unique_rows_(gb.view(-1, 1), plan, wsums.view(-1, 1))
            ops.dense_ftrl_(p[w], *o["ftrl"][w], gb, **ftrl)
            ops.scatter_unique_rows_(gb.view(-1, 1), plan, zeros)
        ops.dense_ftrl_(p["wide_continue_w"], *o["ftrl"]["wide_continue_w"], g["d_wide_cont"], **ftrl)
        ops.dense_ftrl_(p["wide_bias"], *o["ftrl"]["wide_bias"], g["d_wide_bias"], **ftrl)
        if net._mfma:
            ops.dense_adam_slabs_(net.dense_flat.detach(), net.dense_m, net.dense_v, net.dense_grad_flat, net._slab_segments(),
                                  shadow16=net.dense16_flat, grad_scale=1.0 / cfg.sens, **adam)
            net._refresh_tail()
        else:
            ops.dense_adam_(net.dense_flat.detach(), net.dense_m, net.dense_v, net.dense_grad_flat, grad_scale=1.0 / cfg.sens, **adam)
        return g["loss"]

    # ---- the step as one linear chain with constant arguments, and its captured form (cfg.graphs == "step") ----------------------------
    def _step_chain(self, batch, label):
        """One training step, launch by launch, every argument constant from step to step (capturable): the step state's advance, steps
        1 - 4 of the module docstring's list, ops.multitable_optim_ for steps 5 and 6, the dense net's Adam and the weight copies -- the
        Adam step size comes from the device-side step state.  No side stream, no parallel branch."""
        net, cfg, p, o = self._net, self.cfg, self.params, self._opt
        st = o["state"]
        st.advance(cfg.adam_lr, float(o["b1"]), float(o["b2"]))
        g = self._backward(batch, label)
        adam = dict(lr=cfg.adam_lr, beta1=float(o["b1"]), beta2=float(o["b2"]), eps=cfg.adam_eps, beta1_power=0.0, beta2_power=0.0)
        ftrl = dict(lr=cfg.ftrl_lr, l1=cfg.ftrl_l1, l2=cfg.ftrl_l2, lr_power=-0.5, grad_scale=1.0)
        tabs = [ops.MtOptTable(p[t], *o["adam"][t], plan, sums, p[w], *o["ftrl"][w], wsums) for t, w, plan, sums, wsums in g["groups"]]
        vecs = [ops.MtOptVector(p["wide_continue_w"], *o["ftrl"]["wide_continue_w"], g["d_wide_cont"]),
                ops.MtOptVector(p["wide_bias"], *o["ftrl"]["wide_bias"], g["d_wide_bias"])]
        ops.multitable_optim_(tabs, vecs, adam=dict(adam, grad_scale=1.0, l2_scaled=0.0), ftrl=ftrl, step_state=st)
        if net._mfma:
            ops.dense_adam_slabs_(net.dense_flat.detach(), net.dense_m, net.dense_v, net.dense_grad_flat, net._slab_segments(),
                                  shadow16=net.dense16_flat, grad_scale=1.0 / cfg.sens, step_state=st, **adam)
            net._refresh_tail()
        else:
            ops.dense_adam_(net.dense_flat.detach(), net.dense_m, net.dense_v, net.dense_grad_flat, grad_scale=1.0 / cfg.sens,
                            step_state=st, **adam)
        return g["loss"]

    def _batch_tensors(self, batch, label):
        """the 17 tensors a step reads -- continue_val, the ten id tensors, the six masks, the label -- by name, in a fixed order"""
        names = ("continue_val", "indicator_id", "emb_128_id", "emb_64_single_id") + MULTI_KEYS + tuple(k + "_mask" for k in MULTI_KEYS)
        ts = [batch[k] for k in names] + [label]
        for k, t in zip(names + ("label",), ts):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{k} must be a device tensor")
        return names, ts

    @torch.no_grad()
    def _train_step_graph(self, batch, label):
        """train_step with cfg.graphs == "step": the first two steps at a batch shape run _step_chain eagerly (workspaces and the net's
        buffers come into being), the third captures it over static copies of the batch's tensors, later ones copy (ops.copy_many_: one
        launch) and replay.  A batch of another shape drops the graph and starts over.  The host's powers are advanced beside the
        device's, so a StepState.reset after steps that ran elsewhere stays consistent (DeepCrossEngine._train_step_native)."""
        net, o = self._train_state(), self._opt
        names, ts = self._batch_tensors(batch, label)
        key = tuple((tuple(t.shape), t.dtype) for t in ts)
        if key != self._graph_key:          # a batch of a new shape: checked as the chain checks it, before any state moves
            self._segments(batch)
            if label.dtype != torch.float32 or ts[0].dtype != torch.float32 or ts[0].dim() != 2 or ts[0].shape[1] != self.cfg.n_continue:
                raise TypeError(f"label must be float32 [B] or [B, 1] and continue_val float32 [B, {self.cfg.n_continue}]")
            self.release_graphs()
            self._graph_key, self._graph_eager = key, 0
        if o.get("state") is None:
            o["state"], o["state_step"] = ops.StepState(self.device), -1
        if o["state_step"] != net.step_count:
            o["state"].reset(float(o["b1p"]), float(o["b2p"]), net.step_count)
        net.step_count += 1
        o["b1p"], o["b2p"] = np.float32(o["b1p"] * o["b1"]), np.float32(o["b2p"] * o["b2"])
        o["state_step"] = net.step_count
        g = self._graph
        if g is None:
            if self._graph_eager < 2:
                self._graph_eager += 1
                return self._step_chain(batch, label)
            static = [t.clone() for t in ts]
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                loss = self._step_chain(dict(zip(names, static[:-1])), static[-1])
            g = self._graph = {"graph": graph, "static": static, "loss": loss}
        ops.copy_many_(g["static"], ts)
        g["graph"].replay()
        return g["loss"]

    def release_graphs(self):
        """Drops the captured training step (it is re-captured on demand, at once where two steps at the batch shape have run)."""
        if self._graph is not None:
            torch.cuda.synchronize(self.device)
            self._graph = None
            torch.cuda.synchronize(self.device)

    def close(self):
        """Drops the captured step (nothing of it outlives the model; symmetrical with the engines' close).  train_step works after it."""
        self.release_graphs()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def train(self, batches):
        """train.py's loop: train_step over `batches` (mappings as predict_fused's that also hold label); returns the steps' losses (0-d
        device tensors: reading one synchronises)"""
        return [self.train_step(batch, batch["label"]) for batch in batches]
