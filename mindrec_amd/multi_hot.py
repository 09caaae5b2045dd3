"""MultiHotEmbedding: one embedding table looked up by BAGS of ids -- the multi-hot fields of the reference's multitable Wide&Deep
(models/wide_and_deep_multitable/src/wide_and_deep.py:301-346: Gather -> Mul(mask) -> ReduceMean(axis 1), six fields over the
20 900 x 64 table `emb64_multi`; :377-418, the wide side: Gather -> Mul(mask) -> ReduceSum over [V, 1] weights) -- with its sparse
gradient applied in place.

    emb = MultiHotEmbedding(vocab=20900, dim=64, bag=8, mode="mean", optimizer="lazy_adam")
    x = emb.lookup(ids, mask)          # ids [B, L] -> [B, dim];  ids [B, F, L] (F fields of the one table) -> [B, F * dim]
    ...                                # the model's forward and backward produce dy, the gradient of x
    emb.apply_(dy)                     # one plan of the looked-up ids, one pooled apply

Forward: one pooled lookup (ops.gather_pool_fields: no [B * L, dim] intermediate).  Backward: position (b, l) of a bag contributes
(dy[b] * mask[b, l]) * gs to row ids[b, l], gs = grad_scale for mode "sum" and fp32(grad_scale / L) for "mean" (ReduceMean's bprop
divides by the bag's length); ops.sparse_plan over the ids and the pooled sparse apply (the gradient rows are read as dy[i // L], the
L-fold expanded gradient is never written).  An integer `bag` is the one-field case of the fields form below, fields=(L,), over
the ids seen as [B * F, L].  Optimizers:
  "lazy_adam"  nn.LazyAdam on the touched rows (ops.sparse_lazy_adam_);
  "ftrl"       nn.FTRL on the touched rows (ops.sparse_ftrl_): the wide weights, dim = 1, mode "sum";
  "adam"       dense nn.Adam over the whole table, the reference's choice for this model (wide_and_deep.py:532-535): ops.segment_sum
               (fields=) + ops.dense_adam_rows_l2_ with l2_scaled = 0, which gives every row outside the plan a zero gradient -- so an
               untouched row's m and v decay and the row keeps moving on its momentum, exactly as under the dense optimizer.  32-bit
               ids only (that entry numbers rows in 32 bits).

Fields of UNEQUAL bag lengths (every multi-hot field of the reference has its own: src/datasets.py:290-313, input_shape_dict): a tuple
or list for `bag` selects the fields form,

    emb = MultiHotEmbedding(vocab=20900, dim=64, bag=(3, 5, 4, 3, 4, 2), mode="mean", optimizer="adam")
    x = emb.lookup(ids, mask)          # ids, mask [B, Ls], Ls = sum(bag), field f in slots off_f .. off_f + L_f - 1 -> [B, F * dim]
    emb.apply_(dy)                     # ONE plan over all B * Ls ids, ONE apply

Forward: ops.gather_pool_fields, one launch, the mean of field f divided by L_f.  Backward: position (b, s), s a slot of field f,
contributes (dy[b, f * dim : (f + 1) * dim] * mask[b, s]) * gs_f with gs_f = fp32(grad_scale / L_f) for "mean" and grad_scale for "sum"
(ops.* with fields=bag, field_scale=gs).  One plan, so an id that occurs in several fields receives the SUM of their gradients and
ONE optimizer update per step, as the reference's optimizer does with the table's summed gradient -- a lookup and an apply_ per
distinct length would update such a row once per call, which under LazyAdam, FTRL or dense Adam is a different result.  All three
optimizers.  `emb.fields` holds the bag lengths in both forms -- (L,) for an integer `bag` -- and `emb.bag` their sum; a sample's ids may
hold at most ops.MAX_BAG = 4096 slots (a longer `bag` is refused by lookup with ValueError).
The wide side of the reference's multi-hot fields (wide_and_deep.py:377-420: ReduceSum of every field's masked [V, 1] weights, the
fields' sums added up) needs no fields form: a sum over fields of sums over slots is ONE bag of length Ls, mode "sum", dim = 1 --
MultiHotEmbedding(vocab, 1, bag=sum(lengths), mode="sum", optimizer="ftrl") on the same [B, Ls] ids.

Both sides of the same fields at once -- the [V, dim] table AND the [V] wide weights, by the same ids and mask, both applies from ONE
plan: MultiHotWideDeep, at the end of this file.

Fields that hold RAW KEYS -- entity, topic, category ids of a growing catalogue, the input of the reference's hash-table models
(HashEmbeddingLookup over a MapParameter, mindspore_rec/ops/embedding.py:136-205) -- over a hash table instead of a [vocab, dim]
array: MultiHotHashEmbedding, at the end of this file.

max_norm=c on any of the three classes is the ClipByNorm of HashEmbeddingLookup(max_norm=c) / nn.EmbeddingLookup(max_norm=c)
(mindspore_rec/ops/embedding.py:156-161,202-205) over bags: every looked-up row is clipped to norm c before its mask product -- still
one pooled launch (ops.gather_pool_fields(max_norm=c)), train=False included -- and apply_ takes the gradient through the clip's Jacobian
in the same pooled apply (ops.sparse_lazy_adam_(pool_max_norm=c)).  "lazy_adam" only, dim % 4 == 0, dim <= 256: anything else is
refused at construction.

Neither method synchronises with the host, so lookup + apply_ capture into one HIP graph on one stream.  The Adam bias-correction
powers advance on the host with every apply_: a captured graph holds the powers of the steps it captured (replaying K captured
steps repeats those K steps; it does not continue the count).  No torch arithmetic on the step."""
import numpy as np
import torch

from . import ops
from .experimental import MapParameter

_OPTIMIZERS = ("lazy_adam", "ftrl", "adam")


def _clip_arg(max_norm, optimizer, dim):
    """max_norm of a multi-hot class: None, or a finite float > 0 under 'lazy_adam' with float4 rows of one column block"""
    if max_norm is None:
        return None
    c = ops._max_norm(max_norm)
    if optimizer != "lazy_adam":
        raise ValueError(f"max_norm: the pooled apply clips under optimizer 'lazy_adam' only, got {optimizer!r}")
    if dim % 4 != 0 or dim > 256:
        raise ValueError(f"max_norm: dim must be a multiple of 4 and at most 256, got {dim}")
    return c


class MultiHotEmbedding:
    def __init__(self, vocab, dim, bag, mode="mean", optimizer="lazy_adam", device="cuda:0", seed=0, sigma=0.01, lr=None, beta1=0.9,
                 beta2=0.999, eps=1e-8, use_nesterov=False, l1=1e-8, l2=1e-8, lr_power=-0.5, initial_accum=1.0,
                 out_dtype=torch.float32, max_norm=None):
        if mode not in ("sum", "mean"):
            raise ValueError(f"mode must be 'sum' or 'mean', got {mode!r}")
        if optimizer not in _OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {_OPTIMIZERS}, got {optimizer!r}")
        if isinstance(bag, (tuple, list)):
            bag = ops._fields(bag)
        elif int(bag) < 1:
            raise ValueError("vocab, dim and bag must be >= 1")
        else:
            bag = (int(bag),)
        if int(vocab) < 1 or int(dim) < 1:
            raise ValueError("vocab, dim and bag must be >= 1")
        self.fields = bag                   # the bag lengths (L_0, .., L_{F-1}) of a sample; bag is their sum
        self.vocab, self.dim, self.bag = int(vocab), int(dim), sum(bag)
        self.mode, self.optimizer, self.out_dtype = mode, optimizer, out_dtype
        self.max_norm = _clip_arg(max_norm, optimizer, self.dim)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("mindrec_amd ops run on the GPU only (no CPU fallback)")
        self.lr = float(lr) if lr is not None else (5e-2 if optimizer == "ftrl" else 3.5e-4)
        self.eps, self.use_nesterov = float(eps), bool(use_nesterov)
        self.l1, self.l2, self.lr_power = float(l1), float(l2), float(lr_power)
        self.beta1, self.beta2 = np.float32(beta1), np.float32(beta2)
        self.beta1_power, self.beta2_power = np.float32(1.0), np.float32(1.0)
        self.step_count = 0
        # the table, initialised on the device by seed like the engines' (initializer('normal')), and the optimizer's two state arrays
        self.table = torch.empty((self.vocab, self.dim), dtype=torch.float32, device=self.device)
        ops.fill_normal_(self.table, seed=int(seed), sigma=float(sigma))
        if optimizer == "ftrl":
            self.accum = torch.full_like(self.table, float(initial_accum))
            self.linear = torch.zeros_like(self.table)
            self.state = (self.accum, self.linear)
        else:
            self.m = torch.zeros_like(self.table)
            self.v = torch.zeros_like(self.table)
            self.state = (self.m, self.v)
        self._ids = self._mask = None

    def _bags(self, ids):
        """(B, G): ids [B, Ls] are B samples of one group of the fields; one field also takes [B, G, L], G bags of its length per sample"""
        if ids.dim() not in ((2, 3) if len(self.fields) == 1 else (2,)) or ids.shape[-1] != self.bag:
            raise TypeError(f"ids must be [B, {self.bag}] (the bags of lengths {self.fields} back to back), or [B, F, {self.bag}] for one length")
        if self.optimizer == "adam" and ids.dtype != torch.int32:
            raise TypeError("optimizer 'adam' takes int32 ids (the dense row update numbers rows in 32 bits)")
        return ids.shape[0], (ids.shape[1] if ids.dim() == 3 else 1)

    def lookup(self, ids, mask=None, out=None):
        """ids [B, L] -> [B, dim]; ids [B, F, L] -> [B, F * dim] (field f in columns f * dim .. (f + 1) * dim - 1, the reference's
        concat of its pooled fields).  mask: float32 0/1 (or any weight) per id, None = all ones.  out: where the rows go -- for
        [B, L] ids any [B, dim] column block with unit column stride; for [B, F, L] ids a contiguous [B, F * dim] tensor.
        Fields form (bag=(L_0, ..)): ids, mask [B, Ls] -> [B, F * dim]; out: any [B, F * dim] column block with unit column stride."""
        B, G = self._bags(ids)
        if mask is not None and (mask.dtype != torch.float32 or tuple(mask.shape) != tuple(ids.shape)):
            raise TypeError("mask must be float32 of the shape of ids")
        W = len(self.fields) * self.dim        # columns of one group of the fields
        flat = ids.reshape(B * G, self.bag)
        fmask = mask.reshape(B * G, self.bag) if mask is not None else None
        if out is None:
            out = torch.empty((B, G * W), dtype=self.out_dtype, device=self.table.device)
        elif tuple(out.shape) != (B, G * W) or (G > 1 and not out.is_contiguous()):
            raise TypeError("out must be [B, F * dim] (contiguous when ids hold more than one field)")
        ops.gather_pool_fields(self.table, flat, self.fields, fmask, mode=self.mode, out=out if G == 1 else out.view(B * G, W),
                               max_norm=self.max_norm)
        self._ids = flat.contiguous()
        self._mask = fmask.contiguous() if fmask is not None else None
        return out

    def apply_(self, dy, grad_scale=1.0, plan=None):
        """The optimizer step for the gradient dy [B, F * dim] of the last lookup's result (float32; bfloat16 / float16 too under
        'lazy_adam' and 'adam'): in place on the table and the optimizer state.  plan: an ops.sparse_plan to apply with instead of
        building one -- the CALLER's contract: it is ops.sparse_plan of exactly the ids of the last lookup (the same [B, Ls] ids, no
        skip_negative); it is not checked, and a plan of other ids updates other rows.  For several tables looked up by the same
        ids (MultiHotWideDeep below): one plan, handed to each.  None: the plan is built here.  Returns the plan it applied with."""
        if self._ids is None:
            raise RuntimeError("apply_ follows a lookup")
        ids, mask = self._ids, self._mask
        nbags = ids.shape[0] * len(self.fields)
        if dy.dim() != 2 or dy.shape[0] * dy.shape[1] != nbags * self.dim or not dy.is_contiguous():
            raise TypeError("dy must be the contiguous [B, F * dim] gradient of the last lookup's result")
        g = dy.view(nbags, self.dim)
        # one scale per field in place of grad_scale
        fs = tuple(float(np.float32(grad_scale) / np.float32(Lf)) if self.mode == "mean" else float(grad_scale) for Lf in self.fields)
        pkw = dict(fields=self.fields, field_scale=fs)
        if plan is None:
            plan = ops.sparse_plan(ids)
        elif plan.n != ids.numel():
            raise ValueError(f"plan holds {plan.n} positions, the last lookup's ids {ids.numel()}")
        self.beta1_power = np.float32(self.beta1_power * self.beta1)
        self.beta2_power = np.float32(self.beta2_power * self.beta2)
        self.step_count += 1
        akw = dict(lr=self.lr, beta1=float(self.beta1), beta2=float(self.beta2), eps=self.eps, beta1_power=float(self.beta1_power),
                   beta2_power=float(self.beta2_power), use_nesterov=self.use_nesterov)
        if self.optimizer == "lazy_adam":
            ops.sparse_lazy_adam_(self.table, self.m, self.v, plan, g, mask, pool_max_norm=self.max_norm, **pkw, **akw)
        elif self.optimizer == "ftrl":
            ops.sparse_ftrl_(self.table, self.accum, self.linear, plan, g, mask, lr=self.lr, l1=self.l1, l2=self.l2,
                             lr_power=self.lr_power, **pkw)
        else:
            sums = ops.segment_sum(plan, g, mask, **pkw)
            ops.dense_adam_rows_l2_(self.table, self.m, self.v, plan, sums, 0.0, grad_scale=1.0, **akw)
        return plan


class MultiHotWideDeep:
    """The deep and the wide side of multi-hot fields, looked up by the same ids and the same mask (every id field of the reference's
    multitable Wide&Deep is read twice: rows of a [V, D] table, pooled per field, wide_and_deep.py:291-346, and a [V] weight vector,
    summed over everything, :366-420; the table belongs to Adam and the weights to FTRL, :525-535):

        pair = MultiHotWideDeep(vocab=20900, dim=64, bag=(3, 5, 4, 3, 4, 2), mode="mean", optimizer="adam", wide_optimizer="ftrl")
        x, w = pair.lookup(ids, mask)      # ids, mask [B, Ls] -> x [B, F * dim], w [B] float32: the two halves' lookups
        ...
        pair.apply_(dy, dwide)             # dy [B, F * dim], dwide [B]: ONE plan of the ids, then the deep apply and the wide apply

    pair.deep is MultiHotEmbedding(vocab, dim, bag, mode, optimizer) and pair.wide is MultiHotEmbedding(vocab, 1, sum(bag), "sum",
    wide_optimizer): they hold the tables and the optimizer state, and x, w and every table and state array are bit for bit what those
    two objects give when driven separately (deep.lookup / wide.lookup, deep.apply_ / wide.apply_ -- two plans where this builds one).
    The lookup is the two halves' two launches: a one-launch kernel for both sides was built and measured, and was slower than the two
    where the table sits in cache, so it is not here.
    Arguments without a prefix go to the deep half, wide_* to the wide half.  bag: an int (one field) or a tuple; ids are [B, Ls]
    only.  bag=(1,) * n with mask=None is the single-hot case: n rows side by side (Gather + Flatten) and the sum of their n wide
    weights.  max_norm=c clips the deep half's rows (MultiHotEmbedding(max_norm=c)); the wide weights are never clipped, as in the
    fused step, and the plan stays shared.  Neither method synchronises with the host: lookup + apply_ capture into one HIP graph on one stream."""

    def __init__(self, vocab, dim, bag, mode="mean", optimizer="lazy_adam", wide_optimizer="ftrl", device="cuda:0", seed=0, wide_seed=1,
                 sigma=0.01, wide_sigma=0.01, lr=None, wide_lr=None, beta1=0.9, beta2=0.999, eps=1e-8, use_nesterov=False, l1=1e-8, l2=1e-8,
                 lr_power=-0.5, initial_accum=1.0, out_dtype=torch.float32, max_norm=None):
        if wide_optimizer not in _OPTIMIZERS:
            raise ValueError(f"wide_optimizer must be one of {_OPTIMIZERS}, got {wide_optimizer!r}")
        hyper = dict(device=device, beta1=beta1, beta2=beta2, eps=eps, use_nesterov=use_nesterov, l1=l1, l2=l2, lr_power=lr_power,
                     initial_accum=initial_accum)
        self.deep = MultiHotEmbedding(vocab, dim, bag, mode=mode, optimizer=optimizer, seed=seed, sigma=sigma, lr=lr, out_dtype=out_dtype,
                                      max_norm=max_norm, **hyper)      # (the deep half only: the [V] wide weights are never clipped)
        self.wide = MultiHotEmbedding(vocab, 1, self.deep.bag, mode="sum", optimizer=wide_optimizer, seed=wide_seed, sigma=wide_sigma,
                                      lr=wide_lr, **hyper)
        self.fields, self.bag = self.deep.fields, self.deep.bag

    def lookup(self, ids, mask=None, out=None, wide_out=None):
        """ids, mask [B, Ls] -> (x [B, F * dim], w [B] float32).  out: any [B, F * dim] column block with unit column stride;
        wide_out: a float32 [B] tensor of any positive stride (a column of a wider matrix)."""
        deep, wide = self.deep, self.wide
        if ids.dim() != 2:
            raise TypeError(f"ids must be [B, {self.bag}] (the bags of lengths {self.fields} back to back)")
        B = deep._bags(ids)[0]
        if wide_out is None:
            wide_out = torch.empty((B,), dtype=torch.float32, device=wide.table.device)
        elif wide_out.dtype != torch.float32 or wide_out.dim() != 1 or wide_out.shape[0] != B or (B > 1 and wide_out.stride(0) < 1):
            raise TypeError(f"wide_out must be a float32 [{B}] tensor (any positive stride: a column of a wider matrix)")
        x = deep.lookup(ids, mask, out=out)
        wide.lookup(ids, mask, out=wide_out.unsqueeze(1))      # ([B, 1] with wide_out's stride: the lookup's column block)
        wide._ids, wide._mask = deep._ids, deep._mask          # one copy of the ids: apply_ checks that both halves hold it
        return x, wide_out

    def apply_(self, dy, dwide, grad_scale=1.0):
        """The optimizer steps of both halves for dy [B, F * dim], the gradient of x, and dwide [B] (contiguous float32), the gradient
        of w: one ops.sparse_plan of the last lookup's ids, shared.  Returns the plan."""
        if self.deep._ids is None or self.deep._ids is not self.wide._ids:
            raise RuntimeError("apply_ follows a lookup of the pair")
        B = self.deep._ids.shape[0]
        # checked here, before the deep half is touched: a refusal must not leave the pair half-stepped
        if dwide.dtype != torch.float32 or dwide.device != self.wide.table.device or dwide.numel() != B or not dwide.is_contiguous():
            raise TypeError("dwide must be the contiguous float32 [B] gradient of the last lookup's wide sums, on the tables' device")
        plan = ops.sparse_plan(self.deep._ids)
        self.deep.apply_(dy, grad_scale, plan=plan)
        self.wide.apply_(dwide.view(B, 1), grad_scale, plan=plan)
        return plan


class MultiHotHashEmbedding:
    """MultiHotEmbedding over a MapParameter: the multi-hot fields hold raw int keys, rows are created on first sight, admitted and
    evicted by the map's filters, and a key that is not in the table reads as its DEFAULT row (MapTensorGet's contract), not as zeros.

        emb = MultiHotHashEmbedding(dict(key_dtype=torch.int64, value_shape=64, capacity=1 << 20, permit_filter_value=2),
                                    bag=(3, 5, 4, 3, 4, 2), mode="mean", optimizer="lazy_adam")
        x = emb.lookup(keys, mask)               # keys, mask [B, Ls] -> [B, F * dim]; one training step of the table
        ...
        emb.apply_(dy)                           # one plan of the keys' admitted rows, one pooled apply on map.values and the slots
        y = emb.lookup(keys, mask, train=False)  # evaluation / serving: probes only, nothing is inserted or counted

    map_or_kwargs: a MapParameter (float32 values of one dimension, on a GPU) or the keyword arguments to build one; emb.map is it,
    emb.dim its value_shape[0].  bag, mode, fields, MAX_BAG, the `out` column-block rules, out_dtype and the host-side bias-correction
    powers: MultiHotEmbedding's.
    lookup: MapParameter.lookup_rows over the B * Ls keys (train=True: insert=True -- new keys take rows and default values in the
    values AND in the optimizer's slot tables, hits and last-seen steps are counted, map.step advances; train=False: a probe), then ONE
    pooled launch, ops.gather_pool_fields_keyed: a slot whose key has a row contributes map.values[row], any other -- not inserted
    by a probe, or dropped because the table is full -- the key's default row, generated in registers (no [B * Ls, dim] rows, which
    MapParameter.get(insert_default_value=False) has to materialise to overlay them).
    apply_: the keys' rows through MapParameter.admitted_rows -- un-admitted keys (seen in fewer than permit_filter_value training
    lookups) and dropped keys are -1 -- then ops.sparse_plan over them and the pooled ops.sparse_lazy_adam_ / ops.sparse_ftrl_
    (fields=, field_scale=, the mask) on map.values and the slot tables; the windows and the finishing pass of the apply skip a row
    outside [0, capacity), so the -1 group is summed and dropped: such keys are not updated.  A key that occurs in several fields of a
    sample gets the sum of their gradients and ONE update.
    Optimizers: "lazy_adam" (slots "moment1", "moment2": nn.LazyAdam's names over a MapParameter) and "ftrl" ("accum" from
    initial_accum, "linear"), created through MapParameter.add_slot so that every new key's slot rows start at their initial
    values.  "adam", the dense whole-table update, is refused: a hash table has no "every row".  dim = 1, mode "sum", optimizer "ftrl"
    over the same keys is the wide side.  max_norm=c: HashEmbeddingLookup(max_norm=c) over bags -- every slot's row, a missing key's
    default row included, is clipped before its mask product, and apply_ applies through the clip ("lazy_adam" only).  Eviction is the map's (emb.map.evict()): an evicted key seen again is a new key.
    Neither method synchronises with the host."""

    def __init__(self, map_or_kwargs, bag, mode="mean", optimizer="lazy_adam", lr=None, beta1=0.9, beta2=0.999, eps=1e-8, use_nesterov=False,
                 l1=1e-8, l2=1e-8, lr_power=-0.5, initial_accum=1.0, out_dtype=torch.float32, max_norm=None):
        if mode not in ("sum", "mean"):
            raise ValueError(f"mode must be 'sum' or 'mean', got {mode!r}")
        if optimizer == "adam":
            raise ValueError("optimizer 'adam' updates every row of a table: a hash table has no 'every row' (use 'lazy_adam' or 'ftrl')")
        if optimizer not in ("lazy_adam", "ftrl"):
            raise ValueError(f"optimizer must be 'lazy_adam' or 'ftrl', got {optimizer!r}")
        if isinstance(bag, (tuple, list)):
            bag = ops._fields(bag)
        elif int(bag) < 1:
            raise ValueError("bag must be >= 1")
        else:
            bag = (int(bag),)
        device = map_or_kwargs.device if isinstance(map_or_kwargs, MapParameter) else torch.device(map_or_kwargs.get("device", "cuda:0"))
        if device.type != "cuda":
            raise RuntimeError("mindrec_amd ops run on the GPU only (no CPU fallback)")
        self.map = map_or_kwargs if isinstance(map_or_kwargs, MapParameter) else MapParameter(**map_or_kwargs)
        self.fields, self.bag = bag, sum(bag)
        self.dim = self.map.value_shape[0]
        self.mode, self.optimizer, self.out_dtype = mode, optimizer, out_dtype
        self.max_norm = _clip_arg(max_norm, optimizer, self.dim)
        self.device = self.map.device
        self.lr = float(lr) if lr is not None else (5e-2 if optimizer == "ftrl" else 3.5e-4)
        self.eps, self.use_nesterov = float(eps), bool(use_nesterov)
        self.l1, self.l2, self.lr_power = float(l1), float(l2), float(lr_power)
        self.beta1, self.beta2 = np.float32(beta1), np.float32(beta2)
        self.beta1_power, self.beta2_power = np.float32(1.0), np.float32(1.0)
        self.step_count = 0
        if optimizer == "ftrl":
            self.state = (self.map.add_slot("accum", float(initial_accum)), self.map.add_slot("linear", 0.0))
        else:
            self.state = (self.map.add_slot("moment1", 0.0), self.map.add_slot("moment2", 0.0))
        self._rows = self._mask = None

    def lookup(self, keys, mask=None, out=None, train=True):
        """keys [B, Ls] of the map's key dtype (one field: [B, G, L] too, G bags per sample) -> [B, F * dim]; mask, out: as
        MultiHotEmbedding.lookup.  train=True: one training step of the table (see the class); train=False: a probe, and no apply_
        may follow it."""
        if keys.dtype != self.map.key_dtype:
            raise TypeError(f"keys must be {self.map.key_dtype}, the map's key dtype, got {keys.dtype}")
        if keys.dim() not in ((2, 3) if len(self.fields) == 1 else (2,)) or keys.shape[-1] != self.bag:
            raise TypeError(f"keys must be [B, {self.bag}] (the bags of lengths {self.fields} back to back), or [B, G, {self.bag}] for one length")
        ops._need_cuda(keys, mask, out)
        B, G = keys.shape[0], (keys.shape[1] if keys.dim() == 3 else 1)
        if mask is not None and (mask.dtype != torch.float32 or tuple(mask.shape) != tuple(keys.shape)):
            raise TypeError("mask must be float32 of the shape of keys")
        W = len(self.fields) * self.dim
        if out is None:
            out = torch.empty((B, G * W), dtype=self.out_dtype, device=self.device)
        elif tuple(out.shape) != (B, G * W) or (G > 1 and not out.is_contiguous()):
            raise TypeError("out must be [B, F * dim] (contiguous when keys hold more than one bag per sample)")
        flat = keys.reshape(B * G, self.bag).contiguous()
        fmask = mask.reshape(B * G, self.bag).contiguous() if mask is not None else None
        m = self.map
        rows = m.lookup_rows(flat.view(-1), insert=bool(train))[2].view(B * G, self.bag)
        ops.gather_pool_fields_keyed(m.values, rows, flat, self.fields, fmask, mode=self.mode, out=out if G == 1 else out.view(B * G, W),
                                     max_norm=self.max_norm, default=(m._sigma, m._fill, m.seed))
        self._rows = m.admitted_rows(rows) if train else None
        self._mask = fmask
        return out

    def apply_(self, dy, grad_scale=1.0, plan=None):
        """The optimizer step for the gradient dy [B, F * dim] of the last training lookup's result: in place on map.values and the
        two slot tables.  plan: ops.sparse_plan of exactly that lookup's admitted rows (emb.rows), to apply with instead of building
        one; not checked beyond its length.  Returns the plan it applied with."""
        if self._rows is None:
            raise RuntimeError("apply_ follows a lookup with train=True")
        rows, mask = self._rows, self._mask
        nbags = rows.shape[0] * len(self.fields)
        if dy.dim() != 2 or dy.shape[0] * dy.shape[1] != nbags * self.dim or not dy.is_contiguous():
            raise TypeError("dy must be the contiguous [B, F * dim] gradient of the last lookup's result")
        g = dy.view(nbags, self.dim)
        fs = tuple(float(np.float32(grad_scale) / np.float32(Lf)) if self.mode == "mean" else float(grad_scale) for Lf in self.fields)
        pkw = dict(fields=self.fields, field_scale=fs)
        if plan is None:
            plan = ops.sparse_plan(rows)
        elif plan.n != rows.numel():
            raise ValueError(f"plan holds {plan.n} positions, the last lookup's keys {rows.numel()}")
        self.beta1_power = np.float32(self.beta1_power * self.beta1)
        self.beta2_power = np.float32(self.beta2_power * self.beta2)
        self.step_count += 1
        s0, s1 = self.state
        if self.optimizer == "lazy_adam":
            ops.sparse_lazy_adam_(self.map.values, s0, s1, plan, g, mask, lr=self.lr, beta1=float(self.beta1), beta2=float(self.beta2),
                                  eps=self.eps, beta1_power=float(self.beta1_power), beta2_power=float(self.beta2_power),
                                  use_nesterov=self.use_nesterov, pool_max_norm=self.max_norm, **pkw)
        else:
            ops.sparse_ftrl_(self.map.values, s0, s1, plan, g, mask, lr=self.lr, l1=self.l1, l2=self.l2, lr_power=self.lr_power, **pkw)
        return plan

    @property
    def rows(self):
        """int32 [B, Ls]: the admitted rows of the last training lookup's keys (-1: un-admitted or dropped), what apply_ plans over"""
        return self._rows
