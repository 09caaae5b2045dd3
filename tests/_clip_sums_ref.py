"""TEST INFRASTRUCTURE ONLY: max_norm in front of a DENSE optimizer, restated in float64 on top of the oracle -- the op set of the
oracle-side DeepFM / Deep&Cross engines with a clip (tests/_oracle_clip_ops.py: gather_rows(max_norm=) and the Jacobian), plus
  clip_group_sums_: each group's fp32 sum G (segment_sum's, group order) replaced by J(x) G = (c / n)(G - (x.G / n^2) x) in float64
  where n = |x| > c, x = the group's row of p BEFORE the optimizer's update, rounded to fp32 once; groups whose row is outside the
  table, and everything behind the U groups, stay as they are.
The engines take their op set from `_kernels`; the classes below are the oracle-side engines (tests/_oracle_engine.py) over this one."""
import sys

import numpy as np
import torch
import torch.nn.functional as F

import _oracle_clip_ops
from _oracle_clip_ops import *  # noqa: F401,F403
from _oracle_clip_ops import _np, jacobian_apply64
from _oracle_engine import OracleDeepCrossEngine, OracleDeepFMEngine


def gather_rows(table, ids, row_scale=None, max_norm=None):
    """_oracle_clip_ops.gather_rows in the shape the engines expect of ops.gather_rows: ids.shape + (D,)"""
    out = _oracle_clip_ops.gather_rows(table, ids, row_scale, max_norm)
    return out.view(tuple(ids.shape) + (out.shape[-1],))


def clip_sums64(x, G, c):
    """the float64 model of mrec_clip_group_sums_f32 over rows x [U, D] and sums G [U, D]: (J(x) G as fp32, the clipped groups)"""
    x64 = np.asarray(x, np.float64)
    hit = np.sqrt((x64 * x64).sum(axis=1)) > c
    return jacobian_apply64(x, G, c).astype(np.float32), hit


def clip_group_sums_(sums, plan, p, max_norm):
    """ops.clip_group_sums_ over the oracle's plan (segment_sum left the groups' rows in plan._uniq)"""
    u = plan._uniq
    t, s = _np(p), _np(sums)
    ok = (u >= 0) & (u < t.shape[0])
    g = np.flatnonzero(ok)
    s[g], _ = clip_sums64(t[u[g]], s[g], float(max_norm))
    return sums


class OracleClipDeepFMEngine(OracleDeepFMEngine):
    """DeepFMEngine.train_step / predict as they stand, over the oracle's ops with the clip"""
    _kernels = sys.modules[__name__]


class OracleClipDeepCrossEngine(OracleDeepCrossEngine):
    """The oracle-side Deep&Cross step (tests/_torch_net.py, TorchDeepCrossMixin._train_step_generic) with the clipped lookup and
    the table's gradient sums through the clip's Jacobian before the dense Adam; max_norm None: that step itself."""
    _kernels = sys.modules[__name__]

    def _train_step_generic(self, ids, wts, label):
        c = self.cfg.max_norm
        if c is None:
            return super()._train_step_generic(ids, wts, label)
        cfg = self.cfg
        self.step_count += 1
        B, Fd = ids.shape
        D = cfg.emb_dim
        self.beta1_power = np.float32(self.beta1_power * self.beta1)
        self.beta2_power = np.float32(self.beta2_power * self.beta2)
        emb = self.k.gather_rows(self.table, ids, wts, max_norm=c).view(B, Fd * D)
        emb.requires_grad_(True)
        self.dense_grad_flat.zero_()
        logit = self._forward_autograd(emb)
        loss = F.binary_cross_entropy_with_logits(logit, label)
        (loss * cfg.loss_scale).backward()
        plan = self.k.sparse_plan(ids)
        sums = self.k.segment_sum(plan, emb.grad.view(B * Fd, D), wts)
        self.k.clip_group_sums_(sums, plan, self.table, c)
        gtab = torch.zeros_like(self.table)
        self.k.scatter_unique_rows_(gtab, plan, sums)
        kw = dict(lr=cfg.learning_rate, beta1=float(self.beta1), beta2=float(self.beta2), eps=cfg.eps,
                  beta1_power=float(self.beta1_power), beta2_power=float(self.beta2_power), grad_scale=1.0 / cfg.loss_scale)
        self.k.dense_adam_(self.table, self.table_m, self.table_v, gtab, **kw)
        self.k.dense_adam_(self.dense_flat, self.dense_m, self.dense_v, self.dense_grad_flat, **kw)
        return loss.detach()
