"""Evaluation metrics that stay on the device: exact AUC, and MAP@k grouped by display.

  DeviceAUCMetric       models/wide_deep/src/metrics.py:23-52 (AUCMetric) -- the protocol of mindspore.nn.metrics.Metric: clear(),
                        update(logit, predict, label), eval() -> AUC.  update() appends to device buffers and never synchronises;
                        eval() is one ops.auc_counts launch sequence and one read of four integers.
  DeviceAUCMAPMetric    models/wide_and_deep_multitable/src/metrics.py:70-152 -- update(logit, predict, label, display_id), eval() -> AUC,
                        .map = MAP@topk over the displays (new_compute_mAP), .rank_hist the counts behind it.

Both numbers come from integer counts (include/mrec.h 'evaluation metrics'), so they are exact -- the AUC is the trapezoidal ROC area
roc_auc_score computes, to the rounding of one float64 division -- and the same bits on every run.  wide_deep_run.AUCMetric (host lists +
sklearn) stays what it is; these classes are opt-in: WideDeepRunner(engine, metrics={"auc": DeviceAUCMetric()}), EvalCallBack, or, with
the compat package on the path before this module is imported (the classes then derive from its Metric, which Model(metrics=...) asks
for), mindspore's Model.eval.

Where the reference is implementation-defined, MAP resolves in favour of the clicked row: rows of a display predicted EQUAL to the clicked
row, and a clicked prediction of exactly 0.0 against the pads, do not count as ranked above it (the reference ranks with an unstable
np.argsort, reversed: ties fall either way).

Distributed evaluation -- gathering the predictions of all ranks before counting -- is out of scope: each instance counts what its own
process fed it.
"""
import numpy as np
import torch

from . import ops

try:                                        # the compat package (or MindSpore itself), when it is there
    from mindspore.nn.metrics import Metric as _Metric
except ImportError:
    _Metric = object


def _flat(x):
    """x (torch tensor on any device, numpy array, or an object with asnumpy()) as a flat torch tensor."""
    if isinstance(x, torch.Tensor):
        t = x.detach().as_subclass(torch.Tensor)
    else:
        t = torch.from_numpy(np.ascontiguousarray(x.asnumpy() if hasattr(x, "asnumpy") else np.asarray(x)))
    return t.reshape(-1)


class DeviceAUCMetric(_Metric):
    """Area under the ROC curve over everything update() has seen since clear(), counted on the device.  A row is positive iff its
    label > 0.5.  capacity: rows the buffers hold at first (they double when full)."""

    _columns = (torch.float32, torch.float32)                           # predict, label

    def __init__(self, capacity=1 << 20, device="cuda:0"):
        super().__init__()
        if not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"capacity must be an int >= 1, got {capacity!r}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} counts on the GPU (mindrec_amd has no CPU fallback); got device {device!r}")
        self._cap, self._bufs = capacity, None
        self.clear()

    def clear(self):
        self._n, self.counts = 0, None

    def _append(self, cols):
        """cols: one flat tensor per column, all of one length (known from shapes: nothing here waits for the device)."""
        k = cols[0].numel()
        if any(c.numel() != k for c in cols):
            raise ValueError(f"update() got columns of {[c.numel() for c in cols]} rows")
        if self._bufs is None or self._n + k > self._cap:
            while self._n + k > self._cap:
                self._cap *= 2
            old = self._bufs
            self._bufs = [torch.empty(self._cap, dtype=dt, device=self.device) for dt in self._columns]
            if old is not None and self._n:
                for new, o in zip(self._bufs, old):
                    new[: self._n].copy_(o[: self._n])
        for buf, c in zip(self._bufs, cols):
            buf[self._n: self._n + k].copy_(c)
        self._n += k

    def update(self, *inputs):
        """inputs = (logits, predict, label), as PredictWithSigmoid returns them (wide_and_deep.py:495-518)."""
        self._append([_flat(inputs[1]), _flat(inputs[2])])

    def _auc(self, counts):
        twoU, P, N, n_nan = counts
        self.counts = {"twoU": twoU, "P": P, "N": N, "n_nan": n_nan}
        if n_nan:
            raise ValueError(f"Input contains NaN: {n_nan} of {self._n} predictions")
        if P == 0 or N == 0:
            raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
        return twoU / (2 * P * N)

    def _rows(self):
        if self._n == 0:
            raise ValueError(f"{type(self).__name__}.eval(): update() has seen no rows since clear()")
        return [b[: self._n] for b in self._bufs]

    def eval(self):
        pred, label = self._rows()
        auc = self._auc(ops.auc_counts(pred, label).tolist())
        print("====" * 20 + " auc_metric  end")
        print("====" * 20 + " auc: {}".format(auc))
        return auc


class DeviceAUCMAPMetric(DeviceAUCMetric):
    """The multitable Wide&Deep's metric: eval() returns the AUC, as the reference's does, and leaves .map = MAP@topk over the displays
    (every display counted as padded to pad_to candidates of score 0.0, as the reference pads to 30) and .rank_hist = displays per rank
    of the clicked row, a list of topk ints; .groups = displays.  Ties: module docstring."""

    _columns = (torch.float32, torch.float32, torch.int64)             # predict, label, display_id

    def __init__(self, topk=12, pad_to=30, capacity=1 << 20, device="cuda:0"):
        if not isinstance(topk, int) or not 1 <= topk <= 64:
            raise ValueError(f"topk must be an int in 1..64, got {topk!r}")
        if not isinstance(pad_to, int) or pad_to < 0:
            raise ValueError(f"pad_to must be an int >= 0, got {pad_to!r}")
        self.topk, self.pad_to = topk, pad_to
        super().__init__(capacity, device)

    def clear(self):
        super().clear()
        self.map = self.rank_hist = self.groups = None

    def update(self, *inputs):
        """inputs = (logits, predict, label, display_id)."""
        self._append([_flat(inputs[1]), _flat(inputs[2]), _flat(inputs[3])])

    def eval(self):
        pred, label, display = self._rows()
        both = torch.cat([ops.auc_counts(pred, label), ops.group_rank_hist(pred, label, display, self.topk, self.pad_to)]).tolist()
        self.rank_hist, self.groups = both[4: 4 + self.topk], both[4 + self.topk]
        s = 0.0
        for r, h in enumerate(self.rank_hist):
            s += h / (r + 1)
        self.map = s / self.groups
        auc = self._auc(both[:4])
        print("Eval result:" + " auc: {}, map: {}".format(auc, self.map))
        return auc
