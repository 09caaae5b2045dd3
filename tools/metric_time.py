"""Evaluation-metric time: mindrec_amd.metrics.DeviceAUCMetric against the host wide_deep_run.AUCMetric in one process.

N = 2^22 rows fed as 256 updates of 16384 rows (device tensors, as WideDeepRunner.eval feeds predict()'s outputs).  Timed: clear() + the
updates + eval(), with a device synchronisation at the end; median of 5 runs after 2 warm-up runs.  For the device metric the run is
also split at the end of the updates (one more synchronisation there, so the split run is timed separately from the total).
Prints one JSON line; DESIGN.md §5 "Evaluation metrics on the device" quotes it.

    python tools/metric_time.py [--rows-log2 22] [--updates 256] [--runs 5] [--warmup 2]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=22)
    ap.add_argument("--updates", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from mindrec_amd.metrics import DeviceAUCMetric
    from mindrec_amd.wide_deep_run import AUCMetric
    dev = torch.device("cuda:0")
    n, k = 1 << a.rows_log2, a.updates
    b = n // k
    rng = np.random.default_rng(2024)
    logit = rng.standard_normal(n).astype(np.float32)
    label = (rng.random(n) < 1 / (1 + np.exp(-logit - 1))).astype(np.float32)         # a signal: AUC well off 0.5
    prob = torch.sigmoid(torch.from_numpy(logit)).to(dev).view(k, b, 1)
    label = torch.from_numpy(label).to(dev).view(k, b, 1)
    sync = torch.cuda.synchronize

    def run(metric, split=False):
        sync()
        t0 = time.perf_counter()
        metric.clear()
        for i in range(k):
            metric.update(None, prob[i], label[i])
        if split:
            sync()
        t1 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            auc = metric.eval()
        sync()
        t2 = time.perf_counter()
        return auc, (t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3

    out = {"rows": n, "updates": k, "runs": a.runs, "warmup": a.warmup}
    aucs = {}
    for name, metric in (("device", DeviceAUCMetric(capacity=1 << 20, device=dev)), ("host", AUCMetric())):
        res = [run(metric) for _ in range(a.warmup + a.runs)][a.warmup:]
        aucs[name] = res[-1][0]
        out[name + "_total_ms"] = round(statistics.median(r[1] for r in res), 3)
        if name == "device":
            res = [run(metric, split=True) for _ in range(a.runs)]
            out["device_update_ms"] = round(statistics.median(r[2] for r in res), 3)
            out["device_eval_ms"] = round(statistics.median(r[3] for r in res), 3)
            out["device_counts"] = metric.counts
    out["auc_device"], out["auc_host"] = aucs["device"], aucs["host"]
    out["auc_abs_diff"] = abs(aucs["device"] - aucs["host"])
    # floor from the bytes moved: key/class build (8 B read, 8 B written per row), three sort passes (keys read twice -- histogram and
    # scatter --, classes once, both written: 20 B), two reads of the sorted pairs (8 B each) and the compacted boundaries (<= 16 B)
    out["eval_bytes_per_row"] = 8 + 8 + 3 * 20 + 2 * 8 + 16
    print(json.dumps(out))


if __name__ == "__main__":
    main()
