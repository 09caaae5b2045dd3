#!/usr/bin/env python3
"""MultiTableWideDeep.train_step at the reference's shape -- tables 650 000 x 128, 17 300 x 64, 20 900 x 64, 16 x 64, field counts 2 / 3 / 2,
bags (3, 5, 4, 3, 4, 2), 32 continuous values, five layers of 1024 in fp16, B = 16384, ids uniform over each table -- in its three forms:
graphs="none" (the launch list one by one: ~26 optimizer launches for the tables), the fused chain issued eagerly (ops.multitable_optim_:
three nodes) and the chain replayed as one HIP graph (graphs="step").

  timeout -k 10 600 python tools/mt_step_bench.py time
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/mt_step_bench.py trace chain
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT2 -- python tools/mt_step_bench.py trace none
  python tools/mt_step_bench.py reduce OUT/.../*kernel_trace.csv

time: WARM steps of every arm (the graph arm captures in its third), then STEPS rounds; a round times one step of each arm in turn --
the arms alternate, so a neighbour's load on the machine falls on all three -- with a host clock between two device synchronisations,
over ROTATE distinct batches.  One JSON line: the median, minimum and maximum per arm in microseconds.  Profiler off.
trace ARM: WARM steps, a synchronise, one more step -- under rocprofv3's kernel trace, in a run of its own, the program after `--`.
reduce: the last step of a trace: its launches in order from the backward launch's end on (the optimizer stage, the dense net's Adam and
the weight copies), each with its duration, and their count and sum; one JSON line.  DESIGN.md section 6."""
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, WARM, STEPS, ROTATE = 16384, 5, 24, 4


def batches(cfg, dev):
    import numpy as np
    import torch
    from mindrec_amd.multitable import MULTI_KEYS
    out = []
    for s in range(ROTATE):
        rng = np.random.default_rng(s)
        b = {"continue_val": rng.random((B, cfg.n_continue)).astype(np.float32),
             "indicator_id": rng.integers(0, cfg.indicator_vocab, (B, cfg.n_indicator)).astype(np.int32),
             "emb_128_id": rng.integers(0, cfg.emb128_vocab, (B, cfg.n_emb128)).astype(np.int32),
             "emb_64_single_id": rng.integers(0, cfg.emb64_single_vocab, (B, cfg.n_emb64_single)).astype(np.int32)}
        for key, L in zip(MULTI_KEYS, cfg.multi_bags):
            b[key] = rng.integers(0, cfg.emb64_multi_vocab, (B, L)).astype(np.int32)
            b[key + "_mask"] = (rng.random((B, L)) < 0.7).astype(np.float32)
        b["label"] = (rng.random(B) < 0.4).astype(np.float32)
        out.append({k: torch.from_numpy(v).to(dev) for k, v in b.items()})
    return out


def arm(kind):
    """(model, step function) of an arm: "none", "chain" (the fused chain, never captured) or "graph" """
    from mindrec_amd.multitable import MultiTableConfig, MultiTableWideDeep
    net = MultiTableWideDeep(MultiTableConfig(graphs="none" if kind == "none" else "step"))

    def step(batch):
        if kind == "chain":
            net._graph_eager = 0          # (the engine captures after two eager steps at a shape: this arm stays eager)
        return net.train_step(batch, batch["label"])
    return net, step


def run_time():
    import torch
    arms = {k: arm(k) for k in ("none", "chain", "graph")}
    dev = arms["none"][0].device
    bs = batches(arms["none"][0].cfg, dev)
    for k, (net, step) in arms.items():
        for i in range(WARM):
            step(bs[i % ROTATE])
    torch.cuda.synchronize()
    assert arms["graph"][0]._graph is not None and arms["chain"][0]._graph is None
    # the three arms trained on the same batches from the same seed: the same parameters, bit for bit
    for k in ("chain", "graph"):
        for name, p in arms["none"][0].params.items():
            assert torch.equal(p, arms[k][0].params[name]), (k, name)
    us = {k: [] for k in arms}
    for i in range(STEPS):
        for k, (net, step) in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(bs[i % ROTATE])
            torch.cuda.synchronize()
            us[k].append((time.perf_counter() - t0) * 1e6)
    print(json.dumps({"B": B, "steps": STEPS, "warm": WARM, **{k + "_us": {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                                                                           "max": round(max(v), 1)} for k, v in us.items()}}))


def run_trace(kind):
    import torch
    net, step = arm(kind)
    bs = batches(net.cfg, net.device)
    for i in range(WARM):
        step(bs[i % ROTATE])
    torch.cuda.synchronize()
    step(bs[0])
    torch.cuda.synchronize()
    print(json.dumps({"arm": kind, "steps": WARM + 1}))


def reduce(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    first = max(i for i, n in enumerate(names) if "k_mt_input" in n and "k_mt_input_bwd" not in n)      # the last step's input launch
    last_bwd = max(i for i, n in enumerate(names) if "k_mt_input_bwd" in n)
    stage = [(r["Kernel_Name"][:48], round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, 2)) for r in rows[last_bwd + 1:]]
    span = (int(rows[-1]["End_Timestamp"]) - int(rows[first]["Start_Timestamp"])) / 1e3
    fused = [d for n, d in stage if "k_mt_optim" in n or "k_mt_rows_to_groups" in n]
    print(json.dumps({"step_launches": len(rows) - first, "step_span_us": round(span, 1), "after_backward_launches": len(stage),
                      "after_backward_sum_us": round(sum(d for _, d in stage), 2), "mt_optim_kernels_us": fused, "after_backward": stage}))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "time":
        run_time()
    elif len(sys.argv) == 3 and sys.argv[1] == "trace" and sys.argv[2] in ("none", "chain"):
        run_trace(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "reduce":
        reduce(sys.argv[2])
    else:
        sys.exit(__doc__)
