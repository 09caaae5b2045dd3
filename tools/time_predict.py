#!/usr/bin/env python3
"""ms per call of WideDeepEngine.predict against predict_fused (without and with a label) on ONE engine, at the benchmark shape
(vocabulary as large as fits, dim 80, 39 fields, batch 16384, fp16, the reference net) and at batch 1024:
    python tools/time_predict.py [vocab] [dist] [pairs] [calls per block]
Device events around blocks of calls, the three arms alternating in rotation inside one process, every arm warmed up first (which
also captures predict_fused's graphs), so that the difference is read against the block-to-block spread of the same box.  The
vocabulary is halved until the tables fit.  One JSON line per batch size: median, min and max of the blocks per arm."""
import json
import os
import sys
from statistics import median

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch  # noqa: E402

args = sys.argv[1:]
V = int(args[0]) if len(args) > 0 else 200_000_000
dist = args[1] if len(args) > 1 else "zipf"
P = int(args[2]) if len(args) > 2 else 7
N = int(args[3]) if len(args) > 3 else 200
dev = torch.device("cuda:0")


def engine(V):
    while True:
        cfg = WideDeepConfig(vocab_size=V, emb_dim=80, field_size=39, batch_size=16384, mlp_dtype="fp16")
        try:
            return cfg, WideDeepEngine(cfg, dev)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            V //= 2
            if V < 1_000_000:
                raise


cfg, eng = engine(V)
for i in range(4):                                   # weights and their 16-bit copies have moved
    eng.train_step(*synthetic_batch(cfg, dev, dist, seed=1000 + i))
ARMS = {"predict": lambda b: eng.predict(b[0], b[1]),
        "predict_fused": lambda b: eng.predict_fused(b[0], b[1]),
        "predict_fused+loss": lambda b: eng.predict_fused(b[0], b[1], b[2])}


def block(fn, batches, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(n):
        fn(batches[i % len(batches)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


for B in (16384, 1024):
    bcfg = WideDeepConfig(vocab_size=cfg.vocab_size, emb_dim=80, field_size=39, batch_size=B)
    batches = [synthetic_batch(bcfg, dev, dist, seed=2000 + i) for i in range(8)]
    for fn in ARMS.values():
        block(fn, batches, 20)                       # warm-up: workspaces, code objects, the captured graphs
    names = list(ARMS)
    res = {k: [] for k in names}
    for p in range(P):
        for q in range(len(names)):
            k = names[(p + q) % len(names)]
            res[k].append(block(ARMS[k], batches, N))
    out = {"tool": "time_predict", "vocab": cfg.vocab_size, "batch": B, "dist": dist, "blocks": P, "calls_per_block": N,
           "graphs": sorted(str(k) for k, v in eng._predict_graphs.items() if v["g"] is not None)}
    for k in names:
        out[k] = {"median_ms": round(median(res[k]), 4), "min_ms": round(min(res[k]), 4), "max_ms": round(max(res[k]), 4)}
    out["fused/predict"] = round(out["predict_fused"]["median_ms"] / out["predict"]["median_ms"], 4)
    print(json.dumps(out), flush=True)
eng.close()
