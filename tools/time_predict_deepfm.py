#!/usr/bin/env python3
"""ms per call of DeepFMEngine.predict against predict_fused (without and with a label) on ONE engine, at the reference's DeepFM shape
(vocabulary 184965, dim 80, 39 fields, the net 1024-512-256-128, fp16) at batch 16000 and at batch 1024:
    python tools/time_predict_deepfm.py [dist] [pairs] [calls per block]
Device events around blocks of calls, the three arms alternating in rotation inside one process, every arm warmed up first (which
also captures predict_fused's graphs), so that the difference is read against the block-to-block spread of the same box.
One JSON line per batch size: median, min and max of the blocks per arm."""
import json
import os
import sys
from statistics import median

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mindrec_amd.deepfm import DeepFMConfig, DeepFMEngine  # noqa: E402
from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch  # noqa: E402

args = sys.argv[1:]
dist = args[0] if len(args) > 0 else "zipf"
P = int(args[1]) if len(args) > 1 else 7
N = int(args[2]) if len(args) > 2 else 100
dev = torch.device("cuda:0")

cfg = DeepFMConfig()                                  # the reference's shape and net, fp16
eng = DeepFMEngine(cfg, dev)


def batch_cfg(B):
    return WideDeepConfig(vocab_size=cfg.data_vocab_size, emb_dim=cfg.data_emb_dim, field_size=cfg.data_field_size, batch_size=B)


for i in range(4):                                   # weights and their 16-bit copies have moved
    eng.train_step(*synthetic_batch(batch_cfg(cfg.batch_size), dev, dist, seed=1000 + i))
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


for B in (cfg.batch_size, 1024):
    batches = [synthetic_batch(batch_cfg(B), dev, dist, seed=2000 + i) for i in range(8)]
    for fn in ARMS.values():
        block(fn, batches, 20)                       # warm-up: workspaces, code objects, the captured graphs
    names = list(ARMS)
    res = {k: [] for k in names}
    for p in range(P):
        for q in range(len(names)):
            k = names[(p + q) % len(names)]
            res[k].append(block(ARMS[k], batches, N))
    out = {"tool": "time_predict_deepfm", "vocab": cfg.data_vocab_size, "batch": B, "dist": dist, "blocks": P, "calls_per_block": N,
           "graphs": sorted(str(k) for k, v in eng._predict_graphs.items() if v["g"] is not None)}
    for k in names:
        out[k] = {"median_ms": round(median(res[k]), 4), "min_ms": round(min(res[k]), 4), "max_ms": round(max(res[k]), 4)}
    out["fused/predict"] = round(out["predict_fused"]["median_ms"] / out["predict"]["median_ms"], 4)
    print(json.dumps(out), flush=True)
eng.close()
