#!/usr/bin/env python3
"""ms per step of the Wide&Deep step at the benchmark shape (B 16384, D 80, fp16 net, whole-step graphs, sinks of 5) with
max_norm on and off, measured in alternating A/B blocks on one device, so that the cost of the clip is read against the run-to-run
noise of the same box:  python tools/max_norm_ab.py [vocab] [fields] [dist] [max_norm] [pairs]
(--one on|off: one engine alone -- fresh processes alternating on / off, free of the placement of two engines in one process;
also what runs under rocprofv3 --kernel-trace --stats; --no-const: const_columns=False on both,
so that the clip is the only difference -- max_norm turns the hot-column apply off; --control: a second engine without max_norm,
created after the other two, timed in the same rotation: the spread between two identical engines)"""
import os
import sys
import time
from statistics import median

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
one = sys.argv[sys.argv.index("--one") + 1] if "--one" in sys.argv else None
if one:
    args = [a for a in args if a != one]
V = int(args[0]) if len(args) > 0 else 10_000_000
F = int(args[1]) if len(args) > 1 else 26
dist = args[2] if len(args) > 2 else "uniform"
C = float(args[3]) if len(args) > 3 else 0.09          # about the median initial row norm (0.01 * sqrt(80)): both branches occur
P = int(args[4]) if len(args) > 4 else 6
dev = torch.device("cuda:0")
S = 5


no_const = "--no-const" in sys.argv


def engine(max_norm):
    cfg = WideDeepConfig(vocab_size=V, emb_dim=80, field_size=F, batch_size=16384, max_norm=max_norm,
                         const_columns=not no_const)
    return cfg, WideDeepEngine(cfg, dev)


def block(eng, batches, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        eng.train_steps([batches[(i * S + j) % len(batches)] for j in range(S)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (k * S) * 1e3


cfg = WideDeepConfig(vocab_size=V, emb_dim=80, field_size=F, batch_size=16384)
batches = [synthetic_batch(cfg, dev, dist, seed=1000 + i) for i in range(8)]
engs = {}
names = ["off", "on"] + (["off2"] if "--control" in sys.argv else [])
for name in (names if one is None else [one]):
    _, e = engine(C if name == "on" else None)
    for i in range(6):
        e.train_step(*batches[i % 8])
    block(e, batches, 10)                         # capture + warm-up of the whole-step graphs
    engs[name] = e
if one is not None:
    bl = [block(engs[one], batches, 6) for _ in range(P)]
    print(f"{one}: median {median(bl):.4f} ms/step (blocks {', '.join(f'{x:.4f}' for x in bl)})")
    sys.exit(0)
res = {k: [] for k in names}
for p in range(P):
    for q in range(len(names)):
        name = names[(p + q) % len(names)]
        res[name].append(block(engs[name], batches, 6))
med = {k: median(v) for k, v in res.items()}
print(f"V={V} F={F} {dist} max_norm={C}{' const_columns=False' if no_const else ''}: " +
      "; ".join(f"{k} {med[k]:.4f} ms/step (blocks {', '.join(f'{x:.4f}' for x in res[k])})" for k in names) +
      f"; on/off {med['on'] / med['off']:.4f}")
