#!/usr/bin/env python3
"""The evaluation tail as one launch (ops.tail_predict) against the three launches it replaces, on one MI355X:
    python tools/time_tail_predict.py [vocab] [dist] [samples] [calls per sample]
1. engine: WideDeepEngine.predict_fused replayed from its captured graph with fused_tail_eval on and off, without and with a label, at
   the benchmark shape (vocabulary as large as fits, dim 80, 39 fields, fp16, the reference net) at batch 16384 and 1024.  ONE engine
   (two would not fit beside each other at this vocabulary): an arm sets the switch and its own graph cache before it calls, so both
   arms are code paths of this build on the same tables and weights.  A sample is a host clock around `calls` calls ending in a
   synchronise.
2. launch: ops.tail_predict against dense_fwd, dense_fwd, head_predict in sequence at the same two batch sizes, the wide branch as
   39 products a row, without and with a label.  Each arm is captured once as a graph of `calls` repetitions; a sample is device events
   around one replay (the device's time for the launches, no host time between them).
The arms alternate in rotation after a warm-up that captures the graphs; one JSON line per (part, batch) with the median, min and max
of the samples per arm, ms per call."""
import json
import os
import sys
import time
from statistics import median

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mindrec_amd import ops  # noqa: E402
from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch  # noqa: E402

args = sys.argv[1:]
V = int(args[0]) if len(args) > 0 else 200_000_000
dist = args[1] if len(args) > 1 else "zipf"
P = int(args[2]) if len(args) > 2 else 9
N = int(args[3]) if len(args) > 3 else 20
dev = torch.device("cuda:0")
K2, N2, N3, F = 512, 256, 128, 39


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


def rotate(arms, sample):
    """P samples per arm, the arms alternating in rotation"""
    names = list(arms)
    res = {k: [] for k in names}
    for p in range(P):
        for q in range(len(names)):
            k = names[(p + q) % len(names)]
            res[k].append(sample(arms[k]))
    return {k: {"median_ms": round(median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)} for k, v in res.items()}


# ---- 1. the engine ------------------------------------------------------------------------------------------------------------------
cfg, eng = engine(V)
assert eng._tail_ok
for i in range(4):                                   # weights and their 16-bit copies have moved
    eng.train_step(*synthetic_batch(cfg, dev, dist, seed=1000 + i))


def engine_arm(flag, labelled):
    graphs = {}

    def run(b):
        eng._tail_eval, eng._predict_graphs = flag, graphs
        return eng.predict_fused(b[0], b[1], b[2] if labelled else None)
    run.graphs = graphs
    return run


def host_block(fn, batches, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


for B in (16384, 1024):
    bcfg = WideDeepConfig(vocab_size=cfg.vocab_size, emb_dim=80, field_size=39, batch_size=B)
    batches = [synthetic_batch(bcfg, dev, dist, seed=2000 + i) for i in range(8)]
    arms = {f"fused_tail_eval={flag}{'+loss' if lab else ''}": engine_arm(flag, lab) for lab in (False, True) for flag in (True, False)}
    for fn in arms.values():
        host_block(fn, batches, 20)                  # warm-up: workspaces, code objects, the captured graphs
        assert all(v["g"] is not None for v in fn.graphs.values()) and len(fn.graphs) == 1
    out = {"tool": "time_tail_predict", "part": "engine", "vocab": cfg.vocab_size, "batch": B, "dist": dist, "samples": P, "calls_per_sample": N}
    out.update(rotate(arms, lambda fn: host_block(fn, batches, N)))
    print(json.dumps(out), flush=True)
    for fn in arms.values():
        fn.graphs.clear()
eng._predict_graphs = {}
eng.close()
del eng
torch.cuda.empty_cache()


# ---- 2. the launch alone ------------------------------------------------------------------------------------------------------------
def launch_arm(fn):
    """fn captured as one graph of N repetitions and replayed once: the graph and the last repetition's outputs"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(N):
            keep = fn()
    g.replay()
    torch.cuda.synchronize()
    return {"g": g, "keep": keep}


def event_sample(arm):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    arm["g"].replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / N


gen = torch.Generator(device=dev).manual_seed(7)
rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)      # noqa: E731
w2, w3 = (rnd(K2, N2) * 0.06).half(), (rnd(N2, N3) * 0.08).half()
b2, b3, w5, b5, wb = rnd(N2) * 0.1, rnd(N3) * 0.1, rnd(N3) * 0.1, rnd(1) * 0.1, rnd(1) * 0.1
packed = ops.tail_pack_weights(w2, w3)
for B in (16384, 1024):
    x = torch.relu(rnd(B, K2)).half()
    wide = torch.zeros((B, F, 2), device=dev)
    wide[:, :, 0] = rnd(B, F) * 0.05
    label = (torch.rand(B, device=dev, generator=gen) < 0.3).float()

    def chain(lab):
        y3 = ops.dense_fwd(ops.dense_fwd(x, w2, b2, relu=True), w3, b3, relu=True)
        return ops.head_predict(y3, w5, b5, wide_prod=wide, wide_bias=wb, label=lab)

    def tail(lab, out):
        return ops.tail_predict(x, packed, b2, b3, w5, b5, wide, wide_bias=wb, label=lab, out=out)

    arms = {}
    for lab in (None, label):
        sfx = "+loss" if lab is not None else ""
        arms["tail_predict" + sfx] = launch_arm(lambda lab=lab, out={}: tail(lab, out))
        arms["three_launches" + sfx] = launch_arm(lambda lab=lab: chain(lab))
        assert all(torch.equal(p, q) for p, q in zip(arms["tail_predict" + sfx]["keep"][:2], arms["three_launches" + sfx]["keep"][:2]))
    out = {"tool": "time_tail_predict", "part": "launch", "batch": B, "F": F, "samples": P, "calls_per_sample": N}
    out.update(rotate(arms, event_sample))
    print(json.dumps(out), flush=True)
