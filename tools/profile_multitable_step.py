"""The multitable Wide&Deep's training step at the reference shape (default MultiTableConfig, B = 16384), for a kernel trace:

    rocprofv3 --kernel-trace --stats -d OUT -o step -- python tools/profile_multitable_step.py step
    rocprofv3 --kernel-trace --stats -d OUT -o compare -- python tools/profile_multitable_step.py compare
    python tools/profile_multitable_step.py compare          # device-event times, profiler off

  step     two warm-up steps, then ten train_step calls on one seeded batch
  compare  one backward for a real g_x / g_wide, then -- alternating, ten times each after two warm-ups -- ops.multitable_input_bwd
           and the composition it replaces on the same inputs and plans: four .contiguous() column copies and eight ops.segment_sum
           calls (deep and wide side of each table); prints both device-event times and checks that the two agree."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mindrec_amd import ops                                              # noqa: E402
from mindrec_amd.multitable import MULTI_KEYS, MultiTableConfig, MultiTableWideDeep   # noqa: E402


def make_batch(cfg, B, seed=0):
    rng = np.random.default_rng(seed)
    b = {"continue_val": rng.random((B, cfg.n_continue)).astype(np.float32),
         "indicator_id": rng.integers(0, cfg.indicator_vocab, (B, cfg.n_indicator)).astype(np.int32),
         "emb_128_id": np.minimum(rng.zipf(1.2, (B, cfg.n_emb128)), cfg.emb128_vocab - 1).astype(np.int32),
         "emb_64_single_id": np.minimum(rng.zipf(1.2, (B, cfg.n_emb64_single)), cfg.emb64_single_vocab - 1).astype(np.int32)}
    for key, L in zip(MULTI_KEYS, cfg.multi_bags):
        b[key] = np.minimum(rng.zipf(1.2, (B, L)), cfg.emb64_multi_vocab - 1).astype(np.int32)
        b[key + "_mask"] = (rng.random((B, L)) < 0.7).astype(np.float32)
    b["label"] = (rng.random(B) < 0.3).astype(np.float32)
    return {k: torch.from_numpy(v).cuda() for k, v in b.items()}


def composed(g_x, g_wide, groups, gs):
    """the stage from the older ops: per table a contiguous copy of its column block and two segment sums"""
    out = []
    for q in groups:
        segs = q.segments
        D, B = segs[0].table.shape[1], g_x.shape[0]
        blk = g_x[:, segs[0].col:segs[-1].col + segs[-1].width].contiguous()
        lens = [s.ids.shape[1] for s in segs]
        rsc = None if segs[0].mask is None else torch.cat([s.mask for s in segs], dim=1)
        gwp = g_wide.view(B, 1).expand(B, sum(lens)).reshape(-1, 1)
        if segs[0].pooled:
            deep = ops.segment_sum(q.plan, blk, row_scale=rsc, fields=lens, field_scale=[gs / L for L in lens])
        else:
            deep = ops.segment_sum(q.plan, blk.view(-1, D), grad_scale=gs)
        out.append((deep, ops.segment_sum(q.plan, gwp, row_scale=rsc, grad_scale=gs)))
    return out


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "step"
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
    cfg = MultiTableConfig()
    net = MultiTableWideDeep(cfg)
    batch = make_batch(cfg, B)
    if mode == "step":
        for _ in range(2):
            net.train_step(batch, batch["label"])
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        losses = [net.train_step(batch, batch["label"]) for _ in range(10)]
        t1.record()
        torch.cuda.synchronize()
        print(f"train_step x10 at B = {B}: {t0.elapsed_time(t1) / 10:.3f} ms per step (eager, host included); loss {float(losses[0]):.5f} -> {float(losses[-1]):.5f}")
        return
    g = net._backward(batch, batch["label"])
    groups = net._groups(batch, net._segments(batch))
    gs = 1.0 / cfg.sens
    new = lambda: ops.multitable_input_bwd(g["g_x"], g["g_wide"], groups, cont=batch["continue_val"], grad_scale=gs)
    old = lambda: composed(g["g_x"], g["g_wide"], groups, gs)
    times = {"multitable_input_bwd": [], "composed": []}
    for it in range(12):
        for name, f in (("multitable_input_bwd", new), ("composed", old)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = f()
            t1.record()
            torch.cuda.synchronize()
            if it >= 2:
                times[name].append(t0.elapsed_time(t1))
    (a, _), b = new(), old()
    worst = 0.0
    for q, (s, w), (s2, w2) in zip(groups, a, b):
        U = q.plan.U
        worst = max(worst, float(((s[:U] - s2[:U]).abs().max() / s2[:U].abs().max()).cpu()), float(((w[:U] - w2[:U, 0]).abs().max() / w2[:U, 0].abs().max()).cpu()))
    for name, t in times.items():
        print(f"{name} at B = {B}: median {np.median(t) * 1e3:.1f} us, min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f} (device events around the call, 10 runs)")
    print(f"largest difference between the two, relative to the largest sum: {worst:.2e}")


if __name__ == "__main__":
    main()
