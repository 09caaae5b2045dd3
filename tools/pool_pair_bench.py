#!/usr/bin/env python3
"""The deep and the wide side of multi-hot fields from one plan, against the two plans it replaces, kernel time by kernel time
("Deep and wide side from one plan").

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/pool_pair_bench.py run ref > OUT/labels.json      (or large)
  python tools/pool_pair_bench.py reduce OUT/labels.json <the run's *_kernel_trace.csv>

The method is tools/pool_bench.py's: `run` issues, five times each and in rotation, the two variants at one shape, every repeat
behind a marker launch, and prints the order of the repeats; `reduce` cuts the trace's dispatches (in start order) at the markers
and adds up the kernel times of every repeat.  Nothing is timed on the host.  One job per shape.
  bwd_two    what two MultiHotEmbedding objects do: ops.sparse_plan + ops.sparse_lazy_adam_(fields=...) for the deep table, then
             ops.sparse_plan over the same ids again + ops.sparse_ftrl_ (one bag of Ls) for the wide weights.  THE YARDSTICK.
  bwd_pair   what MultiHotWideDeep.apply_ does: ONE ops.sparse_plan, then the same two applies
(profiles/pool_pair_bench.txt also holds fwd_two / fwd_pair: the two lookups against a one-launch pair lookup that was measured with
this tool and not kept.)
Fields (3, 5, 4, 3, 4, 2) of one table, B 131 072, D 64, a 0/1 mask; "ref" = V 20 900, Zipf-like ids; "large" = V 20 000 000,
uniform ids (rows do not sit in cache)."""
import csv
import json
import os
import sys
from statistics import median

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_bench  # noqa: E402

VARIANTS = ("bwd_two", "bwd_pair")
FIELDS = pool_bench.FIELDS


def run(shape):
    D, B, lens = 64, 131072, FIELDS
    F, Ls = len(lens), sum(lens)
    ops, torch, V, tid, mask, table, m, v, dy, marker = pool_bench._setup("fields-" + shape, (B, Ls), (B, F * D))
    dev = table.device
    wide = torch.empty((V, 1), dtype=torch.float32, device=dev)
    ops.fill_normal_(wide, seed=2, sigma=0.01)
    accum, linear = torch.ones_like(wide), torch.zeros_like(wide)
    dw = dy[:, :1].contiguous()
    akw = dict(beta1_power=0.9, beta2_power=0.999)
    fs = tuple(1.0 / L for L in lens)

    def applies(plan_deep, plan_wide):
        ops.sparse_lazy_adam_(table, m, v, plan_deep, dy, mask, fields=lens, field_scale=fs, **akw)
        ops.sparse_ftrl_(wide, accum, linear, plan_wide, dw, mask, fields=(Ls,), field_scale=(1.0,))

    def variant(name):
        if name == "bwd_two":
            applies(ops.sparse_plan(tid), ops.sparse_plan(tid))
        else:
            plan = ops.sparse_plan(tid)
            applies(plan, plan)

    order = pool_bench._rotate(ops, torch, marker, VARIANTS, variant)
    print(json.dumps(dict(shape=shape, V=V, D=D, L=list(lens), B=B, order=order, variants=list(VARIANTS))))


def reduce(labels_path, trace_path):
    lab = json.load(open(labels_path))
    rows = list(csv.DictReader(open(trace_path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    order = lab["order"]
    marks = [i for i, r in enumerate(rows) if "k_fill_normal" in r["Kernel_Name"]][-(len(order) + 1):]
    assert len(marks) == len(order) + 1, (len(marks), len(order))
    per = {k: [] for k in VARIANTS}
    kernels = {k: {} for k in VARIANTS}
    for j, name in enumerate(order):
        seg = rows[marks[j] + 1: marks[j + 1]]
        per[name].append(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in seg) / 1e3)
        for r in seg:
            k = r["Kernel_Name"].replace("(anonymous namespace)::", "")[:90]
            kernels[name].setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"shape {lab['shape']}: V={lab['V']} D={lab['D']} fields={lab['L']} B={lab['B']}; sum of kernel times per repeat, us")
    spread = {}
    for name in VARIANTS:
        x = per[name]
        spread[name] = max(x) - min(x)
        print(f"  {name:9s} median {median(x):9.1f}  min {min(x):9.1f}  max {max(x):9.1f}  spread {spread[name]:7.1f} us = "
              f"{100 * spread[name] / median(x):5.1f} %  ({', '.join(f'{t:.1f}' for t in x)})")
        for k, ts in kernels[name].items():
            print(f"      {median(ts):9.1f} us x {len(ts) // len(x)}  {k}")
    bt, bp = (median(per[k]) for k in VARIANTS)
    big = max(spread["bwd_two"], spread["bwd_pair"])
    print(f"  plan(s) + both applies: two - pair = {bt - bp:+.1f} us (pair / two = {bp / bt:.3f}); the larger spread {big:.1f} us: "
          f"{'faster beyond it' if bt - bp > big else 'NOT faster by more than the spread'}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run" and sys.argv[2] in ("ref", "large"):
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "reduce":
        reduce(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
