#!/usr/bin/env python3
"""The keyed pooled lookup (mrec_gather_pool_fields_keyed: multi-hot fields over a hash table) kernel time by kernel time, in the
manner of tools/pool_bench.py ("Multi-hot fields over a hash table").

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/pool_hash_bench.py run SHAPE > OUT/labels.json
  python tools/pool_hash_bench.py reduce OUT/labels.json <the run's *_kernel_trace.csv>

D = 64, fields (3, 5, 4, 3, 4, 2), B = 131 072, int64 keys, a 0/1 mask, mean; SHAPE "small": a map of 32 Ki rows (8 MB of values: in
cache), "large": 32 Mi rows (8 GB: not).  Every row of the map is live (key i holds row i).  `run` issues the four variants five times
each in rotation, every repeat behind a marker launch (a one-row k_fill_normal); `reduce` cuts the trace at the markers and adds up
the kernel times of every repeat.  Nothing is timed on the host.
  (a) all keys resident -- the two pooled kernels over the SAME row numbers, nothing else in the repeat:
    a_plain   ops.gather_pool_fields(values, rows)              k_gather_pool_fields, the kernel the dense MultiHotEmbedding runs
    a_keyed   ops.gather_pool_fields_keyed(values, rows, keys)  k_gather_pool_fields_keyed
  (b) half of the key positions miss -- a lookup that does not insert (evaluation, serving), the probe included on both sides:
    b_comp    the composition available without the keyed kernel: KeyIndex.lookup (probe), ops.gather_rows into [B * 21, D],
              KeyIndex.fill_missing over them, ops.gather_pool_fields from those rows
    b_keyed   KeyIndex.lookup (probe) + ops.gather_pool_fields_keyed"""
import csv
import json
import os
import sys
from statistics import median

REPEATS = 5
VARIANTS = ("a_plain", "a_keyed", "b_comp", "b_keyed")
FIELDS = (3, 5, 4, 3, 4, 2)


def run(shape):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from mindrec_amd import ops
    dev = torch.device("cuda:0")
    C = {"small": 32 << 10, "large": 32 << 20}[shape]
    D, B, lens = 64, 131072, FIELDS
    F, Ls = len(lens), sum(lens)
    seed, sigma = 5, 0.01
    rng = np.random.default_rng(7)
    values = torch.empty((C, D), dtype=torch.float32, device=dev)
    ops.fill_normal_(values, seed=1, sigma=0.01)
    index = ops.KeyIndex(C, dev)
    rows0 = index.lookup(torch.arange(C, dtype=torch.int64, device=dev), insert=True, unique=True)      # key i -> row i
    assert bool((rows0 == torch.arange(C, dtype=torch.int32, device=dev)).all())
    del rows0
    keys_a = torch.from_numpy(rng.integers(0, C, size=(B, Ls))).to(dev)
    rows_a = keys_a.to(torch.int32)
    kb = rng.integers(0, C, size=(B, Ls))
    miss = rng.random((B, Ls)) < 0.5
    kb[miss] += C                                                     # keys C .. 2 C - 1 are not in the map
    keys_b = torch.from_numpy(kb).to(dev)
    mask = torch.from_numpy((rng.random((B, Ls)) < 0.7).astype(np.float32)).to(dev)
    pooled = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    buf = torch.empty((B * Ls, D), dtype=torch.float32, device=dev)
    pos = torch.arange(B * Ls, dtype=torch.int32, device=dev).view(B, Ls)
    marker = torch.empty((1, 4), dtype=torch.float32, device=dev)
    dflt = (sigma, None, seed)

    def variant(name):
        if name == "a_plain":
            ops.gather_pool_fields(values, rows_a, lens, mask, mode="mean", out=pooled)
        elif name == "a_keyed":
            ops.gather_pool_fields_keyed(values, rows_a, keys_a, lens, mask, mode="mean", out=pooled, default=dflt)
        elif name == "b_comp":
            rows = index.lookup(keys_b, insert=False)
            ops.gather_rows(values, rows, out=buf)
            index.fill_missing(keys_b, rows, buf, sigma, None, seed)
            ops.gather_pool_fields(buf, pos, lens, mask, mode="mean", out=pooled)
        else:
            rows = index.lookup(keys_b, insert=False)
            ops.gather_pool_fields_keyed(values, rows.view(B, Ls), keys_b, lens, mask, mode="mean", out=pooled, default=dflt)

    results = {}
    for name in VARIANTS:                                             # warm-up, and: both sides of an arm give the same bits
        variant(name)
        results[name] = pooled.clone()
    torch.cuda.synchronize()
    same = {arm: bool(torch.equal(results[f"{arm}_{x}"].view(torch.int32), results[f"{arm}_keyed"].view(torch.int32)))
            for arm, x in (("a", "plain"), ("b", "comp"))}
    del results
    order = []
    for r in range(REPEATS):
        for q in range(len(VARIANTS)):
            name = VARIANTS[(r + q) % len(VARIANTS)]
            ops.fill_normal_(marker, seed=r, sigma=1.0)
            variant(name)
            order.append(name)
    ops.fill_normal_(marker, seed=99, sigma=1.0)
    torch.cuda.synchronize()
    need = B * Ls * D * 4 + B * F * D * 4 + B * Ls * 8                # rows read, pooled rows written, row numbers + mask read
    print(json.dumps(dict(shape=shape, capacity=C, D=D, L=list(lens), bags=B * F, missing=float(miss.mean()), bitwise_equal=same, order=order,
                          bytes_needed=need, variants=list(VARIANTS))))


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
    print(f"shape {lab['shape']}: capacity={lab['capacity']} D={lab['D']} L={lab['L']} bags={lab['bags']} missing in (b)={lab['missing']:.3f} "
          f"bitwise equal: {lab['bitwise_equal']}; sum of kernel times per repeat, us")
    for name in VARIANTS:
        x = per[name]
        print(f"  {name:8s} median {median(x):9.1f}  min {min(x):9.1f}  max {max(x):9.1f}  ({', '.join(f'{t:.1f}' for t in x)})")
        for k, ts in kernels[name].items():
            print(f"      {median(ts):9.1f} us x {len(ts) // len(x)}  {k}")
    ap, ak, bc, bk = (median(per[k]) for k in VARIANTS)
    inside = min(per["a_plain"]) <= ak <= max(per["a_plain"])
    print(f"  (a) keyed / plain = {ak / ap:.3f}: the keyed median {ak:.1f} lies {'INSIDE' if inside else 'OUTSIDE'} the plain kernel's own "
          f"min - max {min(per['a_plain']):.1f} - {max(per['a_plain']):.1f};  {lab['bytes_needed'] / 1e6:.1f} MB needed -> "
          f"{lab['bytes_needed'] / ak / 1e6:.3f} TB/s")
    print(f"  (b) keyed / composition = {bk / bc:.3f}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run" and sys.argv[2] in ("small", "large"):
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "reduce":
        reduce(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
