#!/usr/bin/env python3
"""The multi-hot path against the composition it replaces, kernel time by kernel time ("multi-hot fields").

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/pool_bench.py run SHAPE > OUT/labels.json
  python tools/pool_bench.py reduce OUT/labels.json <the run's *_kernel_trace.csv>

`run` issues, five times each and in rotation, the four variants at one shape, every repeat behind a marker launch (a one-row
k_fill_normal), and prints the order of the repeats; `reduce` cuts the trace's dispatches (in start order) at the markers and adds
up the kernel times of every repeat.  Nothing is timed on the host.
  fwd_pool   ops.gather_pool (mean)                                       -- one kernel
  fwd_comp   the composition available without it: ops.gather_rows into [B*F*L, D] with the mask as row_scale, torch sum over the
             bag axis, torch divide by L
  bwd_pool   ops.sparse_lazy_adam_(pool=L) on dy [B*F, D]
  bwd_comp   dy expanded to [B*F*L, D] (torch repeat_interleave) + the plain ops.sparse_lazy_adam_
The plan of the ids is built once, outside the repeats: both backward variants take the same one.
SHAPE: "ref" = V 20 900, D 64, B 131 072, F 6, L 8, Zipf-like ids (the reference's multi-hot table; L stands in for its
dataset's bag lengths); "large" = V 20 000 000, D 64, B*F 786 432 bags, L 8, uniform ids (rows do not sit in cache).

The FIELDS form (bags of unequal length: fields (3, 5, 4, 3, 4, 2) of one table, B 131 072, D 64) against what it replaces:

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/pool_bench.py run fields-ref > OUT/labels.json   (or fields-large)
  python tools/pool_bench.py reduce OUT/labels.json <the run's *_kernel_trace.csv>

  fwd_fields  ops.gather_pool_fields on the [B, 21] ids                    -- one kernel
  fwd_perlen  the composition available without it: one ops.gather_pool per DISTINCT length (fields of a length gathered into a
              [B, k, L] batch -- the gather copies are part of its cost), results written to their column blocks
  fwd_padded  every field padded to the longest bag (mask 0 in the padding), one ops.gather_pool at L = 5: cheaper to call, and
              WRONG for the mean (it divides by 5, not by L_f) -- a lower-cost comparison point, not an alternative
  bwd_fields  ONE ops.sparse_plan over the B * 21 ids + ONE ops.sparse_lazy_adam_(fields=...)
  bwd_perlen  per distinct length: gather its ids, ops.sparse_plan, ops.sparse_lazy_adam_(pool=L) -- four plans and four applies over
              the same table (and an id that occurs under two lengths is updated twice: not the reference's result either)
  bwd_padded  one plan over the B * 6 * 5 padded ids + one ops.sparse_lazy_adam_(pool=5) (wrong scale for the mean, as above)
Here the plans are INSIDE the repeats: planning once instead of once per length is part of what the fields form changes.
"fields-ref" = V 20 900, Zipf-like ids; "fields-large" = V 20 000 000, uniform ids.

max_norm over the fields form (every looked-up row clipped before its mask product, the apply through the clip's Jacobian), at the
same two shapes, c = the median row norm of the table so that both branches run:

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/pool_bench.py run clip-fields-ref > OUT/labels.json   (or clip-fields-large)
  python tools/pool_bench.py reduce OUT/labels.json <the run's *_kernel_trace.csv>

  fwd_fields     ops.gather_pool_fields, no clip                              -- what the clip costs on top of
  fwd_clip       ops.gather_pool_fields(max_norm=c)                           -- one kernel
  fwd_clip_comp  the composition it replaces: ops.gather_rows(max_norm=c) into [B * 21, D] with the mask as row_scale, then a torch
                 sum over each field's slots and a divide by L_f into its column block
  bwd_fields     ops.sparse_lazy_adam_(fields=...), no clip
  bwd_clip       ops.sparse_lazy_adam_(fields=..., pool_max_norm=c)
  bwd_clip_comp  the composition it replaces: dy expanded to [B * 21, D] (index_select by the position's bag), row_scale = mask / L_f,
                 then the plain clipped ops.sparse_lazy_adam_(max_norm=c)
The plan is built once, outside the repeats: all three backward variants take the same one."""
import csv
import json
import os
import sys
from statistics import median

REPEATS = 5
VARIANTS = ("fwd_comp", "fwd_pool", "bwd_comp", "bwd_pool")
FIELD_VARIANTS = ("fwd_perlen", "fwd_fields", "fwd_padded", "bwd_perlen", "bwd_fields", "bwd_padded")
CLIP_VARIANTS = ("fwd_fields", "fwd_clip", "fwd_clip_comp", "bwd_fields", "bwd_clip", "bwd_clip_comp")
FIELDS = (3, 5, 4, 3, 4, 2)


def _setup(shape, id_shape, dy_shape):
    """what both forms measure on: the table (V 20 900 and Zipf-like ids for "ref" / "fields-ref", else V 20 000 000 and uniform ids),
    its LazyAdam state, ids and a 0/1 mask of id_shape, the pooled rows' gradient, and the one-row tensor of the marker launches"""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from mindrec_amd import ops
    dev = torch.device("cuda:0")
    ref = shape in ("ref", "fields-ref", "clip-fields-ref")
    V = 20900 if ref else 20_000_000
    rng = np.random.default_rng(7)
    if ref:
        ids = np.minimum(rng.zipf(1.2, size=id_shape) - 1, V - 1).astype(np.int32)
    else:
        ids = rng.integers(0, V, size=id_shape).astype(np.int32)
    tid = torch.from_numpy(ids).to(dev)
    mask = torch.from_numpy((rng.random(id_shape) < 0.7).astype(np.float32)).to(dev)
    table = torch.empty((V, 64), dtype=torch.float32, device=dev)
    ops.fill_normal_(table, seed=1, sigma=0.01)
    m, v = torch.zeros_like(table), torch.zeros_like(table)
    dy = torch.from_numpy(rng.standard_normal(dy_shape).astype(np.float32)).to(dev)
    marker = torch.empty((1, 4), dtype=torch.float32, device=dev)
    return ops, torch, V, tid, mask, table, m, v, dy, marker


def _rotate(ops, torch, marker, variants, variant):
    """every variant once (warm-up: code objects, workspaces, the allocator), then REPEATS rounds of all of them in rotation, each
    repeat behind a marker launch; returns the order of the repeats"""
    for name in variants:
        variant(name)
    torch.cuda.synchronize()
    order = []
    for r in range(REPEATS):
        for q in range(len(variants)):
            name = variants[(r + q) % len(variants)]
            ops.fill_normal_(marker, seed=r, sigma=1.0)
            variant(name)
            order.append(name)
    ops.fill_normal_(marker, seed=99, sigma=1.0)
    torch.cuda.synchronize()
    return order


def run_fields(shape):
    D, B, lens = 64, 131072, FIELDS
    F, Ls, Lmax = len(lens), sum(lens), max(lens)
    ops, torch, V, tid, mask, table, m, v, dy, marker = _setup(shape, (B, Ls), (B, F * D))
    dev = table.device
    pooled = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    offs = [sum(lens[:f]) for f in range(F)]
    by_len = {}                                   # distinct length -> its fields
    for f, L in enumerate(lens):
        by_len.setdefault(L, []).append(f)
    slots = {L: torch.tensor([offs[f] + l for f in fs for l in range(L)], device=dev) for L, fs in by_len.items()}
    cols = {L: torch.tensor([f * D + c for f in fs for c in range(D)], device=dev) for L, fs in by_len.items()}
    pad_slots = torch.tensor([offs[f] + min(l, L - 1) for f, L in enumerate(lens) for l in range(Lmax)], device=dev)
    pad_keep = torch.tensor([1.0 if l < L else 0.0 for L in lens for l in range(Lmax)], device=dev)
    akw = dict(beta1_power=0.9, beta2_power=0.999)

    def variant(name):
        if name == "fwd_fields":
            ops.gather_pool_fields(table, tid, lens, mask, mode="mean", out=pooled)
        elif name == "fwd_perlen":
            for L, fs in by_len.items():
                k = len(fs)
                x = ops.gather_pool(table, tid[:, slots[L]].view(B, k, L), mask[:, slots[L]].view(B, k, L), mode="mean")
                if k == 1:
                    pooled[:, fs[0] * D:(fs[0] + 1) * D] = x.view(B, D)
                else:
                    pooled[:, cols[L]] = x.view(B, k * D)
        elif name == "fwd_padded":
            ops.gather_pool(table, tid[:, pad_slots].view(B, F, Lmax), (mask[:, pad_slots] * pad_keep).view(B, F, Lmax), mode="mean",
                            out=pooled.view(B * F, D))
        elif name == "bwd_fields":
            plan = ops.sparse_plan(tid)
            ops.sparse_lazy_adam_(table, m, v, plan, dy, mask, fields=lens, field_scale=tuple(1.0 / L for L in lens), **akw)
        elif name == "bwd_perlen":
            for L, fs in by_len.items():
                k = len(fs)
                plan = ops.sparse_plan(tid[:, slots[L]].contiguous())
                g = dy[:, cols[L]].contiguous() if k > 1 else dy[:, fs[0] * D:(fs[0] + 1) * D].contiguous()
                ops.sparse_lazy_adam_(table, m, v, plan, g.view(B * k, D), mask[:, slots[L]].contiguous(), pool=L, grad_scale=1.0 / L, **akw)
        else:
            plan = ops.sparse_plan(tid[:, pad_slots].contiguous())
            ops.sparse_lazy_adam_(table, m, v, plan, dy.view(B * F, D), (mask[:, pad_slots] * pad_keep).contiguous(), pool=Lmax,
                                  grad_scale=1.0 / Lmax, **akw)

    order = _rotate(ops, torch, marker, FIELD_VARIANTS, variant)
    need_fwd = B * Ls * D * 4 + B * F * D * 4 + B * Ls * 8          # rows read, pooled rows written, ids + mask read
    print(json.dumps(dict(shape=shape, V=V, D=D, L=list(lens), bags=B * F, warmup_markers=0, order=order, fwd_bytes_needed=need_fwd,
                          variants=list(FIELD_VARIANTS))))


def run_clip(shape):
    D, B, lens = 64, 131072, FIELDS
    F, Ls = len(lens), sum(lens)
    ops, torch, V, tid, mask, table, m, v, dy, marker = _setup(shape, (B, Ls), (B, F * D))
    dev = table.device
    c = float(table[:65536].norm(dim=1).median())            # the median row norm: half of the rows are clipped
    pooled = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    rows = torch.empty((B * Ls, D), dtype=torch.float32, device=dev)
    offs = [sum(lens[:f]) for f in range(F)]
    fs = tuple(1.0 / L for L in lens)
    slot_field = torch.tensor([f for f, L in enumerate(lens) for _ in range(L)], device=dev)
    bag_row = (torch.arange(B, device=dev).view(B, 1) * F + slot_field.view(1, Ls)).reshape(-1)      # position -> its bag's gradient row
    slot_scale = torch.tensor([fs[f] for f, L in enumerate(lens) for _ in range(L)], dtype=torch.float32, device=dev)
    plan = ops.sparse_plan(tid)
    akw = dict(beta1_power=0.9, beta2_power=0.999)

    def variant(name):
        if name == "fwd_fields":
            ops.gather_pool_fields(table, tid, lens, mask, mode="mean", out=pooled)
        elif name == "fwd_clip":
            ops.gather_pool_fields(table, tid, lens, mask, mode="mean", out=pooled, max_norm=c)
        elif name == "fwd_clip_comp":
            ops.gather_rows(table, tid, mask, out=rows, max_norm=c)
            r3 = rows.view(B, Ls, D)
            for f, L in enumerate(lens):
                blk = pooled[:, f * D:(f + 1) * D]
                torch.sum(r3[:, offs[f]:offs[f] + L], dim=1, out=blk)
                blk.div_(float(L))
        elif name == "bwd_fields":
            ops.sparse_lazy_adam_(table, m, v, plan, dy, mask, fields=lens, field_scale=fs, **akw)
        elif name == "bwd_clip":
            ops.sparse_lazy_adam_(table, m, v, plan, dy, mask, fields=lens, field_scale=fs, pool_max_norm=c, **akw)
        else:
            big = dy.view(B * F, D).index_select(0, bag_row)
            rs = (mask * slot_scale).view(-1)
            ops.sparse_lazy_adam_(table, m, v, plan, big, rs, max_norm=c, **akw)

    order = _rotate(ops, torch, marker, CLIP_VARIANTS, variant)
    need_fwd = B * Ls * D * 4 + B * F * D * 4 + B * Ls * 8          # rows read, pooled rows written, ids + mask read
    print(json.dumps(dict(shape=shape, V=V, D=D, L=list(lens), bags=B * F, warmup_markers=0, order=order, fwd_bytes_needed=need_fwd,
                          variants=list(CLIP_VARIANTS), max_norm=c)))


def run(shape):
    if shape.startswith("clip-fields-"):
        return run_clip(shape)
    if shape.startswith("fields-"):
        return run_fields(shape)
    D, L, bags = 64, 8, 131072 * 6
    ops, torch, V, tid, mask, table, m, v, dy, marker = _setup(shape, (bags, L), (bags, D))
    plan = ops.sparse_plan(tid)
    rows = torch.empty((bags * L, D), dtype=torch.float32, device=table.device)
    pooled = torch.empty((bags, D), dtype=torch.float32, device=table.device)
    kw = dict(beta1_power=0.9, beta2_power=0.999, grad_scale=1.0 / L)

    def variant(name):
        if name == "fwd_pool":
            ops.gather_pool(table, tid, mask, mode="mean", out=pooled)
        elif name == "fwd_comp":
            ops.gather_rows(table, tid, mask, out=rows)
            torch.sum(rows.view(bags, L, D), dim=1, out=pooled)
            pooled.div_(float(L))
        elif name == "bwd_pool":
            ops.sparse_lazy_adam_(table, m, v, plan, dy, mask, pool=L, **kw)
        else:
            big = dy.repeat_interleave(L, 0)
            ops.sparse_lazy_adam_(table, m, v, plan, big, mask, **kw)

    order = _rotate(ops, torch, marker, VARIANTS, variant)
    need_fwd = bags * L * D * 4 + bags * D * 4 + bags * L * 8          # rows read, pooled rows written, ids + mask read
    print(json.dumps(dict(shape=shape, V=V, D=D, L=L, bags=bags, warmup_markers=0, order=order, fwd_bytes_needed=need_fwd)))


def reduce(labels_path, trace_path):
    lab = json.load(open(labels_path))
    rows = list(csv.DictReader(open(trace_path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "k_fill_normal" in r["Kernel_Name"]]
    order = lab["order"]
    marks = marks[-(len(order) + 1):]         # (the table's own initialisation is the first k_fill_normal of the run)
    assert len(marks) == len(order) + 1, (len(marks), len(order))
    variants = tuple(lab.get("variants", VARIANTS))
    per = {k: [] for k in variants}
    kernels = {k: {} for k in variants}
    for j, name in enumerate(order):
        seg = rows[marks[j] + 1: marks[j + 1]]
        per[name].append(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in seg) / 1e3)
        for r in seg:
            k = r["Kernel_Name"].replace("(anonymous namespace)::", "")[:90]
            kernels[name].setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"shape {lab['shape']}: V={lab['V']} D={lab['D']} L={lab['L']} bags={lab['bags']}; sum of kernel times per repeat, us")
    for name in variants:
        x = per[name]
        print(f"  {name:9s} median {median(x):9.1f}  min {min(x):9.1f}  max {max(x):9.1f}  spread {100 * (max(x) - min(x)) / median(x):5.1f} %  ({', '.join(f'{t:.1f}' for t in x)})")
        for k, ts in kernels[name].items():
            print(f"      {median(ts):9.1f} us x {len(ts) // len(x)}  {k}")
    if "fwd_clip" in per:
        ff, fc, fcc, bf, bc, bcc = (median(per[k]) for k in CLIP_VARIANTS)
        print(f"  max_norm = {lab['max_norm']:.6f}")
        print(f"  forward  clip / plain pooled = {fc / ff:.3f};  clip / composition = {fc / fcc:.3f};  needed bytes "
              f"{lab['fwd_bytes_needed'] / 1e6:.1f} MB -> {lab['fwd_bytes_needed'] / fc / 1e6:.3f} TB/s")
        print(f"  backward clip / plain pooled = {bc / bf:.3f};  clip / composition = {bc / bcc:.3f}")
        return
    if "fwd_fields" in per:
        ff, fl, fpad, bf, bl, bpad = (median(per[k]) for k in ("fwd_fields", "fwd_perlen", "fwd_padded", "bwd_fields", "bwd_perlen", "bwd_padded"))
        print(f"  forward  fields / per-length = {ff / fl:.3f};  fields / padded (wrong mean) = {ff / fpad:.3f};  needed bytes "
              f"{lab['fwd_bytes_needed'] / 1e6:.1f} MB -> {lab['fwd_bytes_needed'] / ff / 1e6:.3f} TB/s")
        print(f"  backward (plan + apply) fields / per-length = {bf / bl:.3f};  fields / padded (wrong mean) = {bf / bpad:.3f}")
        return
    fp, fc, bp, bc = (median(per[k]) for k in ("fwd_pool", "fwd_comp", "bwd_pool", "bwd_comp"))
    print(f"  forward  pooled / composition = {fp / fc:.3f};  needed bytes {lab['fwd_bytes_needed'] / 1e6:.1f} MB -> {lab['fwd_bytes_needed'] / fp / 1e6:.3f} TB/s "
          f"= {100 * lab['fwd_bytes_needed'] / fp / 1e6 / 8.0:.1f} % of 8 TB/s")
    print(f"  backward pooled / composition = {bp / bc:.3f}")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "reduce":
        reduce(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
