#!/usr/bin/env python3
"""The multitable Wide&Deep's input stage as one launch (ops.multitable_input, k_mt_input) against the same work composed from the
ops that existed before it, at the reference's layout: tables 650 000 x 128, 17 300 x 64, 20 900 x 64, 16 x 64; field counts 2 / 3 / 2,
bags (3, 5, 4, 3, 4, 2), 32 continuous values, B = 16384, fp16 rows (K0 = 1056).

  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/mt_input_bench.py run
  python tools/mt_input_bench.py reduce OUT/.../*kernel_trace.csv

The profiled run goes under a time limit, in a run of its own (no counters, no other tracing beside it); the library is built
beforehand -- the profiled command only runs -- with at most 16 build jobs on a shared machine.

run: REPEATS times in rotation, after a warm-up of each arm, (a) ops.multitable_input and (b) the composition: gather_rows x3 (fp16
rows), gather_pool_fields over the six fields' ids back to back (mean, fp16), the cast of the continuous values and the cat of the
five parts; wide_sum x3 and gather_pool (sum, D = 1) for the four dim-1 lookups.  What (b) leaves out -- the continuous values' dot
product with wide_continue_w, the adds of the five wide parts and the bias -- would be torch arithmetic on top: (b) is a lower bound
of the composition.  Ids are uniform over each table (no hot rows: the large table's rows come from HBM) and are made on the host, the
tables are filled by k_fill_normal, so every other kernel in the trace belongs to (b).  Both arms are compared before timing: the
deep rows bit for bit.
reduce: from the kernel trace, with the warm-up call of each arm dropped: k_mt_input's median (min, max) duration over the REPEATS
calls, the summed medians of (b)'s kernels per repeat; the bytes the launch has to move in all (mostly rows of cache-resident tables)
with their rate, and the bytes that have to cross HBM -- the large table's rows, the row written, ids, masks and continuous values
once -- as a fraction of 8 TB/s; one JSON line.  DESIGN.md section 6, "Multitable Wide&Deep"."""
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 20
B, BAGS, N_IND, N_128, N_64, C = 16384, (3, 5, 4, 3, 4, 2), 2, 3, 2, 32
TABLES = {"emb128": (650000, 128), "single": (17300, 64), "multi": (20900, 64), "ind": (16, 64)}
K0 = C + N_IND * 64 + N_128 * 128 + N_64 * 64 + len(BAGS) * 64


def bytes_moved():
    """what one call has to read and write: every looked-up row once (no reuse assumed), ids, masks, wide weights, the continuous values,
    the fp16 row and the wide term"""
    slots = {"ind": N_IND, "emb128": N_128, "single": N_64, "multi": sum(BAGS)}
    rows = sum(n * TABLES[k][1] * 4 for k, n in slots.items())
    ids = sum(slots.values()) * 4 * 2                       # the deep item and the wide sum read them
    mask = sum(BAGS) * 4 * 2
    wide = sum(slots.values()) * 4
    return B * (rows + ids + mask + wide + C * 4 * 2 + K0 * 2 + 4)


def bytes_hbm():
    """the part of bytes_moved() that has to cross HBM: the rows of the one table that is not cache resident (650 000 x 128), the fp16
    row and the wide term written, and ids, masks and continuous values once (their second read hits cache); the three small tables
    and the wide weights stay resident from call to call"""
    slots = N_IND + N_128 + N_64 + sum(BAGS)
    return B * (N_128 * TABLES["emb128"][1] * 4 + K0 * 2 + 4 + slots * 4 + sum(BAGS) * 4 + C * 4)


def run():
    import numpy as np
    import torch
    from mindrec_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    t, w = {}, {}
    for i, (k, (V, D)) in enumerate(TABLES.items()):
        t[k] = ops.fill_normal_(torch.empty((V, D), device=dev), seed=i)
        w[k] = ops.fill_normal_(torch.empty((V, 1), device=dev), seed=10 + i)
    up = lambda a: torch.from_numpy(a).to(dev)
    cont = up(rng.random((B, C)).astype(np.float32))
    wc, wb = up(rng.standard_normal(C).astype(np.float32)), up(np.zeros(1, np.float32))
    ids = {"ind": up(rng.integers(0, 16, (B, N_IND)).astype(np.int32)), "emb128": up(rng.integers(0, 650000, (B, N_128)).astype(np.int32)),
           "single": up(rng.integers(0, 17300, (B, N_64)).astype(np.int32))}
    ones = {k: up(np.ones(tuple(v.shape), np.float32)) for k, v in ids.items()}
    mids = up(rng.integers(0, 20900, (B, sum(BAGS))).astype(np.int32))
    mmask = up((rng.random((B, sum(BAGS))) < 0.7).astype(np.float32))
    segs, col = [], C
    for k in ("ind", "emb128", "single"):
        segs.append(ops.MtSegment(t[k], ids[k], col, False, None, w[k].view(-1)))
        col += segs[-1].width
    off = 0
    for L in BAGS:                                          # the six fields: separate descriptors over column slices of the one array
        segs.append(ops.MtSegment(t["multi"], mids[:, off:off + L], col, True, mmask[:, off:off + L], w["multi"].view(-1)))
        col, off = col + 64, off + L
    x = torch.empty((B, K0), dtype=torch.float16, device=dev)
    wide = torch.empty(B, device=dev)

    def fused():
        return ops.multitable_input(cont, wc, wb, segs, K0=K0, out=x, wide_out=wide)

    def composed():
        parts = [cont.to(torch.float16)] + [ops.gather_rows(t[k], ids[k], out_dtype=torch.float16).view(B, -1) for k in ("ind", "emb128", "single")]
        parts.append(ops.gather_pool_fields(t["multi"], mids, BAGS, mmask, mode="mean", out_dtype=torch.float16))
        ws = [ops.wide_sum(w[k], ids[k], ones[k]) for k in ("ind", "emb128", "single")]
        ws.append(ops.gather_pool(w["multi"], mids, mmask, mode="sum"))
        return torch.cat(parts, dim=1), ws

    a, _ = fused()
    b, _ = composed()
    torch.cuda.synchronize()
    assert torch.equal(a, b), "the two arms differ"
    for _ in range(REPEATS):
        fused()
        composed()
    torch.cuda.synchronize()
    print(json.dumps({"B": B, "K0": K0, "repeats": REPEATS + 1, "bytes": bytes_moved()}))


def reduce(path):
    import statistics
    calls = {}                                                  # kernel name -> durations in dispatch order, us
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        calls.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    one = [k for k in calls if "k_mt_input" in k]
    assert len(one) == 1 and len(calls[one[0]]) == REPEATS + 1, {k: len(v) for k, v in calls.items()}
    fused = calls[one[0]][1:]                                   # (the first call of each arm is its warm-up)
    comp = {}
    for k, d in calls.items():
        # (b)'s kernels run once or three times per repeat; the set-up's and the comparison's run fewer times than there are repeats
        if k in one or "k_fill_normal" in k or len(d) < REPEATS + 1:
            continue
        per = len(d) // (REPEATS + 1)
        comp[k[:60]] = [per, round(statistics.median(d[per:]) * per, 2)]
    fused_us, by, hb = statistics.median(fused), bytes_moved(), bytes_hbm()
    print(json.dumps({"mt_input_us": round(fused_us, 2), "mt_input_min_max_us": [round(min(fused), 2), round(max(fused), 2)],
                      "composition_us": round(sum(v[1] for v in comp.values()), 2), "composition_kernels": comp, "repeats": REPEATS,
                      "bytes": by, "tb_per_s": round(by / fused_us / 1e6, 3), "hbm_bytes": hb, "hbm_tb_per_s": round(hb / fused_us / 1e6, 3),
                      "hbm_fraction_of_8_tb_s": round(hb / fused_us / 1e6 / 8.0, 3)}))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "reduce":
        reduce(sys.argv[2])
    else:
        sys.exit(__doc__)
