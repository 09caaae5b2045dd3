"""The dequantizing lookup over row-wise 8-bit records (ops.gather_rows_q8, compact and 128-byte records) and over row-wise 4-bit
records (ops.gather_rows_q4, compact 64-byte and 128-byte records) against the fp32 folded lookup (ops.gather_rows_wide over fused
training rows) on the same ids, all arms in one rotation, and the two quantize passes over the same table.

    python tools/q8_lookup_bench.py [vocab] [blocks] [calls]

Benchmark shape: 16384 x 39 positions, D = 80, vocabulary 2e7 (fused rows: 20 GB), fp16 rows, uniform ids and the benchmark's Zipf
stream.  Each arm is warmed, then timed as `blocks` blocks of `calls` calls between two device events, the arms alternating in
rotation; one JSON line per id distribution with the median (min, max) microseconds per call and the GB/s that implies against the
arm's algorithmic bytes per position: the record or the 336 bytes of the fp32 row, the fp16 output row, the 8-byte wide pair, id and
weight.  The quantize pass is timed the same way (read 4 D + 4, write row_bytes per row).  Then DeepFM's evaluation lookup over the same
16384 x 39 ids, four arms timed the same way: ops.fm_lookup_q8 over the compact 8-bit records, ops.fm_lookup_q4 over the compact 4-bit
records, the composition the former replaces (ops.gather_rows_q8 into fp32 rows, then ops.fm_forward with the 16-bit copy; without the
linear sum) and ops.fm_lookup over contiguous fp32 tables."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(arms, blocks, calls):
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(blocks):
        for k, f in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / calls)
    return {k: sorted(v) for k, v in us.items()}


def _line(us, nbytes):
    med = us[len(us) // 2]
    return {"us": round(med, 2), "min": round(us[0], 2), "max": round(us[-1], 2), "GB/s": round(nbytes / med / 1e3, 1)}


def main():
    from mindrec_amd import ops
    from mindrec_amd.wide_deep import WideDeepConfig, synthetic_batch
    V = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20_000_000
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    dev = torch.device("cuda:0")
    D, B, F = 80, 16384, 39
    ld = -(-(3 * D + 4) // 32) * 32
    state = torch.zeros((V, ld), dtype=torch.float32, device=dev)
    deep, wide = state[:, :D], state[:, D:D + 1]
    ops.fill_normal_(deep, 1000)
    ops.fill_normal_(wide, 1001)
    compact = ops.q8_row_bytes(D)
    q8 = {rb: ops.quantize_rows_q8(deep, wide, row_bytes=rb) for rb in (compact, 128)}
    q4 = {rb: ops.quantize_rows_q4(deep, wide, row_bytes=rb) for rb in (ops.q4_row_bytes(D), 128)}
    n = B * F
    for bits, quantize, tables in ((8, ops.quantize_rows_q8, q8), (4, ops.quantize_rows_q4, q4)):
        for rb, t in tables.items():
            us = _time({"q": lambda t=t, rb=rb: quantize(deep, wide, row_bytes=rb, out=t.records)}, max(blocks // 3, 3), 2)["q"]
            print(json.dumps({"what": "quantize", "bits": bits, "V": V, "row_bytes": rb, **_line(us, V * (4 * D + 4 + rb))}), flush=True)
    cfg = WideDeepConfig(vocab_size=V, emb_dim=D, field_size=F, batch_size=B)
    for dist in ("uniform", "zipf"):
        ids, wts, _ = synthetic_batch(cfg, dev, dist, seed=1000)
        out = torch.empty((n, D), dtype=torch.float16, device=dev)
        arms = {"fp32_folded": lambda: ops.gather_rows_wide(deep, ids, wts, D, out=out, out_dtype=torch.float16)}
        for rb, t in q8.items():
            arms[f"q8_{rb}"] = lambda t=t: ops.gather_rows_q8(t, ids, wts, out=out)
        for rb, t in q4.items():
            arms[f"q4_{rb}"] = lambda t=t: ops.gather_rows_q4(t, ids, wts, out=out)
        us = _time(arms, blocks, calls)
        common = 2 * D + 8 + 4 + 4
        res = {"fp32_folded": _line(us["fp32_folded"], n * (4 * D + 16 + common))}
        for rb in q8:
            res[f"q8_{rb}"] = _line(us[f"q8_{rb}"], n * (rb + common))
        for rb in q4:
            res[f"q4_{rb}"] = _line(us[f"q4_{rb}"], n * (rb + common))
        print(json.dumps({"what": "lookup", "ids": dist, "positions": n, "V": V, **res}), flush=True)
    # DeepFM's evaluation lookup: (i) the one launch over records, (ii) the composition it replaces -- q8 gather to fp32 rows (no wide
    # pair), then the FM kernel with the 16-bit copy; its linear sum is missing, which favours it --, (iii) ops.fm_lookup over DeepFM's own
    # contiguous fp32 [V, D] and [V, 1] tables (the same values the records were made from)
    t, t4 = q8[compact], q4[ops.q4_row_bytes(D)]
    Vc, Wc = deep.contiguous(), wide.contiguous()
    rows32 = torch.empty((B, F, D), dtype=torch.float32, device=dev)
    rows16 = torch.empty((B, F, D), dtype=torch.float16, device=dev)
    lin0 = torch.zeros(B, dtype=torch.float32, device=dev)
    o_q8, o_q4, o_fm, o_f32 = {}, {}, {}, {}
    for dist in ("uniform", "zipf"):
        ids, wts, _ = synthetic_batch(cfg, dev, dist, seed=1000)

        def composed():
            ops.gather_rows_q8(t, ids, wts, out=rows32, wide=False)
            ops.fm_forward(rows32, add=lin0, out16=rows16, out=o_fm)
        us = _time({"fm_q8": lambda: ops.fm_lookup_q8(t, ids, wts, out=o_q8), "fm_q4": lambda: ops.fm_lookup_q4(t4, ids, wts, out=o_q4),
                    "q8_gather+fm_forward": composed,
                    "fm_fp32": lambda: ops.fm_lookup(Vc, Wc, ids, wts, out=o_f32)}, blocks, calls)
        per = 4 + 4 + 2 * D                             # id, weight and the fp16 row of a position
        res = {"fm_q8": _line(us["fm_q8"], n * (compact + per) + 4 * B), "fm_q4": _line(us["fm_q4"], n * (t4.row_bytes + per) + 4 * B),
               "q8_gather+fm_forward": _line(us["q8_gather+fm_forward"], n * (compact + 8 + 4 * D) + n * (4 * D + 2 * D) + B * (8 + 4 * D)),
               "fm_fp32": _line(us["fm_fp32"], n * (4 * D + 4 + per) + 4 * B)}
        same = torch.equal(o_q8["rows"].view(torch.int16), rows16.view(torch.int16))       # the two q8 arms round the same fp32 values once
        same4 = torch.equal(o_q4["rows"].view(torch.int16), ops.gather_rows_q4(t4, ids, wts, wide=False)[0].view(torch.int16))
        print(json.dumps({"what": "fm_lookup", "ids": dist, "samples": B, "fields": F, "V": V, "q8_rows_equal": same, "q4_rows_equal": same4,
                          **res}), flush=True)


def keyed(n, blocks, calls):
    """python tools/q8_lookup_bench.py keyed [live keys] [blocks] [calls] -- DeepFM's evaluation lookup over HASH tables of n live int64
    keys, 16384 x 39 positions of which ~1 % hold a key the tables have not seen, D = 80, fp16 rows; per bit width (i) the keyed one-launch
    lookup over records, (ii) FrozenKeyIndex.find, then the unkeyed lookup over those rows, and once (iii) the key path of
    DeepFMHashEngine.predict_fused -- Unique, the two MapParameter lookups (inserting), ops.fm_lookup over the fp32 values (the tables here
    carry no optimizer slots, which favours it).  All arms in one rotation; one JSON line per key distribution."""
    import numpy as np
    from mindrec_amd import ops
    from mindrec_amd.experimental import MapParameter
    dev = torch.device("cuda:0")
    D, B, F = 80, 16384, 39
    keys_all = torch.arange(n, dtype=torch.int64, device=dev) * -7046029254386353131 + 3            # (an odd multiplier: n distinct keys)
    table = torch.empty((n, D), dtype=torch.float32, device=dev)
    wide = torch.empty((n, 1), dtype=torch.float32, device=dev)
    ops.fill_normal_(table, 1000)
    ops.fill_normal_(wide, 1001)
    q = {8: ops.quantize_rows_q8(table, wide), 4: ops.quantize_rows_q4(table, wide)}
    kidx = ops.FrozenKeyIndex(keys_all)
    del table, wide
    mk = dict(key_dtype=torch.int64, default_value="normal", capacity=n + 2 * B * F, device=dev)
    Vm, Wm = MapParameter(value_shape=(D,), name="V", seed=1000, **mk), MapParameter(value_shape=(1,), name="W", seed=1001, **mk)
    for c in range(0, n, 1 << 21):
        for m in (Vm, Wm):
            m.lookup_rows(keys_all[c: c + (1 << 21)], insert=True)
    torch.cuda.synchronize()
    print(json.dumps({"what": "frozen_index", "n": n, "slots": kidx.n_slots, "bytes_per_key": round(16 * kidx.n_slots / n, 1),
                      "max_probe": kidx.max_probe(), "record_bytes": {b: t.row_bytes for b, t in q.items()}}), flush=True)
    rng = np.random.default_rng(1000)
    out = {a: {} for a in ("k8", "f8", "k4", "f4")}
    for dist in ("uniform", "zipf"):
        pick = rng.integers(0, n, (B, F)) if dist == "uniform" else np.minimum(rng.zipf(1.05, (B, F)) + 12, n - 1)
        kb = keys_all[torch.from_numpy(pick).to(dev)]
        kb = torch.where(torch.from_numpy(rng.random((B, F)) < 0.01).to(dev), kb + 1, kb)
        wts = torch.from_numpy(rng.random((B, F), dtype=np.float32)).to(dev)

        def live():
            flat = kb.view(-1)
            d = ops.unique(flat)
            pv, pw = (m.lookup_rows(flat, insert=True, dedup=d)[2].view(B, F) for m in (Vm, Wm))
            ops.fm_lookup(Vm.values, Wm.values, pv, wts, ids_w=pw, out_dtype=torch.float16)
        arms = {"live_maps": live}
        for b, keyed_op, plain in ((8, ops.fm_lookup_q8_keyed, ops.fm_lookup_q8), (4, ops.fm_lookup_q4_keyed, ops.fm_lookup_q4)):
            arms[f"q{b}_keyed"] = lambda b=b, f=keyed_op: f(q[b], kidx, kb, wts, out=out[f"k{b}"])
            arms[f"q{b}_find+lookup"] = lambda b=b, f=plain: f(q[b], kidx.find(kb), wts, out=out[f"f{b}"])
        us = _time(arms, blocks, calls)
        same = all(torch.equal(out[f"k{b}"][k].view(torch.int16), out[f"f{b}"][k].view(torch.int16)) for b in (8, 4) for k in ("rows", "lin_fm"))
        res = {k: {"us": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)} for k, v in us.items()}
        print(json.dumps({"what": "fm_lookup_keyed", "keys": dist, "samples": B, "fields": F, "n": n, "keyed_equals_find_then_lookup": same, **res}),
              flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "keyed":
        a = sys.argv[2:]
        keyed(int(float(a[0])) if a else 20_000_000, int(a[1]) if len(a) > 1 else 9, int(a[2]) if len(a) > 2 else 20)
    else:
        main()
