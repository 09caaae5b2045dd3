"""The multi-hot lookup served from row-wise 8-bit records (serving.MultiHotQ8 with wide=True: ops.gather_pool_fields_q8, ONE launch for the
pooled rows and the wide sum; compact and 128-byte records) and from compact row-wise 4-bit records (ops.gather_pool_fields_q4: 48 bytes
an id at D = 64 against 80) against MultiHotWideDeep.lookup over the fp32 tables (its two launches) on the same ids and mask.

    python tools/q8_pool_bench.py [blocks] [calls]

Shape: the reference's multi-hot fields -- B = 16384, bag = (3, 5, 4, 3, 4, 2), D = 64, fp32 outputs, uniform ids -- over its own table
(V = 20 900, cache-resident) and over V = 2e7.  The protocol is tools/q8_lookup_bench.py's: every arm warmed, then `blocks` blocks of
`calls` calls between two device events, the arms alternating in rotation; one JSON line per vocabulary with the median (min, max)
microseconds per call and the GB/s that implies against the arm's own algorithmic bytes per sample (duplicates not discounted): Ls
records -- or Ls fp32 rows and wide weights, with the ids and the mask read by both launches --, ids and mask in, the [F * D] row and
the wide sum out.  The line also carries the largest |x_q8 - x_fp32| and |w_q8 - w_fp32| at that size, and the largest |x_q4 - x_fp32|."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from q8_lookup_bench import _line, _time      # noqa: E402  (the sibling tool: the timing protocol)


def main():
    from mindrec_amd.multi_hot import MultiHotWideDeep
    blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    B, bag, D = 16384, (3, 5, 4, 3, 4, 2), 64
    F, Ls = len(bag), sum(bag)
    gen = torch.Generator(device=dev).manual_seed(1000)
    mask = torch.rand((B, Ls), device=dev, generator=gen)
    for V in (20_900, 20_000_000):
        pair = MultiHotWideDeep(vocab=V, dim=D, bag=bag, mode="mean", device=dev)
        ids = torch.randint(0, V, (B, Ls), device=dev, generator=gen, dtype=torch.int32)
        q8 = {rb: pair.freeze_q8(row_bytes=rb) for rb in (None, 128)}
        q4 = pair.freeze_q8(bits=4)
        outs = {k: (torch.empty((B, F * D), device=dev), torch.empty((B,), device=dev)) for k in ("fp32", None, 128, "q4")}
        arms = {"fp32_two_launches": lambda: pair.lookup(ids, mask, out=outs["fp32"][0], wide_out=outs["fp32"][1])}
        for rb, t in q8.items():
            arms[f"q8_{t.q8.row_bytes}"] = lambda t=t, rb=rb: t.lookup(ids, mask, out=outs[rb][0], wide_out=outs[rb][1])
        arms[f"q4_{q4.q8.row_bytes}"] = lambda: q4.lookup(ids, mask, out=outs["q4"][0], wide_out=outs["q4"][1])
        us = _time(arms, blocks, calls)
        wr = F * D * 4 + 4
        res = {"fp32_two_launches": _line(us["fp32_two_launches"], B * (Ls * (4 * D + 4 + 2 * 8) + wr))}
        for rb, t in q8.items():
            res[f"q8_{t.q8.row_bytes}"] = _line(us[f"q8_{t.q8.row_bytes}"], B * (Ls * (t.q8.row_bytes + 8) + wr))
        res[f"q4_{q4.q8.row_bytes}"] = _line(us[f"q4_{q4.q8.row_bytes}"], B * (Ls * (q4.q8.row_bytes + 8) + wr))
        dx4 = float((outs["q4"][0] - outs["fp32"][0]).abs().max())
        dx = float((outs[None][0] - outs["fp32"][0]).abs().max())
        dw = float((outs[None][1] - outs["fp32"][1]).abs().max())
        print(json.dumps({"what": "multi_hot_lookup", "samples": B, "bag": bag, "D": D, "V": V, "max_dx": dx, "max_dw": dw, "max_dx_q4": dx4,
                          **res}), flush=True)
        del pair, q8, q4


if __name__ == "__main__":
    main()
