"""The FP8 hidden-layer GEMM (ops.dense_fwd_fp8, csrc/mrec_gemm_fp8.hip) against the 16-bit forward GEMM it can replace in a serving
predictor, and a WideDeepQ8Predictor with and without dense_fp8.

    python tools/fp8_dense_bench.py [blocks] [calls]

GEMM arms at (M, K, N) = (16384, 2080, 1024) and (16384, 1024, 512), the reference net's layers 0 and 1 at the benchmark batch:
(i) ops.dense_fwd(..., wt=) in fp16, (ii) fp16 rows in, e4m3 codes out (the conversion inside the staging), (iii) e4m3 codes in, fp16
out.  Predictor arms: predict_fused over 4-bit records, reference net [2080, 1024, 512, 256, 128, 1], B = 16384 and 1024, dense_fp8 off /
on.  Every arm is warmed at every shape, then timed as `blocks` blocks of `calls` calls between two device events, the arms
alternating in one process; one JSON line per shape with the median (min, max) microseconds per call and, for the GEMMs, the TFLOP/s
2 M K N / time implies."""
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


def _line(us, flop=None):
    med = us[len(us) // 2]
    r = {"us": round(med, 2), "min": round(us[0], 2), "max": round(us[-1], 2)}
    if flop is not None:
        r["TFLOP/s"] = round(flop / med / 1e6, 1)
    return r


def main():
    from mindrec_amd import ops
    from mindrec_amd.serving import WideDeepQ8Predictor
    blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    f16, f8 = torch.float16, torch.float8_e4m3fn
    g = torch.Generator().manual_seed(7)
    for M, K, N in ((16384, 2080, 1024), (16384, 1024, 512)):
        x = torch.randn((M, K), generator=g).to(f16).to(dev)
        wt = (torch.randn((N, K), generator=g) * 0.03).to(f16).to(dev)
        bias = torch.zeros(N, device=dev)
        codes, sw = ops.quantize_rows_fp8(wt)
        sa = float(x.float().abs().max()) / 448
        y16 = torch.empty((M, N), dtype=f16, device=dev)
        y8 = torch.empty((M, N), dtype=f8, device=dev)
        x8 = ops.dense_fwd_fp8(x, torch.eye(K).to(f8).to(dev), torch.ones(K, device=dev), None, sa, relu=False, out_scale=sa)
        us = _time({"fp16_wt": lambda: ops.dense_fwd(x, None, bias, out=y16, wt=wt),
                    "a16_to_fp8": lambda: ops.dense_fwd_fp8(x, codes, sw, bias, sa, out_scale=1.0, out=y8),
                    "a8_to_fp16": lambda: ops.dense_fwd_fp8(x8, codes, sw, bias, sa, out_dtype=f16, out=y16)}, blocks, calls)
        print(json.dumps({"what": "gemm", "M": M, "K": K, "N": N, **{k: _line(v, 2.0 * M * K * N) for k, v in us.items()}}), flush=True)
    dims, F, D, V = [2080, 1024, 512, 256, 128, 1], 26, 80, 1_000_000
    table = torch.empty((V, D), dtype=torch.float32, device=dev)
    wide = torch.empty((V, 1), dtype=torch.float32, device=dev)
    ops.fill_normal_(table, 1000)
    ops.fill_normal_(wide, 1001)
    q4 = ops.quantize_rows_q4(table, wide)
    Ws = [torch.randn((dims[i], dims[i + 1]), generator=g) * (2.0 / dims[i]) ** 0.5 for i in range(5)]
    bs = [torch.zeros(dims[i + 1]) for i in range(5)]
    for B in (16384, 1024):
        ids = torch.randint(0, V, (B, F), generator=g).to(dev)
        wts = torch.rand((B, F), generator=g).to(dev)
        mk = lambda **kw: WideDeepQ8Predictor(q4, dims, Ws, bs, torch.zeros(1), mlp_dtype=f16, **kw)
        p16, p8 = mk(), mk(dense_fp8=True, calib=(ids, wts))
        us = _time({"fp16": lambda: p16.predict_fused(ids, wts), "dense_fp8": lambda: p8.predict_fused(ids, wts)}, blocks, calls)
        diff = float((p16.predict_fused(ids, wts)[1] - p8.predict_fused(ids, wts)[1]).abs().max())
        print(json.dumps({"what": "predict_fused", "B": B, "fp8_layers": sorted(p8.net._fp8), "max_prob_diff": round(diff, 5),
                          **{k: _line(v) for k, v in us.items()}}), flush=True)


if __name__ == "__main__":
    main()
