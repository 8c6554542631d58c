"""Isolated encoder GEMMs: ``ops.linear_i8`` (int8 MFMA, operands already quantised) against
``ops.linear`` (bf16 MFMA) at the BERT-base shapes of a 131072-token batch.

Random full-range data (zero-filled operands run 1.27-1.30x faster on this part); both kernels
take bias; warm-up, then hipEvent-timed launches, the two kernels alternating per round in one
process. Prints one JSON line per shape and writes them to ``--out``.

Usage: ``python bench/gemm_i8.py [--M 131072] [--iters 20] [--rounds 3] [--out FILE]``
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from agent_tpu_amd import ops  # noqa: E402

SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]


def timed(fn, warmup: int, iters: int) -> float:
    """Mean milliseconds per launch over ``iters`` back-to-back launches."""
    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=131072)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    M, rows = a.M, []
    for N, K in SHAPES:
        x = torch.randn((M, K), generator=g, device=dev).to(torch.bfloat16)
        w = (torch.randn((N, K), generator=g, device=dev) * 0.02).to(torch.bfloat16)
        bias = torch.randn(N, generator=g, device=dev)
        xq = torch.randint(-127, 128, (M, K), generator=g, device=dev, dtype=torch.int8)
        wq = torch.randint(-127, 128, (N, K), generator=g, device=dev, dtype=torch.int8)
        xs = torch.rand(M, generator=g, device=dev) * 0.01 + 0.001
        ws = torch.rand(N, generator=g, device=dev) * 0.001 + 0.0001
        bf, i8, qt = [], [], []
        for _ in range(a.rounds):
            bf.append(timed(lambda: ops.linear(x, w, bias), a.warmup, a.iters))
            i8.append(timed(lambda: ops.linear_i8(xq, xs, wq, ws, bias), a.warmup, a.iters))
            qt.append(timed(lambda: ops.quantize_rows_i8(x), a.warmup, a.iters))
        ops_n = 2.0 * M * N * K
        b, i, q = statistics.median(bf), statistics.median(i8), statistics.median(qt)
        row = {"M": M, "N": N, "K": K, "iters": a.iters, "rounds": a.rounds,
               "bf16_ms": round(b, 4), "int8_ms": round(i, 4), "quantize_rows_ms": round(q, 4),
               "bf16_tflops": round(ops_n / b / 1e9, 1), "int8_tops": round(ops_n / i / 1e9, 1),
               "int8_speedup": round(b / i, 3), "int8_plus_quantize_speedup": round(b / (i + q), 3),
               "bf16_ms_min": round(min(bf), 4), "int8_ms_min": round(min(i8), 4)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, w, xq, wq
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"bench": "gemm_i8", "device": torch.cuda.get_device_name(0), "shapes": rows}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
