#!/usr/bin/env python3
"""Isolated ``pool_embed`` against ``ops.layernorm`` + a torch masked mean on one MI355X.

A: ``pool_embed(g, fin, gamma, beta)`` over the raw rows (the LayerNorm applied to the pooled
vector). B: what it replaces, ``ops.layernorm`` over every row, then a masked mean and
``F.normalize`` in torch. Shape of the headline batch (B = 1024, S = 128, H = 768 by default), all
rows full and rows of ``--short`` tokens. The inputs rotate through ``--buffers`` copies (4 x 201 MB
by default) so that no call finds its rows in the 256 MiB Infinity Cache; A and B alternate for
``--rounds`` rounds. One JSON line per (lens, variant, round): time per call from hipEvents, and
for A the achieved GB/s over the bytes of the real tokens (rows, statistics, output).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--short", type=int, default=32)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/pool_embed] needs a ROCm GPU", file=sys.stderr, flush=True)
        return 3
    from agent_tpu_amd import ops

    dev = torch.device("cuda", 0)
    B, S, H = a.rows, a.seq_len, a.hidden
    gen = torch.Generator(device=dev).manual_seed(0)
    gs = [torch.randn(B * S, H, device=dev, generator=gen).bfloat16() for _ in range(a.buffers)]
    fins = []
    for g in gs:
        x = g.float()
        rs = torch.rsqrt(x.var(1, unbiased=False) + 1e-12)
        fins.append(torch.stack([rs, rs * x.mean(1)], -1).contiguous())
        del x
    gamma = 1 + 0.1 * torch.randn(H, device=dev, generator=gen)
    beta = 0.05 * torch.randn(H, device=dev, generator=gen)
    out = torch.empty((B, H), dtype=torch.float32, device=dev)

    def fused(i, lens):
        return ops.pool_embed(gs[i], lens, B, fins[i], gamma, beta, "mean", True, out=out)

    def unfused(i, lens):
        h = ops.layernorm(gs[i], gamma, beta, 1e-12).view(B, S, H)
        n = lens.clamp(1, S).view(B, 1)
        live = (torch.arange(S, device=dev).view(1, S) < n).view(B, S, 1)
        return F.normalize(torch.where(live, h.float(), 0.0).sum(1) / n, dim=1, eps=1e-12)

    def timed(fn, lens):
        for i in range(a.buffers):
            fn(i, lens)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.iters):
            fn(k % a.buffers, lens)
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / a.iters  # us per call

    for name, n in (("full", S), (f"len{a.short}", a.short)):
        lens = torch.full((B,), n, dtype=torch.int32, device=dev)
        err = (fused(0, lens) - unfused(0, lens)).abs().max().item()  # bf16 LayerNorm output in B
        real = B * n * (H * 2 + 8) + B * H * 4
        for r in range(a.rounds):
            for variant, fn in (("pool_embed", fused), ("layernorm+torch_mean", unfused)):
                us = timed(fn, lens)
                line = {"bench": "pool_embed", "lens": name, "variant": variant, "round": r, "us_per_call": round(us, 2),
                        "shape": [B, S, H], "max_abs_diff_between_variants": err}
                if variant == "pool_embed":
                    line.update(real_token_bytes=real, achieved_gbs=round(real / us / 1e3, 1))
                print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
