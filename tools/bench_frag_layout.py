#!/usr/bin/env python3
"""FFN pair and out-proj with the activations in K-tile image order vs in fragment order.

The LN-folded BERT-base GEMMs at M = rows x 128 on random bf16 data of the encoder's scale, timed
with hipEvents in interleaved rounds in one process, the two arms being what ATPU_ACT_LAYOUT=3 and 4
run: hidden rows, FFN intermediate and outputs in image order (`ops.to_image_order`) or in fragment
order (`ops.to_fragment_order`); the attention context (out-proj's A) in image order in both. The
arms' outputs are compared first (bit-identical after un-permuting, or the tool fails). One JSON
line per (what, arm), then a verdict per item: fragment order "wins" only if every fragment-order
round beats every image-order round.
Usage: python tools/bench_frag_layout.py [--rows 1024] [--rounds 8] [--iters 50]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=8)
    a = ap.parse_args()
    from agent_tpu_amd import ops

    dev = torch.device("cuda", 0)
    M, H, I = a.rows * 128, 768, 3072
    gen = torch.Generator(device=dev).manual_seed(1)

    def rand(shape, scale, shift=0.0, dtype=torch.bfloat16):
        return (torch.randn(shape, generator=gen, device=dev) * scale + shift).to(dtype)

    x = rand((M, H), 2.0, 0.3)  # raw pre-LN hidden rows
    ctx = ops.to_image_order(rand((M, H), 0.5))
    w1, w2, wo = rand((I, H), 0.04), rand((H, I), 0.04), rand((H, H), 0.04)
    b1, b2, bo = (rand((n,), 0.1, dtype=torch.float32) for n in (I, H, H))
    gam, bet = 1 + rand((H,), 0.1, dtype=torch.float32), rand((H,), 0.05, dtype=torch.float32)
    w1f, c1, b1f = ops.fold_ln_into_linear(w1, b1, gam, bet)
    b2f, bof = (b2 + bet).contiguous(), (bo + bet).contiguous()
    fin = ops.ln_finalize(ops.ln_partials_ref(x.float()), H, 1e-12)
    xs = [ops.to_image_order(x), ops.to_fragment_order(x)]
    undo = [ops.from_image_order, ops.from_fragment_order]
    LA = [ops.LAYOUT_A, ops.LAYOUT_A_FRAG]
    LC = [ops.LAYOUT_C, ops.LAYOUT_C_FRAG]
    LR = [ops.LAYOUT_R, ops.LAYOUT_R_FRAG]
    del x
    ff = [torch.empty((M, I), dtype=torch.bfloat16, device=dev) for _ in range(2)]
    out = [torch.empty((M, H), dtype=torch.bfloat16, device=dev) for _ in range(2)]
    oa = [torch.empty((M, H), dtype=torch.bfloat16, device=dev) for _ in range(2)]
    part = [torch.empty((H // 256, M, 2), dtype=torch.float32, device=dev) for _ in range(4)]

    def ffn1(arm):
        ops.linear_ln(xs[arm], w1f, b1f, act="gelu", in_fin=fin, colsum=c1, out=ff[arm], layout=LA[arm] | LC[arm])

    def ffn2(arm):
        ops.linear_ln(ff[arm], w2, b2f, residual=xs[arm], res_fin=fin, res_gamma=gam, part_out=part[arm],
                      out=out[arm], layout=LA[arm] | LC[arm] | LR[arm])

    def pair(arm):
        ffn1(arm)
        ffn2(arm)

    def out_proj(arm):
        ops.linear_ln(ctx, wo, bof, residual=xs[arm], res_fin=fin, res_gamma=gam, part_out=part[2 + arm],
                      out=oa[arm], layout=ops.LAYOUT_A | LC[arm] | LR[arm])

    for arm in (0, 1):
        pair(arm)
        out_proj(arm)
    torch.cuda.synchronize()
    same = all(torch.equal(undo[0](t[0]), undo[1](t[1])) for t in (ff, out, oa))
    same = same and torch.equal(part[0], part[1]) and torch.equal(part[2], part[3])
    print(json.dumps({"M": M, "outputs_bit_identical": same}), flush=True)
    if not same:
        return 1
    what = {"pair": pair, "ffn1": ffn1, "ffn2": ffn2, "out_proj": out_proj}
    res = {(k, arm): [] for k in what for arm in (0, 1)}
    for _ in range(a.rounds):
        for k, f in what.items():
            for arm in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f(arm)
                e1.record()
                e1.synchronize()
                res[(k, arm)].append(e0.elapsed_time(e1) * 1000.0 / a.iters)
    for (k, arm), v in res.items():
        print(json.dumps({"what": k, "layout": "fragment" if arm else "image", "us_min": round(min(v), 1),
                          "us_max": round(max(v), 1), "us_all": [round(t, 1) for t in v]}), flush=True)
    for k in ("pair", "out_proj"):
        i, f = res[(k, 0)], res[(k, 1)]
        print(json.dumps({"what": k, "verdict": "fragment order wins every round" if max(f) < min(i) else "no gain",
                          "image_us": [round(min(i), 1), round(max(i), 1)],
                          "fragment_us": [round(min(f), 1), round(max(f), 1)]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
