#!/usr/bin/env python3
"""FFN1 -> FFN2 with the intermediate row-major vs in K-tile image order (ops.to_image_order).

The LN-folded BERT-base FFN pair at M = rows x 128 on random bf16 data of the encoder's scale,
timed with hipEvents in interleaved rounds in one process: per round, each arm runs `iters`
back-to-back pairs, and FFN1 / FFN2 alone. The arms' outputs are compared first (bit-identical
or the tool fails). One JSON line per (what, arm), then a verdict line: image order "wins" only
if every image-order round beats every row-major round.
Usage: python tools/bench_act_layout.py [--rows 1024] [--rounds 6] [--iters 20]
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    from agent_tpu_amd import ops

    dev = torch.device("cuda", 0)
    M, H, I = a.rows * 128, 768, 3072
    gen = torch.Generator(device=dev).manual_seed(1)

    def rand(shape, scale, shift=0.0, dtype=torch.bfloat16):
        return (torch.randn(shape, generator=gen, device=dev) * scale + shift).to(dtype)

    # raw pre-LN hidden rows (std ~2 around a small mean), BERT-scale weights
    x = rand((M, H), 2.0, 0.3)
    w1, w2 = rand((I, H), 0.04), rand((H, I), 0.04)
    b1, b2 = rand((I,), 0.1, dtype=torch.float32), rand((H,), 0.1, dtype=torch.float32)
    gam, bet = 1 + rand((H,), 0.1, dtype=torch.float32), rand((H,), 0.05, dtype=torch.float32)
    w1f, c1, b1f = ops.fold_ln_into_linear(w1, b1, gam, bet)
    b2f = (b2 + bet).contiguous()
    xf = x.float()
    fin = ops.ln_finalize(ops.ln_partials_ref(xf), H, 1e-12)
    del xf
    ff = [torch.empty((M, I), dtype=torch.bfloat16, device=dev) for _ in range(2)]
    out = [torch.empty((M, H), dtype=torch.bfloat16, device=dev) for _ in range(2)]
    part = [torch.empty((H // 256, M, 2), dtype=torch.float32, device=dev) for _ in range(2)]

    def ffn1(arm):
        ops.linear_ln(x, w1f, b1f, act="gelu", in_fin=fin, colsum=c1, out=ff[arm], layout=ops.LAYOUT_C if arm else 0)

    def ffn2(arm):
        ops.linear_ln(ff[arm], w2, b2f, residual=x, res_fin=fin, res_gamma=gam, part_out=part[arm], out=out[arm],
                      layout=ops.LAYOUT_A if arm else 0)

    def pair(arm):
        ffn1(arm)
        ffn2(arm)

    for arm in (0, 1):
        pair(arm)
    torch.cuda.synchronize()
    same = (torch.equal(out[0], out[1]) and torch.equal(part[0], part[1])
            and torch.equal(ops.from_image_order(ff[1]), ff[0]))
    print(json.dumps({"M": M, "outputs_bit_identical": same}), flush=True)
    if not same:
        return 1
    what = {"pair": pair, "ffn1": ffn1, "ffn2": ffn2}
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
        print(json.dumps({"what": k, "layout": "image" if arm else "row-major", "us_min": round(min(v), 1),
                          "us_max": round(max(v), 1), "us_all": [round(t, 1) for t in v]}), flush=True)
    r, i = res[("pair", 0)], res[("pair", 1)]
    print(json.dumps({"verdict": "image order wins every round" if max(i) < min(r) else "no gain",
                      "pair_row_major_us": [round(min(r), 1), round(max(r), 1)],
                      "pair_image_us": [round(min(i), 1), round(max(i), 1)]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
