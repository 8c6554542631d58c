#!/usr/bin/env python3
"""``term_max`` + ``term_select`` against the PyTorch composition on one MI355X, and ``map_sparse_embed`` end to end.

Kernels, at bert-base shape (``V = 30522``, ``H = 768``, ``--batch`` texts of ``--seq`` tokens, lens mixed between
``seq / 4`` and ``seq``), on the same bf16 tensors, alternating for ``--rounds`` rounds in one process:

* ``term_max_64`` / ``term_max_32``: ``ops.term_max`` with a vocabulary tile of 64 / 32 entries per workgroup;
* ``term_select``: ``ops.term_select`` of the result, ``k = --max-terms``;
* ``torch``: the only other way to the same answer: bf16 ``t @ E.T`` (the ``[B*S, V]`` logits written), a masked
  ``amax`` over the tokens, ``+ bias``, ``topk``, ``log1p``.

End to end: ``ClassifyEngine.sparse_texts`` (random-init bert-base with an MLM head, captured graphs) in texts per
second, next to ``embed_texts`` on the same texts. One JSON line per (variant, round): us per call from hipEvents
after warm-up; ``--log1p-sweep`` adds the largest ulp error of the device ``log1pf`` (through ``term_select``)
against float64 on 4M points of (0, 64].
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def timed(fn, dev, iters: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1000.0 / iters


def log1p_sweep(ops, dev) -> float:
    x = torch.linspace(0, 64, 4096 * 1024 + 1, dtype=torch.float64, device=dev)[1:].float().view(4096, 1024)
    tok, xs, w, _ = ops.term_select(x.contiguous(), torch.zeros(1024, device=dev), 1024)
    ref = torch.log1p(xs.double())
    ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref).exponent - 24)
    return ((w.double() - ref).abs() / ulp).max().item()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--max-terms", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--texts", type=int, default=256, help="end to end: texts per call (0: skip)")
    ap.add_argument("--log1p-sweep", action="store_true")
    a = ap.parse_args(argv)
    from agent_tpu_amd import ops

    dev = torch.device("cuda", 0)
    B, S, V, H, k = a.batch, a.seq, a.vocab, a.hidden, a.max_terms
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.randn(B * S, H, device=dev, generator=g).bfloat16()
    E = (0.05 * torch.randn(V, H, device=dev, generator=g)).bfloat16()
    bias = 0.1 * torch.randn(V, device=dev, generator=g)
    lens = torch.randint(max(1, S // 4), S + 1, (B,), device=dev, generator=g, dtype=torch.int32)
    lens[0] = S
    live = (torch.arange(S, device=dev)[None, :] < lens[:, None])[:, :, None]

    def torch_way():
        lg = (t @ E.T).view(B, S, V).masked_fill(~live, float("-inf")).amax(1).float() + bias
        top = torch.topk(lg, k, dim=1)
        return top.indices, torch.log1p(torch.relu(top.values))

    xmax = ops.term_max(t, lens, E, S)
    assert torch.equal(xmax, ops.term_max(t, lens, E, S, vocab_tile=32))
    arms = [("term_max_64", lambda: ops.term_max(t, lens, E, S, vocab_tile=64)),
            ("term_max_32", lambda: ops.term_max(t, lens, E, S, vocab_tile=32)),
            ("term_select", lambda: ops.term_select(xmax, bias, k)), ("torch", torch_way)]
    for rnd in range(a.rounds):
        for name, fn in arms:
            print(json.dumps({"bench": "sparse_kernels", "variant": name, "round": rnd, "B": B, "S": S, "V": V, "H": H,
                              "k": k, "tokens": int(lens.sum()), "us": round(timed(fn, dev, a.iters), 2)}), flush=True)
    if a.log1p_sweep:
        print(json.dumps({"bench": "log1pf_sweep", "points": 4096 * 1024, "max_ulp": log1p_sweep(ops, dev)}), flush=True)
    if a.texts:
        from agent_tpu_amd.models.bert import config_for, init_random
        from agent_tpu_amd.runtime.classify import ClassifyEngine
        from agent_tpu_amd.utils.synthetic import make_text_rows

        cfg = config_for("bert-base", num_labels=1, mlm_head=True)
        eng = ClassifyEngine(cfg, init_random(cfg, seed=1, bias_std=0.02), dev, batch_rows=B, seq_len=S, topk=1)
        texts = make_text_rows(a.texts, words_per_row=60, seed=1)
        for name, fn in (("sparse_texts", lambda: eng.sparse_texts(texts, k)), ("embed_texts", lambda: eng.embed_texts(texts))):
            fn()
            for rnd in range(a.rounds):
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                print(json.dumps({"bench": "sparse_e2e", "variant": name, "round": rnd, "texts": len(texts), "B": B,
                                  "S": S, "k": k, "texts_per_s": round(len(texts) / dt, 1)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
