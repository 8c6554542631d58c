#!/usr/bin/env python3
"""map_fill throughput: BERT masked-token prediction with the fused vocabulary top-k on one MI355X.

Shaped like ``bench/tag.py``: ``bert-base?mlm=1``, S = 128, one step = one engine call of ``batch_rows``
strings with one mask each, end to end (strings split at the mask -> pinned staging -> GPU tokenizer ->
``fill_assemble`` -> encoder, every layer in full -> ``mask_gather`` -> transform -> ``vocab_topk`` -> candidates
D2H -> candidate lists on the host). ``value`` is that whole step; ``device_rows_per_sec`` is the same call
without the host mapping (``fill_rows`` and a synchronize). ``ATPU_FILL_FUSED=0`` is the A/B partner of the
gathered LayerNorm. ``--kernel`` times ``vocab_topk`` alone (partial + merge, hipEvents around ``--steps``
launches) against ``torch.topk(torch.log_softmax(t @ E.float().T + b, -1), k)`` on the same tensors, the two
alternating for ``--rounds`` rounds in one process (the method of ``bench/search.py``). Prints one JSON line.
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

UNIQUE_BATCHES = 4  # distinct batches of synthetic text; a longer run repeats them


def _timed(fn, steps: int, warmup: int, dev) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1000.0 / steps


def kernel(a, dev) -> int:
    from agent_tpu_amd import ops

    R, V, H, k = a.batch_rows, a.vocab, a.hidden, a.top_k
    g = torch.Generator().manual_seed(0)
    t = torch.randn(R, H, generator=g).to(dev)
    E = (torch.randn(V, H, generator=g) * 0.05).bfloat16().to(dev)
    b = torch.randn(V, generator=g).to(dev)
    ours = lambda: ops.vocab_topk(t, E, b, k)  # noqa: E731
    ref = lambda: torch.topk(torch.log_softmax(t @ E.float().T + b, -1), k)  # noqa: E731
    a_us, b_us = [], []
    for _ in range(a.rounds):
        a_us.append(_timed(ours, a.steps, a.warmup, dev))
        b_us.append(_timed(ref, a.steps, a.warmup, dev))
    tok, _, _, _ = ours()
    same = float((tok.long() == ref().indices).float().mean().item())
    flops = 2.0 * R * V * H
    print(json.dumps({
        "metric": f"vocab_topk us per call R={R} V={V} H={H} k={k} on 1 MI355X", "value": round(min(a_us), 2),
        "unit": "us", "higher_is_better": False, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
        "vocab_topk_us": [round(x, 2) for x in a_us], "torch_us": [round(x, 2) for x in b_us],
        "speedup_vs_torch": round(min(b_us) / min(a_us), 3), "tflops": round(flops / (min(a_us) * 1e-6) / 1e12, 2),
        "top_k_agreement_with_torch": round(same, 5),
        "config": {"slots": R, "vocab": V, "hidden": H, "top_k": k, "splits": ops.vocab_topk_splits(V)},
    }), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-base?mlm=1")
    ap.add_argument("--batch-rows", type=int, default=1024)
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--words-per-row", type=int, default=150)
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel", action="store_true", help="time vocab_topk alone against the torch composition")
    ap.add_argument("--rounds", type=int, default=3, help="--kernel: alternating rounds")
    ap.add_argument("--vocab", type=int, default=30522, help="--kernel: vocabulary size")
    ap.add_argument("--hidden", type=int, default=768, help="--kernel: hidden size")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/fill] needs a ROCm GPU", file=sys.stderr, flush=True)
        return 3
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.kernel:
        return kernel(a, dev)
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from agent_tpu_amd.utils.synthetic import make_text_rows
    from ops._gpu_runtime import parse_spec

    spec = parse_spec(a.model)
    cfg = config_for(spec.preset, num_labels=spec.labels, mlm_head=spec.mlm)
    B = a.batch_rows

    def masked(rows):  # one mask per row, within the first 60 words (inside the 126 tokens of a row)
        out = []
        for i, r in enumerate(rows):
            w = r.split()
            at = (7 * i + 3) % min(60, len(w))
            out.append(" ".join(w[:at] + ["[MASK]"] + w[at + 1:]))
        return out

    batches = [masked(make_text_rows(B, words_per_row=a.words_per_row, seed=1234 + i)) for i in range(UNIQUE_BATCHES)]
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=dev), dev, batch_rows=B, seq_len=a.seq_len)
    for i in range(a.warmup):
        eng.fill_texts(batches[i % UNIQUE_BATCHES], a.top_k)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    cands = 0
    for i in range(a.steps):
        res = eng.fill_texts(batches[i % UNIQUE_BATCHES], a.top_k)
        cands += sum(len(m["candidates"]) for r in res.fills for m in r)
    elapsed = time.perf_counter() - t0
    t1 = time.perf_counter()
    for i in range(a.steps):
        eng.fill_rows(batches[i % UNIQUE_BATCHES], a.top_k)
        torch.cuda.synchronize(dev)
    device_elapsed = time.perf_counter() - t1
    rows = a.steps * B
    assert cands > 0
    print(json.dumps({
        "metric": f"filled rows/sec map_fill {spec.preset} on 1 MI355X",
        "value": round(rows / elapsed, 2), "unit": "rows/s", "higher_is_better": True,
        "ms_per_step": round(elapsed * 1000.0 / a.steps, 3), "steps": a.steps, "warmup": a.warmup,
        "device_rows_per_sec": round(rows / device_elapsed, 2),
        "device_ms_per_step": round(device_elapsed * 1000.0 / a.steps, 3),
        "candidates_per_row": round(cands / rows, 2),
        "config": {"model": a.model, "batch_rows": B, "seq_len": a.seq_len, "words_per_row": a.words_per_row,
                   "top_k": a.top_k, "vocab": cfg.vocab_size,
                   "fill_fused": bool(eng.model.fill_fused and eng.model.can_fold(B, a.seq_len)),
                   "flops_per_row": cfg.flops_per_row(a.seq_len), "hipgraph": eng.use_graph},
    }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
