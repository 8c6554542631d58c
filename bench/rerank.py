#!/usr/bin/env python3
"""map_rerank throughput: cross-encoder scoring of (query, passage) pairs on one MI355X.

The rerank counterpart of ``bench.py``: ``ClassifyEngine.rerank_pairs`` on ``bert-base?labels=1``,
one step = one call of 32 queries x 32 passages (1024 pairs) of seeded synthetic text end to end
(strings -> pinned staging -> GPU tokenizer over queries and passages -> ``pair_assemble`` ->
encoder -> head -> ``group_topk`` -> top-k and scores on the host). A pair is one encoder row, the
work the headline measures per classified row, plus the second tokenize and the assemble; unlike
the headline's CSV pipeline the texts are packed by Python and every call ends in a D2H. Prints
one JSON line.
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

UNIQUE_STEPS = 8  # distinct steps of synthetic text; a longer run repeats them


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-base")
    ap.add_argument("--batch-rows", type=int, default=0, help="0: the batch the agent serves this model with")
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--passages", type=int, default=32, help="candidates per query")
    ap.add_argument("--query-words", type=int, default=8)
    ap.add_argument("--words-per-row", type=int, default=150)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/rerank] needs a ROCm GPU", file=sys.stderr, flush=True)
        return 3
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from agent_tpu_amd.utils.synthetic import make_text_rows

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = a.batch_rows
    if B <= 0:
        from worker_sizing import classify_batch_rows

        B = classify_batch_rows(torch.cuda.get_device_properties(dev).total_memory, a.model, a.seq_len)
    cfg = config_for(a.model, num_labels=1)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=dev), dev, batch_rows=B, seq_len=a.seq_len, topk=1)
    Q, P = a.queries, a.queries * a.passages
    goff = [q * a.passages for q in range(Q + 1)]
    steps = [(make_text_rows(Q, a.query_words, seed=1234 + 2 * s), make_text_rows(P, a.words_per_row, seed=1235 + 2 * s))
             for s in range(min(UNIQUE_STEPS, a.warmup + a.steps))]
    res = None
    for s in range(a.warmup):
        res = eng.rerank_pairs(*steps[s % len(steps)], goff, top_k=a.top_k)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for s in range(a.warmup, a.warmup + a.steps):
        res = eng.rerank_pairs(*steps[s % len(steps)], goff, top_k=a.top_k)  # ends in its D2H: synchronized
    elapsed = time.perf_counter() - t0
    assert res.idx.shape == (Q, a.top_k) and bool(torch.isfinite(res.scores).all()) and bool((res.idx >= 0).all())
    pairs = a.steps * P
    fpr = cfg.flops_per_row_executed(a.seq_len)
    print(json.dumps({
        "metric": f"scored pairs/sec map_rerank {a.model} on 1 MI355X",
        "value": round(pairs / elapsed, 2), "unit": "pairs/s", "higher_is_better": True,
        "pairs_per_sec": round(pairs / elapsed, 2), "ms_per_step": round(elapsed * 1000.0 / a.steps, 3),
        "steps": a.steps, "warmup": a.warmup, "achieved_tflops": round(fpr * pairs / elapsed / 1e12, 1),
        "config": {"model": a.model + "?labels=1", "batch_rows": B, "seq_len": a.seq_len, "queries": Q,
                   "passages_per_query": a.passages, "pairs_per_step": P, "query_words": a.query_words,
                   "words_per_row": a.words_per_row, "top_k": a.top_k, "flops_per_row": fpr,
                   "max_query_tokens": min(32, (a.seq_len - 3) // 2), "hipgraph": eng.use_graph},
    }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
