#!/usr/bin/env python3
"""map_zero_shot throughput: NLI scoring of (text, label) pairs on one MI355X.

The zero-shot counterpart of ``bench/rerank.py``: ``ClassifyEngine.zero_shot`` on ``bert-base?nli=1``, one
step = one call of 128 texts x 8 candidate labels (1024 pairs) of seeded synthetic text end to end
(strings -> pinned staging -> GPU tokenizer over the distinct texts and hypotheses -> ``premise_assemble``
-> encoder -> head -> ``nli_rank`` -> ranked labels and scores on the host). A pair is one encoder row,
as in the re-ranker's bench, so the two rates differ by the host and tail work of the ops alone: here a
text is packed and tokenized once for its 8 labels, and every label of every text is ranked. Prints one
JSON line.
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
    ap.add_argument("--texts", type=int, default=128)
    ap.add_argument("--labels", type=int, default=8, help="candidate labels per text")
    ap.add_argument("--words-per-row", type=int, default=150)
    ap.add_argument("--multi-label", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/zero_shot] needs a ROCm GPU", file=sys.stderr, flush=True)
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
    cfg = config_for(a.model, num_labels=3)  # ?nli=1: contradiction, neutral, entailment
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=dev), dev, batch_rows=B, seq_len=a.seq_len, topk=1)
    Tn, L = a.texts, a.labels
    P = Tn * L
    ranges = [(0, L)] * Tn
    steps = []
    for s in range(min(UNIQUE_STEPS, a.warmup + a.steps)):
        names = [w.lower() for w in make_text_rows(1, L, seed=2235 + 2 * s)[0].split()]
        steps.append((make_text_rows(Tn, a.words_per_row, seed=2234 + 2 * s), ["This example is %s." % n for n in names]))
    res = None
    for s in range(a.warmup):
        res = eng.zero_shot(*steps[s % len(steps)], ranges, a.multi_label, ent=2, con=0)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for s in range(a.warmup, a.warmup + a.steps):
        res = eng.zero_shot(*steps[s % len(steps)], ranges, a.multi_label, ent=2, con=0)  # ends in its D2H: synchronized
    elapsed = time.perf_counter() - t0
    assert res.order.shape == (P,) and bool(torch.isfinite(res.logits).all()) and bool((res.order >= 0).all())
    assert sorted(res.ranked(Tn - 1)[0]) == list(range(L))
    pairs = a.steps * P
    fpr = cfg.flops_per_row_executed(a.seq_len)
    print(json.dumps({
        "metric": f"scored pairs/sec map_zero_shot {a.model} on 1 MI355X",
        "value": round(pairs / elapsed, 2), "unit": "pairs/s", "higher_is_better": True,
        "pairs_per_sec": round(pairs / elapsed, 2), "ms_per_step": round(elapsed * 1000.0 / a.steps, 3),
        "steps": a.steps, "warmup": a.warmup, "achieved_tflops": round(fpr * pairs / elapsed / 1e12, 1),
        "config": {"model": a.model + "?nli=1", "batch_rows": B, "seq_len": a.seq_len, "texts": Tn,
                   "labels_per_text": L, "pairs_per_step": P, "words_per_row": a.words_per_row,
                   "multi_label": a.multi_label, "flops_per_row": fpr,
                   "max_hypothesis_tokens": min(32, (a.seq_len - 3) // 2), "hipgraph": eng.use_graph},
    }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
