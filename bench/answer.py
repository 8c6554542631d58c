#!/usr/bin/env python3
"""map_answer throughput: extractive question answering over (question, passage) pairs on one MI355X.

The reader counterpart of ``bench/rerank.py``: ``ClassifyEngine.answer_pairs`` on ``bert-base?qa=1``,
one step = one call of 32 questions x 32 passages (1024 pairs) of seeded synthetic text end to end
(strings -> pinned staging -> GPU tokenizer over questions and passages -> ``pair_assemble`` ->
encoder, every layer in full -> ``span_topk`` -> ``group_topk`` -> spans on the host -> character
offsets of the returned answers). ``ATPU_ANSWER_FUSED=0`` is the A/B partner: the last LayerNorm run
over every row instead of folded into the span head. ``--doc-stride N`` reads long passages in overlapping
windows (``window_assemble`` -> encoder -> ``span_topk`` with owned starts -> ``window_best``) and also reports
window rows per second; without it the run is the one it always was. Prints one JSON line.
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
    ap.add_argument("--questions", type=int, default=32)
    ap.add_argument("--passages", type=int, default=32, help="passages per question")
    ap.add_argument("--question-words", type=int, default=8)
    ap.add_argument("--words-per-row", type=int, default=150)
    ap.add_argument("--top-k", type=int, default=3)
    ap.add_argument("--max-answer-tokens", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--doc-stride", type=int, default=None, help="read long passages in windows (default: cut them)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/answer] needs a ROCm GPU", file=sys.stderr, flush=True)
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
    cfg = config_for(a.model, num_labels=1, qa_head=True)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=dev), dev, batch_rows=B, seq_len=a.seq_len, topk=1)
    Q, P = a.questions, a.questions * a.passages
    goff = [q * a.passages for q in range(Q + 1)]
    steps = [(make_text_rows(Q, a.question_words, seed=1234 + 2 * s),
              make_text_rows(P, a.words_per_row, seed=1235 + 2 * s))
             for s in range(min(UNIQUE_STEPS, a.warmup + a.steps))]
    kw = dict(top_k=a.top_k, max_answer_tokens=a.max_answer_tokens)
    if a.doc_stride is not None:
        kw["doc_stride"] = a.doc_stride
    res, windows = None, 0
    for s in range(a.warmup):
        res = eng.answer_pairs(*steps[s % len(steps)], goff, **kw)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for s in range(a.warmup, a.warmup + a.steps):
        res = eng.answer_pairs(*steps[s % len(steps)], goff, **kw)  # ends in its D2H: synchronized
        windows += res.window_count or 0
    elapsed = time.perf_counter() - t0
    assert res.span.shape == (P, a.top_k, 2) and bool(torch.isfinite(res.null).all())
    assert all(len(row) == a.top_k and all(e["text"] for e in row) for row in res.answers)
    pairs = a.steps * P
    fpr = cfg.flops_per_row(a.seq_len)  # every layer in full
    extra, cfg_extra = {}, {}
    if a.doc_stride is not None:  # a window row is a pair row: the encoder's work is per window
        extra = {"window_rows_per_sec": round(windows / elapsed, 2), "windows_per_pair": round(windows / pairs, 3)}
        cfg_extra = {"doc_stride": a.doc_stride}
    print(json.dumps({
        "metric": f"read pairs/sec map_answer {a.model} on 1 MI355X",
        "value": round(pairs / elapsed, 2), "unit": "pairs/s", "higher_is_better": True,
        "pairs_per_sec": round(pairs / elapsed, 2), "ms_per_step": round(elapsed * 1000.0 / a.steps, 3),
        "steps": a.steps, "warmup": a.warmup,
        "achieved_tflops": round(fpr * (windows if a.doc_stride is not None else pairs) / elapsed / 1e12, 1), **extra,
        "config": {"model": a.model + "?qa=1", "batch_rows": B, "seq_len": a.seq_len, "questions": Q,
                   "passages_per_question": a.passages, "pairs_per_step": P, "question_words": a.question_words,
                   "words_per_row": a.words_per_row, "top_k": a.top_k, "max_answer_tokens": a.max_answer_tokens,
                   "flops_per_row": fpr, "max_query_tokens": min(32, (a.seq_len - 3) // 2),
                   "answer_fused": eng.model.answer_fused, "hipgraph": eng.use_graph, **cfg_extra},
    }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
