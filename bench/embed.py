#!/usr/bin/env python3
"""map_embed throughput: BERT sentence embeddings on one MI355X.

The embed counterpart of ``bench.py``: ``ClassifyEngine.embed_table`` over a synthetic CSV (the
same generator, rows and default batch), one step = one engine batch end to end (CSV rows ->
pinned staging -> GPU tokenizer -> encoder -> ``pool_embed`` -> ``[rows, H]`` fp32 on the device).
``mean`` pooling runs every layer in full, so its FLOPs are ``cfg.flops_per_row``; ``cls`` prunes
the last layer as classify does (``flops_per_row_executed``). ``ATPU_EMBED_FUSED=0`` is the A/B
partner of the pooled LayerNorm. Prints one JSON line.
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

UNIQUE_BATCHES = 32  # distinct batches of synthetic text; a longer run repeats them (as bench.py)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-base")
    ap.add_argument("--batch-rows", type=int, default=0, help="0: the batch the agent serves this model with")
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--words-per-row", type=int, default=150)
    ap.add_argument("--pooling", default="mean", choices=["mean", "cls"])
    ap.add_argument("--no-normalize", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/embed] needs a ROCm GPU", file=sys.stderr, flush=True)
        return 3
    from agent_tpu_amd._native import native
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from agent_tpu_amd.utils.synthetic import write_csv

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = a.batch_rows
    if B <= 0:
        from worker_sizing import classify_batch_rows

        B = classify_batch_rows(torch.cuda.get_device_properties(dev).total_memory, a.model, a.seq_len)
    cfg = config_for(a.model)
    rows_needed = (a.warmup + a.steps) * B
    unique = UNIQUE_BATCHES * B
    tiled = f"_u{unique}" if rows_needed > unique else ""
    path = f"/tmp/atpu_bench_r0_{rows_needed}_{a.words_per_row}{tiled}.csv"  # bench.py's file, when it exists
    if not os.path.exists(path):
        write_csv(path, rows_needed, a.words_per_row, seed=1234, unique_rows=unique)
    table = native().CsvTable(path)
    col = table.column_index("text")
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=dev), dev, batch_rows=B, seq_len=a.seq_len)
    normalize = not a.no_normalize
    eng.embed_table(table, 0, a.warmup * B, col, a.pooling, normalize)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    emb, st = eng.embed_table(table, a.warmup * B, a.steps * B, col, a.pooling, normalize)
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    rows = a.steps * B
    assert emb.shape == (rows, cfg.hidden) and bool(torch.isfinite(emb).all())
    fpr = cfg.flops_per_row(a.seq_len) if a.pooling == "mean" else cfg.flops_per_row_executed(a.seq_len)
    fused = eng.model.embed_fused and eng.model.can_fold(B, a.seq_len)
    print(json.dumps({
        "metric": f"embedded rows/sec map_embed {a.model} on 1 MI355X",
        "value": round(rows / elapsed, 2), "unit": "rows/s", "higher_is_better": True,
        "ms_per_step": round(elapsed * 1000.0 / a.steps, 3), "steps": a.steps, "warmup": a.warmup,
        "achieved_tflops": round(fpr * rows / elapsed / 1e12, 1),
        "config": {"model": a.model, "batch_rows": B, "seq_len": a.seq_len, "words_per_row": a.words_per_row,
                   "pooling": a.pooling, "normalize": normalize, "dim": cfg.hidden,
                   "pooled_layernorm": bool(fused and a.pooling == "mean"), "flops_per_row": fpr,
                   "hipgraph": eng.use_graph, "concurrent_batches": eng.n_slots if eng.concurrent else 1},
    }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
