#!/usr/bin/env python3
"""map_tag throughput: BERT token classification with entity grouping on one MI355X.

Shaped like ``bench/embed.py``: ``bert-base?tags=9``, S = 128, one step = one engine call of ``batch_rows``
strings end to end (strings -> pinned staging -> GPU tokenizer -> encoder, every layer in full ->
``tag_entities`` -> entity records D2H -> character offsets on the host). ``value`` is that whole step;
``device_rows_per_sec`` is the same call without the host mapping (``tag_rows`` and a synchronize).
``ATPU_TAG_FUSED=0`` is the A/B partner of the folded LayerNorm. ``--kernel`` times ``tag_entities`` alone on
random rows (hipEvents around ``--steps`` launches) for ``--labels`` and reports it against the copy rate
over the bytes it reads. Prints one JSON line.
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
COPY_RATE = 6.29e12  # bytes/s, the measured device copy rate the kernels here are held against


def kernel(a, dev) -> int:
    from agent_tpu_amd import ops

    B, S, H, L = a.batch_rows or 1024, a.seq_len, a.hidden, a.labels
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B * S, H, generator=g).bfloat16().to(dev)
    u = (torch.randn(L, H, generator=g) * 0.05).to(dev)
    su, c = u.double().sum(1).float(), torch.randn(L, generator=g).to(dev)
    fin = torch.stack([torch.rand(B * S, generator=g) + 0.5, torch.randn(B * S, generator=g) * 0.1], 1).to(dev)
    lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    _, lt, lb = ops.tag_tables(ops.default_tag_names(L))
    lt, lb = lt.to(dev), lb.to(dev)
    E = a.max_entities
    outs = dict(ent=torch.empty((B, E, 4), dtype=torch.int32, device=dev), ent_sum=torch.empty((B, E), device=dev),
                count=torch.empty((B,), dtype=torch.int32, device=dev))
    run = lambda: ops.tag_entities(x, lens, B, S, u, su, c, lt, lb, 1, E, fin=fin, **outs)  # noqa: E731
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        run()
    e1.record()
    torch.cuda.synchronize(dev)
    us = e0.elapsed_time(e1) * 1000.0 / a.steps
    read = B * S * H * 2 + B * S * 8 + L * H * 4
    print(json.dumps({
        "metric": f"tag_entities us per call {B}x{S}x{H} L={L} on 1 MI355X", "value": round(us, 2), "unit": "us",
        "higher_is_better": False, "steps": a.steps, "warmup": a.warmup, "bytes_read": read,
        "share_of_copy_rate": round(read / (us * 1e-6) / COPY_RATE, 3),
        "config": {"rows": B, "seq_len": S, "hidden": H, "labels": L, "mode": "simple", "max_entities": E,
                   "fin": True},
    }), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-base?tags=9")
    ap.add_argument("--batch-rows", type=int, default=1024)
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--words-per-row", type=int, default=150)
    ap.add_argument("--aggregation", default="simple", choices=["simple", "none"])
    ap.add_argument("--max-entities", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel", action="store_true", help="time tag_entities alone")
    ap.add_argument("--labels", type=int, default=9, help="--kernel: labels of the head")
    ap.add_argument("--hidden", type=int, default=768, help="--kernel: hidden size")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/tag] needs a ROCm GPU", file=sys.stderr, flush=True)
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
    cfg = config_for(spec.preset, num_labels=spec.labels, tag_labels=spec.tags)
    B = a.batch_rows
    batches = [make_text_rows(B, words_per_row=a.words_per_row, seed=1234 + i) for i in range(UNIQUE_BATCHES)]
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=dev), dev, batch_rows=B, seq_len=a.seq_len)
    eng.set_tag_labels()
    for i in range(a.warmup):
        eng.tag_texts(batches[i % UNIQUE_BATCHES], a.aggregation, a.max_entities)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    entities = 0
    for i in range(a.steps):
        res = eng.tag_texts(batches[i % UNIQUE_BATCHES], a.aggregation, a.max_entities)
        entities += sum(len(r) for r in res.entities)
    elapsed = time.perf_counter() - t0
    t1 = time.perf_counter()
    for i in range(a.steps):
        eng.tag_rows(batches[i % UNIQUE_BATCHES], a.aggregation, a.max_entities)
        torch.cuda.synchronize(dev)
    device_elapsed = time.perf_counter() - t1
    rows = a.steps * B
    assert entities > 0
    fpr = cfg.flops_per_row(a.seq_len)
    print(json.dumps({
        "metric": f"tagged rows/sec map_tag {spec.preset} on 1 MI355X",
        "value": round(rows / elapsed, 2), "unit": "rows/s", "higher_is_better": True,
        "ms_per_step": round(elapsed * 1000.0 / a.steps, 3), "steps": a.steps, "warmup": a.warmup,
        "device_rows_per_sec": round(rows / device_elapsed, 2),
        "device_ms_per_step": round(device_elapsed * 1000.0 / a.steps, 3),
        "entities_per_row": round(entities / rows, 2),
        "config": {"model": a.model, "batch_rows": B, "seq_len": a.seq_len, "words_per_row": a.words_per_row,
                   "aggregation": a.aggregation, "max_entities": a.max_entities, "labels": cfg.tag_labels,
                   "tag_fused": bool(eng.model.tag_fused and eng.model.can_fold(B, a.seq_len)),
                   "flops_per_row": fpr, "hipgraph": eng.use_graph},
    }), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
