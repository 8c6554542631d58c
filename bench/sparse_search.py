#!/usr/bin/env python3
"""The inverted-index build and scan (``sparse_index.hip``) against the PyTorch composition on one MI355X.

Corpus, seeded and generated on the device by groups of 16 blocks: ``--rows`` rows (default 2^20) over
``V = 30522``; row ``r`` draws ``96 + r % 64`` token ids (96..159) from a Zipf law (``p(t) ~ 1 / (t + 1)``, by the
inverse CDF of a log-uniform), duplicates inside a row dropped, so the realised mean (printed as ``nnz / rows``) is
lower; weights uniform in [0.05, 3.05). Queries: ``--query-terms`` draws (default 32) each from the same law,
deduplicated, weights uniform in [0.1, 2.1); batches of 1, 32 and 256.

* ``build``: ``ops.sparse_index_build`` of every group (its checks included) and the join, once;
* ``scan``: ``ops.sparse_scan_topk`` at ``k = 10``;
* ``torch``: the only other way on the same device: the corpus as a ``torch.sparse`` CSR tensor (the fp16-rounded
  weights as fp32) times the dense ``[V, nq]`` query matrix, then ``topk`` over the rows.

Both arms alternate for ``--rounds`` rounds in one process after warm-up; one JSON line per (variant, nq, round) with
us per call from hipEvents. ``scan`` lines carry the bytes the scan must read, from the shapes: 4 B per posting of
the queries' terms plus 8 B of offsets per (block, term); ``torch`` lines the CSR's bytes. Before timing, the scan
of a two-block slice is asserted equal to the PyTorch twin. ``--no-torch`` runs the scan alone (for a profiler).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

GROUP_BLOCKS = 16


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


def zipf(n: int, V: int, gen, dev) -> torch.Tensor:
    u = torch.rand(n, device=dev, generator=gen, dtype=torch.float64)
    return (torch.exp(u * math.log(V + 1.0)) - 1.0).long().clamp_(0, V - 1)


def csr_rows(lens: torch.Tensor, V: int, lo: float, span: float, gen, dev):
    """(indptr int64, indices int32, data fp32) of rows with ``lens`` Zipf draws each, duplicates dropped, weights in [lo, lo + span)."""
    n = int(lens.numel())
    row = torch.repeat_interleave(torch.arange(n, device=dev), lens)
    key = torch.unique(row * V + zipf(int(row.numel()), V, gen, dev))
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(key // V, minlength=n), 0)
    data = torch.rand(int(key.numel()), device=dev, generator=gen) * span + lo
    return indptr, (key % V).int().contiguous(), data.contiguous()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2 ** 20)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--query-terms", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args(argv)
    from agent_tpu_amd import ops
    from agent_tpu_amd.ops.sparse_index import BLOCK_ROWS

    dev = torch.device("cuda", 0)
    N, V, k = a.rows, a.vocab, a.top_k
    gen = torch.Generator(device=dev).manual_seed(0)
    step, parts, rows_csr, build_s = GROUP_BLOCKS * BLOCK_ROWS, [], [], 0.0
    for r0 in range(0, N, step):
        r = torch.arange(r0, min(r0 + step, N), device=dev)
        indptr, tok, w = csr_rows(96 + r % 64, V, 0.05, 3.0, gen, dev)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        parts.append(ops.sparse_index_build(indptr, tok, w, V))
        torch.cuda.synchronize(dev)
        build_s += time.perf_counter() - t0
        rows_csr.append((indptr, tok, w))
    t0 = time.perf_counter()
    index = ops.sparse_index_cat(parts)
    torch.cuda.synchronize(dev)
    build_s += time.perf_counter() - t0
    nb = -(-N // BLOCK_ROWS)
    print(json.dumps({"bench": "sparse_search", "variant": "build", "rows": N, "V": V, "nnz": index.nnz,
                      "terms_per_row": round(index.nnz / N, 1), "blocks": nb, "ms": round(build_s * 1000, 1),
                      "index_bytes": 4 * index.nnz + 4 * nb * (V + 1)}), flush=True)
    del parts

    batches = {nq: csr_rows(torch.full((nq,), a.query_terms, device=dev), V, 0.1, 2.0, gen, dev) for nq in (1, 32, 256)}
    indptr, tok, w = rows_csr[0]  # the slice: the first two blocks
    n = min(2 * BLOCK_ROWS, int(indptr.numel()) - 1)
    e = int(indptr[n])
    sl = ops.sparse_index_build(indptr[:n + 1].contiguous(), tok[:e].contiguous(), w[:e].contiguous(), V)
    for got, want in zip(ops.sparse_scan_topk(sl, *batches[32], k), ops.sparse_scan_topk_ref(sl, *batches[32], k)):
        assert torch.equal(got, want), "the scan differs from its PyTorch twin"
    del sl

    tok_postings = (index.offsets[:, 1:] - index.offsets[:, :-1]).sum(0, dtype=torch.int64)  # per token, all blocks
    csr = None
    if not a.no_torch:
        base, ptrs = 0, [torch.zeros(1, dtype=torch.int64, device=dev)]
        for indptr, _, _ in rows_csr:
            ptrs.append(indptr[1:] + base)
            base += int(indptr[-1])
        csr = torch.sparse_csr_tensor(torch.cat(ptrs), torch.cat([t for _, t, _ in rows_csr]).long(),
                                      torch.cat([w for _, _, w in rows_csr]).half().float(), size=(N, V))
    csr_bytes = base * 12 + 8 * (N + 1) if csr is not None else None  # int64 column ids, fp32 values
    del rows_csr

    for rnd in range(a.rounds):
        for nq, (q_ptr, q_tok, q_w) in batches.items():
            us = timed(lambda: ops.sparse_scan_topk(index, q_ptr, q_tok, q_w, k), dev, a.iters)
            nbytes = 4 * int(tok_postings[q_tok.long()].sum()) + 8 * nb * int(q_tok.numel())
            print(json.dumps({"bench": "sparse_search", "variant": "scan", "nq": nq, "round": rnd, "k": k,
                              "query_terms": int(q_tok.numel()), "us": round(us, 1), "bytes": nbytes,
                              "GB_per_s": round(nbytes / us / 1e3, 1)}), flush=True)
            if csr is not None:
                Q = torch.zeros((V, nq), device=dev)
                Q[q_tok.long(), torch.repeat_interleave(torch.arange(nq, device=dev), q_ptr[1:] - q_ptr[:-1])] = q_w
                us = timed(lambda: torch.topk((csr @ Q).T, k, dim=1), dev, a.iters)
                print(json.dumps({"bench": "sparse_search", "variant": "torch", "nq": nq, "round": rnd, "k": k,
                                  "us": round(us, 1), "bytes": csr_bytes}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
