#!/usr/bin/env python3
"""Isolated ``sim_topk`` against ``torch.topk(q @ c.T, k)`` on one MI355X.

A: ``ops.sim_topk(q, c, k)``: the fp32 similarity GEMM with the top-k in its epilogue (the
``[queries, N]`` scores never written). B: the same tensors through torch: an fp32 GEMM that
writes the scores, then ``torch.topk``. D = 768, ``top_k`` 10, N in ``--rows`` and the query counts
in ``--queries``. A corpus smaller than 512 MiB rotates through ``--buffers`` copies so that no call
finds it in the 256 MiB Infinity Cache. A and B alternate for ``--rounds`` rounds in one process;
one JSON line per (N, queries, variant, round): us per call from hipEvents after warm-up, the
effective corpus rate ``N * D * 4 / t`` in TB/s (for B too: what the same answer costs per corpus
byte), and TF/s (``2 * queries * N * D / t``). ``--splits`` overrides the automatic split count.

``--corpus-dtype float16`` compares the two corpus kernels instead, on the same values: A is
``ops.sim_topk(q, c16, k)`` over ``c16 = normalize(randn).half()`` (twice the buffers, so that the
rotation covers the same bytes), B is ``ops.sim_topk(q, c16.float(), k)``. The corpus rate is then
that of the bytes actually read (2 or 4 per element).

``--filter-density d [d ...]`` with ``--filter-pattern {blocks,random}`` measures the row filter
instead (:func:`filter_bench`): the unfiltered search, the masked one, torch's masked top-k and the
gather routes, alternating; one JSON line per (N, queries, density, variant, round).

``--ivf-clusters K`` with ``--nprobe n [n ...]`` measures the IVF index instead (:func:`ivf_bench`): the
exact search and ``ops.sim_topk_ivf`` on the same tensors, alternating, with recall against the exact result,
the build time and the probe-and-plan time; one JSON line per (N, queries, nprobe, variant, round).

``--pq-subvectors M`` measures the product-quantized search instead (:func:`pq_bench`): the exact fp16-resident
search and ``ops.sim_topk_pq`` over ``M``-byte codes of the same rows, alternating, with the resident bytes of
both, recall against the exact result and the training and encoding times; one JSON line per (N, queries, variant,
round).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def filter_bench(a, ops, dev) -> int:
    """``--filter-density``: what a row filter costs and saves, per (N, queries, density) point of
    ``--filter-pattern``. Five arms alternate for ``--rounds`` rounds on the same tensors:
    ``unfiltered`` (``sim_topk`` without a mask: the yardstick), ``masked`` (``sim_topk`` with the
    mask), ``torch_masked_topk`` (``torch.topk((q @ c.T).masked_fill(~m, -inf), k)``; fp32 corpus
    only), ``gather_then_sim_topk`` (``c[rows]`` gathered inside the timed call) and
    ``sim_topk_on_gathered`` (the gather done beforehand). ``blocks`` allows one contiguous run of
    rows (it starts at row N // 3 + 5, inside a word); ``random`` allows every row independently."""
    D, k = a.dim, a.top_k
    gen = torch.Generator(device=dev).manual_seed(0)
    half = a.corpus_dtype == "float16"
    size = 2 if half else 4
    for N in a.rows:
        nbuf = a.buffers if N * D * size < 512 * 2 ** 20 else 1
        cs = [torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1) for _ in range(nbuf)]
        if half:
            cs = [c.half() for c in cs]
        for density in a.filter_density:
            if a.filter_pattern == "blocks":
                m = max(1, min(N, round(density * N)))
                lo = min(N // 3 + 5, N - m)
                n = torch.arange(N, device=dev)
                bits = (n >= lo) & (n < lo + m)
            else:
                bits = torch.rand(N, device=dev, generator=gen) < density
                bits[0] = True  # never empty
            mask = ops.row_mask_from_bits(bits)
            rows = bits.nonzero().flatten()
            gathered = [c[rows].contiguous() for c in cs]
            for nq in a.queries:
                q = torch.nn.functional.normalize(torch.randn(nq, D, device=dev, generator=gen), dim=1)
                arms = [("unfiltered", lambda i: ops.sim_topk(q, cs[i], k, splits=a.splits or None)),
                        ("masked", lambda i: ops.sim_topk(q, cs[i], k, splits=a.splits or None, mask=mask))]
                if not half:
                    arms.append(("torch_masked_topk",
                                 lambda i: torch.topk((q @ cs[i].T).masked_fill(~bits, float("-inf")), min(k, mask.count))))
                arms += [("gather_then_sim_topk", lambda i: ops.sim_topk(q, cs[i][rows].contiguous(), k)),
                         ("sim_topk_on_gathered", lambda i: ops.sim_topk(q, gathered[i], k))]

                def timed(fn):
                    for i in range(max(nbuf, 2)):
                        fn(i % nbuf)
                    torch.cuda.synchronize(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for it in range(a.iters):
                        fn(it % nbuf)
                    e1.record()
                    torch.cuda.synchronize(dev)
                    return e0.elapsed_time(e1) * 1e3 / a.iters  # us per call

                ms, mi = arms[1][1](0)
                gs, gi = arms[-1][1](0)
                same = bool(torch.equal(ms, gs) and torch.equal(mi, rows[gi]))  # bit for bit, by construction
                for r in range(a.rounds):
                    for variant, fn in arms:
                        us = timed(fn)
                        print(json.dumps({"bench": "search_filter", "variant": variant, "pattern": a.filter_pattern,
                                          "density": density, "N": N, "filter_rows": mask.count,
                                          "live_words": int(mask.live.numel()), "words": int(mask.words.numel()),
                                          "queries": nq, "dim": D, "top_k": k, "corpus_dtype": a.corpus_dtype,
                                          "round": r, "us_per_call": round(us, 2),
                                          "masked_equals_gathered": same}), flush=True)
            del gathered
        del cs
    return 0


def ivf_bench(a, ops, dev) -> int:
    """``--ivf-clusters K`` with ``--nprobe n [n ...]``: the IVF search against the exact one on the same
    tensors. The corpus is a seeded mixture of ``K`` Gaussians (unit-norm centres, noise of
    ``--ivf-noise`` per column, rows normalised): no real embeddings are at hand, so the recall figures say how the
    index does on clustered synthetic data, not on a text corpus. The index is built by ``runtime.ivf.build``
    (timed once, host clock around a synchronise). Per (N, queries, nprobe) two arms alternate for ``--rounds``
    rounds: ``exact`` (``ops.sim_topk`` over the original-order rows) and ``ivf`` (``ops.sim_topk_ivf``, the
    probe and the plan included); ``--query-sets`` query batches rotate in both arms, so that a call does not
    find the clusters it probes in the Infinity Cache from the call before. ``plan_us`` is the probe plus the
    plan alone, ``recall`` the mean share of the exact top-k that the IVF list holds."""
    import time

    from agent_tpu_amd.runtime import ivf
    from agent_tpu_amd.runtime.search import normalize_rows

    D, k, K = a.dim, a.top_k, a.ivf_clusters
    gen = torch.Generator(device=dev).manual_seed(0)

    def mixture(n, centres):
        pick = torch.randint(0, centres.shape[0], (n,), device=dev, generator=gen)
        return normalize_rows(centres[pick] + a.ivf_noise * torch.randn(n, D, device=dev, generator=gen)).contiguous()

    for N in a.rows:
        centres = normalize_rows(torch.randn(K, D, device=dev, generator=gen))
        x = mixture(N, centres)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        vec, rid, off, cent, iters, converged = ivf.build(x, K, a.ivf_train_iterations)
        torch.cuda.synchronize(dev)
        build_ms = (time.perf_counter() - t0) * 1e3
        sizes = (off[1:] - off[:-1]).float()
        for nq in a.queries:
            qs = [mixture(nq, centres) for _ in range(a.query_sets)]
            for nprobe in a.nprobe:
                items = int(min(nq * nprobe, K) + nq * nprobe // 16)

                def exact(i):
                    return ops.sim_topk(qs[i], x, k, splits=a.splits or None)

                def approx(i):
                    return ops.sim_topk_ivf(qs[i], vec, rid, off, cent, k, nprobe)

                def plan(i):
                    return ops.ivf_plan(ops.sim_topk(qs[i], cent, nprobe)[1], K, items)

                def timed(fn):
                    for i in range(a.query_sets):
                        fn(i)
                    torch.cuda.synchronize(dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for it in range(a.iters):
                        fn(it % a.query_sets)
                    e1.record()
                    torch.cuda.synchronize(dev)
                    return e0.elapsed_time(e1) * 1e3 / a.iters  # us per call

                hit = 0
                for i in range(a.query_sets):
                    ei, ai = exact(i)[1], approx(i)[1]
                    hit += int((ai[:, :, None] == ei[:, None, :]).any(1).sum())
                recall = hit / (a.query_sets * nq * k)
                full = approx(0) if nprobe == K else None
                for r in range(a.rounds):
                    for variant, fn in (("exact", exact), ("ivf", approx), ("ivf_probe_and_plan", plan)):
                        us = timed(fn)
                        print(json.dumps({"bench": "search_ivf", "variant": variant, "N": N, "queries": nq, "dim": D,
                                          "top_k": k, "clusters": K, "nprobe": nprobe, "round": r,
                                          "us_per_call": round(us, 2), "recall": round(recall, 4),
                                          "build_ms": round(build_ms, 1), "train_iterations": iters,
                                          "converged": converged, "largest_cluster": int(sizes.max()),
                                          "mean_cluster": round(float(sizes.mean()), 1), "noise": a.ivf_noise,
                                          "query_sets": a.query_sets,
                                          "splits": ops.search.ivf_splits(nq, nprobe, K, N, dev),
                                          "exact_when_all_probed": None if full is None else bool(
                                              torch.equal(full[1], exact(0)[1]))}), flush=True)
        del x, vec
    return 0


def pq_bench(a, ops, dev) -> int:
    """``--pq-subvectors M``: the product-quantized search against the exact fp16-resident one on the same rows.
    The corpus is :func:`ivf_bench`'s seeded Gaussian mixture (``--ivf-clusters`` centres, default 1024 here;
    ``--ivf-noise``): the recall figures say how PQ does on clustered synthetic data, not on a text corpus. The
    codebooks are trained by ``runtime.pq.train`` on the seeded sample of ``--pq-train-rows`` rows and the corpus is
    encoded in chunks (both timed once, host clock around a synchronise). Per (N, queries) three arms alternate for
    ``--rounds`` rounds: ``exact_f16`` (``ops.sim_topk`` over the rows as fp16), ``pq`` (``ops.sim_topk_pq``: the
    table kernel, the scan and the merge) and ``pq_lut`` (the table kernel alone); ``--query-sets`` query batches
    rotate in every arm. ``recall`` is the mean share of the exact fp16 top-k that the PQ list holds,
    ``resident_bytes`` what each arm keeps on the device."""
    import time

    from agent_tpu_amd.runtime import pq
    from agent_tpu_amd.runtime.search import CHUNK_BYTES, normalize_rows

    D, k, M = a.dim, a.top_k, a.pq_subvectors
    K = a.ivf_clusters or 1024
    gen = torch.Generator(device=dev).manual_seed(0)

    def mixture(n, centres):
        pick = torch.randint(0, centres.shape[0], (n,), device=dev, generator=gen)
        return normalize_rows(centres[pick] + a.ivf_noise * torch.randn(n, D, device=dev, generator=gen)).contiguous()

    for N in a.rows:
        centres = normalize_rows(torch.randn(K, D, device=dev, generator=gen))
        x = mixture(N, centres)
        T = min(N, a.pq_train_rows)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        books = pq.train(x[pq.sample_rows(N, T).to(dev)].contiguous(), M, a.pq_train_iterations)
        torch.cuda.synchronize(dev)
        train_ms = (time.perf_counter() - t0) * 1e3
        bias = ops.pq_bias(books)
        rows = max(64, CHUNK_BYTES // (D * 4) // 64 * 64)
        t0 = time.perf_counter()
        codes = ops.pq_interleave(torch.cat([ops.pq_encode(x[lo:lo + rows], books, bias) for lo in range(0, N, rows)]))
        torch.cuda.synchronize(dev)
        encode_ms = (time.perf_counter() - t0) * 1e3
        err = float((x[:65536] - ops.pq_decode(ops.pq_deinterleave(codes)[:65536], books)).norm(dim=1).mean())
        x16 = x.half()
        del x
        resident = {"exact_f16": x16.numel() * 2, "pq": codes.data.numel() + books.numel() * 4, "pq_lut": 0}
        for nq in a.queries:
            qs = [mixture(nq, centres) for _ in range(a.query_sets)]

            def exact(i):
                return ops.sim_topk(qs[i], x16, k, splits=a.splits or None)

            def approx(i):
                return ops.sim_topk_pq(qs[i], books, codes, k, splits=a.splits or None)

            def lut(i):
                return ops.pq_lut(qs[i], books)

            def timed(fn):
                for i in range(a.query_sets):
                    fn(i)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for it in range(a.iters):
                    fn(it % a.query_sets)
                e1.record()
                torch.cuda.synchronize(dev)
                return e0.elapsed_time(e1) * 1e3 / a.iters  # us per call

            hit = top1 = 0
            for i in range(a.query_sets):
                ei, ai = exact(i)[1], approx(i)[1]
                hit += int((ai[:, :, None] == ei[:, None, :]).any(1).sum())
                top1 += int((ai[:, 0] == ei[:, 0]).sum())
            recall = hit / (a.query_sets * nq * k)
            for r in range(a.rounds):
                for variant, fn in (("exact_f16", exact), ("pq", approx), ("pq_lut", lut)):
                    us = timed(fn)
                    print(json.dumps({"bench": "search_pq", "variant": variant, "N": N, "queries": nq, "dim": D,
                                      "top_k": k, "subvectors": M, "bytes_per_row": M, "round": r,
                                      "us_per_call": round(us, 2), "resident_bytes": resident[variant],
                                      "recall": round(recall, 4), "top1_agreement": round(top1 / (a.query_sets * nq), 4),
                                      "train_ms": round(train_ms, 1), "encode_ms": round(encode_ms, 1),
                                      "train_rows": T, "train_iterations": a.pq_train_iterations,
                                      "mean_reconstruction_error": round(err, 4), "mixture_centres": K,
                                      "noise": a.ivf_noise, "query_sets": a.query_sets,
                                      "splits": a.splits or ops.pq.pq_auto_splits(N, dev)}), flush=True)
        del x16, codes
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--corpus-dtype", choices=("float32", "float16"), default="float32")
    ap.add_argument("--filter-density", type=float, nargs="+", default=None,
                    help="run the row-filter comparison at these fractions of allowed rows instead")
    ap.add_argument("--filter-pattern", choices=("blocks", "random"), default="blocks")
    ap.add_argument("--ivf-clusters", type=int, default=0, help="run the IVF comparison with this many clusters instead")
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--ivf-train-iterations", type=int, default=10)
    ap.add_argument("--ivf-noise", type=float, default=0.05, help="per-column noise of the IVF mixture corpus")
    ap.add_argument("--query-sets", type=int, default=16, help="query batches that the IVF comparison rotates through")
    ap.add_argument("--pq-subvectors", type=int, default=0,
                    help="run the product-quantization comparison with this many bytes per row instead")
    ap.add_argument("--pq-train-rows", type=int, default=65536)
    ap.add_argument("--pq-train-iterations", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/search] needs a ROCm GPU", file=sys.stderr, flush=True)
        return 3
    from agent_tpu_amd import ops

    dev = torch.device("cuda", 0)
    if a.filter_density:
        return filter_bench(a, ops, dev)
    if a.pq_subvectors:
        return pq_bench(a, ops, dev)
    if a.ivf_clusters:
        return ivf_bench(a, ops, dev)
    D, k = a.dim, a.top_k
    gen = torch.Generator(device=dev).manual_seed(0)
    half = a.corpus_dtype == "float16"
    for N in a.rows:
        nbuf = a.buffers if N * D * 4 < 512 * 2 ** 20 else 1
        cs = [torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1) for _ in range(nbuf)]
        if half:
            c16 = [c.half() for c in cs]
            cs = [c.float() for c in c16]
            if nbuf > 1:
                c16 += [torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1).half()
                        for _ in range(nbuf)]
        for nq in a.queries:
            q = torch.nn.functional.normalize(torch.randn(nq, D, device=dev, generator=gen), dim=1)

            def fused(i):
                return ops.sim_topk(q, cs[i], k, splits=a.splits or None)

            def partner(i):
                return torch.topk(q @ cs[i].T, k)

            def fused16(i):
                return ops.sim_topk(q, c16[i], k, splits=a.splits or None)

            def timed(fn, nb):
                for i in range(max(nb, 2)):
                    fn(i % nb)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for it in range(a.iters):
                    fn(it % nb)
                e1.record()
                torch.cuda.synchronize(dev)
                return e0.elapsed_time(e1) * 1e3 / a.iters  # us per call

            if half:  # (variant, call, buffers it rotates through, bytes per corpus element)
                variants = (("sim_topk_f16", fused16, len(c16), 2), ("sim_topk_f32_same_values", fused, nbuf, 4))
            else:
                variants = (("sim_topk", fused, nbuf, 4), ("torch_matmul_topk", partner, nbuf, 4))
            same = torch.equal(variants[0][1](0)[1], variants[1][1](0)[1])  # random data: no ties expected
            for r in range(a.rounds):
                for variant, fn, nb, size in variants:
                    us = timed(fn, nb)
                    print(json.dumps({"bench": "search", "variant": variant, "N": N, "queries": nq, "dim": D, "top_k": k,
                                      "round": r, "us_per_call": round(us, 2),
                                      "corpus_tbs": round(N * D * size / us / 1e6, 3),
                                      "tflops": round(2.0 * nq * N * D / us / 1e6, 2),
                                      "ids_equal_between_variants": same}), flush=True)
        del cs
        if half:
            del c16
    return 0


if __name__ == "__main__":
    sys.exit(main())
