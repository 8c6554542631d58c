#!/usr/bin/env python3
"""The near-duplicate kernels and the ``map_dedup`` op on one MI355X.

Per N at D = ``--dim`` on unit-norm random rows of which about 1 % are noisy copies of other rows, at three
thresholds that give roughly 0, N / 100 and N pairs, one JSON line per (variant, round), the variants of a
group alternating for ``--rounds`` rounds in one process:

* ``join`` group: ``ops.sim_join(x, x, t)`` (the whole self-join in one call) against a blocked
  ``torch.nonzero((x_blk @ x[b0:].T) >= t)`` restricted to ``I < J`` (an fp32 GEMM that writes the block's scores,
  a compare, a compaction; the baseline is given the triangle too: a block skips the columns below its first
  row). ``TFps`` counts only the triangle's flops, ``N (N - 1) D``, for both; the f32 rate that
  ``kmeans_assign`` reaches at K = 1024 (profiles/cluster/) is the yardstick for the GEMM part.
  ``--panel-rows`` adds ``sim_join`` variants with other column-panel heights at the middle threshold.
* ``cc``: ``ops.cc_min_labels`` on the sorted pairs of the lowest threshold (E about N), with its round count.

Times are hipEvent windows after a warm-up call, sized to about ``--window`` seconds (at least two calls).
``--op-rows`` rows go to an ``.npy`` and through ``ops.map_dedup`` (``vectors_uri``, ``output: "summary"``), first call
and cached call.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def timed(fn, dev, window: float) -> tuple:
    """(us per call, calls): one warm-up call, one sizing call, then a window of about ``window`` seconds."""
    fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    one = max(time.perf_counter() - t0, 1e-6)
    iters = int(min(200, max(2, window / one)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters, iters


def corpus(N: int, D: int, dev, gen) -> torch.Tensor:
    """Unit rows; N / 100 of them are copies of other rows plus noise (cosine about 0.98)."""
    x = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1)
    n = max(1, N // 100)
    perm = torch.randperm(N, device=dev, generator=gen)
    src, dst = perm[:n], perm[n:2 * n]
    x[dst] = x[src] + 0.2 / math.sqrt(D) * torch.randn(n, D, device=dev, generator=gen)
    return torch.nn.functional.normalize(x, dim=1).contiguous()


def torch_join(x: torch.Tensor, t: float, block: int):
    """Baseline: per block of rows one GEMM against the rows from the block's first on, compare, nonzero."""
    N = x.shape[0]
    out = []
    for b0 in range(0, N, block):
        b1 = min(b0 + block, N)
        hit = (x[b0:b1] @ x[b0:].T) >= t
        hit[:, :b1 - b0].triu_(1)  # the diagonal block: I < J
        ij = hit.nonzero()
        ij += b0
        out.append(ij)
    return torch.cat(out)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--block", type=int, default=2048, help="rows per GEMM of the torch baseline")
    ap.add_argument("--panel-rows", type=int, nargs="*", default=[], help="extra sim_join variants (multiples of 32)")
    ap.add_argument("--op-rows", type=int, default=262144)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/dedup] needs a ROCm GPU", file=sys.stderr, flush=True)
        return 3
    from agent_tpu_amd import ops

    dev = torch.device("cuda", 0)
    D = a.dim
    gen = torch.Generator(device=dev).manual_seed(0)
    sink = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for N in a.rows:
        x = corpus(N, D, dev, gen)
        cap = max(4 * N, 65536)
        # random unit rows: cosine about N(0, 1 / D); about N of the N^2 / 2 pairs lie above z sigma, P(z) = 2 / N
        z = math.sqrt(2.0) * float(torch.erfinv(torch.tensor(1.0 - 4.0 / N, dtype=torch.float64)))
        thresholds = {"none": 1.5, "planted": 0.9, "about_N": z / math.sqrt(D)}
        flops = float(N) * (N - 1) * D
        edges = None
        for label, t in thresholds.items():
            pairs, scores, count = ops.sim_join(x, x, t, cap=cap)
            n_kernel = int(count.item())
            n_torch = int(torch_join(x, t, a.block).shape[0])
            if label == "about_N":
                edges = ops.sort_pairs(pairs[:min(n_kernel, cap)], scores[:min(n_kernel, cap)])[0]
            variants = {"sim_join": lambda t=t: ops.sim_join(x, x, t, cap=cap),
                        "torch_blocked_nonzero": lambda t=t: torch_join(x, t, a.block)}
            if label == "planted":
                for pr in a.panel_rows:
                    variants[f"sim_join_panel{pr}"] = lambda t=t, pr=pr: ops.sim_join(x, x, t, cap=cap, panel_rows=pr)
            for rnd in range(a.rounds):
                for name, fn in variants.items():
                    us, iters = timed(fn, dev, a.window)
                    emit({"bench": "dedup", "group": "join", "variant": name, "N": N, "D": D, "threshold": round(t, 6),
                          "case": label, "round": rnd, "us": round(us, 1), "iters": iters,
                          "pairs": n_torch if name.startswith("torch") else n_kernel,
                          "triangle_TFps": round(flops / us / 1e6, 2)})
            del pairs, scores, count, variants
        labels, rounds = ops.cc_min_labels(edges, N, with_rounds=True)
        groups = int((torch.bincount(labels.long(), minlength=N) >= 2).sum())
        for rnd in range(a.rounds):
            us, iters = timed(lambda: ops.cc_min_labels(edges, N), dev, a.window)
            emit({"bench": "dedup", "group": "cc", "variant": "cc_min_labels", "N": N, "E": int(edges.shape[0]),
                  "round": rnd, "us": round(us, 1), "iters": iters, "rounds": rounds, "groups": groups})
        del x, edges, labels
        torch.cuda.empty_cache()
    if a.op_rows > 0:
        import numpy as np

        from ops.map_dedup import map_dedup

        N = a.op_rows
        x = corpus(N, D, dev, gen)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "vectors.npy")
            np.save(path, x.cpu().numpy())
            del x
            for call in ("first", "cached"):
                t0 = time.perf_counter()
                r = map_dedup({"vectors_uri": path, "threshold": 0.9, "output": "summary"})
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                emit({"bench": "dedup", "group": "op", "variant": f"map_dedup_vectors_uri_{call}", "N": N, "D": D,
                      "wall_ms": round(dt * 1000.0, 1), "index_cached": r["index_cached"], "pair_count": r["pair_count"],
                      "group_count": r["group_count"], "duplicate_count": r["duplicate_count"],
                      "largest_group": r["largest_group"]})
    if sink:
        sink.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
