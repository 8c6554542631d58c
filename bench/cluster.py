#!/usr/bin/env python3
"""The k-means kernels and the ``map_cluster`` op on one MI355X.

Per (N, K) at D = ``--dim`` on unit-norm random rows with random unit centroids, one JSON line per
(variant, round), the variants of a group alternating for ``--rounds`` rounds in one process:

* ``assign`` group: ``ops.kmeans_assign(x, c)`` against ``ops.sim_topk(x, c, 1)`` (the same answer through the
  search kernel: a workspace, a merge kernel, no bias, no changed count) and against
  ``torch.argmax(x @ c.T, 1)`` (an fp32 GEMM that writes the ``[N, K]`` scores, then a reduction). TF/s is
  ``2 N K D / t``, the row rate ``4 N D / t`` in TB/s.
* ``update`` group: ``ops.kmeans_update(x, labels, K, s)`` (int64 order-free sums) against
  ``torch.zeros(K, D).index_add_(0, labels, x)`` in fp32; the labels are those of the assign step. TB/s is
  ``4 N D / t``.
* ``iteration``: assign + update + finalize as the loop runs them (no copy back), once per round.

Times are hipEvent windows after a warm-up call, sized to about ``--window`` seconds. ``--op-rows`` rows go to
an ``.npy`` and through ``ops.map_cluster`` (``vectors_uri``, ``output: "summary"``), first call and cached call.
"""
from __future__ import annotations

import argparse
import json
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
    iters = int(min(200, max(3, window / one)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters, iters


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--k", type=int, nargs="+", default=[16, 256, 1024])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--op-rows", type=int, default=262144)
    ap.add_argument("--op-k", type=int, default=256)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/cluster] needs a ROCm GPU", file=sys.stderr, flush=True)
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
        x = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1).contiguous()
        shift = ops.fixed_shift(N, float(x.abs().max()))
        for K in a.k:
            c = torch.nn.functional.normalize(torch.randn(K, D, device=dev, generator=gen), dim=1).contiguous()
            labels, best, _ = ops.kmeans_assign(x, c)
            s1, i1 = ops.sim_topk(x, c, 1)
            same = bool(torch.equal(labels.long(), i1[:, 0])) and bool(torch.equal(best, s1[:, 0]))
            agree = float((torch.argmax(x @ c.T, 1) == labels).float().mean())
            del s1, i1
            sums, counts = ops.kmeans_update(x, labels, K, shift)
            ref = torch.zeros(K, D, device=dev).index_add_(0, labels.long(), x)
            err = float((sums.double() / 2.0 ** shift - ref.double()).abs().max())
            lab64 = labels.long()
            groups = {
                "assign": {"kmeans_assign": lambda: ops.kmeans_assign(x, c, None, labels),
                           "sim_topk_k1": lambda: ops.sim_topk(x, c, 1),
                           "torch_argmax_gemm": lambda: torch.argmax(x @ c.T, 1)},
                "update": {"kmeans_update": lambda: ops.kmeans_update(x, labels, K, shift),
                           "torch_index_add_f32": lambda: torch.zeros(K, D, device=dev).index_add_(0, lab64, x)},
            }

            def iteration():
                lb, _, _ = ops.kmeans_assign(x, c, None, labels)
                sm, ct = ops.kmeans_update(x, lb, K, shift)
                return ops.kmeans_finalize(sm, ct, c, shift, "cosine")

            groups["iteration"] = {"assign_update_finalize": iteration}
            for rnd in range(a.rounds):
                for group, variants in groups.items():
                    for name, fn in variants.items():
                        us, iters = timed(fn, dev, a.window)
                        rec = {"bench": "cluster", "group": group, "variant": name, "N": N, "K": K, "D": D, "round": rnd,
                               "us": round(us, 1), "iters": iters, "row_TBps": round(4.0 * N * D / us / 1e6, 3)}
                        if group != "update":
                            rec["TFps"] = round(2.0 * N * K * D / us / 1e6, 2)
                        if name == "kmeans_assign":
                            rec.update(bit_equal_sim_topk=same, argmax_agreement=round(agree, 6))
                        if name == "kmeans_update":
                            rec["max_abs_diff_vs_fp32_index_add"] = err
                        emit(rec)
            del c, labels, best, sums, counts, ref, lab64, groups
        del x
        torch.cuda.empty_cache()
    if a.op_rows > 0:
        import numpy as np

        from ops.map_cluster import map_cluster

        N = a.op_rows
        x = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "vectors.npy")
            np.save(path, x.cpu().numpy())
            del x
            for call in ("first", "cached"):
                t0 = time.perf_counter()
                r = map_cluster({"vectors_uri": path, "k": a.op_k, "max_iter": 10, "output": "summary"})
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                emit({"bench": "cluster", "group": "op", "variant": f"map_cluster_vectors_uri_{call}", "N": N, "K": a.op_k,
                      "D": D, "wall_ms": round(dt * 1000.0, 1), "iterations": r["iterations"], "converged": r["converged"],
                      "index_cached": r["index_cached"], "ms_per_iteration": round(dt * 1000.0 / r["iterations"], 2),
                      "objective": r["objective"], "empty_clusters": r["empty_clusters"]})
    if sink:
        sink.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
