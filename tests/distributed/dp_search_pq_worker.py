"""Rank body of the compressed (PQ) map_search DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line; the test compares it with a single-process run of the same jobs.

Nothing here depends on a summation order across rows: the codebooks come from a sample that every rank reads from
the file, the update sums are integers, a row's code and a row's ADC score depend on that row alone. The ``dot``
jobs take Gaussian rows as they are; the ``cosine`` job takes rows of sixteen +-1 entries, whose normalisation (a
division by 4) is exact.

``DP_PQ_EMPTY_LAST=1`` replaces ``split_range`` in every rank's process by a split that leaves the last rank
without rows: a compressed corpus has at least 256 rows, so the balanced split cannot produce an empty slice at
the world sizes of the test."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

N, D, M = 300, 64, 16  # slice starts 150 (world 2) and 100, 200 (world 3)
KEYS = ("ids", "scores", "compression", "corpus_rows", "top_k")
TIED = (99, 100, 149, 150, 199, 200)


def blob_rows(gen):
    proto = torch.randn(M, 16, D // M, generator=gen)
    pick = torch.randint(0, 16, (N, M), generator=gen)
    x = proto[torch.arange(M)[None, :], pick] + 0.05 * torch.randn(N, M, D // M, generator=gen)
    return x.reshape(N, D).contiguous()


def sign_rows(gen):
    x = torch.zeros(N, D)
    for r in range(N):
        x[r, torch.randperm(D, generator=gen)[:16]] = torch.randint(0, 2, (16,), generator=gen).float() * 2 - 1
    return x


def data():
    gen = torch.Generator().manual_seed(13)
    c, s = blob_rows(gen), sign_rows(gen)
    for r in TIED:  # one vector on both sides of every slice boundary: equal codes, ties across ranks
        c[r], s[r] = c[2], s[2]
    q = torch.cat([c[2:3], c[40:44]])
    return q, c, torch.cat([s[2:3], s[40:44]]), s


def patch_split():
    real = dp.split_range

    def split_range(start, n, world_size, rank):
        if world_size < 2:
            return real(start, n, world_size, rank)
        return real(start, n, world_size - 1, rank) if rank < world_size - 1 else (start + n, 0)

    dp.split_range = split_range


def run_jobs(tmp):
    from ops.map_search import PQ_ERRORS, map_search, map_search_batch

    q, c, qs, s = data()
    cpath, spath = os.path.join(tmp, "corpus.npy"), os.path.join(tmp, "signs.npy")
    if not os.path.exists(spath):
        np.save(cpath, c.numpy())
        np.save(spath, s.numpy())
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "top_k": 8, "metric": "dot"}
    cp = lambda **kw: dict({"type": "pq", "subvectors": M}, **kw)  # noqa: E731
    jobs = {"plain": dict(job, query_vectors=qs.tolist(), corpus_uri=spath, metric="cosine"),  # exact in any order
            "pq": dict(job, compression=cp()),
            "deep": dict(job, top_k=32, compression=cp(train_rows=256, train_iterations=3)),
            "sub8": dict(job, compression=cp(subvectors=8)),
            "cosine": dict(job, query_vectors=qs.tolist(), corpus_uri=spath, metric="cosine", compression=cp()),
            "again": dict(job, top_k=3, compression=cp())}
    out = {}
    for name, payload in jobs.items():
        r = map_search(dict(payload))
        out[name] = {k: r.get(k) for k in KEYS}
        out[name]["world"] = r.get("dp_world_size", 1)
        out[name]["cached"] = r["index_cached"]
        out[name]["keys"] = sorted(k for k in r if k not in ("elapsed_ms", "queries_per_sec", "dp_world_size"))
    try:  # the same input error on every rank keeps its type and message
        map_search(dict(job, compression=cp(train_rows=301)))
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), PQ_ERRORS["compression"]]
    res = map_search_batch([dict(jobs["deep"]), dict(jobs["pq"], top_k=3)])  # query_vectors jobs: the single-job path
    out["batch"] = {"kinds": [r[0] for r in res], "ids": [r[1]["ids"] for r in res]}
    return out


def scenario():
    rank, ws = dp.world()
    if rank != 0:
        dp_ops.worker_loop()
        return None
    out = run_jobs(os.environ["DP_TEST_DIR"])
    dp_ops.shutdown_workers()
    return out


def main():
    if os.environ.get("DP_PQ_EMPTY_LAST"):
        patch_split()
    if os.environ.get("DP_PQ_SINGLE"):  # the single-process reference: no process group
        print("RESULT " + json.dumps(run_jobs(os.environ["DP_TEST_DIR"])), flush=True)
        return
    dist.init_process_group("gloo")
    try:
        res = scenario()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    if int(os.environ.get("RANK", "0")) == 0:
        print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
