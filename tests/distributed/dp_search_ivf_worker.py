"""Rank body of the IVF map_search DP test (launched by torch.distributed.run, gloo, CPU engines via
CLASSIFY_DEVICE=cpu): rank 0 runs the op, the others serve in ``worker_loop``. Rank 0 prints one
``RESULT {json}`` line; the test compares it with a single-process run of the same jobs.

The rows have sixteen entries of +-1, so a normalised row is sixteen entries of +-0.25 and every dot product
of a query and a row is exact in any summation order: the CPU twin's matmul over a slice has the bits of the
matmul over the whole corpus."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from agent_tpu_amd.parallel import dp, dp_ops  # noqa: E402

N, D = 101, 64  # slice starts 51 (world 2) and 34, 68 (world 3)
KEYS = ("ids", "scores", "index", "corpus_rows", "top_k")


def sign_rows(n, gen):
    x = torch.zeros(n, D)
    for r in range(n):
        x[r, torch.randperm(D, generator=gen)[:16]] = torch.randint(0, 2, (16,), generator=gen).float() * 2 - 1
    return x


def data():
    gen = torch.Generator().manual_seed(9)
    c = sign_rows(N, gen)
    for r in (33, 34, 50, 51, 67, 68, 100):  # one vector on both sides of every slice boundary: ties across ranks
        c[r] = c[2]
    q = sign_rows(5, gen)
    q[0] = c[2]
    return q, c


def run_jobs(tmp):
    from ops.map_search import IVF_ERRORS, map_search, map_search_batch

    q, c = data()
    cpath, tpath = os.path.join(tmp, "corpus.npy"), os.path.join(tmp, "two.npy")
    if not os.path.exists(cpath):
        np.save(cpath, c.numpy())
        np.save(tpath, c[:2].numpy())
    job = {"query_vectors": q.tolist(), "corpus_uri": cpath, "top_k": 8}
    ix = lambda **kw: dict({"type": "ivf", "clusters": 7, "train_iterations": 4}, **kw)  # noqa: E731
    jobs = {"plain": dict(job),
            "full": dict(job, index=ix(nprobe=7)),
            "two": dict(job, top_k=32, index=ix(nprobe=2)),
            "one": dict(job, index=ix(nprobe=1)),
            "defaults": dict(job, index={"type": "ivf"}),
            "again": dict(job, index=ix(nprobe=7)),
            # two rows: under world 3 the last rank's slice is empty
            "tiny": dict(job, corpus_uri=tpath, index={"type": "ivf", "clusters": 2, "nprobe": 1}),
            "tiny_full": dict(job, corpus_uri=tpath, index={"type": "ivf", "clusters": 2, "nprobe": 2})}
    out = {}
    for name, payload in jobs.items():
        r = map_search(dict(payload))
        out[name] = {k: r.get(k) for k in KEYS}
        out[name]["world"] = r.get("dp_world_size", 1)
        out[name]["cached"] = r["index_cached"]
        out[name]["keys"] = sorted(k for k in r if k not in ("elapsed_ms", "queries_per_sec", "dp_world_size"))
    try:  # the same input error on every rank keeps its type and message
        map_search(dict(job, index=ix(clusters=102)))
        out["bad"] = None
    except Exception as exc:
        out["bad"] = [type(exc).__name__, str(exc), IVF_ERRORS["index"]]
    res = map_search_batch([dict(jobs["two"]), dict(jobs["one"], top_k=3)])  # query_vectors jobs: the single-job path
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
    if os.environ.get("DP_IVF_SINGLE"):  # the single-process reference: no process group
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
