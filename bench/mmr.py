"""Per-call time of ``ops.mmr_select`` beside the ``sim_topk`` call that produced its candidates: device events around
the op call, 10 warm-up and 200 timed calls, median with p10 / p90, one JSON line per (rows, queries, store)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agent_tpu_amd import ops  # noqa: E402

assert torch.cuda.is_available(), "bench/mmr.py needs a ROCm GPU"

dev = torch.device("cuda", 0)
D, R, K = 768, 32, 10


def timed(fn, warm=10, reps=200):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return {"median_us": round(statistics.median(ts), 2), "p10_us": round(ts[len(ts) // 10], 2),
            "p90_us": round(ts[(9 * len(ts)) // 10], 2)}


for N in (65536, 1048576):
    gen = torch.Generator(device=dev).manual_seed(N)
    c32 = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=gen), dim=1).contiguous()
    c16 = c32.half().contiguous()
    for nq in (1, 32, 256):
        q = torch.nn.functional.normalize(torch.randn(nq, D, device=dev, generator=gen), dim=1).contiguous()
        for name, c in (("float32", c32), ("float16", c16)):
            s, i = ops.sim_topk(q, c, R)
            cand = i.to(torch.int32).contiguous()
            rec = {"rows": N, "nq": nq, "store": name,
                   "sim_topk_k32": timed(lambda: ops.sim_topk(q, c, R)),
                   "sim_topk_k10": timed(lambda: ops.sim_topk(q, c, K)),
                   "mmr_select": timed(lambda: ops.mmr_select(s, cand, c, K, 0.5))}
            print(json.dumps(rec), flush=True)
    del c32, c16
