#!/usr/bin/env python3
"""map_maxsim measurements on one MI355X. Four modes, each an alternating comparison over ``--rounds``
rounds; one JSON line per measured case.

``--mode kernel``: ``ops.maxsim`` alone on random unit vectors (S tokens of width P per row, every token
live, ``n`` pairs over 32 query rows and ``n / 32`` or 1024 passage rows) against the PyTorch expression on
the same tensors: ``einsum`` of the gathered rows, masked fill, ``amax``, ``sum`` (in chunks of 1024 pairs:
the gathered rows of 32 768 pairs at P = 768 would be 26 GB). FLOPs = ``2 * S * S * P`` per pair.

``--mode pairs``: ``ClassifyEngine.maxsim_rank`` on ``bert-base`` with a late head of ``--late`` columns, 32
queries x 32 own passages of seeded synthetic text end to end, next to ``rerank_pairs`` of the same engine
on the same strings (``bench/rerank.py``'s step).

``--mode shared``: 32 queries x 1024 shared passages (the shared form: 1056 encoder rows and 32 768 MaxSim
pairs) against ``rerank_pairs`` on the same 32 768 (query, passage) pairs.

``--mode index``: the resident token-vector index. Kernel part: ``ops.maxsim_index`` (all form, fp16 and fp32
storage) over a seeded SYNTHETIC index (random unit rows, passage lengths spread uniformly over 40..128
tokens) at 1 and 32 queries x 1024 and 32 768 passages, against ``ops.maxsim`` on the padded fp32 copy of the
same values, outputs compared (fp32: bit for bit). FLOPs count live tokens only. End-to-end part:
``maxsim_index_rank`` over an index that ``maxsim_build`` made from 1024 synthetic passages, against
``maxsim_rank`` on the same strings in the shared form.
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


def _torch_maxsim(qv, lens_q, dv, lens_d, qidx, didx, chunk=1024):
    S = qv.shape[1]
    out = torch.empty(qidx.numel(), dtype=torch.float32, device=qv.device)
    pos = torch.arange(S, device=qv.device)
    for c0 in range(0, qidx.numel(), chunk):
        qi, di = qidx[c0:c0 + chunk].long(), didx[c0:c0 + chunk].long()
        sim = torch.einsum("nip,njp->nij", qv[qi], dv[di])
        sim = sim.masked_fill((pos.view(1, 1, S) >= lens_d[di].view(-1, 1, 1)), float("-inf"))
        m = sim.amax(-1).masked_fill(pos.view(1, S) >= lens_q[qi].view(-1, 1), 0.0)
        out[c0:c0 + chunk] = m.sum(-1)
    return out


def _device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernel_mode(a, dev) -> None:
    from agent_tpu_amd import ops

    S = a.seq_len
    for P in (128, 768):
        for n in (1024, 32768):
            g = torch.Generator().manual_seed(P + n)
            Qn, Dn = 32, 1024
            qv = torch.nn.functional.normalize(torch.randn(Qn, S, P, generator=g), dim=-1).to(dev)
            dv = torch.nn.functional.normalize(torch.randn(Dn, S, P, generator=g), dim=-1).to(dev)
            lens_q = torch.full((Qn,), S, dtype=torch.int32, device=dev)
            lens_d = torch.full((Dn,), S, dtype=torch.int32, device=dev)
            if n == Qn * Dn:  # every query against every passage
                qidx = torch.arange(Qn, dtype=torch.int32, device=dev).repeat_interleave(Dn)
                didx = torch.arange(Dn, dtype=torch.int32, device=dev).repeat(Qn)
            else:  # passage p with query p // 32
                didx = torch.arange(n, dtype=torch.int32, device=dev)
                qidx = (didx // (n // Qn)).to(torch.int32)
            out = torch.empty(n, dtype=torch.float32, device=dev)
            ours = lambda: ops.maxsim(qv, lens_q, dv, lens_d, qidx, didx, out=out)  # noqa: E731
            theirs = lambda: _torch_maxsim(qv, lens_q, dv, lens_d, qidx, didx)  # noqa: E731
            err = (ours() - theirs()).abs().max().item()  # also the warm-up of both
            # windows of about a.window_ms of device time each
            r_ours = max(3, int(a.window_ms / _device_ms(ours, 3)))
            r_torch = max(3, int(a.window_ms / _device_ms(theirs, 3)))
            t_ours, t_torch = [], []
            for _ in range(a.rounds):
                t_ours.append(_device_ms(ours, r_ours))
                t_torch.append(_device_ms(theirs, r_torch))
            flops = 2.0 * S * S * P * n
            mo, mt = min(t_ours), min(t_torch)
            print(json.dumps({
                "metric": f"maxsim kernel S={S} P={P} n={n} on 1 MI355X", "unit": "ms", "higher_is_better": False,
                "value": round(mo, 4), "maxsim_ms": [round(t, 4) for t in t_ours],
                "torch_ms": [round(t, 4) for t in t_torch], "maxsim_tflops": round(flops / mo / 1e9, 2),
                "torch_tflops": round(flops / mt / 1e9, 2), "torch_over_maxsim": round(mt / mo, 3),
                "max_abs_diff": err, "config": {"S": S, "P": P, "n": n, "Qn": Qn, "Dn": Dn, "reps": [r_ours, r_torch],
                                                "rounds": a.rounds, "lens": "all S"},
            }), flush=True)


def engine_mode(a, dev) -> None:
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from agent_tpu_amd.utils.synthetic import make_text_rows

    B = a.batch_rows
    if B <= 0:
        from worker_sizing import classify_batch_rows

        B = classify_batch_rows(torch.cuda.get_device_properties(dev).total_memory, a.model, a.seq_len)
    cfg = config_for(a.model, num_labels=1, late_dim=a.late)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=dev), dev, batch_rows=B, seq_len=a.seq_len, topk=1)
    Q = a.queries
    queries = make_text_rows(Q, a.query_words, seed=1234)
    if a.mode == "pairs":
        N = Q * a.passages
        passages = make_text_rows(N, a.words_per_row, seed=1235)
        goff = [q * a.passages for q in range(Q + 1)]
        late = lambda: eng.maxsim_rank(queries, passages, goff, top_k=a.top_k)  # noqa: E731
        cross = lambda: eng.rerank_pairs(queries, passages, goff, top_k=a.top_k)  # noqa: E731
        pairs = N
    else:
        pool = make_text_rows(a.shared, a.words_per_row, seed=1235)
        flat, goff = pool * Q, [q * a.shared for q in range(Q + 1)]
        late = lambda: eng.maxsim_rank(queries, pool, None, top_k=a.top_k)  # noqa: E731
        cross = lambda: eng.rerank_pairs(queries, flat, goff, top_k=a.top_k)  # noqa: E731
        pairs = Q * a.shared

    def wall(fn, steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            res = fn()  # ends in its D2H: synchronized
        assert bool(torch.isfinite(res.scores).all())
        return (time.perf_counter() - t0) * 1000.0 / steps

    for _ in range(a.warmup):
        late(), cross()
    t_late, t_cross = [], []
    for _ in range(a.rounds):
        t_late.append(wall(late, a.steps))
        t_cross.append(wall(cross, max(1, a.steps // a.cross_div)))
    ml, mc = min(t_late), min(t_cross)
    print(json.dumps({
        "metric": f"scored pairs/sec map_maxsim ({a.mode} form) {a.model}?late={a.late} on 1 MI355X",
        "value": round(pairs / ml * 1000.0, 2), "unit": "pairs/s", "higher_is_better": True,
        "maxsim_ms_per_step": [round(t, 3) for t in t_late], "rerank_ms_per_step": [round(t, 3) for t in t_cross],
        "rerank_pairs_per_sec": round(pairs / mc * 1000.0, 2), "rerank_over_maxsim": round(mc / ml, 3),
        "config": {"model": a.model, "late": a.late, "batch_rows": B, "seq_len": a.seq_len, "queries": Q,
                   "pairs_per_step": pairs, "passages_per_query": a.passages if a.mode == "pairs" else None,
                   "shared_passages": a.shared if a.mode == "shared" else None, "query_words": a.query_words,
                   "words_per_row": a.words_per_row, "top_k": a.top_k, "steps": a.steps, "warmup": a.warmup,
                   "rounds": a.rounds, "hipgraph": eng.use_graph},
    }), flush=True)


def index_mode(a, dev) -> None:
    from agent_tpu_amd import ops
    from agent_tpu_amd.runtime.maxsim_index import TokenIndex

    S, P = a.seq_len, a.late
    for N in (1024, 32768):
        g = torch.Generator().manual_seed(P + N)
        lens = torch.randint(40, 129, (N,), generator=g)
        off = torch.zeros(N + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(lens, 0)
        T = int(off[-1])
        tok16 = torch.nn.functional.normalize(torch.randn(T, P, generator=g), dim=-1).half()  # both dtypes hold these values
        tok32 = tok16.float()
        dv = torch.zeros(N, S, P)
        dv[torch.arange(S).view(1, S) < lens.view(-1, 1)] = tok32  # the padded fp32 copy
        tok16, tok32, dv, off_d = tok16.to(dev), tok32.to(dev), dv.to(dev), off.to(dev)
        lens_d = lens.to(torch.int32).to(dev)
        for Qn in (1, 32):
            qv = torch.nn.functional.normalize(torch.randn(Qn, S, P, generator=g), dim=-1).to(dev)
            lens_q = torch.full((Qn,), 32, dtype=torch.int32, device=dev)  # a 32-token query
            qidx = torch.arange(Qn, dtype=torch.int32, device=dev).repeat_interleave(N)
            didx = torch.arange(N, dtype=torch.int32, device=dev).repeat(Qn)
            out_i, out_p = torch.empty((Qn, N), device=dev), torch.empty(Qn * N, device=dev)
            f16 = lambda: ops.maxsim_index(qv, lens_q, tok16, off_d, out=out_i)  # noqa: E731
            f32 = lambda: ops.maxsim_index(qv, lens_q, tok32, off_d, out=out_i)  # noqa: E731
            pad = lambda: ops.maxsim(qv, lens_q, dv, lens_d, qidx, didx, out=out_p)  # noqa: E731
            want = pad().clone()
            equal32 = bool(torch.equal(f32().reshape(-1), want))
            diff16 = (f16().reshape(-1) - want).abs().max().item()  # the same stored values: only the k order differs
            fns = (f16, f32, pad)
            reps = [max(3, int(a.window_ms / _device_ms(f, 3))) for f in fns]
            times = [[], [], []]
            for _ in range(a.rounds):
                for i, f in enumerate(fns):
                    times[i].append(_device_ms(f, reps[i]))
            flops = 2.0 * 32 * P * T * Qn
            m16, m32, mp = (min(t) for t in times)
            print(json.dumps({
                "metric": f"maxsim_index kernel (synthetic index) P={P} Qn={Qn} N={N} on 1 MI355X", "unit": "ms",
                "higher_is_better": False, "value": round(m16, 4), "index_f16_ms": [round(t, 4) for t in times[0]],
                "index_f32_ms": [round(t, 4) for t in times[1]], "maxsim_padded_ms": [round(t, 4) for t in times[2]],
                "index_f16_tflops": round(flops / m16 / 1e9, 2), "index_f32_tflops": round(flops / m32 / 1e9, 2),
                "maxsim_padded_live_tflops": round(flops / mp / 1e9, 2), "padded_over_index_f16": round(mp / m16, 3),
                "padded_over_index_f32": round(mp / m32, 3), "f32_bit_equal_to_maxsim": equal32, "f16_max_abs_diff": diff16,
                "config": {"synthetic": True, "S": S, "P": P, "Qn": Qn, "N": N, "T": T, "passage_lens": "uniform 40..128",
                           "len_q": 32, "reps": reps, "rounds": a.rounds,
                           "index_bytes": {"f16": T * P * 2, "f32": T * P * 4, "padded_f32": N * S * P * 4}},
            }), flush=True)
        del tok16, tok32, dv

    # end to end: the index built by the engine itself, against the shared form on the same strings
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine
    from agent_tpu_amd.utils.synthetic import make_text_rows

    B = a.batch_rows
    if B <= 0:
        from worker_sizing import classify_batch_rows

        B = classify_batch_rows(torch.cuda.get_device_properties(dev).total_memory, a.model, a.seq_len)
    cfg = config_for(a.model, num_labels=1, late_dim=a.late)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=dev), dev, batch_rows=B, seq_len=a.seq_len, topk=1)
    Q = a.queries
    queries = make_text_rows(Q, a.query_words, seed=1234)
    pool = make_text_rows(a.shared, a.words_per_row, seed=1235)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    tok, lens = eng.maxsim_build(pool)
    torch.cuda.synchronize(dev)
    build_ms = (time.perf_counter() - t0) * 1000.0
    off = torch.zeros(len(pool) + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lens.to(torch.int64), 0)
    idx = {d: TokenIndex(tok.to(t).contiguous(), off, 0, len(pool), d, False)
           for d, t in (("float16", torch.float16), ("float32", torch.float32))}
    fns = (lambda: eng.maxsim_index_rank(queries, idx["float16"], None, a.top_k),
           lambda: eng.maxsim_index_rank(queries, idx["float32"], None, a.top_k),
           lambda: eng.maxsim_rank(queries, pool, None, top_k=a.top_k))

    def wall(fn, steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            res = fn()  # ends in its D2H: synchronized
        assert bool(torch.isfinite(res.scores).all())
        return (time.perf_counter() - t0) * 1000.0 / steps, res

    for _ in range(a.warmup):
        for f in fns:
            f()
    times, last = [[], [], []], [None, None, None]
    for _ in range(a.rounds):
        for i, f in enumerate(fns):
            t, last[i] = wall(f, a.steps)
            times[i].append(t)
    pairs = Q * len(pool)
    m16, m32, ms = (min(t) for t in times)
    print(json.dumps({
        "metric": f"scored pairs/sec map_maxsim (index form, float16) {a.model}?late={a.late} on 1 MI355X",
        "value": round(pairs / m16 * 1000.0, 2), "unit": "pairs/s", "higher_is_better": True,
        "index_f16_ms_per_step": [round(t, 3) for t in times[0]], "index_f32_ms_per_step": [round(t, 3) for t in times[1]],
        "shared_ms_per_step": [round(t, 3) for t in times[2]], "shared_over_index_f16": round(ms / m16, 3),
        "shared_over_index_f32": round(ms / m32, 3), "build_ms_once": round(build_ms, 3),
        "f32_scores_bit_equal_to_shared": bool(torch.equal(last[1].scores, last[2].scores)),
        "f32_ranking_equal_to_shared": bool(torch.equal(last[1].idx, last[2].idx)),
        "f16_max_abs_diff_to_shared": (last[0].scores - last[2].scores).abs().max().item(),
        "config": {"model": a.model, "late": a.late, "batch_rows": B, "seq_len": a.seq_len, "queries": Q,
                   "pairs_per_step": pairs, "passages": len(pool), "tokens": int(tok.shape[0]), "query_words": a.query_words,
                   "words_per_row": a.words_per_row, "top_k": a.top_k, "steps": a.steps, "warmup": a.warmup,
                   "rounds": a.rounds, "hipgraph": eng.use_graph, "text": "seeded synthetic"},
    }), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernel", "pairs", "shared", "index"), default="kernel")
    ap.add_argument("--model", default="bert-base")
    ap.add_argument("--late", type=int, default=128)
    ap.add_argument("--batch-rows", type=int, default=0, help="0: the batch the agent serves this model with")
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--passages", type=int, default=32, help="pairs mode: candidates per query")
    ap.add_argument("--shared", type=int, default=1024, help="shared mode: the size of the shared pool")
    ap.add_argument("--query-words", type=int, default=8)
    ap.add_argument("--words-per-row", type=int, default=150)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--cross-div", type=int, default=1, help="the re-ranker runs steps / cross_div steps per round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=250.0, help="kernel mode: device time per timed window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("[bench/maxsim] needs a ROCm GPU", file=sys.stderr, flush=True)
        return 3
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.mode == "index":
        index_mode(a, dev)
    else:
        kernel_mode(a, dev) if a.mode == "kernel" else engine_mode(a, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
