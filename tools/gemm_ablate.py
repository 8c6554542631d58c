#!/usr/bin/env python3
"""Timing-only ablations of the persistent 256x256 GEMM (results WRONG), against the production kernel.

The library dispatches no DBG build of `gemm256s_kernel`. This tool compiles tools/gemm_ablate.hip
(which includes the kernel source) into tools/_gemm_ablate.so and times, in one process and in
interleaved rounds with hipEvents, the production instantiation against a DBG one:

  --dbg 512   the line epilogue without its LDS transposes (the bound on what fragment-order
              activations can save: same loads, stores and addresses, no scratch round trips)

on the BERT-base encoder GEMMs at M = rows x 128, random bf16 data of the encoder's scale:
out-proj (K = N = 768), FFN2 (K = 3072, N = 768), both ResNorm + StatsOut with residual, and
FFN1 (K = 768, N = 3072), InNorm + GELU; all operands in K-tile image order.
One JSON line per (gemm, arm) and a summary line with the saving per encoder layer.
Usage: python tools/gemm_ablate.py [--build-only] [--rows 1024] [--rounds 8] [--iters 50]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
LIB = REPO / "tools" / "_gemm_ablate.so"


def build_lib(force: bool = False) -> Path:
    if LIB.exists() and not force:
        return LIB
    from agent_tpu_amd.csrc import build as b

    cmd = [b._hipcc(), f"--offload-arch={b.ARCH}", "-std=c++17", "-O3", "-DNDEBUG", "-fPIC", "-shared",
           "-fvisibility=hidden", f"-I{b.HERE / 'include'}", str(REPO / "tools" / "gemm_ablate.hip"), "-o", str(LIB)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"build failed: {' '.join(cmd)}\n{res.stdout}\n{res.stderr}")
    return LIB


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true", help="compile the library (no GPU needed) and exit")
    ap.add_argument("--rebuild", action="store_true")
    ap.add_argument("--dbg", type=int, default=512)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=8)
    a = ap.parse_args()
    lib_path = build_lib(a.rebuild or a.build_only)
    if a.build_only:
        print(lib_path)
        return 0
    import torch

    from agent_tpu_amd import ops

    lib = ctypes.CDLL(str(lib_path))
    lib.atpu_gemm_ablate.restype = ctypes.c_int
    lib.atpu_gemm_ablate.argtypes = ([ctypes.c_int] * 2 + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3
                                     + [ctypes.c_void_p] * 6)
    dev = torch.device("cuda", 0)
    M, H, I = a.rows * 128, 768, 3072
    gen = torch.Generator(device=dev).manual_seed(1)

    def rand(shape, scale, shift=0.0, dtype=torch.bfloat16):
        return (torch.randn(shape, generator=gen, device=dev) * scale + shift).to(dtype)

    x = rand((M, H), 2.0, 0.3)            # raw pre-LN hidden rows: A of FFN1, residual of the other two
    ctx = rand((M, H), 0.5)               # attention context: A of out-proj
    ff = rand((M, I), 0.3)                # FFN intermediate: A of FFN2
    w = {"out_proj": rand((H, H), 0.04), "ffn2": rand((H, I), 0.04), "ffn1": rand((I, H), 0.04)}
    bias = {k: rand((v.shape[0],), 0.1, dtype=torch.float32) for k, v in w.items()}
    gam = 1 + rand((H,), 0.1, dtype=torch.float32)
    colsum = w["ffn1"].float().sum(1).contiguous()
    fin = ops.ln_finalize(ops.ln_partials_ref(x.float()), H, 1e-12)
    part = torch.empty((H // 256, M, 2), dtype=torch.float32, device=dev)
    out_h = torch.empty((M, H), dtype=torch.bfloat16, device=dev)
    out_i = torch.empty((M, I), dtype=torch.bfloat16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def run(name, dbg):
        if name == "ffn1":
            rc = lib.atpu_gemm_ablate(0, dbg, p(x), p(w[name]), p(out_i), p(bias[name]), None, M, I, H,
                                      p(fin), p(colsum), None, None, None, stream)
        else:
            A = ctx if name == "out_proj" else ff
            rc = lib.atpu_gemm_ablate(1, dbg, p(A), p(w[name]), p(out_h), p(bias[name]), p(x), M, H, A.shape[1],
                                      None, None, p(fin), p(gam), p(part), stream)
        if rc != 0:
            raise RuntimeError(f"atpu_gemm_ablate({name}, dbg={dbg}) returned {rc}")

    names = ("out_proj", "ffn2", "ffn1")
    arms = (0, a.dbg)
    for n in names:
        for d in arms:
            run(n, d)
    torch.cuda.synchronize()
    res = {(n, d): [] for n in names for d in arms}
    for _ in range(a.rounds):
        for n in names:
            for d in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    run(n, d)
                e1.record()
                e1.synchronize()
                res[(n, d)].append(e0.elapsed_time(e1) * 1000.0 / a.iters)
    saving = 0.0
    for n in names:
        for d in arms:
            v = res[(n, d)]
            print(json.dumps({"gemm": n, "M": M, "dbg": d, "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                              "us_median": round(sorted(v)[len(v) // 2], 1), "us_all": [round(t, 1) for t in v]}),
                  flush=True)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        saving += med(res[(n, 0)]) - med(res[(n, a.dbg)])
    print(json.dumps({"summary": f"dbg {a.dbg} vs production, medians", "M": M,
                      "saving_us_per_layer": round(saving, 1)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
