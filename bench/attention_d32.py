"""Packed head-dim-32 attention kernel (csrc/kernels/attention_d32.hip) at B*H = 1024*12, S = 128 against
torch's scaled_dot_product_attention on the same bf16 tensors and mask, and against the D = 64 packed kernel
at equal bytes (B*H = 1024*6), alternating, 3 rounds; plus a device copy of the same bytes as the yardstick.

    python bench/attention_d32.py [--batch 1024] [--iters 50] [--rounds 3]

Prints one JSON line: per variant the best and median time per call (device events around ``iters`` calls)
and the bytes it must move (QKV read + context written) over that time as a fraction of the copy's rate."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from agent_tpu_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("bench/attention_d32.py needs a ROCm device")
    dev = torch.device("cuda", 0)
    B, S, hid = a.batch, 128, 384
    qkv = (torch.randn((B * S, 3 * hid), device=dev) * 0.5).to(torch.bfloat16)
    lens = torch.randint(16, S + 1, (B,), device=dev, dtype=torch.int32)
    out = torch.empty((B * S, hid), dtype=torch.bfloat16, device=dev)
    mask = (torch.arange(S, device=dev).view(1, 1, 1, S) < lens.view(B, 1, 1, 1))
    q4, k4, v4 = (qkv[:, i * hid:(i + 1) * hid].view(B, S, 12, 32).transpose(1, 2) for i in range(3))
    dst = torch.empty_like(qkv)
    nbytes = qkv.numel() * 2 + out.numel() * 2
    crows = nbytes // (12 * hid)  # a copy of crows QKV rows reads and writes nbytes in all (to rounding)

    runs = {
        "d32_packed": lambda: ops.attention_packed(qkv, lens, B, S, 12, out=out, head_dim=32),
        "d64_packed_equal_bytes": lambda: ops.attention_packed(qkv, lens, B, S, 6, out=out),
        "torch_sdpa_d32": lambda: F.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask),
        "copy_same_bytes": lambda: dst[:crows].copy_(qkv[:crows]),
    }
    times = {n: [] for n in runs}
    for f in runs.values():  # warm every shape
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for n, f in runs.items():  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / a.iters)  # us per call
    copy_rate = (crows * 12 * hid) / min(times["copy_same_bytes"])  # bytes read + written per us
    res = {"shape": {"B": B, "S": S, "heads_d32": 12, "heads_d64": 6}, "bytes": nbytes, "iters": a.iters, "variants": {}}
    for n, t in times.items():
        res["variants"][n] = {"best_us": round(min(t), 2), "median_us": round(statistics.median(t), 2),
                              "rounds_us": [round(x, 2) for x in t],
                              "fraction_of_copy_rate": round((nbytes / min(t)) / copy_rate, 3)}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
