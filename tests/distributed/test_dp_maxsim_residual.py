"""map_maxsim's residual-compressed index under DP on CPU (gloo): a world-2 build writes the world-1 files byte
for byte (rank 0 compresses the gathered rows; no collective is added) and whole-index and candidate queries
return the single-process floats."""
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def run_ranks(world):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu"})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(HERE, "dp_maxsim_residual_worker.py")]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


def test_residual_index_under_dp_equals_single_process():
    one, two = run_ranks(1), run_ranks(2)
    assert one["world"] == 1 and two["world"] == 2 and two["whole"][3] == 2
    assert one["build"]["dtype"] == "residual2" and one["build"]["passage_count"] == 7 and one["whole"][1] == "residual2"
    assert two["build"] == one["build"] and two["files"] == one["files"]
    assert two["whole"][:3] == one["whole"][:3] and [len(x) for x in one["whole"][0]] == [3, 3, 3]
    assert two["cand"] == one["cand"] and [len(s) for s in one["cand"][1]] == [4, 0, 3]
