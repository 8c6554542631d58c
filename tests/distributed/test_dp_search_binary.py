"""map_search ``compression: {"type": "binary"}`` under DP on CPU (gloo, 2 ranks): the plain binary result equals the
single-process one exactly (both thresholds; the 32 best rows of a query cross the slice boundary), and the refined
result equals the uncompressed search on the mixture of test_search_binary_cpu.py, where every rank's shortlist of
its own slice holds the slice's share of the exact top-k."""
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
WORKER = os.path.join(HERE, "dp_search_binary_worker.py")


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, tmp_path, **extra):
    e = dict(os.environ)
    for k in ("MI355X_FAULT", "SEARCH_INDEX_DTYPE", "SEARCH_INDEX_MAX_GB", "SEARCH_REFINE_MAX_GB"):
        e.pop(k, None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_DIR": str(tmp_path), "SEARCH_INDEX_LRU_SIZE": "8"})
    e.update(extra)
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


def test_binary_search_under_dp(tmp_path):
    single = _run([sys.executable, WORKER], tmp_path, DP_BINARY_SINGLE="1")
    res = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                "--master-addr=127.0.0.1", f"--master-port={_port()}", WORKER], tmp_path)
    for name in ("exact", "zero", "mean"):
        assert res[name]["world"] == 2 and single[name]["world"] == 1, name
        for key in ("ids", "scores", "compression", "corpus_rows", "top_k"):
            assert res[name][key] == single[name][key], (name, key)  # json floats round-trip: equal bits
    assert res["zero"]["compression"] == {"type": "binary", "threshold": "zero", "bits": 64, "bytes_per_row": 8}
    assert all(len(r) == 32 and any(i < 2048 for i in r) and any(i >= 2048 for i in r) for r in res["zero"]["ids"][:4])
    assert res["mean"]["ids"] != [r[:5] for r in res["zero"]["ids"]]
    for run in (single, res):  # refined: the uncompressed search, bit for bit, at both world sizes
        assert run["refined"]["ids"] == run["exact"]["ids"] and run["refined"]["scores"] == run["exact"]["scores"]
        assert run["refined"]["ids"] != [r[:5] for r in run["zero"]["ids"]]
    assert res["refined"]["refine"] == {"candidates": 256, "vectors": "float32", "store": "host", "rescored_rows": 512}
