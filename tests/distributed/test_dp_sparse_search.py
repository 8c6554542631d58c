"""map_sparse_search under DP on CPU (gloo, 2 ranks): both query forms and a lease batch equal the single-process
results bit for bit; the 32 best rows of the tie query lie in rank 0's slice and a mixed query's cross the boundary."""
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
WORKER = os.path.join(HERE, "dp_sparse_search_worker.py")
SKIP = ("elapsed_ms", "rows_per_sec", "index_cached", "dp_world_size")


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, tmp_path, **extra):
    e = dict(os.environ)
    for k in ("MI355X_FAULT", "SEARCH_INDEX_MAX_GB", "TASKS"):
        e.pop(k, None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_DIR": str(tmp_path), "SEARCH_INDEX_LRU_SIZE": "8"})
    e.update(extra)
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


def test_sparse_search_under_dp(tmp_path):
    single = _run([sys.executable, WORKER], tmp_path, DP_SPARSE_SINGLE="1")
    res = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                "--master-addr=127.0.0.1", f"--master-port={_port()}", WORKER], tmp_path)
    strip = lambda r: {k: v for k, v in r.items() if k not in SKIP}  # noqa: E731
    for name in ("terms", "texts"):
        assert res[name]["dp_world_size"] == 2 and "dp_world_size" not in single[name], name
        assert strip(res[name]) == strip(single[name]), name  # json floats round-trip: equal bits
    assert [strip(r) for r in res["batch"]] == [strip(r) for r in single["batch"]]
    assert strip(res["batch"][1]) == strip(res["terms"]) and res["batch"][0]["top_k"] == 5
    ids = [r["ids"] for r in res["terms"]["results"]]
    assert ids[0] == list(range(0, 96, 3)) and res["terms"]["results"][2]["hits"] == 0
    assert any(i < 4500 for i in ids[1]) and any(i >= 4500 for i in ids[1])
    assert res["texts"]["results"][0]["ids"][0] == 3
