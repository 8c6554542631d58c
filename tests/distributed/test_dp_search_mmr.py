"""map_search with ``diversify`` under DP on CPU (gloo, world 2) equals the single-process result exactly (ids,
relevance scores and MMR values), for a float32 and for a float16 resident corpus."""
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def test_diversified_search_under_dp_equals_single_process(tmp_path):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.pop("SEARCH_INDEX_DTYPE", None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_DIR": str(tmp_path)})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(HERE, "dp_search_mmr_worker.py")]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1][7:])
    assert res["world"] == 2
    for name in ("float32_cosine", "float16_cosine", "float16_dot"):
        r = res[name]
        assert r["world"] == 2 and r["diversify"] == {"lambda": 0.25, "candidates": 16}
        assert r["dp"] == r["ref"], name
        assert len(r["dp"]["ids"]) == 5 and all(len(row) == 6 for row in r["dp"]["ids"])
        assert r["dp"]["ids"] != r["plain"]
        for row in r["dp"]["ids"]:  # picks from both ranks' slices
            assert min(row) < 19 <= max(row), name
