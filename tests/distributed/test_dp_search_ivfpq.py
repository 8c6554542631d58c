"""map_search ``index: {"type": "ivfpq"}`` under DP on CPU (gloo): world sizes 1, 2 and 3 and a run without a process
group give the same ids and score bits. Duplicated rows sit on both sides of every slice boundary."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
WORKER = os.path.join(HERE, "dp_search_ivfpq_worker.py")


def _run(cmd, tmp_path, **extra):
    e = dict(os.environ)
    for k in ("MI355X_FAULT", "SEARCH_INDEX_DTYPE", "SEARCH_INDEX_MAX_GB", "DP_IVFPQ_SINGLE"):
        e.pop(k, None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_DIR": str(tmp_path), "SEARCH_INDEX_LRU_SIZE": "8"}, **extra)
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    res = _run([sys.executable, WORKER], tmp_path_factory.mktemp("single"), DP_IVFPQ_SINGLE="1")
    assert res["two"]["ids"][0][:7] == [2, 99, 100, 149, 150, 199, 200]  # equal codes in one cluster: ascending id
    assert len(set(res["two"]["scores"][0][:7])) == 1
    assert res["two"]["index_cached"] is False and res["again"]["index_cached"] is True
    return res


@pytest.mark.parametrize("world", [1, 2, 3])
def test_ivfpq_search_under_dp_equals_single_process(tmp_path, single, world):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    res = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                "--master-addr=127.0.0.1", f"--master-port={port}", WORKER], tmp_path)
    for name in ("two", "all", "again"):
        assert res[name]["world"] == world and single[name]["world"] == 1, name
        for key in ("ids", "scores", "index", "corpus_rows", "top_k", "index_cached"):
            assert res[name][key] == single[name][key], (name, key)  # json floats round-trip: equal bits
