"""map_search ``compression`` (PQ) under DP on CPU (gloo): world sizes 1, 2 and 3 and a run without a process group
give identical results, key for key and bit for bit. Every rank trains the same codebooks from the same sample of
the file (no collective), encodes and scans its own slice, and the existing all-gather and merge run. Duplicated
rows sit on both sides of every slice boundary, so equal ADC scores cross the ranks; a fourth run of world 3 uses a
split that leaves the last rank without rows."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
WORKER = os.path.join(HERE, "dp_search_pq_worker.py")
JOBS = ("plain", "pq", "deep", "sub8", "cosine", "again")


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env(tmp_path, **extra):
    e = dict(os.environ)
    for k in ("MI355X_FAULT", "SEARCH_INDEX_DTYPE", "SEARCH_INDEX_MAX_GB", "DP_PQ_EMPTY_LAST", "DP_PQ_SINGLE"):
        e.pop(k, None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_DIR": str(tmp_path), "SEARCH_INDEX_LRU_SIZE": "8"})  # no entry of the jobs below is evicted
    e.update(extra)
    return e


def _result(p):
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("single")
    p = subprocess.run([sys.executable, WORKER], cwd=REPO, env=_env(tmp, DP_PQ_SINGLE="1"), capture_output=True,
                       text=True, timeout=240)
    res = _result(p)
    # what the single-process run must itself satisfy
    for name in ("pq", "cosine"):
        assert res[name]["ids"][0][:7] == [2, 99, 100, 149, 150, 199, 200], name  # equal codes: ties in ascending id
        assert len(set(res[name]["scores"][0][:7])) == 1 and res[name]["scores"][0][7] < res[name]["scores"][0][0]
    assert res["pq"]["compression"] == {"type": "pq", "subvectors": 16, "train_rows": 300, "train_iterations": 10,
                                        "bytes_per_row": 16}
    assert res["deep"]["compression"]["train_rows"] == 256 and all(len(x) == 32 for x in res["deep"]["ids"])
    assert res["sub8"]["compression"]["bytes_per_row"] == 8
    assert res["pq"]["cached"] is False and res["again"]["cached"] is True
    assert res["again"]["ids"] == [r[:3] for r in res["pq"]["ids"]]
    assert "compression" not in res["plain"]["keys"]
    assert res["pq"]["keys"] == sorted(res["plain"]["keys"] + ["compression"])
    assert res["plain"]["ids"][0][:7] == [2, 99, 100, 149, 150, 199, 200]
    return res


@pytest.mark.parametrize("world,empty_last", [(1, False), (2, False), (3, False), (3, True)])
def test_compressed_search_under_dp_equals_single_process(tmp_path, single, world, empty_last):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", WORKER]
    extra = {"DP_PQ_EMPTY_LAST": "1"} if empty_last else {}
    res = _result(subprocess.run(cmd, cwd=REPO, env=_env(tmp_path, **extra), capture_output=True, text=True, timeout=240))
    for name in JOBS:
        assert res[name]["world"] == world and single[name]["world"] == 1, name
        for key in ("ids", "scores", "compression", "corpus_rows", "top_k", "cached", "keys"):
            assert res[name][key] == single[name][key], (name, key)  # json floats round-trip: equal bits
    assert res["bad"] == single["bad"] and res["bad"][0] == "ValueError" and res["bad"][1] == res["bad"][2]
    assert res["batch"] == single["batch"] and res["batch"]["kinds"] == ["ok", "ok"]
    assert res["batch"]["ids"][0] == res["deep"]["ids"] and res["batch"]["ids"][1] == [r[:3] for r in res["pq"]["ids"]]
