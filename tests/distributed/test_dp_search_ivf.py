"""map_search ``index`` (IVF) under DP on CPU (gloo): world sizes 1, 2 and 3 and a run without a process group
give identical results, key for key. k-means is a collective over the whole 101-row corpus (integer
all-reduces), so the centroids are global; every rank probes with them and searches its own cluster-sorted
slice, and the union of the ranks' probed rows is the probed clusters of the whole corpus. Ties cross the rank
boundaries, a two-row corpus leaves the last rank of world 3 with an empty slice, and probing every cluster
equals the job without an index."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
WORKER = os.path.join(HERE, "dp_search_ivf_worker.py")
JOBS = ("plain", "full", "two", "one", "defaults", "again", "tiny", "tiny_full")


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env(tmp_path, **extra):
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.pop("SEARCH_INDEX_DTYPE", None)
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
    p = subprocess.run([sys.executable, WORKER], cwd=REPO, env=_env(tmp, DP_IVF_SINGLE="1"), capture_output=True,
                       text=True, timeout=240)
    res = _result(p)
    # what the single-process run must itself satisfy
    assert res["full"]["ids"] == res["plain"]["ids"] and res["full"]["scores"] == res["plain"]["scores"]
    assert res["plain"]["ids"][0] == [2, 33, 34, 50, 51, 67, 68, 100] and len(set(res["plain"]["scores"][0])) == 1
    assert res["defaults"]["index"]["clusters"] == 11 and res["defaults"]["index"]["nprobe"] == 8
    assert res["full"]["cached"] is False and res["two"]["cached"] is True and res["again"]["cached"] is True
    assert "index" not in res["plain"]["keys"] and res["full"]["keys"] == sorted(res["plain"]["keys"] + ["index"])
    assert any(len(x) < 32 for x in res["two"]["ids"])  # two of seven clusters: a ragged list somewhere
    assert res["tiny_full"]["ids"][0] == [0, 1] or res["tiny_full"]["ids"][0] == [1, 0]
    assert all(len(x) <= 2 for x in res["tiny"]["ids"])
    return res


@pytest.mark.parametrize("world", [1, 2, 3])
def test_ivf_search_under_dp_equals_single_process(tmp_path, single, world):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", WORKER]
    res = _result(subprocess.run(cmd, cwd=REPO, env=_env(tmp_path), capture_output=True, text=True, timeout=240))
    for name in JOBS:
        assert res[name]["world"] == world and single[name]["world"] == 1, name
        for key in ("ids", "scores", "index", "corpus_rows", "top_k", "cached", "keys"):
            assert res[name][key] == single[name][key], (name, key)  # json floats round-trip: equal bits
    assert res["bad"] == single["bad"] and res["bad"][0] == "ValueError" and res["bad"][1] == res["bad"][2]
    assert res["batch"] == single["batch"] and res["batch"]["kinds"] == ["ok", "ok"]
    assert res["batch"]["ids"][0] == res["two"]["ids"] and res["batch"]["ids"][1] == [r[:3] for r in res["one"]["ids"]]
