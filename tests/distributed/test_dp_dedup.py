"""map_dedup under DP on CPU (gloo, world 2 and 3, 101 rows): every rank holds all rows and joins its blocks of
them, the pairs meet in a ragged all-gather, and the result equals the single-process one key for key (groups,
counts, pairs and their scores; json floats round-trip: equal bits); a bad payload fails on all ranks together
and a rank fault fails the job and names the rank."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
WORKER = os.path.join(HERE, "dp_dedup_worker.py")


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env(tmp_path, **extra):
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_DIR": str(tmp_path)})
    e.update(extra)
    return e


def _result(p):
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


def _launch(tmp_path, world, **extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", WORKER]
    return subprocess.run(cmd, cwd=REPO, env=_env(tmp_path, **extra), capture_output=True, text=True, timeout=240)


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("single")
    p = subprocess.run([sys.executable, WORKER], cwd=REPO, env=_env(tmp, DP_DEDUP_SINGLE="1"), capture_output=True,
                       text=True, timeout=240)
    return _result(p)


@pytest.mark.parametrize("world", [2, 3])
def test_dedup_under_dp_equals_single_process_key_for_key(tmp_path, single, world):
    res = _result(_launch(tmp_path, world))
    for name in ("cosine", "dot", "vectors", "none"):
        assert res[name]["world"] == world and single[name]["world"] == 1
        assert set(res[name]) == set(single[name])
        for key in set(single[name]) - {"world"}:
            assert res[name][key] == single[name][key], (name, key)
    g = res["cosine"]["group"]
    assert len(g) == 101 and g[49] == g[50] == g[51] == 49 and g[100] == 0 and g[16] == 15
    assert len({g[i] for i in range(30, 37)}) == 1 and res["cosine"]["largest_group"] >= 7
    assert res["dot"]["pair_count"] == len(res["dot"]["pairs"]) > 0 and res["none"]["pair_count"] == 0
    assert "group" not in res["vectors"] and len(res["vectors"]["pairs"]) == 5
    assert res["bad"][0] == "ValueError" and res["bad"][1] == res["bad"][2] and res["after_bad"] == 0


def test_rank_fault_fails_the_job_and_names_the_rank(tmp_path):
    res = _result(_launch(tmp_path, 2, MI355X_FAULT="rank:1:dedup", DP_DEDUP_FAULT="1"))
    assert res["fault"] is not None and "rank 1" in res["fault"][1] and "injected fault" in res["fault"][1]
