"""map_zero_shot under DP on CPU (gloo, world 2 and 3): a job whose pairs split unevenly (a text's labels on
two ranks), a one-text job and a lease batch equal the single-process results; errors keep the op's
contract; an error on one rank fails the job, names that rank, and the group serves the next job."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(*args, world=2, env=None):
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu"})
    e.update(env or {})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "dp_zero_shot_worker.py"), *args]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


def _same(got, ref):
    """CPU engines: a pair's fp32 sums depend on the rows it is batched with, hence the last-bit tolerance; the
    labels are compared in full where the reference's neighbouring scores are further apart than that."""
    assert len(got) == len(ref)
    for (gl, gs), (rl, rs) in zip(got, ref):
        assert sorted(gl) == sorted(rl) and len(gs) == len(rs)
        by_label = dict(zip(gl, gs))
        assert np.allclose([by_label[name] for name in rl], rs, atol=1e-6, rtol=0)
        gap = np.abs(np.diff(rs)) > 4e-6
        clear = np.concatenate([[True], gap]) & np.concatenate([gap, [True]])
        assert [n for n, c in zip(gl, clear) if c] == [n for n, c in zip(rl, clear) if c]


@pytest.mark.parametrize("world", [2, 3])
def test_zero_shot_under_dp_equals_single_process(world):
    res = run_ranks(world=world)
    assert res["world"] == world
    many = res["many"]
    assert many["world"] == world and many["rows"] == 7 and many["pairs"] == 35  # 35 pairs: 18 + 17, 12 + 12 + 11
    _same(many["got"], many["ref"])
    assert all(len(labels) == 5 and abs(sum(scores) - 1) < 1e-5 for labels, scores in many["got"])
    _same(res["one"]["got"], res["one"]["ref"])
    assert len(res["one"]["got"]) == 1 and len(res["one"]["got"][0][0]) == 2
    assert res["bad"][0] == "ValueError" and res["bad"][1] == res["bad"][2]
    assert res["batch"]["kinds"] == ["ok", "err", "ok"]
    for got, ref in zip(res["batch"]["got"], res["batch"]["ref"]):
        _same(got, ref)
    assert [len(x[0]) for x in res["batch"]["got"][1]] == [3, 3, 3]


def test_error_on_one_rank_fails_the_job_and_names_the_rank():
    res = run_ranks("fault", env={"MI355X_FAULT": "rank:1:zero_shot:1"})
    assert res["err"] is not None and "rank 1" in res["err"][1] and "injected fault" in res["err"][1]
    assert "rank 0" not in res["err"][1]
    assert res["after"] == [3, 2, 3, 15]
