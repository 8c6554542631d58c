"""map_fill under DP on CPU (gloo, world 2): a job whose rows split unevenly, a one-row job with targets and
a lease batch equal the single-process results; errors keep the op's contract; an error on one rank fails
the job, names that rank, and the group serves the next job."""
import json
import os
import socket
import subprocess
import sys

import numpy as np

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
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "dp_fill_worker.py"), *args]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


def test_fill_under_dp_equals_single_process():
    res = run_ranks(world=2)
    assert res["world"] == 2
    many = res["many"]
    assert many["world"] == 2 and many["rows"] == 11 and len(many["keys"]) == 11
    # CPU engines: a row's fp32 sums depend on the rows it is batched with, hence the last-bit tolerance
    assert many["keys"] == many["ref"]["keys"] and all(many["keys"])
    assert many["truncated"] == many["ref"]["truncated"] == [[10, 0]] and many["keys"][10][0][2] == []
    assert np.allclose(many["scores"], many["ref"]["scores"], atol=1e-6, rtol=0)
    assert res["one"]["keys"] == res["one"]["ref_keys"] and len(res["one"]["keys"][0][0][2]) == 3
    assert res["bad"][0] == "ValueError" and res["bad"][1] == res["bad"][2]
    assert res["batch"]["kinds"] == ["ok", "err", "ok"]
    assert res["batch"]["keys"] == many["ref"]["keys"] and res["batch"]["truncated"] == [[], [[5, 0]]]


def test_error_on_one_rank_fails_the_job_and_names_the_rank():
    res = run_ranks("fault", env={"MI355X_FAULT": "rank:1:fill:1"})
    assert res["err"] is not None and "rank 1" in res["err"][1] and "injected fault" in res["err"][1]
    assert "rank 0" not in res["err"][1]
    assert res["after"] == [3, 2, 3]
