"""map_answer with ``doc_stride`` under DP on CPU (gloo, world 2): long passages whose pairs split inside a
group, a one-pair job and a lease batch equal the single-process results, window counts included; the
``doc_stride`` error keeps the op's contract."""
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
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "dp_window_worker.py"), *args]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


def _flat(groups):
    return [v for g in groups for v in g]


def test_windowed_answer_under_dp_equals_single_process():
    res = run_ranks(world=2)
    assert res["world"] == 2
    many, ref = res["many"], res["many"]["ref"]
    assert many["world"] == 2 and many["pairs"] == 11 and many["doc_stride"] == 8
    assert [len(s) for s in many["null"]] == [5, 2, 0, 4]
    # the long passages have several windows each, and the counts of both ranks add up to the single-process count
    assert sorted(ref["per_pair"])[-4] >= 3 and many["windows"] == ref["windows"] == sum(ref["per_pair"]) > 11
    # CPU engines: a pair's fp32 sums depend on the rows it is batched with, hence the last-bit tolerance
    assert many["keys"] == ref["keys"] and [len(x) for x in many["keys"]] == [3, 3, 0, 3]
    assert np.allclose(_flat(many["scores"]), _flat(ref["scores"]), atol=1e-6, rtol=0)
    assert np.allclose(_flat(many["null"]), ref["null"], atol=1e-6, rtol=0)
    # an answer past the end of every answer the unwindowed reader can return
    assert max(_flat(many["ends"])) > max(_flat(res["plain_ends"]))
    assert res["one"]["keys"] == res["one"]["ref_keys"] and res["one"]["windows"] == res["one"]["ref_windows"] >= 3
    assert res["bad"][0] == "ValueError" and res["bad"][1] == res["bad"][2]
    assert res["batch"]["kinds"] == ["ok", "err", "ok"]
    assert res["batch"]["keys"] == [w[:k] for w, k in zip(ref["keys"], (3, 3, 2, 2))]
    assert res["batch"]["windows"] == [sum(ref["per_pair"][:7]), sum(ref["per_pair"][7:])]
