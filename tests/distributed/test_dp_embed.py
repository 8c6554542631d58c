"""map_embed under DP on CPU (gloo, world 2): the ``texts`` job and the CSV job, both with an odd
row count, equal the single-process results in order; errors keep the op's contract; the lease
batch handler splits its rows over the ranks too."""
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


def test_embed_texts_and_csv_under_dp_equal_single_process(tmp_path):
    from agent_tpu_amd.utils.synthetic import write_csv

    csv = write_csv(str(tmp_path / "t.csv"), 20, 10)
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_CSV": csv})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "dp_embed_worker.py")]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1][7:])
    assert res["world"] == 2
    for form, n in (("texts", 7), ("csv", 11)):
        r = res[form]
        assert r["world"] == 2 and r["rows"] == n and np.asarray(r["dp"]).shape == (n, 256)
        assert np.allclose(np.asarray(r["dp"]), np.asarray(r["ref"]), atol=1e-6, rtol=0), form
    assert res["csv"]["end_row"] == 13
    assert np.allclose(np.asarray(res["one"]["dp"]), np.asarray(res["one"]["ref"]), atol=1e-6, rtol=0)
    assert res["bad"][0] == "ValueError" and res["bad"][1] == res["bad"][2]
    assert res["batch"]["kinds"] == ["ok", "err", "ok"]
    assert np.allclose(np.asarray(res["batch"]["dp"]), np.asarray(res["texts"]["ref"]), atol=1e-6, rtol=0)
