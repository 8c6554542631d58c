"""map_search under DP on CPU (gloo, world 2): every rank searches its slice of the corpus and the
merged result equals the single-process one exactly (ids and scores, the tie order across the
rank boundary included); a ``top_k`` above one rank's slice, an empty slice, errors and the lease
batch handler."""
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_search_under_dp_equals_single_process(tmp_path):
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_DIR": str(tmp_path)})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "dp_search_worker.py")]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1][7:])
    assert res["world"] == 2
    for metric in ("cosine", "dot"):
        r = res[metric]
        assert r["world"] == 2 and r["rows"] == 37 and r["cached"] is False
        assert r["dp"]["ids"] == r["ref"]["ids"] and r["dp"]["scores"] == r["ref"]["scores"], metric
        assert all(len(row) == 8 for row in r["dp"]["ids"]) and len(r["dp"]["ids"]) == 5
    # the duplicated rows 17 .. 20 tie for the query that is their text: ascending id across the rank boundary
    assert res["cosine"]["dp"]["ids"][0][:4] == [17, 18, 19, 20] and res["cosine"]["dp"]["ids"][1][:2] == [5, 30]
    s = res["cosine"]["dp"]["scores"][0]
    assert s[0] == s[1] == s[2] == s[3]
    for form in ("small", "one", "vectors"):
        assert res[form]["dp"] == res[form]["ref"], form
    assert all(len(row) == 8 for row in res["small"]["dp"]["ids"])  # 9 rows over 2 ranks still give 8
    assert res["one"]["dp"]["ids"] == [[0], [0]]
    assert res["texts"]["ids"] == res["cosine"]["dp"]["ids"]
    assert res["bad"][0] == "ValueError" and res["bad"][1] == res["bad"][2]
    assert res["batch"]["kinds"] == ["ok", "err", "ok"] and res["batch"]["world"] == 2
    assert res["batch"]["ids"] == [row[:3] for row in res["cosine"]["dp"]["ids"][:2]] + res["cosine"]["dp"]["ids"][2:]
    assert res["batch"]["scores"] == ([row[:3] for row in res["cosine"]["dp"]["scores"][:2]]
                                      + res["cosine"]["dp"]["scores"][2:])
