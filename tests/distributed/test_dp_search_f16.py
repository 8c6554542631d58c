"""map_search with ``corpus_dtype: "float16"`` under DP on CPU (gloo, world 2): every rank keeps its
slice of the corpus as fp16 (with its slice of the row scale for cosine) and the merged result
equals the single-process one exactly, ids and scores, the tie order across the rank boundary
included; for a float16 and for a float32 file."""
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


def test_float16_search_under_dp_equals_single_process(tmp_path):
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.pop("SEARCH_INDEX_DTYPE", None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_DIR": str(tmp_path)})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "dp_search_f16_worker.py")]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1][7:])
    assert res["world"] == 2
    for name in ("f16", "f32"):
        for metric in ("cosine", "dot"):
            r = res[f"{name}_{metric}"]
            assert r["world"] == 2 and r["rows"] == 37 and r["cached"] is False and r["corpus_dtype"] == "float16"
            assert r["dp"]["ids"] == r["ref"]["ids"] and r["dp"]["scores"] == r["ref"]["scores"], (name, metric)
            assert all(len(row) == 8 for row in r["dp"]["ids"]) and len(r["dp"]["ids"]) == 5
        # the duplicated rows 17 .. 20 tie for the query that is their vector: ascending id across the rank boundary
        ids, s = res[f"{name}_cosine"]["dp"]["ids"], res[f"{name}_cosine"]["dp"]["scores"]
        assert ids[0][:4] == [17, 18, 19, 20] and s[0][0] == s[0][1] == s[0][2] == s[0][3]
        assert ids[1][:2] == [5, 30]
    assert res["f16_dot"]["dp"] == res["f32_dot"]["dp"]  # the same resident rows
    assert res["again_cached"] is True and "corpus_dtype" not in res["plain_keys"]
