"""map_search ``filter`` under DP on CPU (gloo, worlds 2 and 3): every rank masks and searches its
own slice of a 101-row corpus (slice starts 51, and 34 and 68: no multiple of the mask's 32-row
words), and the merged result equals the single-process one key for key: ids, scores and
``filter_rows``, with ties across the rank boundaries, ranks whose slice has no allowed row, and
fewer allowed rows than ``top_k``."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 3])
def test_filtered_search_under_dp_equals_single_process(tmp_path, world):
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu",
              "DP_TEST_DIR": str(tmp_path)})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "dp_search_filter_worker.py")]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1][7:])
    assert res["world"] == world
    assert set(res["cases"]) == {"ids_all_ranks", "ids_first_slice", "ids_few", "exclude", "range_last_slice",
                                 "range_middle", "labels", "nothing"}
    for name, r in res["cases"].items():
        assert r["world"] == world and r["rows"] == 101, name
        assert r["dp"] == r["ref"], name  # ids, scores and filter_rows
        assert r["keys"] == sorted(res["plain_keys"] + ["filter_rows"]), name
        kk = min(8, r["ref"]["filter_rows"])
        assert all(len(row) == kk for row in r["dp"]["ids"]) and len(r["dp"]["ids"]) == 5, name
    # query 0 is the vector copied to both sides of every boundary: its copies tie, ascending id across the ranks
    first = res["cases"]["ids_all_ranks"]["dp"]
    assert first["ids"][0] == [2, 33, 34, 50, 51, 67, 68, 100] and len(set(first["scores"][0])) == 1
    assert res["cases"]["ids_few"]["dp"]["ids"][0] == [2, 51, 100]
    assert res["cases"]["nothing"]["dp"] == {"ids": [[]] * 5, "scores": [[]] * 5, "filter_rows": 0}
    assert res["cases"]["range_last_slice"]["dp"]["filter_rows"] == 31
    assert res["plain"]["dp"] == res["plain"]["ref"] and "filter_rows" not in res["plain_keys"]
    assert res["errors"]["got"] == res["errors"]["want"]
    assert res["batch"]["kinds"] == ["ok", "ok"] and res["batch"]["rows"] == [3, 31]
    assert res["batch"]["ids"][0] == res["cases"]["ids_few"]["dp"]["ids"]
    assert res["batch"]["ids"][1] == [row[:3] for row in res["cases"]["range_last_slice"]["dp"]["ids"]]
