"""map_maxsim's index forms under DP on CPU (gloo, world 2 and 3): a build writes the world-1 files byte for
byte, and whole-index and candidate queries (an index with fewer passages than ranks included, and a lease
batch) equal the single-process results exactly: a score depends on its own query and passage only, and the
merge of the per-rank top-k is the total order of the whole."""
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


def run_ranks(world):
    e = dict(os.environ)
    e.pop("MI355X_FAULT", None)
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu"})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "dp_maxsim_index_worker.py")]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


def _ranked_of(ref, k):
    return [[(i, s) for i, s in zip(row_i[:k], row_s[:k]) if i >= 0] for row_i, row_s in zip(ref["idx"], ref["score"])]


def _equals_ref(got, world, pairs, passages, dtype, k, scores):
    assert got["world"] == world and got["form"] == "index" and got["pairs"] == pairs
    assert got["passages"] == passages and got["dtype"] == dtype
    assert [[(e["index"], e["score"]) for e in x] for x in got["ranked"]] == _ranked_of(got["ref"], k)
    if scores:
        assert [v for s in got["scores"] for v in s] == got["ref"]["scores"]  # the same floats: bit-equal to world 1
    else:
        assert got["scores"] is None


@pytest.mark.parametrize("world", [2, 3])
def test_maxsim_index_under_dp_equals_single_process(world):
    res = run_ranks(world)
    assert res["world"] == world
    for name, n in (("build16", 7), ("build32", 7), ("build1", 1)):
        b = res[name]
        assert b["same_files"] and b["world"] == world and b["passages"] == n and b["form"] == "build" and b["tokens"] >= 3 * n
    for name, dtype in (("f16", "float16"), ("f32", "float32")):
        _equals_ref(res["whole_" + name], world, 21, 7, dtype, 3, False)
        assert [len(x) for x in res["whole_" + name]["ranked"]] == [3, 3, 3]
        _equals_ref(res["cand_" + name], world, 7, 7, dtype, 3, True)
        assert [len(s) for s in res["cand_" + name]["scores"]] == [4, 0, 3]
        assert [len(x) for x in res["cand_" + name]["ranked"]] == [3, 0, 3]
    # an fp32 index ranks as the shared form on the same strings does
    assert [[(e["index"], e["score"]) for e in x] for x in res["whole_f32"]["ranked"]] == _ranked_of(res["shared_ref"], 3)
    _equals_ref(res["whole_one"], world, 2, 1, "float16", 10, False)  # the other ranks' slices are empty
    assert [len(x) for x in res["whole_one"]["ranked"]] == [1, 1]
    _equals_ref(res["cand_one"], world, 2, 1, "float16", 10, True)
    assert res["bad"] == ["ValueError", "payload.candidates ids must lie in [0, passage count of the index)"]
    assert res["batch"]["kinds"] == ["ok", "err", "ok"]
    want = _ranked_of(res["whole_f16"]["ref"], 3)
    got = [[(e["index"], e["score"]) for e in x] for x in res["batch"]["ranked"]]
    assert got == [want[0], want[1], want[2][:2]]
