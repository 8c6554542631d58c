"""map_maxsim under DP on CPU (gloo, world 2 and 3): the pair form (splits inside a group), the shared form
(every rank encodes all queries and returns its transposed block), jobs with a single passage (ranks with
none) and a lease batch are bit-equal to the single-process results: a score depends on its own two texts
only."""
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
           "--master-addr=127.0.0.1", f"--master-port={_port()}", os.path.join(HERE, "dp_maxsim_worker.py")]
    p = subprocess.run(cmd, cwd=REPO, env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[-1][7:])


def _flat(groups):
    return [v for g in groups for v in g]


def _equals_ref(got, world, form, pairs, k):
    ref = got["ref"]
    assert got["world"] == world and got["form"] == form and got["pairs"] == pairs
    assert _flat(got["scores"]) == ref["scores"]  # the same floats: bit-equal to world 1
    want = [[(i, s) for i, s in zip(row_i[:k], row_s[:k]) if i >= 0] for row_i, row_s in zip(ref["idx"], ref["score"])]
    assert [[(e["index"], e["score"]) for e in x] for x in got["ranked"]] == want


@pytest.mark.parametrize("world", [2, 3])
def test_maxsim_under_dp_equals_single_process(world):
    res = run_ranks(world)
    assert res["world"] == world
    _equals_ref(res["many"], world, "pairs", 11, 3)
    assert [len(s) for s in res["many"]["scores"]] == [5, 2, 0, 4] and [len(x) for x in res["many"]["ranked"]] == [3, 2, 0, 3]
    _equals_ref(res["shared"], world, "shared", 21, 3)
    assert [len(s) for s in res["shared"]["scores"]] == [7, 7, 7]
    _equals_ref(res["one"], world, "pairs", 1, 10)  # the other ranks' slices are empty
    _equals_ref(res["shared_one"], world, "shared", 2, 10)
    assert res["bad"] == ["ValueError", "payload.top_k must be an integer in [1, 32]"]
    assert res["batch"]["kinds"] == ["ok", "err", "ok"]
    assert _flat(res["batch"]["scores"]) == res["many"]["ref"]["scores"]
    want = [[i for i in row if i >= 0] for row in res["many"]["ref"]["idx"]]
    assert res["batch"]["idx"] == [w[:k] for w, k in zip(want, (3, 3, 2, 2))]
