"""map_sparse_embed under DP on CPU (gloo, world 2): an uneven split and a one-row job equal the single-process results."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def test_sparse_embed_under_dp_equals_single_process():
    e = {k: v for k, v in os.environ.items() if k != "MI355X_FAULT"}
    e.update({"ATPU_DP_BACKEND": "gloo", "OMP_NUM_THREADS": "1", "CUDA_VISIBLE_DEVICES": "", "CLASSIFY_DEVICE": "cpu"})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc-per-node=2",
           os.path.join(HERE, "dp_sparse_worker.py")]
    p = subprocess.run(cmd, cwd=os.path.dirname(os.path.dirname(HERE)), env=e, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    got, ref = res["got"], res["ref"]
    ids, ws = [[t["token_ids"] for t in r["terms"]] for r in (got, ref)], [sum((t["weights"] for t in r["terms"]), []) for r in (got, ref)]
    assert got["dp_world_size"] == 2 and got["row_count"] == 11 and got["nnz"] == ref["nnz"]
    assert ids[0] == ids[1] and all(len(i) == 12 for i in ids[0]) and res["one"]["terms"][0]["token_ids"] == ids[0][3]
    assert np.allclose(ws[0], ws[1], atol=1e-6, rtol=0)  # CPU engines: a row's fp32 sums depend on its batch
