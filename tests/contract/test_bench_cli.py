"""bench.py's output dump and the bounded synthetic input file (CPU parts only)."""
import importlib.util
import os

import numpy as np
import torch

from agent_tpu_amd.utils.synthetic import write_csv

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _bench(monkeypatch):
    # importing bench.py and parse() export these; monkeypatch puts the environment back
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    monkeypatch.setenv("ATPU_COMM", os.environ.get("ATPU_COMM", "torch"))
    spec = importlib.util.spec_from_file_location("bench_entry", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # module import only: main() is not run
    return mod


def test_dump_last_step_takes_each_ranks_last_batch(tmp_path, monkeypatch):
    world, steps, B, k = 2, 3, 4, 2
    idx = torch.arange(world * steps * B * k, dtype=torch.int32).reshape(-1, k)
    score = idx.to(torch.float32) / 7.0
    out = tmp_path / "nested" / "dump"
    _bench(monkeypatch).dump_last_step(str(out), idx, score, world, B)
    assert sorted(os.listdir(out)) == ["topk_idx.npy", "topk_score.npy"]
    got_i, got_s = np.load(out / "topk_idx.npy"), np.load(out / "topk_score.npy")
    assert got_i.dtype == got_s.dtype == np.float32 and got_i.shape == got_s.shape == (world * B, k)
    want = torch.cat([idx[(r + 1) * steps * B - B:(r + 1) * steps * B] for r in range(world)])
    assert np.array_equal(got_i, want.numpy().astype(np.float32))
    assert np.array_equal(got_s, (want.to(torch.float32) / 7.0).numpy())


def test_bench_options(monkeypatch):
    b = _bench(monkeypatch)
    monkeypatch.setattr("sys.argv", ["bench.py", "--batch-rows", "8"])
    a = b.parse()
    assert a.full is False and a.dump_outputs == ""
    monkeypatch.setattr("sys.argv", ["bench.py", "--batch-rows", "8", "--full", "--dump-outputs", "d", "--steps", "7"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7


def test_write_csv_unique_rows_repeats_the_same_texts(tmp_path):
    import csv

    def texts(path):
        with open(path, newline="", encoding="utf-8") as f:
            return [r["text"] for r in csv.DictReader(f)]

    full = texts(write_csv(str(tmp_path / "full.csv"), 10, 12, seed=3, quote_every=0))
    tiled = texts(write_csv(str(tmp_path / "tiled.csv"), 25, 12, seed=3, quote_every=0, unique_rows=10))
    assert len(tiled) == 25 and tiled == (full * 3)[:25]
    # no more rows than distinct texts: the file is the plain one, byte for byte
    a = write_csv(str(tmp_path / "a.csv"), 10, 12, seed=3)
    b = write_csv(str(tmp_path / "b.csv"), 10, 12, seed=3, unique_rows=64)
    assert open(a, "rb").read() == open(b, "rb").read()
