"""The residual-compressed index of ``map_maxsim`` on the CPU, through the twins: build and query round trip
(files, bit equality with a float32 index written from the decoded rows), every ``RESIDUAL_ERRORS`` message, a
slice against the whole index, and a float index next to it still on the old path."""
import os

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.runtime import maxsim_index as mi
from agent_tpu_amd.runtime import maxsim_residual as mr

MODEL = "bert-tiny?late=64&batch=4&seq=32"
QUERIES = ["how do gpus multiply matrices", "weather tomorrow", "empty list"]
POOL = ["matrix cores multiply tiles", "a recipe for bread", "", "gpus have many compute units",
        "gpus multiply matrices with matrix cores", "rain is likely", "x"]


@pytest.fixture()
def run(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from agent_tpu_amd.runtime import search as rs
    from ops import get_op

    rs.clear_cache()
    yield get_op("map_maxsim")
    rs.clear_cache()


def _parts(uri):
    return [torch.from_numpy(np.load(p)) for p in (uri, mr.companion(uri, "cids"), mr.companion(uri, "centroids"),
                                                   mr.companion(uri, "weights"))]


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_build_then_query(run, tmp_path, bits):
    uri = str(tmp_path / "rc.npy")
    b = run({"passages": POOL, "model_path": MODEL,
             "index_out": {"uri": uri, "compression": {"type": "residual", "bits": bits, "centroids": 5}}})
    codes, cids, cent, w = _parts(uri)
    off = np.load(b["offsets_uri"])
    T = int(off[-1])
    assert b["form"] == "build" and b["compression"] == "residual" and b["bits"] == bits and b["centroids"] == 5
    assert b["dtype"] == f"residual{bits}" and 1 <= b["kmeans_iterations"] <= 8 and b["token_count"] == T
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (T, 64 * bits // 8) and cids.dtype == torch.int32
    assert tuple(cids.shape) == (T,) and tuple(cent.shape) == (5, 64) and tuple(w.shape) == (2 ** bits,)
    files = [uri, b["offsets_uri"]] + [mr.companion(uri, k) for k in ("cids", "centroids", "weights")]
    assert b["bytes"] == sum(os.path.getsize(f) for f in files) and not [f for f in os.listdir(tmp_path) if ".tmp." in f]
    # the stored form is the encoder's: the labels of kmeans_assign, the codes of the twin (unit rows rebuilt here)
    from ops._gpu_runtime import get_gpu_handle

    tok, lens = get_gpu_handle(MODEL).engine.maxsim_build(POOL)
    assert torch.equal(cids, ops.kmeans_assign(tok, cent)[0])
    dec = ops.residual_decode(codes, cids, cent, w)
    # a float32 index written from the decoded rows answers bit for bit
    ref = str(tmp_path / "dec.npy")
    mi.write_index(ref, dec, lens, "float32")
    cand = [[6, 4, 0], [], [5]]
    for extra in ({"top_k": 5}, {"candidates": cand, "return_scores": True}):
        got = run(dict({"queries": QUERIES, "index_uri": uri, "model_path": MODEL}, **extra))
        want = run(dict({"queries": QUERIES, "index_uri": ref, "model_path": MODEL}, **extra))
        assert got["index_dtype"] == f"residual{bits}" and want["index_dtype"] == "float32" and got["passage_count"] == 7
        assert got["ranked"] == want["ranked"] and got.get("scores") == want.get("scores")
    assert got["index_cached"] is True  # the second query of the same files: served from the LRU
    # a slice scores as the same passages of the whole index
    whole, part = mr.load_index(uri), mr.load_index(uri, 2, 4)
    assert part.start == 2 and part.count == 4 and part.total == 7 and int(part.offsets[0]) == 0
    qv = torch.nn.functional.normalize(torch.randn(2, 5, 64, generator=torch.Generator().manual_seed(bits)), dim=-1)
    lq = torch.tensor([5, 3], dtype=torch.int32)
    score = lambda ix: ops.maxsim_index_rc(qv, lq, ix.codes, ix.cids, ix.centroids, ix.weights, ix.offsets)  # noqa: E731
    assert torch.equal(score(part), score(whole)[:, 2:6])


def test_defaults_and_errors(run, tmp_path, monkeypatch):
    from ops.map_maxsim import INDEX_ERRORS, RESIDUAL_ERRORS

    assert set(mr.ERRORS) <= set(RESIDUAL_ERRORS) and all(RESIDUAL_ERRORS[k] == v for k, v in mr.ERRORS.items())
    uri = str(tmp_path / "d.npy")
    d = run({"passages": POOL, "model_path": MODEL, "index_out": {"uri": uri, "compression": {"type": "residual", "centroids": 3}}})
    assert d["bits"] == 2 and d["centroids"] == 3 and np.load(uri).shape[1] == 16
    codes, cids, cent, w = [t.numpy() for t in _parts(uri)]
    off = np.load(mi.offsets_path(uri))

    def write(name, codes=codes, cids=cids, cent=cent, w=w):
        p = str(tmp_path / f"{name}.npy")
        for path, a in ((mi.offsets_path(p), off), (mr.companion(p, "cids"), cids), (mr.companion(p, "centroids"), cent),
                        (mr.companion(p, "weights"), w), (p, codes)):
            if a is not None:
                np.save(path, a)
        return p

    bo = {"passages": POOL, "model_path": MODEL}
    comp = lambda **kw: dict(bo, index_out={"uri": uri, "compression": dict({"type": "residual", "centroids": 3}, **kw)})  # noqa: E731
    q = {"queries": ["q"], "model_path": MODEL}
    inf = cent.copy()
    inf[1, 2] = np.inf
    cases = [(comp(bits=3), "compression"), (comp(type="pq"), "compression"), (comp(centroids=0), "compression"),
             (comp(centroids=4097), "compression"), (comp(iterations=0), "compression"), (comp(rows=1), "compression"),
             (dict(bo, index_out={"uri": uri, "compression": {"type": "residual"}}), "compression"),
             (dict(bo, index_out={"uri": uri, "dtype": "float16", "compression": {"type": "residual", "centroids": 3}}), "compression"),
             (comp(centroids=4000), "compression_rows"), (dict(comp(), passages=[]), "compression_rows"),
             (dict(q, index_uri=write("nocid", cids=None)), "residual_file"),
             (dict(q, index_uri=write("cidshort", cids=cids[:-1])), "residual_file"),
             (dict(q, index_uri=write("narrow", codes=codes[:, :8].copy())), "residual_file"),
             (dict(q, index_uri=write("inf", cent=inf)), "residual_nonfinite"),
             (dict(q, index_uri=write("nan", w=np.array([0, np.nan, 0, 0], np.float32))), "residual_nonfinite")]
    seen = set()
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == RESIDUAL_ERRORS[key], (payload, key)
        seen.add(key)
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", str(1024 / 2 ** 30))
    with pytest.raises(ValueError) as e:
        run(dict(q, index_uri=uri))
    assert str(e.value) == RESIDUAL_ERRORS["index_too_large"] and seen | {"index_too_large"} == set(RESIDUAL_ERRORS)
    monkeypatch.delenv("SEARCH_INDEX_MAX_GB")
    # the offsets and the width keep the float index's messages
    for payload, key in [(dict(q, index_uri=write("off", codes=codes[:-1].copy(), cids=cids[:-1])), "offsets_file"),
                         (dict(q, index_uri=write("wide", codes=np.concatenate([codes, codes], 1),
                                                  cent=np.concatenate([cent, cent], 1))), "index_dim")]:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == INDEX_ERRORS[key]
    # a float index next to it still loads through the old path
    f = run(dict(bo, index_out={"uri": str(tmp_path / "f.npy"), "dtype": "float32"}))
    r = run(dict(q, index_uri=f["index_uri"]))
    assert r["index_dtype"] == "float32" and isinstance(mi.load_index(f["index_uri"]), mi.TokenIndex)
    assert not mr.is_residual(f["index_uri"]) and mr.is_residual(uri)
