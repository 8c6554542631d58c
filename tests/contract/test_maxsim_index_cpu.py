"""The resident token-vector index of ``map_maxsim`` on the CPU: the twin ``maxsim_index_ref`` against fp64 and
against ``maxsim_ref`` on the padded copy, and the op's build and index forms on a CPU engine (files, bit
equality with the shared form, the fp16 bound, errors, lease batching, the LRU).

Bounds. fp32 storage: ``maxsim``'s, ``len_q * (P + len_q) * 2^-23``. fp16 storage of unit rows: rounding a
unit row to fp16 moves a dot product with a unit row by at most ``2^-11 + P * 2^-25`` and a max moves no
more than its arguments, so a score moves by at most ``len_q * (2^-11 + P * 2^-24)`` on top of the fp32 bound."""
import os

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.ops.maxsim import maxsim_index_ref, maxsim_ref

MODEL = "bert-tiny?late=64&batch=4&seq=32"
LENS = [17, 2, 20, 15, 16, 1, 33]


def _index(P, g, lens=LENS, dyadic=False):
    T = sum(lens)
    if dyadic:
        tok = torch.randint(-2, 3, (T, P), generator=g).float() / 4
    else:
        tok = torch.nn.functional.normalize(torch.randn(T, P, generator=g), dim=-1)
    off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64)
    return tok, off


def _padded(tok, off, S):
    N = off.numel() - 1
    dv = torch.zeros(N, S, tok.shape[1])
    for p in range(N):
        a, b = int(off[p]), int(off[p + 1])
        dv[p, :b - a] = tok[a:b]
    return dv, (off[1:] - off[:-1]).to(torch.int32)


def _loop64(qv, lens_q, tok, off):
    q64, t64 = qv.double().numpy(), tok.double().numpy()
    out = np.zeros((qv.shape[0], off.numel() - 1))
    for a in range(qv.shape[0]):
        for p in range(off.numel() - 1):
            out[a, p] = sum(max(float(np.dot(q64[a, i], t64[j])) for j in range(int(off[p]), int(off[p + 1])))
                            for i in range(int(lens_q[a])))
    return torch.from_numpy(out)


@pytest.mark.parametrize("P", [64, 192])
def test_twin_against_fp64_and_the_padded_maxsim(P):
    S, Qn = 20, 3
    g = torch.Generator().manual_seed(P)
    qv = torch.nn.functional.normalize(torch.randn(Qn, S, P, generator=g), dim=-1)
    lens_q = torch.tensor([16, 20, 1], dtype=torch.int32)
    tok, off = _index(P, g)
    N = len(LENS)
    got = ops.maxsim_index(qv, lens_q, tok, off)  # the CPU path is the twin
    assert got.dtype == torch.float32 and got.shape == (Qn, N) and torch.equal(got, maxsim_index_ref(qv, lens_q, tok, off))
    lq = lens_q.double().view(-1, 1)
    want64 = _loop64(qv, lens_q, tok, off)
    assert ((got.double() - want64).abs() <= lq * (P + lq) * 2.0 ** -23).all()
    # fp32 storage: the bits of maxsim_ref on the padded copy (S of the padded copy: the longest passage)
    dv, lens_d = _padded(tok, off, max(LENS))
    qp = torch.zeros(Qn, max(LENS), P)
    qp[:, :S] = qv
    qidx = torch.arange(Qn, dtype=torch.int32).repeat_interleave(N)
    didx = torch.arange(N, dtype=torch.int32).repeat(Qn)
    assert torch.equal(got.reshape(-1), maxsim_ref(qp, lens_q, dv, lens_d, qidx, didx))
    # fp16 storage: the twin on the widened values, and within the fp16 bound of the fp32 scores
    h = ops.maxsim_index(qv, lens_q, tok.half(), off)
    assert torch.equal(h, maxsim_index_ref(qv, lens_q, tok.half().float(), off))
    assert ((h.double() - want64).abs() <= lq * (2.0 ** -11 + P * 2.0 ** -24) + lq * (P + lq) * 2.0 ** -23).all()
    # dyadic inputs are exact in any order: the twin equals the fp64 loop in both dtypes
    qd = torch.randint(-2, 3, (Qn, S, P), generator=g).float() / 4
    td, _ = _index(P, g, dyadic=True)
    for t in (td, td.half()):
        assert torch.equal(maxsim_index_ref(qd, lens_q, t, off).double(), _loop64(qd, lens_q, td, off))


def test_twin_forms_clamps_and_refusals():
    S, Qn, P = 20, 3, 64
    g = torch.Generator().manual_seed(5)
    qv = torch.nn.functional.normalize(torch.randn(Qn, S, P, generator=g), dim=-1)
    lens_q = torch.tensor([16, 20, 1], dtype=torch.int32)
    tok, off = _index(P, g)
    N, T = len(LENS), sum(LENS)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    full = ops.maxsim_index(qv, lens_q, tok, off)
    # pidx: not monotone, with a repeat
    pidx = i32([4, 0, 6, 0, 2])
    sub = ops.maxsim_index(qv, lens_q, tok, off, pidx)
    assert torch.equal(sub, full[:, pidx.long()])
    # list form: an empty item, a non-monotone qsel; every entry equals the all form's
    qoff, qsel = i32([0, 2, 2, 3, 6, 7]), i32([2, 0, 1, 1, 2, 0, 1])
    lst = ops.maxsim_index(qv, lens_q, tok, off, pidx, qoff, qsel)
    item = [0, 0, 2, 3, 3, 3, 4]
    assert lst.shape == (7,)
    for e in range(7):
        assert lst[e] == full[qsel[e], pidx[item[e]]]
    assert ops.maxsim_index(qv, lens_q, tok, off, pidx, i32([0] * 6), i32([])).shape == (0,)
    assert ops.maxsim_index(qv, lens_q, tok, off, pidx[:0]).shape == (Qn, 0)
    out = torch.empty(Qn, 5)
    assert ops.maxsim_index(qv, lens_q, tok, off, pidx, out=out) is out and torch.equal(out, sub)
    # the clamps: pidx, qsel, qoff, lens_q, and offsets with a zero-length and an over-long entry
    wild = ops.maxsim_index(qv, i32([16, 99, -3]), tok, off, i32([-1, N + 5]), i32([-4, 1, 99]), i32([Qn + 5, -1]))
    want = ops.maxsim_index(qv, i32([16, 20, 1]), tok, off, i32([0, N - 1]), i32([0, 1, 2]), i32([Qn - 1, 0]))
    assert torch.equal(wild, want)
    bad_off = off.clone()
    bad_off[2] = bad_off[1]  # passage 1 has length 0 -> 1; passage 2 starts where 1 does
    bad_off[-1] = T + 50  # the last passage runs past T -> T - start
    zero_len = ops.maxsim_index(qv, lens_q, tok, bad_off)
    a = int(off[1])
    assert torch.equal(zero_len[:, 1], ops.maxsim_index(qv, lens_q, tok, torch.tensor([0, a, a + 1], dtype=torch.int64))[:, 1])
    assert torch.equal(zero_len[:, N - 1], full[:, N - 1])
    # tokens outside a passage never reach its score
    poisoned = tok.clone()
    poisoned[int(off[3]):int(off[4])] = float("nan")
    keep = [p for p in range(N) if p != 3]
    assert torch.equal(ops.maxsim_index(qv, lens_q, poisoned, off)[:, keep], full[:, keep])
    pq = qv.clone()
    pq[torch.arange(S).view(1, S) >= lens_q.view(-1, 1)] = float("nan")
    assert torch.equal(ops.maxsim_index(pq, lens_q, tok, off), full)
    for bad in (lambda: ops.maxsim_index(qv[..., :48].contiguous(), lens_q, tok[:, :48].contiguous(), off),
                lambda: ops.maxsim_index(qv, lens_q, tok[:, :32].contiguous(), off),
                lambda: ops.maxsim_index(qv, lens_q, tok.double(), off),
                lambda: ops.maxsim_index(qv, lens_q, tok.bfloat16(), off),
                lambda: ops.maxsim_index(qv, lens_q, tok, off.int()),
                lambda: ops.maxsim_index(qv, lens_q.long(), tok, off),
                lambda: ops.maxsim_index(qv, lens_q, tok, off, pidx.long()),
                lambda: ops.maxsim_index(qv, lens_q, tok, off, pidx, qoff),
                lambda: ops.maxsim_index(qv, lens_q, tok, off, pidx, qoff[:3], qsel),
                lambda: ops.maxsim_index(qv, lens_q, tok, off, out=torch.empty(N, Qn))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------- op contract
@pytest.fixture()
def op(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from agent_tpu_amd.runtime import search as rs
    from ops import get_batch_op, get_op

    rs.clear_cache()
    yield get_op("map_maxsim"), get_batch_op("map_maxsim")
    rs.clear_cache()


QUERIES = ["how do gpus multiply matrices", "weather tomorrow", "empty list"]
POOL = ["matrix cores multiply tiles", "a recipe for bread", "", "gpus have many compute units",
        "gpus multiply matrices with matrix cores", "rain is likely", "x"]


def _same(a, b, skip=("elapsed_ms", "pairs_per_sec", "index_cached")):
    assert {k: v for k, v in a.items() if k not in skip} == {k: v for k, v in b.items() if k not in skip}


def _build(run, tmp_path, dtype, name="idx"):
    uri = str(tmp_path / f"{name}_{dtype}.npy")
    r = run({"passages": POOL, "index_out": {"uri": uri, "dtype": dtype}, "model_path": MODEL})
    assert r["ok"] and r["form"] == "build" and r["dtype"] == dtype
    return uri, r


def test_build_then_query(op, tmp_path):
    run, _ = op
    from agent_tpu_amd import tokenizer as T
    from ops._gpu_runtime import get_gpu_handle

    uri32, b = _build(run, tmp_path, "float32")
    h = get_gpu_handle(MODEL)
    _, lens_p = T.tokenize_rows([p.encode() for p in POOL], h.engine.S, h.cfg.vocab_size)
    tok, off = np.load(uri32), np.load(b["offsets_uri"])
    assert b["offsets_uri"] == uri32[:-4] + ".offsets.npy" and b["index_uri"] == uri32
    assert tok.dtype == np.float32 and tok.ndim == 2 and tok.shape == (int(lens_p.sum()), 64)
    assert off.dtype == np.int64 and off.tolist() == [0] + np.cumsum(lens_p).tolist()
    assert b["passage_count"] == 7 and b["token_count"] == tok.shape[0] and b["dim"] == 64
    assert b["bytes"] == os.path.getsize(uri32) + os.path.getsize(b["offsets_uri"])
    assert np.abs(np.linalg.norm(tok.astype(np.float64), axis=1) - 1).max() < 1e-5  # unit rows, live tokens only
    assert not [f for f in os.listdir(tmp_path) if ".tmp." in f]

    shared = run({"queries": QUERIES, "shared_passages": POOL, "model_path": MODEL, "top_k": 5, "return_scores": True})
    cand = [list(range(7))] * 3
    c = run({"queries": QUERIES, "index_uri": uri32, "candidates": cand, "model_path": MODEL, "top_k": 5,
             "return_scores": True})
    assert c["form"] == "index" and c["passage_count"] == 7 and c["index_dtype"] == "float32" and c["pair_count"] == 21
    assert c["scores"] == shared["scores"] and c["ranked"] == shared["ranked"]  # bit for bit
    w = run({"queries": QUERIES, "index_uri": uri32, "model_path": MODEL, "top_k": 5})
    assert w["ranked"] == shared["ranked"] and "scores" not in w and w["pair_count"] == 21 and w["query_count"] == 3
    one = run({"query": QUERIES[1], "index_uri": uri32, "model_path": MODEL, "top_k": 2})
    assert one["ranked"] == [shared["ranked"][1][:2]]
    # candidates in their own order, ragged: index is the passage id, scores are in candidate order
    rag = run({"queries": QUERIES, "index_uri": uri32, "candidates": [[6, 4, 0], [], [5]], "model_path": MODEL,
               "return_scores": True, "normalize_by_query_length": True})
    plain = run({"queries": QUERIES, "index_uri": uri32, "candidates": [[6, 4, 0], [], [5]], "model_path": MODEL,
                 "return_scores": True})
    assert plain["scores"] == [[shared["scores"][0][i] for i in (6, 4, 0)], [], [shared["scores"][2][5]]]
    assert sorted(e["index"] for e in plain["ranked"][0]) == [0, 4, 6] and plain["ranked"][1] == []
    assert plain["ranked"][0][0]["score"] == max(plain["scores"][0])
    assert [[e["index"] for e in x] for x in rag["ranked"]] == [[e["index"] for e in x] for x in plain["ranked"]]

    # float16: round to nearest of the same rows; every score within the bound of the fp32 one
    uri16, b16 = _build(run, tmp_path, "float16")
    t16 = np.load(uri16)
    assert t16.dtype == np.float16 and np.array_equal(t16, tok.astype(np.float16)) and b16["bytes"] < b["bytes"]
    assert np.array_equal(np.load(b16["offsets_uri"]), off)
    hres = run({"queries": QUERIES, "index_uri": uri16, "candidates": cand, "model_path": MODEL, "return_scores": True})
    assert hres["index_dtype"] == "float16"
    h.engine.maxsim_scores(QUERIES, [])
    for q, lq in enumerate(h.engine.maxsim_lens_q.tolist()):
        bound = lq * (2.0 ** -11 + 64 * 2.0 ** -24) + lq * (64 + lq) * 2.0 ** -23
        err = np.abs(np.array(hres["scores"][q], dtype=np.float64) - np.array(shared["scores"][q], dtype=np.float64))
        assert (err <= bound).all(), (err, bound)
    # the default dtype is float16
    d = run({"passages": POOL[:2], "index_out": {"uri": str(tmp_path / "d.npy")}, "model_path": MODEL})
    assert d["dtype"] == "float16" and np.load(d["index_uri"]).dtype == np.float16 and d["passage_count"] == 2
    # an empty build has nothing to load
    e = run({"passages": [], "index_out": {"uri": str(tmp_path / "e.npy")}, "model_path": MODEL})
    assert e["passage_count"] == 0 and e["token_count"] == 0


def test_index_errors(op, tmp_path, monkeypatch):
    run, _ = op
    from agent_tpu_amd.runtime import maxsim_index as mi
    from ops.map_maxsim import ERRORS, INDEX_ERRORS

    assert set(ERRORS) == {"missing", "both", "forms", "query", "queries", "passages", "passage_lists", "shared_passages",
                           "shared_queries", "top_k", "return_scores", "min_score", "normalize", "dim", "too_many"}
    for k, v in mi.ERRORS.items():
        assert INDEX_ERRORS[k] == v
    uri, _ = _build(run, tmp_path, "float32")
    tok, off = np.load(uri), np.load(uri[:-4] + ".offsets.npy")

    def write(name, t=tok, o=off):
        p = str(tmp_path / f"{name}.npy")
        np.save(p, t)
        if o is not None:
            np.save(p[:-4] + ".offsets.npy", o)
        return p

    q = {"queries": ["q"], "model_path": MODEL}
    bo = {"passages": ["a"], "model_path": MODEL}
    nonfinite = tok.copy()
    nonfinite[3, 5] = np.inf
    down, short, late = off.copy(), off.copy(), off.copy()
    down[2] = down[1]
    short[-1] -= 1
    late[0] = 1
    cases = [(dict(bo, index_out="x.npy"), "index_out"), (dict(bo, index_out={"uri": 5}), "index_out"),
             (dict(bo, index_out={"uri": "s3://b/x.npy"}), "index_out"),
             (dict(bo, index_out={"uri": uri, "dtype": "bfloat16"}), "index_out"),
             (dict(bo, index_out={"uri": uri, "mode": "a"}), "index_out"),
             (dict(bo, index_out={"uri": uri}, query="q"), "index_out"),
             ({"index_out": {"uri": uri}, "model_path": MODEL}, "index_out"),
             (dict(bo, index_out={"uri": uri}, passages=["a", 3]), "index_out"),
             (dict(q, index_uri=uri, passages=[["a"]]), "index_forms"), (dict(q, index_uri=uri, shared_passages=["a"]), "index_forms"),
             ({"index_uri": uri, "model_path": MODEL}, "index_query"),
             (dict(q, index_uri=uri, candidates=[1]), "candidates"), (dict(q, index_uri=uri, candidates=[[1], [2]]), "candidates"),
             (dict(q, index_uri=uri, candidates=[[1.5]]), "candidates"), (dict(q, index_uri=uri, candidates=[[True]]), "candidates"),
             (dict(q, index_uri=uri, candidates=[[7]]), "candidates_range"), (dict(q, index_uri=uri, candidates=[[-1]]), "candidates_range"),
             (dict(q, index_uri=uri, candidates=[[1, 2, 1]]), "candidates_repeat"),
             (dict(q, index_uri=uri, return_scores=True), "index_scores"),
             (dict(q, index_uri=str(tmp_path / "none.npy")), "index_file"), (dict(q, index_uri=5), "index_file"),
             (dict(q, index_uri="http://host/x.npy"), "index_file"),
             (dict(q, index_uri=write("d1", tok[0])), "index_file"), (dict(q, index_uri=write("f64", tok.astype(np.float64))), "index_file"),
             (dict(q, index_uri=write("nooff", o=None)), "offsets_file"), (dict(q, index_uri=write("i32", o=off.astype(np.int32))), "offsets_file"),
             (dict(q, index_uri=write("down", o=down)), "offsets_file"), (dict(q, index_uri=write("short", o=short)), "offsets_file"),
             (dict(q, index_uri=write("late", o=late)), "offsets_file"),
             (dict(q, index_uri=write("nf", nonfinite)), "index_nonfinite"),
             (dict(q, index_uri=write("wide", np.concatenate([tok, tok], axis=1))), "index_dim")]
    seen = set()
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == INDEX_ERRORS[key], (payload, key)
        seen.add(key)
    from agent_tpu_amd.runtime import search as rs

    rs.clear_cache()  # the cap is checked when a slice is loaded
    monkeypatch.setenv("SEARCH_INDEX_MAX_GB", str(1024 / 2 ** 30))
    with pytest.raises(ValueError) as e:
        run(dict(q, index_uri=uri))
    assert str(e.value) == INDEX_ERRORS["index_too_large"]
    assert seen | {"index_too_large"} == set(INDEX_ERRORS)
    # the existing messages of the shared keys still apply, and passages alone are still "missing"
    for payload, key in [(dict(q, index_uri=uri, query="q"), "both"), ({"query": 3, "index_uri": uri}, "query"),
                         ({"queries": ["q", 2], "index_uri": uri}, "queries"), ({"passages": ["a"]}, "missing"),
                         (dict(q, index_uri=uri, top_k=33), "top_k")]:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == ERRORS[key]


def test_lease_batching_and_the_lru(op, tmp_path):
    run, batch = op
    from agent_tpu_amd.runtime import search as rs

    uri, _ = _build(run, tmp_path, "float16")
    other, _ = _build(run, tmp_path, "float32", "other")
    jobs = [{"queries": QUERIES, "index_uri": uri, "model_path": MODEL, "top_k": 3},
            {"query": 7, "index_uri": uri},
            {"query": QUERIES[1], "index_uri": uri, "model_path": MODEL, "top_k": 7, "normalize_by_query_length": True},
            {"queries": QUERIES[:2], "index_uri": uri, "candidates": [[5, 1], [0]], "model_path": MODEL, "return_scores": True},
            {"passages": POOL[:3], "index_out": {"uri": str(tmp_path / "b.npy")}, "model_path": MODEL},
            {"queries": QUERIES[:1], "index_uri": other, "model_path": MODEL, "top_k": 1, "min_score": -1e9},
            {"queries": QUERIES, "shared_passages": POOL[:5], "model_path": MODEL, "top_k": 2},
            {"queries": QUERIES[:1], "index_uri": uri, "candidates": [[9]], "model_path": MODEL}]
    res = batch(jobs)
    assert [r[0] for r in res] == ["ok", "err", "ok", "ok", "ok", "ok", "ok", "err"]
    assert str(res[1][1]) == "payload.query must be a string"
    assert str(res[7][1]) == "payload.candidates ids must lie in [0, passage count of the index)"
    for job, (kind, got) in zip(jobs, res):
        if kind == "ok":
            _same(got, run(job), skip=("elapsed_ms", "pairs_per_sec", "passages_per_sec", "index_cached"))
    assert len(res[0][1]["ranked"][0]) == 3 and len(res[2][1]["ranked"][0]) == 7
    # a second call is served from the LRU; a rewritten file reloads
    rs.clear_cache()
    first = run(jobs[0])
    again = run(jobs[0])
    assert first["index_cached"] is False and again["index_cached"] is True
    _same(first, again)
    assert rs.cache_info()["resident_bytes"] > 0
    tok = np.load(uri)
    np.save(uri, tok[:, ::-1].copy())  # other values, the same shape
    changed = run(jobs[0])
    assert changed["index_cached"] is False and changed["ranked"] != first["ranked"]
