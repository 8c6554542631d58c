"""Late interaction on the CPU: the twins ``maxsim_ref`` and ``token_unit_ref`` against fp64, the late head in
``param_specs`` / the model path / HF parity through the fp32 oracle, and the ``map_maxsim`` op contract on a
CPU engine (pair forms, shared form, ranking, options, errors, lease batching).

Bounds. ``maxsim`` on unit vectors: a dot product errs by at most about ``P * 2^-24``, the sum of ``len_q``
terms of magnitude at most 1 adds ``len_q * 2^-24`` each: ``|err| <= len_q * (P + len_q) * 2^-23``.
``token_unit``: ``(P + 8) * 2^-24`` per element."""
import json

import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd.models.bert import BertClassifier, BertConfig, config_for, from_hf_state_dict, init_random, param_specs
from agent_tpu_amd.ops.maxsim import maxsim_ref, token_unit_ref

MODEL = "bert-tiny?late=64&batch=4&seq=32"


# ------------------------------------------------------------------ the twins
def _loop64(qv, lens_q, dv, lens_d, qidx, didx):
    q64, d64 = qv.double().numpy(), dv.double().numpy()
    out = []
    for a, b in zip(qidx.tolist(), didx.tolist()):
        total = 0.0
        for i in range(int(lens_q[a])):
            total += max(float(np.dot(q64[a, i], d64[b, j])) for j in range(int(lens_d[b])))
        out.append(total)
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("P", [64, 192])
def test_maxsim_ref_against_the_fp64_loop(P):
    S, Qn, Dn = 20, 3, 5
    g = torch.Generator().manual_seed(P)
    qv = torch.nn.functional.normalize(torch.randn(Qn, S, P, generator=g), dim=-1)
    dv = torch.nn.functional.normalize(torch.randn(Dn, S, P, generator=g), dim=-1)
    lens_q = torch.tensor([16, 20, 1], dtype=torch.int32)
    lens_d = torch.tensor([17, 2, 20, 15, 16], dtype=torch.int32)
    qidx = torch.tensor([2, 0, 1, 1, 2, 0, 0, 2, 1], dtype=torch.int32)
    didx = torch.tensor([0, 4, 2, 3, 1, 1, 4, 3, 0], dtype=torch.int32)
    got = ops.maxsim(qv, lens_q, dv, lens_d, qidx, didx)  # the CPU path is the twin
    assert got.dtype == torch.float32 and torch.equal(got, maxsim_ref(qv, lens_q, dv, lens_d, qidx, didx))
    lq = lens_q.long()[qidx.long()].double()
    err = (got.double() - _loop64(qv, lens_q, dv, lens_d, qidx, didx)).abs()
    assert (err <= lq * (P + lq) * 2.0 ** -23).all(), err
    # padding rows never reach a score; indices and lens are clamped
    pq, pd = qv.clone(), dv.clone()
    pq[torch.arange(S).view(1, S) >= lens_q.view(-1, 1)] = float("nan")
    pd[torch.arange(S).view(1, S) >= lens_d.view(-1, 1)] = 1e30
    assert torch.equal(ops.maxsim(pq, lens_q, pd, lens_d, qidx, didx), got)
    wild = ops.maxsim(qv, lens_q, dv, lens_d, torch.tensor([-1, Qn + 5], dtype=torch.int32),
                      torch.tensor([Dn + 5, -1], dtype=torch.int32))
    assert torch.equal(wild, ops.maxsim(qv, lens_q, dv, lens_d, torch.tensor([0, Qn - 1], dtype=torch.int32),
                                        torch.tensor([Dn - 1, 0], dtype=torch.int32)))
    # exactly representable inputs: the twin equals the fp64 loop
    qd = torch.randint(-2, 3, (Qn, S, P), generator=g).float() / 4
    dd = torch.randint(-2, 3, (Dn, S, P), generator=g).float() / 4
    assert torch.equal(maxsim_ref(qd, lens_q, dd, lens_d, qidx, didx).double(), _loop64(qd, lens_q, dd, lens_d, qidx, didx))
    assert ops.maxsim(qv, lens_q, dv, lens_d, qidx[:0], didx[:0]).shape == (0,)
    for bad in (lambda: ops.maxsim(qv[..., :48].contiguous(), lens_q, dv[..., :48].contiguous(), lens_d, qidx, didx),
                lambda: ops.maxsim(qv, lens_q, dv[:, :5].contiguous(), lens_d, qidx, didx),
                lambda: ops.maxsim(qv, lens_q.long(), dv, lens_d, qidx, didx),
                lambda: ops.maxsim(qv.double(), lens_q, dv, lens_d, qidx, didx),
                lambda: ops.maxsim(qv, lens_q, dv, lens_d, qidx, didx[:3])):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("P", [64, 192])
def test_token_unit_ref_against_fp64(dtype, P):
    g = torch.Generator().manual_seed(P)
    x = (torch.randn(37, P, generator=g) * 3).to(dtype)
    x[5] = 0
    got = ops.token_unit(x)
    assert got.dtype == torch.float32 and torch.equal(got, token_unit_ref(x))
    exact = x.double() / x.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    assert (got.double() - exact).abs().max().item() <= (P + 8) * 2.0 ** -24
    assert got[5].eq(0).all()  # 0 / max(0, 1e-12), not NaN
    out = torch.empty(37, P)
    assert ops.token_unit(x, out=out) is out and torch.equal(out, got)


# ------------------------------------------------------------------ the model
def test_param_specs_and_the_late_head():
    base = config_for("bert-tiny", num_labels=3, qa_head=True, tag_labels=5, mlm_head=True)
    today = [n for n, _, _ in param_specs(base)]
    assert today[-5:] == ["mlm_w", "mlm_b", "mlm_ln_g", "mlm_ln_b", "mlm_out_b"] and "late_w" not in today
    plain = [n for n, _, _ in param_specs(config_for("bert-tiny"))]
    assert plain[-4:] == ["pool_w", "pool_b", "cls_w", "cls_b"]  # late_dim = 0: the list is unchanged
    assert config_for("bert-tiny").late_dim == 0
    late = config_for("bert-tiny", num_labels=3, qa_head=True, tag_labels=5, mlm_head=True, late_dim=64)
    specs = list(param_specs(late))
    assert [n for n, _, _ in specs[:-1]] == today and specs[-1] == ("late_w", (64, 256), torch.bfloat16)
    assert late.param_count() == base.param_count() + 64 * 256
    assert sum(int(np.prod(s)) for _, s, _ in specs) == late.param_count()
    for bad in (32, 100, -64):
        with pytest.raises(ValueError):
            BertConfig(late_dim=bad)
    pack = init_random(config_for("bert-tiny", late_dim=64), seed=1)
    assert pack["late_w"].abs().max() > 0
    assert torch.equal(pack["cls_w"], init_random(config_for("bert-tiny"), seed=1)["cls_w"])


def test_model_path_late(tmp_path, monkeypatch):
    from ops._gpu_runtime import parse_spec

    assert parse_spec("bert-tiny?late=128").late == 128 and parse_spec("bert-tiny").late == 0
    for bad in ("bert-tiny?late=100", "bert-tiny?late=2048"):
        with pytest.raises(ValueError):
            parse_spec(bad)
    f = tmp_path / "colbert.safetensors"
    f.write_bytes(b"")
    (tmp_path / "colbert.safetensors.json").write_text(json.dumps({"preset": "bert-tiny", "head": "late", "late_dim": 64}))
    spec = parse_spec(str(f))
    assert spec.late == 64 and not spec.head and not spec.qa and not spec.mlm and spec.tags == 0
    (tmp_path / "colbert.safetensors.json").write_text(json.dumps({"preset": "bert-tiny", "head": "late"}))
    with pytest.raises(ValueError):
        parse_spec(str(f))


def test_token_vectors_match_hf_colbert():
    transformers = pytest.importorskip("transformers")
    from agent_tpu_amd import tokenizer as T
    from agent_tpu_amd.utils.synthetic import make_text_rows

    hcfg = transformers.BertConfig(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2,
                                   hidden_act="gelu", layer_norm_eps=1e-12, attn_implementation="eager")
    torch.manual_seed(13)
    hf = transformers.BertModel(hcfg, add_pooling_layer=False).eval()  # random init, no download
    linear = torch.nn.Linear(256, 64, bias=False)
    with torch.no_grad():
        for p in list(hf.parameters()) + list(linear.parameters()):  # our pack stores bf16 weights
            p.copy_(p.bfloat16().float())
    sd = {"bert." + k: v for k, v in hf.state_dict().items()}
    sd["linear.weight"] = linear.weight.detach()
    cfg = config_for("bert-tiny", late_dim=64)
    ours = BertClassifier(cfg, from_hf_state_dict(cfg, sd, head="late"), fp32=True)
    with pytest.raises(ValueError):
        from_hf_state_dict(config_for("bert-tiny"), sd, head="late")
    S = 32
    rows = [r.encode() for r in make_text_rows(5, words_per_row=6, seed=4)] + [b"", b"short one"]
    ids, lens = T.tokenize_rows(rows, S, 4096)
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    with torch.no_grad():
        hidden = hf(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask)).last_hidden_state
        ref = torch.nn.functional.normalize(linear(hidden), dim=-1)  # [B, S, 64]
        got = ours.token_vectors(torch.from_numpy(ids), torch.from_numpy(lens)).view(len(rows), S, 64)
    live = torch.from_numpy(mask).bool()
    assert got.dtype == torch.float32
    torch.testing.assert_close(got[live], ref[live], atol=2e-4, rtol=1e-4)
    # scores: within that tolerance times the query's token count
    t_lens = torch.from_numpy(lens)
    qidx = torch.tensor([0, 1, 6, 5], dtype=torch.int32)
    didx = torch.tensor([2, 3, 4, 0], dtype=torch.int32)
    s_got = maxsim_ref(got.contiguous(), t_lens, got.contiguous(), t_lens, qidx, didx)
    s_ref = maxsim_ref(ref.contiguous(), t_lens, ref.contiguous(), t_lens, qidx, didx)
    lq = t_lens[qidx.long()].float()
    assert ((s_got - s_ref).abs() <= lq * (2e-4 + 1e-4 * s_ref.abs() / lq)).all()


# ------------------------------------------------------------- op contract
@pytest.fixture()
def op(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops import get_batch_op, get_op

    return get_op("map_maxsim"), get_batch_op("map_maxsim")


QUERIES = ["how do gpus multiply matrices", "weather tomorrow", "empty list"]
PASSAGES = [["matrix cores multiply tiles", "a recipe for bread", "", "gpus have many compute units",
             "gpus multiply matrices with matrix cores", "rain is likely", "x"],
            ["rain is likely tomorrow", "sunny"], []]
POOL = PASSAGES[0]


def _prefix_of_the_sort(ranked, scores, k):
    order = sorted(range(len(scores)), key=lambda i: (-scores[i], i))[:k]
    assert [e["index"] for e in ranked] == order
    assert [e["score"] for e in ranked] == [scores[i] for i in order]  # the same floats


def _same(a, b):
    skip = ("elapsed_ms", "pairs_per_sec")
    assert {k: v for k, v in a.items() if k not in skip} == {k: v for k, v in b.items() if k not in skip}


def test_op_output_and_ordering(op):
    run, _ = op
    r = run({"queries": QUERIES, "passages": PASSAGES, "model_path": MODEL, "top_k": 4, "return_scores": True})
    for key in ("ok", "op", "query_count", "pair_count", "top_k", "model_path", "elapsed_ms", "pairs_per_sec", "ranked",
                "scores", "dim", "form"):
        assert key in r, key
    assert "label" not in r and "activation" not in r and "dp_world_size" not in r
    assert r["ok"] and r["op"] == "map_maxsim" and r["query_count"] == 3 and r["pair_count"] == 9 and r["top_k"] == 4
    assert r["dim"] == 64 and r["form"] == "pairs"
    assert [len(x) for x in r["ranked"]] == [4, 2, 0] and [len(s) for s in r["scores"]] == [7, 2, 0]
    for ranked, scores in zip(r["ranked"], r["scores"]):
        _prefix_of_the_sort(ranked, scores, 4)
    # the single-query form is the first query alone (bit-equal), a smaller top_k a prefix
    one = run({"query": QUERIES[0], "passages": PASSAGES[0], "model_path": MODEL, "top_k": 2, "return_scores": True})
    assert one["query_count"] == 1 and one["scores"] == [r["scores"][0]] and one["ranked"] == [r["ranked"][0][:2]]
    assert "scores" not in run({"query": QUERIES[0], "passages": PASSAGES[0], "model_path": MODEL})
    none = run({"query": "q", "passages": [], "model_path": MODEL, "return_scores": True})
    assert none["ranked"] == [[]] and none["pair_count"] == 0 and none["top_k"] == 10 and none["scores"] == [[]]
    # min_score cuts the tail
    cut = r["ranked"][0][1]["score"]
    m = run({"queries": QUERIES, "passages": PASSAGES, "model_path": MODEL, "top_k": 4, "min_score": cut})
    assert m["ranked"][0] == r["ranked"][0][:2] and all(e["score"] >= cut for x in m["ranked"] for e in x)
    # normalize_by_query_length: divided by the query's token count in fp32, after the ranking
    from ops._gpu_runtime import get_gpu_handle

    eng = get_gpu_handle(MODEL).engine
    eng.maxsim_scores(QUERIES, [])
    counts = eng.maxsim_lens_q.tolist()
    assert len(counts) == 3 and all(2 < c <= 32 for c in counts)
    n = run({"queries": QUERIES, "passages": PASSAGES, "model_path": MODEL, "top_k": 4, "return_scores": True,
             "normalize_by_query_length": True})
    assert [[e["index"] for e in x] for x in n["ranked"]] == [[e["index"] for e in x] for x in r["ranked"]]
    for q in range(3):
        want = (torch.tensor(r["scores"][q], dtype=torch.float32) / torch.tensor(float(counts[q]))).tolist()
        assert n["scores"][q] == want
        _prefix_of_the_sort(n["ranked"][q], n["scores"][q], 4)
    assert 0 < n["ranked"][0][0]["score"] <= 1.0 + 1e-5  # a mean of cosines


def test_shared_form_equals_the_pair_form_with_the_pool_repeated(op):
    run, _ = op
    s = run({"queries": QUERIES, "shared_passages": POOL, "model_path": MODEL, "top_k": 5, "return_scores": True})
    assert s["form"] == "shared" and s["query_count"] == 3 and s["pair_count"] == 21 and s["dim"] == 64
    p = run({"queries": QUERIES, "passages": [POOL] * 3, "model_path": MODEL, "top_k": 5, "return_scores": True})
    assert p["form"] == "pairs" and s["scores"] == p["scores"] and s["ranked"] == p["ranked"]  # bit-equal
    for ranked, scores in zip(s["ranked"], s["scores"]):
        _prefix_of_the_sort(ranked, scores, 5)  # index: the position in shared_passages
    none = run({"queries": QUERIES, "shared_passages": [], "model_path": MODEL, "return_scores": True})
    assert none["ranked"] == [[], [], []] and none["pair_count"] == 0 and none["scores"] == [[], [], []]
    zero = run({"queries": [], "shared_passages": POOL, "model_path": MODEL})
    assert zero["ranked"] == [] and zero["pair_count"] == 0


def test_op_errors(op):
    run, _ = op
    from ops.map_maxsim import ERRORS

    base = {"query": "q", "passages": ["a", "b"], "model_path": MODEL}
    shared = {"queries": ["q"], "shared_passages": ["a"], "model_path": MODEL}
    cases = [({"passages": ["a"]}, "missing"), ({"query": "q"}, "missing"),
             (dict(base, queries=["q"]), "both"), (dict(base, query=5), "query"),
             (dict(base, passages="a"), "passages"), (dict(base, passages=["a", 3]), "passages"),
             ({"queries": "q", "passages": [["a"]]}, "queries"), ({"queries": ["q", 2], "passages": [["a"], []]}, "queries"),
             ({"queries": ["q"], "passages": ["a"]}, "passage_lists"),
             ({"queries": ["q", "r"], "passages": [["a"]]}, "passage_lists"),
             (dict(shared, passages=[["a"]]), "forms"),
             (dict(shared, shared_passages="a"), "shared_passages"), (dict(shared, shared_passages=["a", 3]), "shared_passages"),
             ({"query": "q", "shared_passages": ["a"]}, "shared_queries"), ({"shared_passages": ["a"]}, "shared_queries"),
             (dict(shared, queries=["q", 2]), "shared_queries"),
             (dict(base, top_k=0), "top_k"), (dict(base, top_k=33), "top_k"), (dict(base, top_k="3"), "top_k"),
             (dict(base, top_k=True), "top_k"), (dict(base, return_scores=1), "return_scores"),
             (dict(base, min_score="0"), "min_score"), (dict(base, min_score=float("nan")), "min_score"),
             (dict(base, normalize_by_query_length=1), "normalize"), (dict(shared, normalize_by_query_length="yes"), "normalize")]
    seen = set()
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == ERRORS[key], (payload, key)
        seen.add(key)
    assert seen == set(ERRORS) - {"dim", "too_many"}
    from types import SimpleNamespace

    from ops.map_maxsim import check_model

    with pytest.raises(ValueError) as e:  # a width the kernel does not take
        check_model(SimpleNamespace(engine=SimpleNamespace(late_dim=96)))
    assert str(e.value) == ERRORS["dim"]


def test_too_many_queries(op, monkeypatch):
    run, _ = op
    from ops.map_maxsim import ERRORS

    monkeypatch.setenv("MAXSIM_QUERY_GB", str(2.5 * 32 * 64 * 4 / 2**30))  # room for two queries
    assert run({"queries": QUERIES[:2], "shared_passages": POOL[:2], "model_path": MODEL})["ok"]
    with pytest.raises(ValueError) as e:
        run({"queries": QUERIES, "shared_passages": POOL[:2], "model_path": MODEL})
    assert ERRORS["too_many"] in str(e.value)


def test_batched_jobs_equal_single_jobs(op):
    run, batch = op
    jobs = [{"queries": QUERIES, "passages": PASSAGES, "model_path": MODEL, "top_k": 3, "return_scores": True},
            {"query": 7, "passages": []},
            {"query": QUERIES[1], "passages": PASSAGES[0], "model_path": MODEL, "top_k": 7,
             "normalize_by_query_length": True, "return_scores": True},
            {"queries": QUERIES[:2], "shared_passages": POOL[:5], "model_path": MODEL, "top_k": 2, "return_scores": True},
            {"query": "q", "passages": [], "model_path": MODEL},
            {"query": QUERIES[0], "passages": PASSAGES[1], "model_path": MODEL, "min_score": 1e9}]
    res = batch(jobs)
    assert [r[0] for r in res] == ["ok", "err", "ok", "ok", "ok", "ok"]
    assert str(res[1][1]) == "payload.query must be a string"
    for job, (kind, got) in zip(jobs, res):
        if kind == "ok":
            _same(got, run(job))  # bit-equal: a score depends on its own two texts only
    assert res[5][1]["ranked"] == [[]] and res[3][1]["form"] == "shared"


def test_engine_forms_and_chunks(op):
    """More passages than ``batch_rows`` (chunks of 4), a group across a chunk boundary, empty groups: pair
    form, shared form and single pairs agree bit for bit, and the scores are the twin's on the model's own
    token vectors."""
    from agent_tpu_amd import tokenizer as T
    from ops._gpu_runtime import get_gpu_handle

    h = get_gpu_handle(MODEL)
    eng = h.engine
    assert eng.late_dim == 64 and eng.B == 4
    flat = [p for ps in PASSAGES for p in ps]
    goff = [0, 7, 9, 9]
    scores = eng.maxsim_scores(QUERIES, flat, goff)
    shared = eng.maxsim_scores(QUERIES, flat)
    assert scores.shape == (9,) and shared.shape == (3, 9)
    counts = eng.maxsim_lens_q.tolist()  # of the last call's queries
    assert torch.equal(scores[:7], shared[0, :7]) and torch.equal(scores[7:], shared[1, 7:])
    assert torch.equal(eng.maxsim_scores(QUERIES[1:2], flat[8:9], [0, 1]), shared[1, 8:9])
    ids_q, lens_q = T.tokenize_rows([q.encode() for q in QUERIES], eng.S, h.cfg.vocab_size)
    ids_p, lens_p = T.tokenize_rows([p.encode() for p in flat], eng.S, h.cfg.vocab_size)
    assert counts == lens_q.tolist()
    tv = lambda ids, lens: torch.cat([eng.model.token_vectors(torch.from_numpy(ids[i:i + 1]), torch.from_numpy(lens[i:i + 1]))  # noqa: E731
                                      for i in range(len(lens))]).view(-1, eng.S, 64)
    qidx = torch.arange(3, dtype=torch.int32).repeat_interleave(9)
    didx = torch.arange(9, dtype=torch.int32).repeat(3)
    want = maxsim_ref(tv(ids_q, lens_q), torch.from_numpy(lens_q), tv(ids_p, lens_p), torch.from_numpy(lens_p), qidx, didx)
    assert torch.equal(shared.reshape(-1), want)
    res = eng.maxsim_rank(QUERIES, flat, goff, top_k=3)
    want_i, want_v = ops.group_topk_ref(scores, torch.tensor(goff, dtype=torch.int32), 3)
    assert torch.equal(res.idx, want_i) and torch.equal(res.score, want_v) and res.idx[2].eq(-1).all()
    both = eng.maxsim_rank(QUERIES, flat, None, top_k=3)
    assert both.idx.shape == (3, 3) and torch.equal(both.scores.view(3, 9), shared)
    for bad in ([0, 7, 9], [1, 7, 9, 9], [0, 9, 7, 9]):
        with pytest.raises(ValueError):
            eng.maxsim_scores(QUERIES, flat, bad)
    with pytest.raises(ValueError):
        eng.maxsim_rank(QUERIES, flat, goff, top_k=33)
