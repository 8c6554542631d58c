"""The re-ranker on the CPU: the pair twin (``atpu-pair v1``) against HF ``BertTokenizer`` pair
encoding and on the edge rows HF has no counterpart for, the CPU references of ``ops.pair_assemble``
and ``ops.group_topk``, HF parity of the pair path (``token_type_ids``) through the fp32 oracle, and
the ``map_rerank`` op contract on a CPU engine, lease batching included."""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

MODEL = "bert-tiny?labels=1&batch=4&seq=32&seed=3"


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    return str(path), T.WordPieceVocab.load(str(path))


# ------------------------------------------------------------------ the twin
@pytest.mark.parametrize("S", [16, 128])
def test_pair_rows_equal_hf_pair_encoding(small, S):
    transformers = pytest.importorskip("transformers")
    path, vocab = small
    hf = transformers.BertTokenizer(path, do_lower_case=True)
    mq = T.default_max_query_tokens(S)
    cand = [" ".join(r.split()[:w]) for w in (1, 2, 3, 5) for r in make_text_rows(12, words_per_row=8, seed=S + w)]
    ids_c, lens_c = vocab.tokenize_rows([c.encode() for c in cand], S)
    # only queries the twin tokenizes to <= mq tokens: HF never truncates the first segment
    queries = [c for c, n in zip(cand, lens_c) if n - 2 <= mq][:12]
    assert len(queries) >= 6
    passages = ["", "ka"] + make_text_rows(10, words_per_row=6, seed=7) + make_text_rows(6, words_per_row=150, seed=8)
    pairs = [(q, p) for q in range(len(queries)) for p in range(len(passages))]
    ids_q, lens_q = vocab.tokenize_rows([q.encode() for q in queries], S)
    ids_p, lens_p = vocab.tokenize_rows([passages[p].encode() for _, p in pairs], S)
    qidx = np.asarray([q for q, _ in pairs], dtype=np.int32)
    ids, types, lens = T.pair_rows(ids_q, lens_q, ids_p, lens_p, qidx, mq, vocab.cls_id, vocab.sep_id, vocab.pad_id)
    enc = hf([queries[q] for q, _ in pairs], [passages[p] for _, p in pairs], truncation="only_second",
             max_length=S, padding="max_length")
    np.testing.assert_array_equal(ids, np.asarray(enc["input_ids"], dtype=np.int32))
    np.testing.assert_array_equal(types, np.asarray(enc["token_type_ids"], dtype=np.int32))
    np.testing.assert_array_equal(lens, np.asarray(enc["attention_mask"], dtype=np.int32).sum(1))
    assert (lens == S).any() and (lens < S).any()  # an overflowing passage and a short one


def _rows(S, toks):
    """Single-segment rows as a tokenizer emits them, token values 1000 + 100 * row + position."""
    ids = np.zeros((len(toks), S), dtype=np.int32)
    lens = np.zeros(len(toks), dtype=np.int32)
    for r, n in enumerate(toks):
        ids[r, 0] = 101
        ids[r, 1:1 + n] = 1000 + 100 * r + np.arange(n)
        ids[r, 1 + n] = 102
        lens[r] = n + 2
    return ids, lens


def test_pair_rows_edge_cases():
    S = 8
    ids_q, lens_q = _rows(S, [3, 0, 6])
    ids_p, lens_p = _rows(S, [2, 0, 6, 1])
    # query longer than mq: cut to mq tokens, the passage takes the room
    ids, types, lens = T.pair_rows(ids_q, lens_q, ids_p, lens_p, np.asarray([0, 0, 2, 2], np.int32), 2)
    assert ids[0].tolist() == [101, 1000, 1001, 102, 1000, 1001, 102, 0] and lens[0] == 7
    assert types[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 0]
    assert ids[1].tolist() == [101, 1000, 1001, 102, 102, 0, 0, 0] and types[1].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert ids[2].tolist() == [101, 1200, 1201, 102, 1200, 1201, 1202, 102] and lens[2] == 8  # passage overflows
    assert types[2].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    # mq = 0: no query tokens
    ids, types, lens = T.pair_rows(ids_q, lens_q, ids_p, lens_p, np.asarray([0, 1, 2, 0], np.int32), 0)
    assert ids[0].tolist() == [101, 102, 1000, 1001, 102, 0, 0, 0] and types[0].tolist() == [0, 0, 1, 1, 1, 0, 0, 0]
    assert ids[2].tolist() == [101, 102, 1200, 1201, 1202, 1203, 1204, 102] and lens.tolist() == [5, 3, 8, 4]
    # mq >= S: the query keeps at most S - 3 tokens, so both [SEP] always fit
    ids, types, lens = T.pair_rows(ids_q, lens_q, ids_p, lens_p, np.asarray([2, 2, 2, 1], np.int32), S + 5)
    assert ids[0].tolist() == [101, 1200, 1201, 1202, 1203, 1204, 102, 102] and lens[0] == 8
    assert types[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert ids[3].tolist() == [101, 102, 1300, 102, 0, 0, 0, 0]  # empty query
    # lens out of range are clamped into [2, S]; qidx out of range is clamped into [0, Q)
    bad_q, bad_p = np.asarray([-4, 1, 99], np.int32), np.asarray([99, -1, 0, 3], np.int32)
    ids, types, lens = T.pair_rows(ids_q, bad_q, ids_p, bad_p, np.asarray([-1, 7, 0, 2], np.int32), 3)
    want = T.pair_rows(ids_q, np.asarray([2, 2, S], np.int32), ids_p, np.asarray([S, 2, 2, 3], np.int32),
                       np.asarray([0, 2, 0, 2], np.int32), 3)
    for a, b in zip((ids, types, lens), want):
        np.testing.assert_array_equal(a, b)
    assert lens.tolist() == [8, 6, 3, 7]
    with pytest.raises(ValueError):
        T.pair_rows(ids_q[:, :3], lens_q, ids_p[:, :3], lens_p, np.zeros(4, np.int32), 2)  # S < 4
    with pytest.raises(ValueError):
        T.pair_rows(ids_q, lens_q, ids_p, lens_p, np.zeros(4, np.int32), -1)


def test_pair_assemble_cpu_ref_equals_twin(small):
    _, vocab = small
    S = 16
    rows = [r.encode() for r in make_text_rows(9, words_per_row=5, seed=2)] + [b""]
    qidx = np.asarray([0, 0, 2, 1, 9, -3, 1, 2, 0, 1], dtype=np.int32)
    for spec in (vocab, None):
        if spec is not None:
            ids_q, lens_q = vocab.tokenize_rows(rows[:3], S)
            ids_p, lens_p = vocab.tokenize_rows(rows, S)
            sp = (vocab.cls_id, vocab.sep_id, vocab.pad_id)
            assert sp != (T.CLS_ID, T.SEP_ID, T.PAD_ID)
        else:  # the hash tokenizer: 101 / 102 / 0
            ids_q, lens_q = T.tokenize_rows(rows[:3], S, 4096)
            ids_p, lens_p = T.tokenize_rows(rows, S, 4096)
            sp = (101, 102, 0)
        want = T.pair_rows(ids_q, lens_q, ids_p, lens_p, qidx, 4, *sp)
        t = [torch.from_numpy(a) for a in (ids_q, lens_q, ids_p, lens_p, qidx)]
        got = ops.pair_assemble(*t, 4, *sp) if spec is not None else ops.pair_assemble(*t, 4)
        for a, b in zip(got, want):
            assert a.dtype == torch.int32 and np.array_equal(a.numpy(), b)
        assert got[0][0, 0] == sp[0] and (got[0] == sp[1]).sum(1).eq(2).all()
        # preallocated outputs, the first `rows` rows only: the rest is not touched
        out = [torch.full((12, S), -7, dtype=torch.int32), torch.full((12, S), -7, dtype=torch.int32),
               torch.full((12,), -7, dtype=torch.int32)]
        ops.pair_assemble(*t, 4, *sp, ids=out[0], type_ids=out[1], lens=out[2], rows=7)
        for a, b in zip(out, want):
            assert np.array_equal(a[:7].numpy(), b[:7]) and (a[7:] == -7).all()
    with pytest.raises(ValueError):
        ops.pair_assemble(t[0].long(), *t[1:], 4)
    with pytest.raises(ValueError):
        ops.pair_assemble(*t, -1)
    with pytest.raises(ValueError):
        ops.pair_assemble(*t[:4], t[4][:5], 4)


# ------------------------------------------------------------- group top-k
def _sorted_ref(scores, goff, k):
    """Stable descending sort over the group, signed zeros folded: (score desc, index asc)."""
    idx = np.full((len(goff) - 1, k), -1, dtype=np.int32)
    val = np.full((len(goff) - 1, k), -np.inf, dtype=np.float32)
    for q in range(len(goff) - 1):
        s = scores[goff[q]:goff[q + 1]]
        order = torch.sort(s + 0.0, descending=True, stable=True).indices[:k]
        idx[q, :len(order)] = order.numpy()
        val[q, :len(order)] = s[order].numpy()
    return idx, val


@pytest.mark.parametrize("k", [1, 10, 32])
def test_group_topk_ref_is_the_stable_sort(k):
    g = torch.Generator().manual_seed(k)
    lens = [0, 1, max(k - 1, 0), k, 300, 0, 5]
    goff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    scores = torch.randn(int(goff[-1]), generator=g)
    scores[goff[4]:goff[5]] = torch.randint(0, 4, (300,), generator=g).float()  # duplicated scores
    scores[goff[6]:goff[7]] = torch.tensor([0.0, -0.0, -1.0, -0.0, 0.0])      # +0.0 and -0.0 tie
    idx, val = ops.group_topk(scores, torch.from_numpy(goff), k)
    want_i, want_v = _sorted_ref(scores, goff.tolist(), k)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.shape == (7, k)
    np.testing.assert_array_equal(idx.numpy(), want_i)
    assert np.array_equal(val.numpy().view(np.int32), want_v.view(np.int32))  # the stored bits, zeros' signs too
    assert idx[0].eq(-1).all() and torch.isinf(val[0]).all()
    assert idx[6, :min(k, 4)].tolist() == [0, 1, 3, 4][:min(k, 4)]
    # a NaN ranks (and is returned) as -inf; offsets are clamped into [0, P]
    s = torch.tensor([1.0, float("nan"), 2.0, float("-inf")])
    idx, val = ops.group_topk(s, torch.tensor([0, 4, 9], dtype=torch.int32), 4)
    assert idx.tolist() == [[2, 0, 1, 3], [-1] * 4] and val[0].tolist() == [2.0, 1.0, float("-inf"), float("-inf")]
    for bad in (0, 33, True, 2.0):
        with pytest.raises(ValueError):
            ops.group_topk(s, torch.tensor([0, 4], dtype=torch.int32), bad)
    with pytest.raises(ValueError):
        ops.group_topk(s.double(), torch.tensor([0, 4], dtype=torch.int32), 2)


# --------------------------------------------------------- HF parity, pairs
def test_pair_scores_match_hf_with_token_type_ids():
    transformers = pytest.importorskip("transformers")
    from agent_tpu_amd.models.bert import BertClassifier, config_for, from_hf_state_dict

    hcfg = transformers.BertConfig(vocab_size=4096, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                                   intermediate_size=1024, max_position_embeddings=512, type_vocab_size=2,
                                   num_labels=1, hidden_act="gelu", layer_norm_eps=1e-12,
                                   attn_implementation="eager")
    torch.manual_seed(11)
    hf = transformers.BertForSequenceClassification(hcfg).eval()
    with torch.no_grad():
        for p in hf.parameters():  # our pack stores bf16 weights: give HF the same values
            p.copy_(p.bfloat16().float())
    cfg = config_for("bert-tiny", num_labels=1)
    ours = BertClassifier(cfg, from_hf_state_dict(cfg, hf.state_dict()), fp32=True)
    S = 64
    rows = [r.encode() for r in make_text_rows(6, words_per_row=12, seed=4)] + [b"", b"short one"]
    ids_q, lens_q = T.tokenize_rows(rows[:2], S, 4096)
    ids_p, lens_p = T.tokenize_rows(rows, S, 4096)
    ids, types, lens = T.pair_rows(ids_q, lens_q, ids_p, lens_p, np.arange(8, dtype=np.int32) % 2, 8)
    assert types.any() and lens.min() < S
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    with torch.no_grad():
        ref = hf(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask),
                 token_type_ids=torch.from_numpy(types).long()).logits[:, 0]
        no_types = hf(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask)).logits[:, 0]
        got = ours.score(torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(types))
    assert got.dtype == torch.float32 and got.shape == (8,)
    torch.testing.assert_close(got, ref, atol=2e-4, rtol=1e-4)
    assert (ref - no_types).abs().max() > 2e-3  # the segment embedding does move the score
    with pytest.raises(ValueError):
        ours.score(torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(types), label=1)


# ------------------------------------------------------------- op contract
@pytest.fixture()
def op(monkeypatch):
    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    from ops import get_batch_op, get_op

    return get_op("map_rerank"), get_batch_op("map_rerank")


QUERIES = ["how do gpus multiply matrices", "weather tomorrow", "empty list"]
PASSAGES = [["matrix cores multiply tiles", "a recipe for bread", "", "gpus have many compute units",
             "gpus multiply matrices with matrix cores", "rain is likely", "x"],
            ["rain is likely tomorrow", "sunny"], []]


def _close(got, want):
    """Two results of the op on a CPU engine: the same ranking, the scores equal up to the last bits (the
    PyTorch reference path is not batch-invariant: a pair's fp32 sums depend on the rows it is batched with)."""
    assert [[e["index"] for e in x] for x in got["ranked"]] == [[e["index"] for e in x] for x in want["ranked"]]
    flat = lambda r, key: [v for x in r[key] for v in ([e["score"] for e in x] if key == "ranked" else x)]  # noqa: E731
    for key in ("ranked", "scores"):
        assert (key in got) == (key in want)
        if key in got:
            np.testing.assert_allclose(flat(got, key), flat(want, key), atol=1e-5, rtol=0)
    skip = ("elapsed_ms", "pairs_per_sec", "ranked", "scores")
    assert {k: v for k, v in got.items() if k not in skip} == {k: v for k, v in want.items() if k not in skip}


def test_op_output_and_ordering(op):
    run, _ = op
    r = run({"queries": QUERIES, "passages": PASSAGES, "model_path": MODEL, "top_k": 4, "return_scores": True})
    for key in ("ok", "op", "query_count", "pair_count", "top_k", "model_path", "elapsed_ms", "pairs_per_sec", "ranked",
                "scores"):
        assert key in r, key
    assert r["ok"] and r["op"] == "map_rerank" and r["query_count"] == 3 and r["pair_count"] == 9 and r["top_k"] == 4
    assert "dp_world_size" not in r
    assert [len(x) for x in r["ranked"]] == [4, 2, 0] and [len(s) for s in r["scores"]] == [7, 2, 0]
    for ranked, scores in zip(r["ranked"], r["scores"]):
        order = sorted(range(len(scores)), key=lambda i: (-scores[i], i))[:4]
        assert [e["index"] for e in ranked] == order
        assert [e["score"] for e in ranked] == [scores[i] for i in order]  # raw logits, the same floats
    # the single-query form is the first query alone, and a smaller top_k is a prefix
    one = run({"query": QUERIES[0], "passages": PASSAGES[0], "model_path": MODEL, "top_k": 2})
    assert one["query_count"] == 1 and "scores" not in one
    _close(one, dict(one, ranked=[r["ranked"][0][:2]]))
    none = run({"query": "q", "passages": [], "model_path": MODEL})
    assert none["ranked"] == [[]] and none["pair_count"] == 0 and none["top_k"] == 10
    # sigmoid after the ranking: same order, values mapped in fp32; min_score cuts the tail
    s = run({"queries": QUERIES, "passages": PASSAGES, "model_path": MODEL, "top_k": 4, "activation": "sigmoid"})
    assert [[e["index"] for e in x] for x in s["ranked"]] == [[e["index"] for e in x] for x in r["ranked"]]
    raw = torch.tensor([e["score"] for e in r["ranked"][0]], dtype=torch.float32)
    np.testing.assert_allclose([e["score"] for e in s["ranked"][0]], torch.sigmoid(raw).numpy(), atol=1e-6, rtol=0)
    cut = r["ranked"][0][1]["score"]
    m = run({"queries": QUERIES, "passages": PASSAGES, "model_path": MODEL, "top_k": 4, "min_score": cut})
    assert [e["index"] for e in m["ranked"][0]] == [e["index"] for e in r["ranked"][0][:2]]
    assert all(e["score"] >= cut for x in m["ranked"] for e in x)
    # max_query_tokens is part of the row: cutting the query changes the scores
    q1 = run({"query": QUERIES[0], "passages": PASSAGES[0], "model_path": MODEL, "max_query_tokens": 1,
              "return_scores": True})
    assert q1["scores"][0] != r["scores"][0]


def test_op_errors(op):
    run, _ = op
    from ops.map_rerank import ERRORS

    base = {"query": "q", "passages": ["a", "b"], "model_path": MODEL}
    cases = [({"passages": ["a"]}, "missing"), ({"query": "q"}, "missing"),
             (dict(base, queries=["q"]), "both"), (dict(base, query=5), "query"),
             (dict(base, passages="a"), "passages"), (dict(base, passages=["a", 3]), "passages"),
             ({"queries": "q", "passages": [["a"]]}, "queries"), ({"queries": ["q", 2], "passages": [["a"], []]}, "queries"),
             ({"queries": ["q"], "passages": ["a"]}, "passage_lists"),
             ({"queries": ["q", "r"], "passages": [["a"]]}, "passage_lists"),
             (dict(base, top_k=0), "top_k"), (dict(base, top_k=33), "top_k"), (dict(base, top_k="3"), "top_k"),
             (dict(base, top_k=True), "top_k"),
             (dict(base, max_query_tokens=0), "max_query_tokens"), (dict(base, max_query_tokens=29), "max_query_tokens"),
             (dict(base, max_query_tokens=2.0), "max_query_tokens"),
             (dict(base, label=-1), "label"), (dict(base, label=1), "label"), (dict(base, label="0"), "label"),
             (dict(base, activation="softmax"), "activation"), (dict(base, return_scores=1), "return_scores"),
             (dict(base, min_score="0"), "min_score"), (dict(base, min_score=float("nan")), "min_score")]
    seen = set()
    for payload, key in cases:
        with pytest.raises(ValueError) as e:
            run(payload)
        assert str(e.value) == ERRORS[key], (payload, key)
        seen.add(key)
    assert seen == set(ERRORS) - {"head"}
    # an encoder without pooler and classifier ("head": "none" in the model json) cannot score
    from types import SimpleNamespace

    from ops.map_rerank import check_model, options

    with pytest.raises(ValueError) as e:
        check_model(SimpleNamespace(spec=SimpleNamespace(head=False)), options(base))
    assert str(e.value) == ERRORS["head"]
    assert run(dict(base, max_query_tokens=28))["ok"]  # seq_len - 4


def test_batched_jobs_equal_single_jobs(op):
    run, batch = op
    jobs = [{"queries": QUERIES, "passages": PASSAGES, "model_path": MODEL, "top_k": 3, "return_scores": True},
            {"query": 7, "passages": []},
            {"query": QUERIES[1], "passages": PASSAGES[0], "model_path": MODEL, "top_k": 7, "activation": "sigmoid"},
            {"query": QUERIES[0], "passages": PASSAGES[1], "model_path": MODEL, "max_query_tokens": 2},
            {"query": "q", "passages": [], "model_path": MODEL},
            {"query": QUERIES[0], "passages": ["a"], "model_path": MODEL, "label": 4}]
    res = batch(jobs)
    assert [r[0] for r in res] == ["ok", "err", "ok", "ok", "ok", "err"]
    assert str(res[1][1]) == "payload.query must be a string" and isinstance(res[5][1], ValueError)
    for job, (kind, got) in zip(jobs, res):
        if kind == "ok":
            _close(got, run(job))


def test_engine_chunks_and_groups(op):
    """More pairs than ``batch_rows`` (chunks of 4), a group across a chunk boundary, empty groups:
    the engine's scores are the model's on the twin's rows."""
    from ops._gpu_runtime import get_gpu_handle

    h = get_gpu_handle(MODEL)
    eng = h.engine
    flat = [p for ps in PASSAGES for p in ps]
    goff = [0, 7, 9, 9]
    res = eng.rerank_pairs(QUERIES, flat, goff, top_k=3)
    ids_q, lens_q = T.tokenize_rows([q.encode() for q in QUERIES], eng.S, h.cfg.vocab_size)
    ids_p, lens_p = T.tokenize_rows([p.encode() for p in flat], eng.S, h.cfg.vocab_size)
    qidx = np.repeat(np.arange(3), np.diff(goff)).astype(np.int32)
    ids, types, lens = T.pair_rows(ids_q, lens_q, ids_p, lens_p, qidx, T.default_max_query_tokens(eng.S))
    want = eng.model.score(torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(types))
    torch.testing.assert_close(res.scores, want, atol=1e-5, rtol=1e-5)
    assert res.idx.shape == (3, 3) and res.idx[2].eq(-1).all() and res.idx[1, 2] == -1
    for bad in ([0, 7, 9], [0, 7, 8, 9, 9], [1, 7, 9, 9], [0, 9, 7, 9]):
        with pytest.raises(ValueError):
            eng.rerank_pairs(QUERIES, flat, bad)
