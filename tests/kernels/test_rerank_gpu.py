"""The re-ranker on the GPU: ``pair_assemble`` and ``group_topk`` bit-equal to their twins on edge
rows, ``embed_layernorm`` with ``type_ids`` (the segment-embedding path and its clamp) against its
CPU reference, and ``ClassifyEngine.rerank_pairs`` against ``BertClassifier.score`` on the twin's
rows, the fp32 CPU oracle, its own eager form, and itself across batch compositions."""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random
from agent_tpu_amd.runtime.classify import ClassifyEngine
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------ pair_assemble
@pytest.mark.parametrize("S", [8, 16, 128])
def test_pair_assemble_kernel_equals_twin(gpu, S):
    rng = np.random.default_rng(S)
    for P in (1, 5, 64):  # 5: not a multiple of the four rows of a workgroup
        for Q in (1, 3):
            ids_q = rng.integers(1000, 4096, (Q, S), dtype=np.int32)
            ids_p = rng.integers(1000, 4096, (P + 3, S), dtype=np.int32)
            lens_q = rng.integers(2, S + 1, Q, dtype=np.int32)
            lens_p = rng.integers(2, S + 1, P + 3, dtype=np.int32)
            lens_q[0] = 2                       # an empty query
            lens_p[0] = 2                       # an empty passage
            lens_p[P // 2] = S                  # a full-length passage
            lens_q[-1] = S if Q > 1 else 2      # a full-length query
            if P >= 5:
                lens_p[1], lens_p[2] = -3, S + 9  # out of range: clamped into [2, S]
            qidx = rng.integers(0, Q, P + 3, dtype=np.int32)  # repeated
            qidx[0] = -1
            qidx[P - 1] = Q
            dev = [torch.from_numpy(a).to(gpu) for a in (ids_q, lens_q, ids_p, lens_p, qidx)]
            for mq in (0, 4, S):
                want = T.pair_rows(ids_q, lens_q, ids_p[:P], lens_p[:P], qidx[:P], mq, 7, 8, 3)
                out = [torch.full((P + 3, S), -7, dtype=torch.int32, device=gpu),
                       torch.full((P + 3, S), -7, dtype=torch.int32, device=gpu),
                       torch.full((P + 3,), -7, dtype=torch.int32, device=gpu)]
                ops.pair_assemble(*dev, mq, 7, 8, 3, ids=out[0], type_ids=out[1], lens=out[2], rows=P)
                for got, ref in zip(out, want):
                    got = got.cpu().numpy()
                    assert np.array_equal(got[:P], ref), (S, P, Q, mq)
                    assert (got[P:] == -7).all(), (S, P, Q, mq)  # rows past P are not touched
    ids, types, lens = ops.pair_assemble(*[t[:P] if t.shape[0] == P + 3 else t for t in dev], 4)  # allocating form
    want = T.pair_rows(ids_q, lens_q, ids_p[:P], lens_p[:P], qidx[:P], 4)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((ids, types, lens), want))


# --------------------------------------------------------------- group_topk
@pytest.mark.parametrize("k", [1, 10, 32])
def test_group_topk_kernel_equals_ref(gpu, k):
    g = torch.Generator().manual_seed(k)
    lens = [0, 1, 63, 64, 65, 1000, 0, 7]
    goff = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    P = int(goff[-1])
    values = torch.tensor([-1.0, -0.0, 0.0, 2.5])  # heavy ties and signed zeros
    for scores in (values[torch.randint(0, 4, (P,), generator=g)], torch.randn(P, generator=g)):
        want_i, want_v = ops.group_topk_ref(scores, goff, k)
        idx, val = ops.group_topk(scores.to(gpu), goff.to(gpu), k)
        assert idx.dtype == torch.int32 and val.dtype == torch.float32
        assert torch.equal(idx.cpu(), want_i)
        assert torch.equal(val.cpu().view(torch.int32), want_v.view(torch.int32))  # the stored bits
    # offsets out of [0, P] are clamped, a decreasing pair is an empty group, a NaN ranks as -inf
    s = torch.tensor([1.0, float("nan"), 2.0, float("-inf"), float("inf")])
    bad = torch.tensor([-4, 3, 2, 99], dtype=torch.int32)
    want_i, want_v = ops.group_topk_ref(s, bad, k)
    idx, val = ops.group_topk(s.to(gpu), bad.to(gpu), k)
    assert torch.equal(idx.cpu(), want_i) and torch.equal(val.cpu(), want_v)
    assert idx[0, 0] == 2 and idx[1].eq(-1).all() and idx[2, 0] == 2
    idx, val = ops.group_topk(torch.empty(0, device=gpu), torch.zeros(3, dtype=torch.int32, device=gpu), k)
    assert idx.shape == (2, k) and idx.eq(-1).all() and torch.isinf(val).all()


# ------------------------------------------------- embed_layernorm, type ids
def _rand(shape, dev, scale=1.0, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def _rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-6)).item()


@pytest.mark.parametrize("N,B,S", [(768, 3, 7), (256, 2, 128)])  # 21 tokens: not a multiple of four per workgroup
def test_embed_layernorm_with_type_ids(gpu, N, B, S):
    V = 1000
    word, pos, typ = _rand((V, N), gpu, seed=31), _rand((512, N), gpu, seed=32), _rand((2, N), gpu, seed=33)
    g = _rand((N,), gpu, 1.0, torch.float32, seed=34)
    b = _rand((N,), gpu, 1.0, torch.float32, seed=35)
    gen = torch.Generator().manual_seed(36)
    ids = torch.randint(0, V, (B, S), dtype=torch.int32, generator=gen)
    tt = torch.randint(0, 2, (B, S), dtype=torch.int32, generator=gen)
    tt[0, 1], tt[1, 2], tt[-1, -1] = -1, 5, 5  # out of range: clamped to 0 / type_vocab - 1
    y = ops.embed_layernorm(ids.to(gpu), word, pos, typ, g, b, 1e-12, type_ids=tt.to(gpu))
    cpu = (word.cpu().float(), pos.cpu().float(), typ.cpu().float(), g.cpu(), b.cpu(), 1e-12)
    ref = ops.embed_layernorm(ids, *cpu, type_ids=tt)
    assert _rel_err(y, ref) < 1e-2
    clamped = ops.embed_layernorm(ids, *cpu, type_ids=tt.clamp(0, 1))
    assert torch.equal(ref, clamped)
    # the segment row matters at this tolerance: all-zero type ids are far from the reference
    assert _rel_err(ops.embed_layernorm(ids.to(gpu), word, pos, typ, g, b, 1e-12), ref) > 5e-2


# ------------------------------------------------------------------ engine
QUERIES = ["how do gpus multiply matrices", "Weather tomorrow?", "kalo mira ten"]
GROUPS = [[], ["a recipe for bread"],
          ["matrix cores multiply tiles", "", "gpus have many compute units", "rain, then sun",
           "kalo " * 90, "it's (not) here", "x"]]


def _flat(groups):
    goff = [0]
    for g in groups:
        goff.append(goff[-1] + len(g))
    return [p for g in groups for p in g], goff


def _twin_rows(eng, queries, flat, goff, bucket):
    """The pair rows of an engine call by the Python twins, padded to ``bucket`` rows as the engine pads
    them (an empty passage of query 0)."""
    enc = lambda rows: [r.encode() for r in rows]  # noqa: E731
    if eng.vocab is not None:
        tok = lambda rows: eng.vocab.tokenize_rows(enc(rows), eng.S)  # noqa: E731
    else:
        tok = lambda rows: T.tokenize_rows(enc(rows), eng.S, eng.cfg.vocab_size)  # noqa: E731
    used = [q for q in range(len(queries)) if goff[q + 1] > goff[q]]
    qidx = np.repeat(np.arange(len(used)), [goff[q + 1] - goff[q] for q in used]).astype(np.int32)
    pad = bucket - len(flat)
    ids_q, lens_q = tok([queries[q] for q in used])
    ids_p, lens_p = tok(list(flat) + [""] * pad)
    return T.pair_rows(ids_q, lens_q, ids_p, lens_p, np.concatenate([qidx, np.zeros(pad, np.int32)]),
                       T.default_max_query_tokens(eng.S), *eng._special_ids())


def _oracle_checks(res, ref, goff, k):
    """Scores within the bound of test_bert_gpu.py; the ranking equals the oracle's wherever the oracle's
    gap to both neighbours exceeds twice that bound."""
    bound = 0.05 * ref.abs().max().item()
    assert (res.scores - ref).abs().max().item() < bound
    want_i, want_v = ops.group_topk_ref(ref, torch.tensor(goff, dtype=torch.int32), k)
    for q in range(len(goff) - 1):
        n = min(k, goff[q + 1] - goff[q])
        v = want_v[q, :n]
        gap = (v[:-1] - v[1:]) > 2 * bound
        clear = torch.cat([torch.tensor([True]), gap]) & torch.cat([gap, torch.tensor([True])]) if n else gap
        assert torch.equal(res.idx[q, :n][clear], want_i[q, :n][clear]), q
        assert res.idx[q, n:].eq(-1).all()


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    cfg = config_for("bert-tiny", num_labels=1)
    # One logit, so the oracle bound 0.05 * max|ref| is relative to a single value: the seeds here are
    # ones whose ORACLE logits sit at the head's scale (0.02 * sqrt(H) * |pooled|: ~0.2 for bert-tiny,
    # ~0.45 for bert-base). A seed whose one logit falls near zero would ask for an absolute error far
    # under one bf16 ulp of the activations, which the bound of test_bert_gpu.py (7 logits) never does.
    return cfg, init_random(cfg, seed=2, bias_std=0.02), T.WordPieceVocab.load(str(path))


@pytest.mark.parametrize("tokenizer", ["wordpiece", "hash"])
def test_rerank_pairs_tiny(gpu, tiny, tokenizer):
    cfg, pack, vocab = tiny
    vocab = vocab if tokenizer == "wordpiece" else None
    kw = dict(batch_rows=16, seq_len=128, topk=1, vocab=vocab)
    eng_g = ClassifyEngine(cfg, pack, gpu, use_graph=True, **kw)
    eng_e = ClassifyEngine(cfg, pack, gpu, use_graph=False, **kw)
    flat, goff = _flat(GROUPS)
    res = eng_g.rerank_pairs(QUERIES, flat, goff, top_k=5)
    again = eng_g.rerank_pairs(QUERIES, flat, goff, top_k=5)  # the second call replays the captured graph
    eager = eng_e.rerank_pairs(QUERIES, flat, goff, top_k=5)
    assert res.scores.shape == (8,) and res.idx.shape == (3, 5) and torch.isfinite(res.scores).all()
    for other in (again, eager):  # graph replay == eager, bit for bit
        assert torch.equal(res.scores, other.scores) and torch.equal(res.idx, other.idx)
        assert torch.equal(res.score, other.score)
    # the engine's scores are BertClassifier.score on the twin's rows, bit for bit
    ids, types, lens = _twin_rows(eng_g, QUERIES, flat, goff, eng_g._bucket(len(flat)))
    assert types.any() and (lens[:8] > 3).any()
    direct = eng_g.model.score(*(torch.from_numpy(a).to(gpu) for a in (ids, lens, types)))[:8].cpu()
    assert torch.equal(res.scores, direct)
    want_i, want_v = ops.group_topk_ref(res.scores, torch.tensor(goff, dtype=torch.int32), 5)
    assert torch.equal(res.idx, want_i) and torch.equal(res.score, want_v)
    oracle = BertClassifier(cfg, pack, fp32=True)
    ref = oracle.score(*(torch.from_numpy(a[:8]) for a in (ids, lens, types)))
    _oracle_checks(res, ref, goff, 5)
    sig = eng_g.rerank_pairs(QUERIES, flat, goff, top_k=5, activation="sigmoid")
    assert torch.equal(sig.idx, res.idx) and torch.equal(sig.scores, res.scores)
    assert torch.equal(sig.score[2], torch.sigmoid(res.score[2])) and sig.score[0].eq(float("-inf")).all()


@pytest.fixture(scope="module")
def base(gpu):
    cfg = config_for("bert-base", num_labels=1)
    pack = init_random(cfg, seed=1, bias_std=0.02)  # the seed: see the tiny fixture
    return cfg, pack, ClassifyEngine(cfg, pack, gpu, batch_rows=32, seq_len=128, topk=1)


def test_rerank_pairs_bert_base_folded_path(gpu, base):
    """16 pairs x 128 tokens: M = 2048 reaches the LayerNorm-folded fused encoder."""
    cfg, pack, eng = base
    assert eng.model.can_fold(16, 128)
    queries = make_text_rows(2, words_per_row=6, seed=1)
    groups = [make_text_rows(9, words_per_row=60, seed=2), make_text_rows(7, words_per_row=150, seed=3)]
    flat, goff = _flat(groups)
    res = eng.rerank_pairs(queries, flat, goff, top_k=8)
    ids, types, lens = _twin_rows(eng, queries, flat, goff, 16)
    assert lens.max() == 128 and types.sum() > 500
    ref = BertClassifier(cfg, pack, fp32=True).score(*(torch.from_numpy(a) for a in (ids, lens, types)))
    _oracle_checks(res, ref, goff, 8)


@pytest.fixture
def invariant():
    prev = ops.set_batch_invariant(True)
    yield
    ops.set_batch_invariant(prev)


def test_rerank_scores_are_batch_invariant(gpu, invariant):
    """A pair's raw score has the same bits alone, among 40 pairs, and across a chunk boundary
    (``batch_rows`` 32: 40 pairs are a chunk of 32 and one of 8, padded to the 16-row bucket)."""
    cfg = config_for("bert-base", num_labels=1)  # an engine of its own: its graphs are captured in this mode
    eng = ClassifyEngine(cfg, init_random(cfg, seed=0, device=gpu), gpu, batch_rows=32, seq_len=128, topk=1)
    queries = make_text_rows(3, words_per_row=7, seed=11)
    groups = [make_text_rows(30, words_per_row=40, seed=12), make_text_rows(6, words_per_row=150, seed=13),
              make_text_rows(4, words_per_row=10, seed=14)]  # group 1 spans rows 30..35: both chunks
    flat, goff = _flat(groups)
    many = eng.rerank_pairs(queries, flat, goff, top_k=4)
    assert many.scores.shape == (40,)
    for q, i in ((0, 0), (0, 29), (1, 1), (1, 2), (2, 3)):  # rows 0, 29, 31 (first chunk), 32, 39 (second)
        one = eng.rerank_pairs([queries[q]], [groups[q][i]], [0, 1], top_k=1)
        assert torch.equal(one.scores[0], many.scores[goff[q] + i]), (q, i)
    half = eng.rerank_pairs(queries[1:], groups[1] + groups[2], [0, 6, 10], top_k=4)
    assert torch.equal(half.scores, many.scores[30:])
