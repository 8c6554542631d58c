"""term_max / term_select (sparse_head.hip) and the engine's sparse_rows against float64 references."""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.models.bert import config_for, init_random
from agent_tpu_amd.runtime.classify import ClassifyEngine, pack_rows
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

pytestmark = pytest.mark.gpu

NINF = float("-inf")
U = 2.0 ** -24  # the unit roundoff of fp32
# device log1pf, measured (no document states it): 0.56 ulp on (0, 64] (docs/PERF_NOTES.md); plus one for the rounding
LOG1P_ULPS = 0.56 + 1.0


def _ref_max(t64, lens, E64, S):  # per text: (max over live tokens of t . E, of |t| . |E|), float64
    zero = torch.zeros((1, E64.shape[0]), dtype=torch.float64, device=t64.device)
    rows = [t64[b * S:b * S + n] for b, n in enumerate(lens)]
    return (torch.stack([torch.cat([r @ E64.T, zero + NINF]).amax(0) for r in rows]),
            torch.stack([torch.cat([r.abs() @ E64.abs().T, zero]).amax(0) for r in rows]))


def _ulps(got, ref):  # |got - ref| in fp32 ulps of ref (float64)
    return (got.double() - ref).abs() / torch.ldexp(torch.ones_like(ref), torch.frexp(ref).exponent - 24)


@pytest.mark.parametrize("tile", [0, 32])
@pytest.mark.parametrize("V,H", [(1, 64), (63, 64), (65, 192), (4101, 768), (300, 1024)])
def test_term_max_exact_on_integers(gpu, V, H, tile):
    """|t| <= 8, |E| <= 16: every partial sum is below 2^24, so fp32 is exact; padding rows hold NaN or 3e38."""
    g = torch.Generator().manual_seed(V + H)
    S, lens, B = 40, [0, 1, 15, 16, 17, 33, 40], 7
    t = torch.randint(-8, 9, (B * S, H), generator=g).double()
    E = torch.randint(-16, 17, (V, H), generator=g).double()
    ref, _ = _ref_max(t, lens, E, S)
    tp = t.clone().view(B, S, H)
    for b, n in enumerate(lens):
        tp[b, n::2] = float("nan")
        tp[b, n + 1::2] = 3e38
    got = ops.term_max(tp.view(B * S, H).to(gpu, torch.bfloat16), torch.tensor(lens, dtype=torch.int32, device=gpu),
                       E.to(gpu, torch.bfloat16), S, vocab_tile=tile).cpu()
    assert (ref[0] == NINF).all() and torch.equal(got.double(), ref)


@pytest.mark.parametrize("V,H", [(33, 64), (4101, 192), (30522, 768)])
def test_term_max_gaussian_within_accumulation_bound(gpu, V, H):
    """Products are exact, the H accumulation steps round: |got - ref| <= H 2^-24 max_i sum_k |t_ik E_k|."""
    g = torch.Generator().manual_seed(V)
    S, lens = 128, [128, 1, 77, 40]
    t = torch.randn((len(lens) * S, H), generator=g).to(gpu, torch.bfloat16)
    E = torch.randn((V, H), generator=g).to(gpu, torch.bfloat16)
    got = ops.term_max(t, torch.tensor(lens, dtype=torch.int32, device=gpu), E, S)
    ref, mag = _ref_max(t.double(), lens, E.double(), S)
    assert ((got.double() - ref).abs() <= H * U * mag).all()


@pytest.fixture(scope="module")
def select_rows():
    """Half-integers (the bias add is exact): heavy ties, a -inf row, few positives among NaN, all equal, wide."""
    g = torch.Generator().manual_seed(5)
    V = 70001
    x = torch.randint(-8, 13, (5, V), generator=g).float() / 2
    x[1] = NINF
    x[2] = torch.where(torch.rand(V, generator=g) < 0.002, x[2].abs() + 1, -x[2].abs())
    x[2, ::7] = float("nan")
    x[3] = 2.5
    x[4] = torch.randint(-50, 2001, (V,), generator=g).float() / 2
    x[0, 5::11] = NINF
    return x, torch.randint(-2, 3, (V,), generator=g).float() / 2


@pytest.mark.parametrize("k", [1, 32, 33, 256, 1024])
@pytest.mark.parametrize("V", [1, 255, 257, 30522, 70001])
def test_term_select_exact(gpu, select_rows, V, k):
    xmax, bias = select_rows[0][:, :V].contiguous(), select_rows[1][:V].contiguous()
    tok, xs, w, nnz = (o.cpu() for o in ops.term_select(xmax.to(gpu), bias.to(gpu), k))
    x = xmax.double() + bias.double()
    for b in range(x.shape[0]):
        ids = torch.nonzero(x[b] > 0).view(-1)
        ids = ids[torch.sort(-x[b, ids], stable=True).indices][:k]  # (x descending, token ascending)
        n = ids.numel()
        assert nnz[b] == (x[b] > 0).sum() and tok[b, :n].tolist() == ids.tolist() and (tok[b, n:] == -1).all()
        assert torch.equal(xs[b, :n].double(), x[b, ids]) and (xs[b, n:] == 0).all() and (w[b, n:] == 0).all()
        if n:
            assert _ulps(w[b, :n], torch.log1p(x[b, ids])).max() <= LOG1P_ULPS


@pytest.fixture(scope="module")
def wp_vocab(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    return T.WordPieceVocab.load(str(path))


def test_sparse_rows_are_batch_invariant(gpu):
    """A text's result has the same bits alone, in a full batch among other texts, and at another position."""
    prev = ops.set_batch_invariant(True)
    try:
        cfg = config_for("bert-base", num_labels=1, mlm_head=True)
        eng = ClassifyEngine(cfg, init_random(cfg, seed=1, bias_std=0.02), gpu, batch_rows=16, seq_len=128, topk=1)
        texts = make_text_rows(8, words_per_row=60, seed=3) + make_text_rows(9, words_per_row=150, seed=4)
        alone = [o.clone() for o in eng.sparse_rows(texts[5:6], 300)]
        full = [o.clone() for o in eng.sparse_rows(texts[:16], 300)]
        moved = [o.clone() for o in eng.sparse_rows(texts[16:] + texts[8:16][::-1] + texts[5:6] + texts[:5], 300)]
        assert alone[3].item() > 300 and (alone[0] >= 0).all()
        for a, f, m in zip(alone, full, moved):
            assert torch.equal(a[0], f[5]) and torch.equal(a[0], m[9])
    finally:
        ops.set_batch_invariant(prev)


@pytest.mark.parametrize("tokenizer", ["wordpiece", "hash"])
def test_sparse_rows_tiny_end_to_end(gpu, wp_vocab, tokenizer):
    """engine.sparse_rows against the float64 chain fed with the GPU's own transform rows, both directions within the
    accumulation bound (plus the fp32 rounding of the bias add); 19 texts on a 16-row engine: a partly filled bucket."""
    cfg = config_for("bert-tiny", mlm_head=True)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=7, bias_std=0.02), gpu, batch_rows=16, seq_len=64, topk=1,
                         vocab=wp_vocab if tokenizer == "wordpiece" else None)
    texts = make_text_rows(9, words_per_row=6, seed=1) + [""] + make_text_rows(9, words_per_row=70, seed=2)
    k, S, H = 64, 64, cfg.hidden
    tok, xs, w, nnz = (o.cpu() for o in eng.sparse_rows(texts, k))
    assert tok.shape == (19, k) and nnz.shape == (19,)
    for o, tail in zip((tok, xs, w, nnz), eng.sparse_rows(texts[16:], k)):  # the second chunk on its own
        assert torch.equal(o[16:], tail.cpu())
    fi = eng.model.fill_inputs()
    E64, bias = fi["E"].double(), fi["bias"].double()
    for b0 in (0, 16):  # the engine's chunks, padded with empty strings to their buckets like the engine's
        chunk = texts[b0:b0 + 16]
        rows = chunk + [""] * (eng._bucket(len(chunk)) - len(chunk))
        text, offs = pack_rows(r.encode("utf-8") for r in rows)
        ids, lens = eng._tokenize(torch.from_numpy(text).to(gpu), torch.from_numpy(offs).to(gpu))
        t64 = eng.model.term_rows(ids, lens).double()
        ref, mag = _ref_max(t64, lens.tolist()[:len(chunk)], E64, S)
        x = (ref + bias).cpu()
        bound = (H * U * mag).cpu() + U * x.abs()
        for i in range(len(chunk)):
            r = b0 + i
            n = int((tok[r] >= 0).sum())
            ids_r = tok[r, :n].long()
            assert n == min(int(nnz[r]), k) and n > 0 and (tok[r, n:] == -1).all() and (w[r, n:] == 0).all()
            assert ((xs[r, :n].double() - x[i, ids_r]).abs() <= bound[i, ids_r]).all()
            assert _ulps(w[r, :n], torch.log1p(xs[r, :n].double())).max() <= LOG1P_ULPS
            floor = xs[r, n - 1].double() if n == k else 0.0
            must = torch.nonzero((x[i] - bound[i] > 0) & (x[i] - bound[i] > floor)).view(-1)
            assert set(must.tolist()) <= set(ids_r.tolist())


def test_sparse_rows_errors(gpu):
    cfg = config_for("bert-tiny", mlm_head=True)
    eng = ClassifyEngine(cfg, init_random(cfg, seed=7), gpu, batch_rows=8, seq_len=32, topk=1, use_graph=False)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="max_terms"):
            eng.sparse_rows(["a"], bad)
    plain = config_for("bert-tiny")
    with pytest.raises(ValueError, match="no MLM head"):
        ClassifyEngine(plain, init_random(plain, seed=7), gpu, batch_rows=8, seq_len=32, use_graph=False).sparse_texts(["a"])
