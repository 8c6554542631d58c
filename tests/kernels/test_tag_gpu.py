"""Token classification on the GPU: ``tag_entities`` logits against the fp64 evaluation of its formula
within the fp32 summation bound, its labels, groups and counts bit-equal to ``tag_select_ref`` on the
kernel's own logits on tie, NaN, infinity and edge rows in all three modes, ``ent_sum`` the sequential
fp32 sum of the kernel's own probabilities, rows that do not depend on their batch, and
``ClassifyEngine.tag_texts`` against ``BertClassifier.tags`` on the twin's rows, the fp32 CPU oracle, its own
eager form, the unfused form, and itself across batch compositions."""
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random
from agent_tpu_amd.runtime.classify import ClassifyEngine
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

pytestmark = pytest.mark.gpu

NINF = float("-inf")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _tables(L):
    """Label 0 is outside; label l >= 1 is B-T{(l-1)//2} when odd, I-T{(l-1)//2} when even."""
    lt = torch.tensor([-1] + [(l - 1) // 2 for l in range(1, L)], dtype=torch.int32)
    lb = torch.tensor([0] + [l & 1 for l in range(1, L)], dtype=torch.int32)
    return lt, lb


def _run(gpu, x, lens, B, S, u, su, c, lt, lb, mode, E, fin=None, ids=None, cont=None):
    L = u.shape[0]
    d = lambda t: None if t is None else t.to(gpu)  # noqa: E731
    logits = torch.full((B, S, L), 7.0, device=gpu)
    label = torch.full((B, S), 77, dtype=torch.int32, device=gpu)
    prob = torch.full((B, S), 7.0, device=gpu)
    ent, ent_sum, count = ops.tag_entities(d(x), d(lens), B, S, d(u), d(su), d(c), d(lt), d(lb), mode, E, fin=d(fin),
                                           ids=d(ids), cont=d(cont), label_out=label, prob_out=prob,
                                           logits_out=logits)
    return tuple(t.cpu() for t in (ent, ent_sum, count, label, prob, logits))


def _check_selection(out, lens, lt, lb, mode, E, ids, cont, tag):
    ent, ent_sum, count, label, prob, logits = out
    want = ops.tag_select_ref(logits, lens, lt, lb, mode, E, ids, cont)
    assert torch.equal(label, want[3]), tag
    assert torch.equal(ent, want[0]), tag
    assert torch.equal(count, want[2]), tag
    # __expf against the fp64 exponentials: the tolerance of classify_head_topk's probabilities
    assert torch.allclose(prob.double(), want[4].double(), atol=2e-4, rtol=1e-3), tag
    # the sums: sequential fp32 adds of the kernel's own probabilities, bit for bit
    own = ops.tag_group_ref(label.clamp(min=0), prob, lens, lt, lb, mode, E, ids, cont)
    assert torch.equal(own[0], ent), tag
    assert torch.equal(_bits(own[1]), _bits(ent_sum)), tag


# ------------------------------------------------------------------- logits
@pytest.mark.parametrize("S", [3, 7, 128, 512])
def test_tag_logits_within_fp32_summation_bound(gpu, S):
    for H in (64, 768, 1024):
        for L in (1, 9, 16, 17, 37, 64):  # 16 | 17: a label group boundary
            for B in (1, 5):
                for use_fin in (True, False):
                    g = torch.Generator().manual_seed(S * 7 + H + B + L)
                    x = torch.randn(B * S, H, generator=g).bfloat16()
                    u = torch.randn(L, H, generator=g) * 0.05
                    su = u.double().sum(1).float()
                    c = torch.randn(L, generator=g)
                    rstd = torch.rand(B * S, generator=g) * 1.5 + 0.5
                    mu = torch.randn(B * S, generator=g) * 0.1
                    fin = torch.stack([rstd, rstd * mu], 1).contiguous() if use_fin else None
                    lens = torch.randint(2, S + 1, (B,), generator=g, dtype=torch.int32)
                    lens[0] = S
                    pos = torch.arange(S).view(1, S)
                    live = (pos < lens.view(B, 1)).view(B * S)
                    text = ((pos >= 1) & (pos <= lens.view(B, 1) - 2)).view(B * S)
                    xd, ud = x.double(), u.double()
                    dot, mag = xd @ ud.t(), xd.abs() @ ud.abs().t()
                    if use_fin:
                        fd = fin.double()
                        ref = fd[:, :1] * dot - fd[:, 1:] * su.double() + c.double()
                        bound = 2 * H * 2.0 ** -24 * (fd[:, :1].abs() * mag + (fd[:, 1:] * su.double()).abs()
                                                      + c.double().abs())
                    else:
                        ref = dot + c.double()
                        bound = 2 * H * 2.0 ** -24 * (mag + c.double().abs())
                    xp, fp = x.clone(), None if fin is None else fin.clone()
                    xp[~live] = float("nan")  # poisoned rows at or past len change nothing
                    if fp is not None:
                        fp[~live] = float("nan")
                    lt, lb = _tables(L)
                    outs = [_run(gpu, xx, lens, B, S, u, su, c, lt, lb, 1, 8, fin=ff) for xx, ff in ((x, fin), (xp, fp))]
                    tag = (S, H, L, B, use_fin)
                    lg = outs[0][5].view(B * S, L)
                    err = (lg.double() - ref).abs()
                    if text.any():
                        assert (err[text] <= bound[text]).all(), (tag, (err[text] / bound[text]).max().item())
                    assert (lg[~text] == NINF).all(), tag
                    for a, b in zip(outs[0], outs[1]):
                        assert torch.equal(_bits(a), _bits(b)), tag
                    if B == 1 and L in (9, 17):
                        _check_selection(outs[0], lens, lt, lb, 1, 8, None, None, tag)


# ---------------------------------------------------------------- selection
def _exact_rows(S, L, su_inf=False, seed=0):
    """Rows whose logits the kernel computes exactly (H = 64, one-hot u, fin = (+-1, 0), c = -0.0): values
    from {-1, 0, 0, 2.5} (heavy ties, signed zeros), infinities (every other label of that token is
    inf * 0 = NaN), an all-NaN token, lens out of range, and the grouping's edge rows. ``su_inf``: one
    label's logit is NaN at every token (0 * inf), among finite ones."""
    g = torch.Generator().manual_seed(seed + S + L)
    B, H, V = 8, 64, 50
    values = torch.tensor([-1.0, 0.0, 0.0, 2.5])
    x = torch.zeros(B, S, H)
    x[:, :, :L] = values[torch.randint(0, 4, (B, S, L), generator=g)]
    rstd = torch.where(torch.rand(B, S, generator=g) < 0.5, -1.0, 1.0)
    if S >= 7:
        x[1, 2, 0] = float("nan")           # an all-NaN token: NaN * 0 in every other label
        x[1, 3, L - 1] = float("inf")
        x[1, 4, 0] = float("-inf")
    lens = torch.full((B,), S, dtype=torch.int32)
    lens[2], lens[3], lens[4] = 2, -5, S + 100
    for b, lab in ((5, 0), (6, min(2, L - 1)), (0, min(1, L - 1))):
        # all outside | one group of S - 2 tokens | S - 2 single-token B- groups
        x[b] = 0.0
        x[b, :, lab] = 2.5
        rstd[b] = 1.0
    lens[7] = max(3, (3 * S) // 4)
    u = torch.zeros(L, H)
    u[torch.arange(L), torch.arange(L)] = 1.0
    su = torch.zeros(L)
    if su_inf:
        su[L // 2] = float("inf")
    ids = torch.randint(-3, V + 3, (B, S), generator=g, dtype=torch.int32)  # negative and >= V too
    cont = (torch.rand(V, generator=g) < 0.4).to(torch.uint8)
    ids[7, 1] = 11
    cont[11] = 1  # cont set on token 1: still not a continuation
    ids[6, 2:] = 11  # the long group's tokens are continuations of token 1 in mode 2
    ids[0], cont[12] = 12, 0  # the B- row: no continuations
    rstd[1] = 1.0
    fin = torch.stack([rstd.view(-1), torch.zeros(B * S)], 1).contiguous()
    return B, x.view(B * S, H).bfloat16(), lens, u, su, torch.full((L,), -0.0), fin, ids, cont


@pytest.mark.parametrize("S,L", [(3, 5), (7, 5), (128, 17), (512, 5), (130, 64), (64, 1)])
def test_tag_selection_equals_ref_on_own_logits(gpu, S, L):
    lt, lb = _tables(L)
    if L >= 5:
        lt[L - 1], lb[L - 1] = 40, 0  # a label whose name has no B- / I- prefix: its own type
    saw_negzero = saw_nan = False
    for su_inf in (False, True):
        B, x, lens, u, su, c, fin, ids, cont = _exact_rows(S, L, su_inf)
        for mode in (0, 1, 2):
            for E in (1, 3, 512):
                tag = (S, L, su_inf, mode, E)
                out = _run(gpu, x, lens, B, S, u, su, c, lt, lb, mode, E, fin=fin, ids=ids, cont=cont)
                _check_selection(out, lens, lt, lb, mode, E, ids, cont, tag)
                ent, ent_sum, count, label, prob, lg = out
                assert (lg[:, 0] == NINF).all() and (lg[:, S - 1] == NINF).all(), tag
                for b in (2, 3):  # len clamped to 2: no text token
                    assert count[b] == 0 and ent[b, :, :3].eq(-1).all() and ent[b, :, 3].eq(0).all(), tag
                    assert (_bits(ent_sum[b]) == 0).all() and label[b].eq(-1).all() and prob[b].eq(0).all(), tag
                assert count[5] == 0, tag  # all outside
                if L >= 3 and not su_inf:
                    n = S - 2
                    if mode == 0:
                        assert count[6] == n and count[0] == n, tag
                    else:
                        assert count[6] == 1 and count[0] == n, tag
                        assert ent[6, 0].tolist() == [0, n - 1, 0, 1 if mode == 2 else n], tag
                    assert ent[0, :min(E, n), 3].eq(1).all(), tag  # B- B-: a group each, truncated at E
                    if E < n:
                        assert ent[0, E - 1, 0] == E - 1, tag
                # finite tokens: the fp64 softmax of the kernel's own logits at its own label
                fin_tok = torch.isfinite(lg).all(-1) & (label >= 0)
                sm = torch.softmax(lg.double(), -1).gather(-1, label.clamp(min=0).long().unsqueeze(-1)).squeeze(-1)
                assert torch.allclose(prob.double()[fin_tok], sm[fin_tok], atol=2e-4, rtol=1e-3), tag
                saw_negzero |= bool(((lg == 0) & (_bits(lg) != 0)).any())
                saw_nan |= bool(torch.isnan(lg).any())
                if S >= 7 and L >= 2:
                    assert torch.isnan(lg[1, 2]).all() and label[1, 2] == 0 and prob[1, 2] == 0, tag  # all NaN
                    assert label[1, 3] == L - 1 and prob[1, 3] == 1, tag  # +inf wins; the rest is NaN
    assert saw_negzero and (saw_nan or S < 7)


def test_tag_rows_alone_and_in_a_batch_and_bounds(gpu):
    S, H, L, B, E, V = 128, 768, 9, 5, 16, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B * S, H, generator=g).bfloat16()
    u = torch.randn(L, H, generator=g) * 0.05
    su, c = u.double().sum(1).float(), torch.randn(L, generator=g)
    fin = torch.stack([torch.rand(B * S, generator=g) + 0.5, torch.randn(B * S, generator=g) * 0.1], 1).contiguous()
    lens = torch.tensor([S, 40, 3, 99, 128], dtype=torch.int32)
    ids = torch.randint(0, V, (B, S), generator=g, dtype=torch.int32)
    cont = (torch.rand(V, generator=g) < 0.4).to(torch.uint8)
    lt, lb = _tables(L)
    for mode in (1, 2):
        whole = _run(gpu, x, lens, B, S, u, su, c, lt, lb, mode, E, fin=fin, ids=ids, cont=cont)
        for b in range(B):
            one = _run(gpu, x[b * S:(b + 1) * S], lens[b:b + 1], 1, S, u, su, c, lt, lb, mode, E,
                       fin=fin[b * S:(b + 1) * S], ids=ids[b:b + 1], cont=cont)
            for a, w in zip(one, whole):
                assert torch.equal(_bits(a[0]), _bits(w[b])), (mode, b)
    # caller's buffers with rows past B: untouched
    d = lambda t: t.to(gpu)  # noqa: E731
    ent = torch.full((B + 2, E, 4), 55, dtype=torch.int32, device=gpu)
    ent_sum = torch.full((B + 2, E), 5.5, device=gpu)
    count = torch.full((B + 2,), 55, dtype=torch.int32, device=gpu)
    label = torch.full((B + 2, S), 55, dtype=torch.int32, device=gpu)
    prob = torch.full((B + 2, S), 5.5, device=gpu)
    logits = torch.full((B + 2, S, L), 5.5, device=gpu)
    lens7 = torch.cat([lens, torch.tensor([S, S], dtype=torch.int32)])
    out = ops.tag_entities(d(x), d(lens7), B, S, d(u), d(su), d(c), d(lt), d(lb), 1, E, fin=d(fin), ent=ent,
                           ent_sum=ent_sum, count=count, label_out=label, prob_out=prob, logits_out=logits)
    assert out[0] is ent and out[1] is ent_sum and out[2] is count
    torch.cuda.synchronize()
    for t, v in ((ent, 55), (ent_sum, 5.5), (count, 55), (label, 55), (prob, 5.5), (logits, 5.5)):
        assert (t[B:] == v).all() and not (t[:B] == v).all()
    whole = _run(gpu, x, lens, B, S, u, su, c, lt, lb, 1, E, fin=fin)
    assert torch.equal(ent[:B].cpu(), whole[0]) and torch.equal(_bits(ent_sum[:B]), _bits(whole[1]))
    # B == 0: no launch
    e0, s0, c0 = ops.tag_entities(d(x[:0]), d(lens), 0, S, d(u), d(su), d(c), d(lt), d(lb), 1, E)
    assert e0.shape == (0, E, 4) and s0.shape == (0, E) and c0.shape == (0,)


def test_tag_unsupported_shapes_raise(gpu):
    def call(S=8, H=64, L=3, E=4, mode=1, B=2):
        lt, lb = _tables(L)
        return ops.tag_entities(torch.zeros(B * S, H, dtype=torch.bfloat16, device=gpu),
                                torch.full((B,), S, dtype=torch.int32, device=gpu), B, S,
                                torch.zeros(L, H, device=gpu), None, torch.zeros(L, device=gpu), lt.to(gpu),
                                lb.to(gpu), mode, E)
    call()
    for kw in (dict(S=2), dict(S=513), dict(H=96), dict(H=1088), dict(L=65), dict(E=0), dict(E=513), dict(mode=3),
               dict(mode=2)):  # mode 2 without ids / cont
        with pytest.raises(ValueError):
            call(**kw)


# ------------------------------------------------------------------ engine
TEXTS = ["matrix cores multiply tiles", "", "gpus have many compute units, naïve café in Zürich", "rain, then sun",
         "kalo " * 150, "it's (not) here", "x"] + make_text_rows(4, words_per_row=9, seed=5)


def _twin_rows(eng, texts, bucket):
    """The rows of an engine call by the Python twins, padded to ``bucket`` rows with empty strings."""
    rows = [t.encode() for t in texts] + [b""] * (bucket - len(texts))
    if eng.vocab is not None:
        ids, lens = eng.vocab.tokenize_rows(rows, eng.S)
    else:
        ids, lens = T.tokenize_rows(rows, eng.S, eng.cfg.vocab_size)
    return torch.from_numpy(ids), torch.from_numpy(lens)


def _oracle_checks(label_g, logits_g, logits_ref):
    """Logits within the project's engine bound 0.05 * max|logit|; the label equals the oracle's wherever
    the oracle's top logit leads its runner-up by more than twice that bound. Returns the share of the
    live tokens that qualified."""
    live = torch.isfinite(logits_ref).all(-1)
    assert torch.equal(torch.isfinite(logits_g).all(-1), live) and live.any()
    bound = 0.05 * logits_ref[live].abs().max().item()
    err = (logits_g[live] - logits_ref[live]).abs().max().item()
    print("logits vs oracle", err, "bound", bound)
    assert err < bound
    top2 = logits_ref[live].topk(2, -1)
    clear = (top2.values[:, 0] - top2.values[:, 1]) > 2 * bound
    assert torch.equal(label_g[live][clear].long(), top2.indices[:, 0][clear])
    return clear.float().mean().item()


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")
    cfg = config_for("bert-tiny", num_labels=1, tag_labels=5)
    # The seed is one at which, in the fp32 CPU ORACLE alone and for both tokenizers, at least a quarter of
    # the live tokens of TEXTS have a top logit that leads the runner-up by more than twice the logit bound
    # 0.05 * max|logit| (computed on the CPU from the oracle's logits, never from what the GPU returns).
    return cfg, init_random(cfg, seed=TINY_SEED, bias_std=0.02), T.WordPieceVocab.load(str(path))


TINY_SEED = 0  # the oracle's share of clear tokens: 0.753 of 320 (wordpiece) and 0.714 of 189 (hash)


@pytest.mark.parametrize("tokenizer", ["wordpiece", "hash"])
def test_tag_texts_tiny(gpu, tiny, tokenizer):
    cfg, pack, vocab = tiny
    vocab = vocab if tokenizer == "wordpiece" else None
    kw = dict(batch_rows=16, seq_len=128, topk=1, vocab=vocab)
    eng_g = ClassifyEngine(cfg, pack, gpu, use_graph=True, **kw)
    eng_e = ClassifyEngine(cfg, pack, gpu, use_graph=False, **kw)
    n = len(TEXTS)
    bucket = eng_g._bucket(n)
    ids, lens = _twin_rows(eng_g, TEXTS, bucket)
    assert lens.max() == 128 and lens[1] == 2
    st = eng_g._tag_state()
    for name, mode in (("simple", 1), ("none", 0)) + ((("first", 2),) if vocab is not None else ()):
        E = 6
        res = eng_g.tag_texts(TEXTS, name, E)
        again = eng_g.tag_texts(TEXTS, name, E)  # replays the captured graph
        eager = eng_e.tag_texts(TEXTS, name, E)
        assert res.ent.shape == (n, E, 4) and res.ent_sum.shape == (n, E) and len(res.counts) == n
        for other in (again, eager):  # graph replay == eager == second call, bit for bit
            assert torch.equal(res.ent, other.ent) and torch.equal(_bits(res.ent_sum), _bits(other.ent_sum))
            assert res.counts == other.counts and res.entities == other.entities
        # the engine's records are BertClassifier.tags on the twin's rows, bit for bit
        logits_g = torch.zeros((bucket, 128, 5), device=gpu)
        label_g = torch.zeros((bucket, 128), dtype=torch.int32, device=gpu)
        direct = eng_g.model.tags(ids.to(gpu), lens.to(gpu), st["label_type"], st["label_begin"], mode, E,
                                  cont=eng_g._tag_cont() if mode == 2 else None, logits_out=logits_g,
                                  label_out=label_g)
        assert torch.equal(res.ent, direct[0][:n].cpu()) and torch.equal(_bits(res.ent_sum), _bits(direct[1][:n]))
        assert res.counts == direct[2][:n].tolist()
        assert res.counts[1] == 0 and res.entities[1] == [] and res.truncated and max(res.counts) > E
        for text, row, count in zip(TEXTS, res.entities, res.counts):
            assert len(row) == min(count, E)
            for e in row:
                assert text[e["start"]:e["end"]] == e["word"] and e["word"] and 0 < e["score"] <= 1
        logits_ref = torch.zeros((n, 128, 5))
        BertClassifier(cfg, pack, fp32=True).tags(ids[:n], lens[:n], st["label_type"].cpu(), st["label_begin"].cpu(),
                                                  mode, E, cont=None if mode != 2 else eng_g._tag_cont().cpu(),
                                                  logits_out=logits_ref)
        assert _oracle_checks(label_g[:n].cpu(), logits_g[:n].cpu(), logits_ref) >= 0.25
    if vocab is None:
        with pytest.raises(ValueError) as e:
            eng_g.tag_texts(TEXTS, "first", 6)
        assert str(e.value) == eng_g.TAG_NEEDS_VOCAB
    assert eng_g.memory_bytes() > eng_e.pack.nbytes


@pytest.fixture(scope="module")
def base():
    cfg = config_for("bert-base", num_labels=1, tag_labels=9)
    return cfg, init_random(cfg, seed=1, bias_std=0.02)


def test_tag_bert_base_folded_path_and_unfused(gpu, base, monkeypatch):
    """16 rows x 128 tokens: M = 2048 reaches the LayerNorm-folded encoder; the fused tag head equals the
    ATPU_TAG_FUSED=0 form and the fp32 oracle within the logit bound."""
    cfg, pack = base
    eng = ClassifyEngine(cfg, pack, gpu, batch_rows=32, seq_len=128, topk=1)
    assert eng.model.can_fold(16, 128) and eng.model.tag_fused
    texts = make_text_rows(9, words_per_row=60, seed=2) + make_text_rows(7, words_per_row=150, seed=3)
    res = eng.tag_texts(texts, "simple", 32)
    ids, lens = _twin_rows(eng, texts, 16)
    assert lens.max() == 128 and lens.min() > 40
    st = eng._tag_state()
    dev = (ids.to(gpu), lens.to(gpu), st["label_type"], st["label_begin"])
    logits_f = torch.zeros((16, 128, 9), device=gpu)
    label_f = torch.zeros((16, 128), dtype=torch.int32, device=gpu)
    fused = eng.model.tags(*dev, 1, 32, logits_out=logits_f, label_out=label_f)
    assert torch.equal(res.ent, fused[0].cpu()) and torch.equal(_bits(res.ent_sum), _bits(fused[1]))
    assert res.counts == fused[2].tolist() and any(res.entities)
    monkeypatch.setenv("ATPU_TAG_FUSED", "0")
    plain = BertClassifier(cfg, eng.pack)
    assert not plain.tag_fused
    logits_u = torch.zeros((16, 128, 9), device=gpu)
    plain.tags(*dev, 1, 32, logits_out=logits_u)
    logits_ref = torch.zeros((16, 128, 9))
    BertClassifier(cfg, pack, fp32=True).tags(ids, lens, st["label_type"].cpu(), st["label_begin"].cpu(), 1, 32,
                                              logits_out=logits_ref)
    live = torch.isfinite(logits_ref)
    bound = 0.05 * logits_ref[live].abs().max().item()
    lf, lu = logits_f.cpu(), logits_u.cpu()
    assert torch.equal(torch.isfinite(lf), live) and torch.equal(torch.isfinite(lu), live)
    print("fused vs unfused", (lf[live] - lu[live]).abs().max().item(), "bound", bound)
    assert (lf[live] - lu[live]).abs().max().item() < bound
    _oracle_checks(label_f.cpu(), lf, logits_ref)


@pytest.fixture
def invariant():
    prev = ops.set_batch_invariant(True)
    yield
    ops.set_batch_invariant(prev)


def test_tag_rows_are_batch_invariant(gpu, base, invariant):
    """A row's records have the same bits alone, among 40 rows, and across a chunk boundary (``batch_rows``
    32: 40 rows are a chunk of 32 and one of 8, padded to the 16-row bucket)."""
    cfg, pack = base
    eng = ClassifyEngine(cfg, pack, gpu, batch_rows=32, seq_len=128, topk=1)  # its graphs are captured in this mode
    texts = (make_text_rows(30, words_per_row=40, seed=12) + make_text_rows(6, words_per_row=150, seed=13)
             + make_text_rows(4, words_per_row=10, seed=14))
    many = eng.tag_texts(texts, "simple", 16)
    assert many.ent.shape == (40, 16, 4) and any(many.entities)
    for r in (0, 29, 31, 32, 39):  # rows of the first chunk and of the second
        one = eng.tag_texts([texts[r]], "simple", 16)
        assert torch.equal(one.ent[0], many.ent[r]) and torch.equal(_bits(one.ent_sum[0]), _bits(many.ent_sum[r])), r
        assert one.counts[0] == many.counts[r] and one.entities[0] == many.entities[r], r
    half = eng.tag_texts(texts[30:], "simple", 16)
    assert torch.equal(half.ent, many.ent[30:]) and torch.equal(_bits(half.ent_sum), _bits(many.ent_sum[30:]))
    assert half.entities == many.entities[30:]
