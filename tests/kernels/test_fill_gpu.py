"""Masked-token prediction on the GPU: ``fill_assemble`` bit-equal to its Python twin (poisoned offsets
included), ``vocab_topk`` exact on integer data, within the fp32 summation bound on Gaussian data and
bit-invariant to the batch, ``mask_gather`` within the LayerNorm bound, and ``ClassifyEngine.fill_texts``
against ``BertClassifier.fills`` on the twin's rows, the fp32 CPU oracle, its own eager form, the unfused
form, and itself across batch compositions."""
import math

import numpy as np
import pytest
import torch

import _exact_ln as E
from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.models.bert import BertClassifier, config_for, init_random
from agent_tpu_amd.runtime.classify import ClassifyEngine
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

pytestmark = pytest.mark.gpu

NINF = float("-inf")
U = 2.0 ** -24  # the unit roundoff of fp32


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def wp_vocab(tmp_path_factory):
    path = tmp_path_factory.mktemp("wp") / "vocab.txt"
    with open(path, "wb") as f:
        f.write("\n".join(make_wordpiece_vocab(300, seed=1)).encode("utf-8") + b"\n")  # it has a [MASK] entry
    return T.WordPieceVocab.load(str(path))


# ------------------------------------------------------------ fill_assemble
def _fill_texts(S):
    """No mask; a mask first and last; adjacent masks (empty pieces); a mask landing exactly at position
    S - 2 (kept) and at S - 1 (cut: a '.' is one token for both tokenizers); 16 masks; an empty text."""
    return ["plain words, no mask", "[MASK] middle words [MASK]", "a [MASK][MASK] b", ". " * (S - 3) + "[MASK]",
            ". " * (S - 2) + "[MASK] tail", " ".join(["x [MASK]"] * 16), "", "[MASK]"]


def _segments(texts, S, vocab):
    pieces, segoff = [], [0]
    for t in texts:
        pieces += T.split_masks(t)[0]
        segoff.append(len(pieces))
    rows = [p.encode() for p in pieces]
    ids_s, lens_s = vocab.tokenize_rows(rows, S) if vocab is not None else T.tokenize_rows(rows, S, 4096)
    return ids_s, lens_s, np.array(segoff, dtype=np.int32)


@pytest.mark.parametrize("tokenizer", ["hash", "wordpiece"])
@pytest.mark.parametrize("S", [3, 4, 8, 128])
def test_fill_assemble_equals_twin(gpu, wp_vocab, S, tokenizer):
    vocab = wp_vocab if tokenizer == "wordpiece" else None
    sp = (vocab.cls_id, vocab.sep_id, vocab.pad_id, vocab.mask_id) if vocab else (101, 102, 0, 103)
    ids_s, lens_s, segoff = _segments(_fill_texts(S), S, vocab)
    B, M = len(segoff) - 1, 16
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    want = T.fill_rows(ids_s, lens_s, segoff, M, *sp)
    got = ops.fill_assemble(dev(ids_s), dev(lens_s), dev(segoff), M, *sp)
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), torch.from_numpy(w))
    assert (want[2][3, 0], want[2][4, 0]) == (S - 2, -1) and want[1].max() == S and (S < 4 or want[2][5, 0] == 2)
    # poisoned offsets and lengths (negative, huge): clamped, equal to the twin, and nothing outside
    # [B, S] / [B] / [B, M] of canary-padded outputs is touched
    for seed in range(3):
        g = np.random.default_rng(seed + S)
        so = segoff.copy()
        ls = lens_s.copy()
        so[g.integers(0, B + 1, 3)] = [-7, 2 ** 31 - 1, -2 ** 31]
        ls[g.integers(0, len(ls), 4)] = [-1, 2 ** 31 - 1, -2 ** 31, S + 1]
        want = T.fill_rows(ids_s, lens_s if seed == 0 else ls, so, M, *sp)
        ids = torch.full((B + 2, S), 77, dtype=torch.int32, device=gpu)
        lens = torch.full((B + 2,), 77, dtype=torch.int32, device=gpu)
        pos = torch.full((B + 2, M), 77, dtype=torch.int32, device=gpu)
        out = ops.fill_assemble(dev(ids_s), dev(lens_s if seed == 0 else ls), dev(so), M, *sp, ids=ids, lens=lens,
                                pos=pos, rows=B)
        assert out[0] is ids and out[1] is lens and out[2] is pos
        for t, w in zip((ids, lens, pos), want):
            assert torch.equal(t[:B].cpu(), torch.from_numpy(w)), seed
            assert (t[B:] == 77).all(), seed
    # B == 0: no launch
    e = ops.fill_assemble(dev(ids_s), dev(lens_s), dev(segoff[:1]), M, *sp)
    assert e[0].shape == (0, S) and e[1].shape == (0,) and e[2].shape == (0, M)
    for bad in (dict(max_masks=0), dict(max_masks=17)):
        with pytest.raises(ValueError):
            ops.fill_assemble(dev(ids_s), dev(lens_s), dev(segoff), bad["max_masks"], *sp)
    if S == 3:
        with pytest.raises(ValueError):
            ops.fill_assemble(dev(ids_s[:, :2]), dev(lens_s), dev(segoff), M, *sp)


# ------------------------------------------------------------ vocab_topk, exact
@pytest.mark.parametrize("V", [1, 31, 33, 4101, 30522])
def test_vocab_topk_exact_on_integers(gpu, V):
    """Small integers: every product and partial sum is an exact fp32 integer whatever the order (|logit| <=
    768 * 3 * 2 + 4 < 2^24), so tok and logit must equal the fp64 (= exact integer) evaluation, with the
    heavy ties that a range of a few hundred values over up to 30522 tokens gives."""
    for H in (64, 192, 768):
        g = torch.Generator().manual_seed(V + H)
        t = torch.randint(-3, 4, (33, H), generator=g).float()
        Ew = torch.randint(-2, 3, (V, H), generator=g).float()
        bias = torch.randint(-4, 5, (V,), generator=g).float()
        if V >= 33:
            Ew[7], bias[7] = Ew[20], bias[20]  # two identical tokens: a tie at every slot
        ref = t.double() @ Ew.double().t() + bias.double()
        assert ref.abs().max() < 2 ** 24
        order = torch.sort(ref, dim=1, descending=True, stable=True).indices
        td, Ed, bd = t.to(gpu), Ew.bfloat16().to(gpu), bias.to(gpu)
        for R in (1, 17, 33):
            valid = torch.ones(R, dtype=torch.int32)
            if R >= 17:
                valid[8] = 0  # an invalid slot in the middle of a tile
            for k in (1, 5, 32):  # k > V at V = 1 and 31
                tok, logit, prob, lse = (x.cpu() for x in ops.vocab_topk(td[:R].contiguous(), Ed, bd, k,
                                                                         valid=valid.to(gpu)))
                kk = min(k, V)
                want_tok = torch.full((R, k), -1, dtype=torch.int64)
                want_val = torch.full((R, k), NINF, dtype=torch.float64)
                want_tok[:, :kk] = order[:R, :kk]
                want_val[:, :kk] = torch.gather(ref[:R], 1, order[:R, :kk])
                bad = valid == 0
                want_tok[bad], want_val[bad] = -1, NINF
                tag = (V, H, R, k)
                assert torch.equal(tok.long(), want_tok), tag
                assert torch.equal(logit.double(), want_val), tag
                assert (prob[bad] == 0).all() and (lse[bad] == 0).all() and (prob[:, kk:] == 0).all(), tag
                lse64 = torch.logsumexp(ref[:R], 1)
                assert torch.allclose(lse[~bad].double(), lse64[~bad], rtol=1e-5, atol=1e-5), tag
                p64 = torch.exp(want_val - lse64.view(-1, 1))
                assert torch.allclose(prob[~bad].double(), p64[~bad], rtol=1e-4, atol=1e-7), tag
    assert ops.vocab_topk(td[:0], Ed, bd, 5)[0].shape == (0, 5)  # R == 0: no launch


def test_vocab_topk_unsupported_shapes_raise(gpu):
    def call(H=64, V=40, k=5, R=2):
        return ops.vocab_topk(torch.zeros(R, H, device=gpu), torch.zeros(V, H, dtype=torch.bfloat16, device=gpu),
                              torch.zeros(V, device=gpu), k)
    call()
    for kw in (dict(H=96), dict(H=1088), dict(k=0), dict(k=33), dict(V=0)):
        with pytest.raises(ValueError):
            call(**kw)


# ------------------------------------------------------------ vocab_topk, Gaussian
def _gauss(V, H, R, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(R, H, generator=g)
    Ew = (torch.randn(V, H, generator=g) * 0.2).bfloat16()
    bias = torch.randn(V, generator=g)
    return t, Ew, bias


def _lse_bound(lg64, V):
    """The bound of the kernel's lse against the fp64 lse of the same logits, from the documented combine
    (mlm_head.hip's header). With m the maximum, D = m - min the spread and u = 2^-24: a term expf(x - m)
    carries the rounding of the difference (u D, which the exponential turns into a relative error), expf's
    own 2 ulps and one rounding where it is added: (D + 3) u. A partial sum is rescaled at most 6 times (4
    steps of its wave, the split's combine, the merge's), each by such a factor and one multiplication:
    6 (D + 4) u. The additions a term passes: 9 per step x 4 steps, 16 in the split's combine, ceil(P / 64)
    + 6 in the merge. All are relative errors of a sum of positive terms, so they add:
    c = depth + 7 (D + 4). Then lse = m + logf(sum): c u through the logarithm (d log s = ds / s), logf's
    2 ulps of |log sum| and the final addition's u |lse|."""
    m = lg64.max(1).values
    D = m - lg64.min(1).values
    P = ops.vocab_topk_splits(V)
    depth = 9 * 4 + 16 + math.ceil(P / 64) + 6
    lse = torch.logsumexp(lg64, 1)
    c = depth + 7 * (D + 4)
    return lse, U * (c + 2 * (lse - m).abs() + lse.abs())


@pytest.mark.parametrize("V,H", [(33, 64), (4101, 192), (30522, 768), (4101, 1024)])
def test_vocab_topk_gaussian_within_bounds(gpu, V, H):
    R = 17
    t, Ew, bias = _gauss(V, H, R, V + H)
    td, Ed, bd = t.to(gpu), Ew.to(gpu), bias.to(gpu)
    t64, E64, b64 = t.double(), Ew.double(), bias.double()
    ref = t64 @ E64.t() + b64
    # H fused multiply-adds and the bias addition, one rounding each: gamma_n with n = H + 1
    n = H + 1
    bound = n * U / (1 - n * U) * (t64.abs() @ E64.abs().t() + b64.abs())
    for k in (5, 32):
        lg = torch.full((R, V), 7.0, device=gpu)
        tok, logit, prob, lse = (x.cpu() for x in ops.vocab_topk(td, Ed, bd, k, logits_out=lg))
        lg = lg.cpu()
        err = (lg.double() - ref).abs()
        print(f"V={V} H={H} k={k}: worst logit error / bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all()
        # the selection is the reference selection of the kernel's own logits, exactly
        want = ops.vocab_select_ref(lg, k)
        assert torch.equal(tok, want[0]) and torch.equal(_bits(logit), _bits(want[1]))
        lse64, lb = _lse_bound(lg.double(), V)
        lerr = (lse.double() - lse64).abs()
        print(f"V={V} H={H} k={k}: worst lse error / bound {(lerr / lb).max().item():.3f}")
        assert (lerr <= lb).all()
        # prob = expf(logit - lse): the difference's rounding and lse's error through the exponential, expf's 2 ulps
        live = tok >= 0
        d = logit.double() - lse64.view(-1, 1)
        p64 = torch.where(live, torch.exp(d), torch.zeros_like(d))
        pb = p64 * (lb.view(-1, 1) + U * (d.abs() + 3))
        perr = (prob.double() - p64).abs()
        print(f"V={V} H={H} k={k}: worst prob error / bound {(perr[live] / pb[live]).max().item():.3f}")
        assert (perr[live] <= pb[live]).all() and (prob[~live] == 0).all()
    # lse_in replaces the normaliser of prob only
    other = torch.linspace(3.0, 9.0, R)
    tok2, logit2, prob2, lse2 = (x.cpu() for x in ops.vocab_topk(td, Ed, bd, 5, lse_in=other.to(gpu)))
    tok1, logit1, _, lse1 = (x.cpu() for x in ops.vocab_topk(td, Ed, bd, 5))
    assert torch.equal(tok1, tok2) and torch.equal(_bits(logit1), _bits(logit2)) and torch.equal(_bits(lse1), _bits(lse2))
    want = torch.exp(logit2.double() - other.double().view(-1, 1))
    assert torch.allclose(prob2.double(), want, rtol=1e-5, atol=0)


def test_vocab_topk_full_vocabulary_probabilities_sum_to_one(gpu):
    V, H, R = 31, 64, 5
    t, Ew, bias = _gauss(V, H, R, 3)
    lg = torch.zeros((R, V), device=gpu)
    tok, logit, prob, lse = (x.cpu() for x in ops.vocab_topk(t.to(gpu), Ew.to(gpu), bias.to(gpu), 32, logits_out=lg))
    assert (tok[:, :V].sort(1).values == torch.arange(V)).all() and (tok[:, V:] == -1).all()
    assert (logit[:, V:] == NINF).all() and (prob[:, V:] == 0).all()
    lse64, lb = _lse_bound(lg.cpu().double(), V)
    d = logit[:, :V].double() - lse64.view(-1, 1)
    pb = torch.exp(d) * (lb.view(-1, 1) + U * (d.abs() + 3))
    assert ((prob.double().sum(1) - 1).abs() <= pb.sum(1)).all()


def test_vocab_topk_nan_and_infinite_logits(gpu):
    V, H = 70, 64
    t = torch.zeros(3, H)
    t[:, 0] = 1.0
    Ew = torch.zeros(V, H)
    Ew[:, 0] = torch.arange(V).float() % 5
    bias = torch.zeros(V)
    bias[3], bias[11], bias[40] = float("nan"), NINF, float("nan")
    lg = torch.zeros((3, V), device=gpu)
    out = [x.cpu() for x in ops.vocab_topk(t.to(gpu), Ew.bfloat16().to(gpu), bias.to(gpu), 32, logits_out=lg)]
    want = ops.vocab_select_ref(lg.cpu(), 32)
    assert torch.isnan(lg.cpu()[:, 3]).all()
    assert torch.equal(out[0], want[0]) and torch.equal(_bits(out[1]), _bits(want[1]))
    assert torch.allclose(out[3], want[3], rtol=1e-6) and torch.allclose(out[2], want[2], rtol=1e-5, atol=1e-9)
    out = [x.cpu() for x in ops.vocab_topk(t.to(gpu), Ew[:3].bfloat16().to(gpu), bias[3:4].expand(3).contiguous().to(gpu), 5)]
    assert (out[0][:, :3] == torch.arange(3)).all() and (out[1] == NINF).all() and (out[2] == 0).all()
    assert (out[3] == NINF).all()  # every logit NaN: an empty sum


# ------------------------------------------------------------ invariance
@pytest.mark.parametrize("V,H,k", [(30522, 768, 5), (4101, 192, 32), (33, 64, 16)])
def test_vocab_topk_slot_bits_do_not_depend_on_the_batch(gpu, V, H, k):
    """A slot's (tok, logit, prob, lse) bits: alone, at slots 0, 16 and 32 of 33, and among 1024 slots."""
    t, Ew, bias = _gauss(V, H, 1024, V + k)
    Ed, bd = Ew.to(gpu), bias.to(gpu)
    row = t[517:518].clone()
    alone = [x.cpu() for x in ops.vocab_topk(row.to(gpu), Ed, bd, k)]
    for place in (0, 16, 32):
        t33 = t[100:133].clone()
        t33[place] = row[0]
        got = [x.cpu() for x in ops.vocab_topk(t33.to(gpu), Ed, bd, k)]
        for a, b in zip(alone, got):
            assert torch.equal(_bits(a[0]), _bits(b[place])), (V, place)
    many = [x.cpu() for x in ops.vocab_topk(t.to(gpu), Ed, bd, k)]
    for a, b in zip(alone, many):
        assert torch.equal(_bits(a[0]), _bits(b[517])), V
    # among invalid neighbours
    valid = torch.zeros(33, dtype=torch.int32)
    valid[16] = 1
    t33 = t[:33].clone()
    t33[16] = row[0]
    got = [x.cpu() for x in ops.vocab_topk(t33.to(gpu), Ed, bd, k, valid=valid.to(gpu))]
    for a, b in zip(alone, got):
        assert torch.equal(_bits(a[0]), _bits(b[16])), V


def test_vocab_topk_target_logits_equal_full_vocabulary_logits(gpu):
    """The k order is a function of H alone: a token's logit over a gathered table has the bits of its logit
    over the whole vocabulary; with lse_in its probability is the full-vocabulary one."""
    V, H, R = 30522, 768, 17
    t, Ew, bias = _gauss(V, H, R, 11)
    td, Ed, bd = t.to(gpu), Ew.to(gpu), bias.to(gpu)
    lg = torch.zeros((R, V), device=gpu)
    full = ops.vocab_topk(td, Ed, bd, 32, logits_out=lg)
    assert torch.equal(_bits(full[1]), _bits(torch.gather(lg, 1, full[0].long())))
    tids = torch.cat([full[0][3, :4].cpu().long(), torch.tensor([0, 511, 512, 30521, 7777, 12345])])
    part = ops.vocab_topk(td, Ed[tids.to(gpu)].contiguous(), bd[tids.to(gpu)].contiguous(), tids.numel(),
                          lse_in=full[3])
    back = tids[part[0].cpu().long()]
    assert torch.equal(_bits(part[1]), _bits(torch.gather(lg.cpu(), 1, back)))
    for r in range(R):  # a target among the full top 32 has the same probability bits
        for j, tk in enumerate(back[r].tolist()):
            hit = (full[0][r].cpu() == tk).nonzero()
            if hit.numel():
                assert _bits(part[2][r, j]).item() == _bits(full[2][r, hit[0, 0]]).item()
    assert (back[3, :4].sort().values == tids[:4].sort().values).all()


# ------------------------------------------------------------ mask_gather
@pytest.mark.parametrize("S", [3, 128])
@pytest.mark.parametrize("H", [64, 768])
def test_mask_gather_within_layernorm_bound(gpu, H, S):
    """The fused rows against the fp64 LayerNorm within the project's per-element LayerNorm bound (_exact_ln:
    2^-8 |ref| + 2^-20 (...)); ops.layernorm-then-gather lies within the same bound of the same reference, so
    the two differ by at most twice it. The plain gather copies. Invalid slots give zeros."""
    B, M = 5, 4
    x, gamma, beta = E.random_rows(B * S, H, seed=H + S)
    x64 = x.double()
    mu = x64.mean(1)
    rstd = 1.0 / torch.sqrt(((x64 - mu.view(-1, 1)) ** 2).mean(1) + 1e-12)
    fin = torch.stack([rstd, rstd * mu], 1).float().contiguous()
    g = torch.Generator().manual_seed(S)
    pos = torch.randint(-1, S, (B, M), generator=g, dtype=torch.int32)
    pos[0, 0], pos[1, 1], pos[2, 2] = 0, S - 1, S  # S: out of range
    mrow = torch.tensor([0, 1, 2, 3, 4, 4, 0, -1, B, 2, 1], dtype=torch.int32)
    mord = torch.tensor([0, 1, 2, 3, 0, 1, 1, 0, 0, -1, M], dtype=torch.int32)
    R = mrow.numel()
    dev = lambda a: a.to(gpu)  # noqa: E731
    xm, valid = ops.mask_gather(dev(x), dev(pos), dev(mrow), dev(mord), B, S, fin=dev(fin), gamma=dev(gamma),
                                beta=dev(beta))
    ok = torch.tensor([0 <= b < B and 0 <= o < M and 0 <= int(pos[b, o]) < S
                       for b, o in zip(mrow.tolist(), mord.tolist())])
    assert torch.equal(valid.cpu().bool(), ok) and ok[:2].all() and not ok[2] and not ok[7:].any()
    assert (xm.cpu()[~ok] == 0).all()
    rows = torch.tensor([b * S + int(pos[b, o]) for b, o, v in zip(mrow.tolist(), mord.tolist(), ok.tolist()) if v])
    ref, tol = E.ln_ref_tol(x, gamma, beta, 1e-12)
    worst = E.worst_ratio(xm.cpu()[ok], ref[rows], tol[rows])
    print(f"H={H} S={S}: fused mask_gather worst error / bound {worst:.3f}")
    assert worst <= 1.0
    # the GPU LayerNorm kernel takes rows of a multiple of 256: at H = 64 the op's CPU path normalises
    normed = ops.layernorm(dev(x), dev(gamma), dev(beta), 1e-12) if H % 256 == 0 else dev(
        ops.layernorm(x, gamma, beta, 1e-12))
    plain, valid2 = ops.mask_gather(normed, dev(pos), dev(mrow), dev(mord), B, S)
    assert torch.equal(valid2.cpu(), valid.cpu()) and torch.equal(plain.cpu()[ok], normed.cpu()[rows])
    assert (plain.cpu()[~ok] == 0).all()
    assert ((xm.cpu()[ok].double() - plain.cpu()[ok].double()).abs() <= 2 * tol[rows]).all()
    twin = ops.mask_gather_ref(x, pos, mrow, mord, B, S, fin, gamma, beta)
    assert torch.equal(twin[1], valid.cpu())
    assert (twin[0][~ok] == 0).all() and E.worst_ratio(twin[0][ok], ref[rows], tol[rows]) <= 1.0
    e = ops.mask_gather(dev(x), dev(pos), dev(mrow[:0]), dev(mord[:0]), B, S)  # R == 0: no launch
    assert e[0].shape == (0, H) and e[1].shape == (0,)


# ------------------------------------------------------------------ engine
def _fill_job_texts():
    extra = [" ".join(w.split()[:4] + ["[MASK]"] + w.split()[4:]) for w in make_text_rows(4, words_per_row=9, seed=5)]
    return ["matrix cores [MASK] tiles", "[MASK]", "gpus have many [MASK] units, naïve café in [MASK]",
            "rain, then [MASK]", "kalo " * 150 + "[MASK]", "it's ([MASK]) here [MASK][MASK]", "no mask at all",
            ""] + extra


TEXTS = _fill_job_texts()


def _twin_fill_rows(eng, texts, bucket):
    """The rows, mask positions and compact slot lists of an engine call by the Python twins, padded to
    ``bucket`` rows without pieces."""
    pieces, segoff, mrow, mord = [], [0], [], []
    for i, t in enumerate(texts):
        ps = T.split_masks(t)[0]
        pieces += ps
        segoff.append(len(pieces))
        mrow += [i] * (len(ps) - 1)
        mord += list(range(len(ps) - 1))
    segoff += [len(pieces)] * (bucket - len(texts))
    rows = [p.encode() for p in pieces]
    if eng.vocab is not None:
        ids_s, lens_s = eng.vocab.tokenize_rows(rows, eng.S)
        sp = (eng.vocab.cls_id, eng.vocab.sep_id, eng.vocab.pad_id, eng.vocab.mask_id)
    else:
        ids_s, lens_s = T.tokenize_rows(rows, eng.S, eng.cfg.vocab_size)
        sp = (T.CLS_ID, T.SEP_ID, T.PAD_ID, T.MASK_ID)
    ids, lens, pos = T.fill_rows(ids_s, lens_s, np.array(segoff, dtype=np.int32), 16, *sp)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    return torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(pos), i32(mrow), i32(mord)


def _oracle_checks(tok_g, logits_g, logits_ref, live):
    """Mask logits within the project's engine bound 0.05 * max|logit|; the top-1 token equals the oracle's
    wherever the oracle's top logit leads its runner-up by more than twice that bound. Returns the share of
    the live masks that qualified."""
    assert live.any()
    bound = 0.05 * logits_ref[live].abs().max().item()
    err = (logits_g[live] - logits_ref[live]).abs().max().item()
    print("mask logits vs oracle", err, "bound", bound)
    assert err < bound
    top2 = logits_ref[live].topk(2, -1)
    clear = (top2.values[:, 0] - top2.values[:, 1]) > 2 * bound
    assert torch.equal(tok_g[live][clear].long(), top2.indices[:, 0][clear])
    return clear.float().mean().item()


TINY_SEED = 9  # the oracle's share of clear masks: 0.417 of 12 (wordpiece) and 0.583 of 12 (hash)


@pytest.fixture(scope="module")
def tiny(wp_vocab):
    cfg = config_for("bert-tiny", mlm_head=True)
    # The seed is one at which, in the fp32 CPU ORACLE alone and for both tokenizers, at least a quarter of
    # the live masks of TEXTS have a top logit that leads the runner-up by more than twice the logit bound
    # 0.05 * max|logit| (computed on the CPU from the oracle's logits, never from what the GPU returns).
    return cfg, init_random(cfg, seed=TINY_SEED, bias_std=0.02), wp_vocab


@pytest.mark.parametrize("tokenizer", ["wordpiece", "hash"])
def test_fill_texts_tiny(gpu, tiny, tokenizer):
    cfg, pack, vocab = tiny
    vocab = vocab if tokenizer == "wordpiece" else None
    kw = dict(batch_rows=16, seq_len=128, topk=1, vocab=vocab)
    eng_g = ClassifyEngine(cfg, pack, gpu, use_graph=True, **kw)
    eng_e = ClassifyEngine(cfg, pack, gpu, use_graph=False, **kw)
    n, k = len(TEXTS), 5
    bucket = eng_g._bucket(n)
    ids, lens, pos, mrow, mord = _twin_fill_rows(eng_g, TEXTS, bucket)
    R = mrow.numel()
    assert lens.max() == 128 and lens[7] == 2 and R == 13
    res = eng_g.fill_texts(TEXTS, k)
    again = eng_g.fill_texts(TEXTS, k)  # replays the captured graph
    eager = eng_e.fill_texts(TEXTS, k)
    assert res.tok.shape == (n, 3, k) and res.prob.shape == (n, 3, k) and res.pos.shape == (n, 3)
    for other in (again, eager):  # graph replay == eager == second call, bit for bit
        assert torch.equal(res.tok, other.tok) and torch.equal(_bits(res.prob), _bits(other.prob))
        assert torch.equal(res.pos, other.pos) and res.fills == other.fills and res.truncated == other.truncated
    # the engine's slots are BertClassifier.fills on the twin's rows, bit for bit
    logits_g = torch.zeros((R, cfg.vocab_size), device=gpu)
    dev = [t.to(gpu) for t in (ids, lens, pos, mrow, mord)]
    direct = [t.cpu() for t in eng_g.model.fills(*dev, k, logits_out=logits_g)]
    assert torch.equal(res.pos, pos[:n, :3])
    for r, (i, j) in enumerate(zip(mrow.tolist(), mord.tolist())):
        assert torch.equal(res.tok[i, j], direct[0][r]) and torch.equal(_bits(res.prob[i, j]), _bits(direct[2][r]))
    assert res.truncated == [(4, 0)] and res.fills[4][0]["candidates"] == [] and res.fills[6] == [] == res.fills[7]
    for text, row in zip(TEXTS, res.fills):
        assert len(row) == text.count("[MASK]")
        for m in row:
            assert text[m["start"]:m["end"]] == "[MASK]"
            sc = [c["score"] for c in m["candidates"]]
            assert sc == sorted(sc, reverse=True) and all(0 < s <= 1 for s in sc) and len(sc) in (0, k)
            for c in m["candidates"]:
                want = None if vocab is None else (vocab.entries[c["token_id"]].decode()
                                                   if c["token_id"] < len(vocab) else None)
                assert c["token"] == want
    # targets: the same logits, the full vocabulary's normaliser, k capped by the target count
    tids = [int(direct[0][0, 0]), 5, int(direct[0][0, 2])]
    tg = eng_g.fill_texts(TEXTS, k, tids=tids)
    assert tg.tok.shape == (n, 3, 3)
    assert sorted(tg.tok[0, 0].tolist()) == sorted(tids)
    assert _bits(tg.prob[0, 0, 0]).item() == _bits(res.prob[0, 0, 0]).item() and tg.tok[0, 0, 0] == tids[0]
    assert torch.equal(tg.tok, eng_e.fill_texts(TEXTS, k, tids=tids).tok)
    # the fp32 CPU oracle
    logits_ref = torch.zeros((R, cfg.vocab_size))
    oracle = BertClassifier(cfg, pack, fp32=True).fills(ids[:n], lens[:n], pos[:n], mrow, mord, k,
                                                        logits_out=logits_ref)
    live = oracle[0][:, 0] >= 0
    assert torch.equal(direct[0][:, 0] >= 0, live)
    share = _oracle_checks(direct[0][:, 0], logits_g.cpu(), logits_ref, live)
    print("share of clear masks", share)
    assert share >= 0.25
    assert eng_g.memory_bytes() > eng_e.pack.nbytes


def test_fill_texts_errors(gpu, tiny, wp_vocab):
    cfg, pack, _ = tiny
    eng = ClassifyEngine(cfg, pack, gpu, batch_rows=16, seq_len=128, topk=1)
    for kw in (dict(top_k=0), dict(top_k=33), dict(mask_token=""), dict(tids=[]), dict(tids=[1, 1]),
               dict(tids=[cfg.vocab_size])):
        with pytest.raises(ValueError):
            eng.fill_texts(["a [MASK]"], **kw)
    with pytest.raises(ValueError) as e:
        eng.fill_texts([" ".join(["[MASK]"] * 17)])
    assert str(e.value) == eng.FILL_TOO_MANY
    plain = config_for("bert-tiny")
    with pytest.raises(ValueError) as e:
        ClassifyEngine(plain, init_random(plain, seed=0), gpu, batch_rows=16, seq_len=128, topk=1).fill_texts(["[MASK]"])
    assert str(e.value) == eng.FILL_NO_HEAD
    assert eng.fill_texts([]).fills == [] and eng.fill_texts(["no mask"]).fills == [[]]


def test_a_long_tailed_text_does_not_depend_on_its_chunk(gpu, tiny, invariant):
    """Texts whose pieces together exceed ``max_row_bytes``: the cut is per text, so the last text of a full
    chunk of them keeps its words before the mask and has the bits it has alone (the chunk's pieces sum to more
    than ``batch_rows * max_row_bytes`` before the cut)."""
    cfg, pack, _ = tiny
    eng = ClassifyEngine(cfg, pack, gpu, batch_rows=16, seq_len=128, topk=1, max_row_bytes=256)
    words = make_text_rows(16, words_per_row=4, seed=9)
    texts = [w + " [MASK] " + "tail " * 80 for w in words]  # about 20 + 400 bytes of pieces per text
    assert sum(len(t) for t in texts) > 16 * 256 + 16 * 100
    many = eng.fill_texts(texts, 5)
    assert many.truncated == [] and (many.pos[:, 0] >= 2).all()  # every mask follows its text's own words
    for r in (0, 14, 15):
        one = eng.fill_texts([texts[r]], 5)
        assert torch.equal(one.pos[0], many.pos[r]) and torch.equal(one.tok[0], many.tok[r]), r
        assert torch.equal(_bits(one.prob[0]), _bits(many.prob[r])), r
    assert len({tuple(t.tolist()) for t in many.tok[:, 0]}) > 1  # the leading words matter


@pytest.fixture(scope="module")
def base():
    cfg = config_for("bert-base", num_labels=1, mlm_head=True)
    return cfg, init_random(cfg, seed=1, bias_std=0.02)


def _base_texts(n_long, n_short, seed):
    out = []
    for i, w in enumerate(make_text_rows(n_long, words_per_row=60, seed=seed)
                          + make_text_rows(n_short, words_per_row=150, seed=seed + 1)):
        ws = w.split()
        at = (7 * i + 3) % 40
        out.append(" ".join(ws[:at] + ["[MASK]"] + ws[at:at + 9] + (["[MASK]"] if i % 3 == 0 else []) + ws[at + 9:]))
    return out


def test_fill_bert_base_folded_path_and_unfused(gpu, base, monkeypatch):
    """16 rows x 128 tokens: M = 2048 reaches the LayerNorm-folded encoder; the fused gather equals the
    ATPU_FILL_FUSED=0 form and the fp32 oracle within the logit bound."""
    cfg, pack = base
    eng = ClassifyEngine(cfg, pack, gpu, batch_rows=32, seq_len=128, topk=1)
    assert eng.model.can_fold(16, 128) and eng.model.fill_fused
    texts = _base_texts(9, 7, 2)
    res = eng.fill_texts(texts, 5)
    ids, lens, pos, mrow, mord = _twin_fill_rows(eng, texts, 16)
    R = mrow.numel()
    assert lens.max() == 128 and lens.min() > 40 and R == 22 and not res.truncated
    dev = [t.to(gpu) for t in (ids, lens, pos, mrow, mord)]
    logits_f = torch.zeros((R, cfg.vocab_size), device=gpu)
    fused = [t.cpu() for t in eng.model.fills(*dev, 5, logits_out=logits_f)]
    for r, (i, j) in enumerate(zip(mrow.tolist(), mord.tolist())):
        assert torch.equal(res.tok[i, j], fused[0][r]) and torch.equal(_bits(res.prob[i, j]), _bits(fused[2][r]))
    monkeypatch.setenv("ATPU_FILL_FUSED", "0")
    plain = BertClassifier(cfg, eng.pack)
    assert not plain.fill_fused
    logits_u = torch.zeros((R, cfg.vocab_size), device=gpu)
    plain.fills(*dev, 5, logits_out=logits_u)
    logits_ref = torch.zeros((R, cfg.vocab_size))
    oracle = BertClassifier(cfg, pack, fp32=True).fills(ids, lens, pos, mrow, mord, 5, logits_out=logits_ref)
    live = oracle[0][:, 0] >= 0
    assert live.all()
    bound = 0.05 * logits_ref.abs().max().item()
    lf, lu = logits_f.cpu(), logits_u.cpu()
    print("fused vs unfused", (lf - lu).abs().max().item(), "bound", bound)
    assert (lf - lu).abs().max().item() < bound
    _oracle_checks(fused[0][:, 0], lf, logits_ref, live)


@pytest.fixture
def invariant():
    prev = ops.set_batch_invariant(True)
    yield
    ops.set_batch_invariant(prev)


def test_fill_rows_are_batch_invariant(gpu, base, invariant):
    """A text's result has the same bits alone, among 40 texts, and across a chunk boundary (``batch_rows``
    32: 40 texts are a chunk of 32 and one of 8, padded to the 16-row bucket)."""
    cfg, pack = base
    eng = ClassifyEngine(cfg, pack, gpu, batch_rows=32, seq_len=128, topk=1)  # its graphs are captured in this mode
    texts = _base_texts(34, 6, 12)
    many = eng.fill_texts(texts, 5)
    assert many.tok.shape == (40, 2, 5) and all(many.fills)
    for r in (0, 29, 31, 32, 39):  # texts of the first chunk and of the second
        one = eng.fill_texts([texts[r]], 5)
        m = one.tok.shape[1]
        assert torch.equal(one.tok[0], many.tok[r, :m]) and torch.equal(_bits(one.prob[0]), _bits(many.prob[r, :m])), r
        assert one.fills[0] == many.fills[r], r
    half = eng.fill_texts(texts[30:], 5)
    assert torch.equal(half.tok, many.tok[30:]) and torch.equal(_bits(half.prob), _bits(many.prob[30:]))
    assert half.fills == many.fills[30:]
