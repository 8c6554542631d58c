"""``atpu-wordpiece v1`` on the GPU: the HIP kernel against the Python and host twins, bit for
bit, and ClassifyEngine with a vocabulary (graph path == eager path == pre-tokenized ids)."""
import numpy as np
import pytest
import torch

from agent_tpu_amd import ops
from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.utils.synthetic import make_text_rows, make_wordpiece_vocab

pytestmark = pytest.mark.gpu

MAX_ROW = 2048
OFFSETS = (0, 1, 3, 23, 40, 61, 62, 63)
LENGTHS = list(range(1, 72)) + list(range(95, 131))


@pytest.fixture(scope="module")
def vocabs():
    return {n: T.WordPieceVocab([e.encode() for e in make_wordpiece_vocab(n, seed=1)]) for n in (300, 30522)}


@pytest.fixture(scope="module")
def rows():
    out = make_text_rows(300, words_per_row=40, seed=3)
    out += ["", "   ", "Hello, WORLD!!", "x" * 100, "naïve café — 東京 ok", "a\tb\nc\x01d", "(" * 300, "abx quiz it's"]
    # words of every length 1..71 and 95..130 at the offsets mod 64 that matter (the 128-bit ballot
    # window, the 64+ byte walk, the 100-character rule): the hash test's upper-case words (most
    # hold a missing letter: [UNK]) and words of syllables, which are matched piece by piece
    syl = "kalomiratenvoquaziberno" * 8
    for L in LENGTHS:
        for off in OFFSETS:
            out.append(" " * off + "".join(chr(65 + (k * 7 + L) % 26) for k in range(L)) + ",ab " + "Q" * (L % 30))
            out.append(" " * off + syl[L % 7:L % 7 + L] + ",ab " + "lo" * (L % 30))
    # the longest entries (24 and 22 bytes) straddling a 64-byte step, and a word of single letters
    for off in range(38, 66):
        out.append("." * off + "lo" * 12 + " a" + "ka" * 11 + " " * (off % 5) + "abcdefghijklmnop")
    out = [r.encode() for r in out]
    rng = np.random.default_rng(7)
    for _ in range(40):
        out.append(bytes(rng.integers(0, 256, int(rng.integers(0, 3000)), dtype=np.uint8)))
    # the last word ends exactly at max_row_bytes; a word cut there; a row of one long word
    out += [b" " * (MAX_ROW - 8) + b"kalokalo", b" " * (MAX_ROW - 6) + b"kalokalomi", b"k" * 3000,
            b"\xe6\x9d\xb1" * 100, b"\xe6\x9d\xb1" * 101, b"\xc3" + b"\xa9" * 150]
    if len(out) % 4 == 0:
        out.append(b"lo ka")
    return out


@pytest.mark.parametrize("n_vocab", [300, 30522])
@pytest.mark.parametrize("S", [8, 128])
def test_kernel_matches_python_and_host(gpu, nat, vocabs, rows, n_vocab, S):
    vocab = vocabs[n_vocab]
    assert len(rows) % 4 != 0  # the last workgroup is partial
    text, offs = T.pack_rows(rows)
    ids_py, lens_py = vocab.tokenize_rows(rows, S, MAX_ROW)
    ids_h, lens_h = nat.wordpiece_host(text, offs, S, vocab.table, MAX_ROW)
    ids_g, lens_g = ops.tokenize_wordpiece(torch.from_numpy(text).to(gpu), torch.from_numpy(offs).to(gpu), S, vocab,
                                           MAX_ROW)
    np.testing.assert_array_equal(ids_h, ids_py)
    np.testing.assert_array_equal(lens_h, lens_py)
    np.testing.assert_array_equal(ids_g.cpu().numpy(), ids_py)
    np.testing.assert_array_equal(lens_g.cpu().numpy(), lens_py)
    assert (ids_py == vocab.unk_id).any() and (lens_py == S).any() and (lens_py == 2).any()


def _engines(gpu, vocab):
    from agent_tpu_amd.models.bert import config_for, init_random
    from agent_tpu_amd.runtime.classify import ClassifyEngine

    cfg = config_for("bert-tiny", num_labels=5)
    pack = init_random(cfg, seed=4)
    return [ClassifyEngine(cfg, pack, gpu, batch_rows=64, seq_len=128, topk=5, use_graph=g, vocab=vocab)
            for g in (True, False)]


def test_engine_with_vocabulary_graph_eager_and_ids_agree(gpu, vocabs):
    vocab = vocabs[300]
    texts = make_text_rows(36, words_per_row=30, seed=8) + ["", "abx quiz", "Hello, WORLD!!", "lo" * 12 + " kalomi " * 60]
    eng_g, eng_e = _engines(gpu, vocab)
    assert eng_g.use_graph and not eng_e.use_graph and eng_g.vocab is vocab
    a, b = eng_g.classify_texts(texts), eng_e.classify_texts(texts)
    assert a.idx.shape == (40, 5)
    assert torch.equal(a.idx, b.idx) and torch.equal(a.score, b.score)
    ids, lens = vocab.tokenize_rows([t.encode() for t in texts], 128, eng_g.max_row_bytes)
    np.testing.assert_array_equal(eng_g.ids_s[0][:40].cpu().numpy(), ids)
    np.testing.assert_array_equal(eng_g.lens_s[0][:40].cpu().numpy(), lens)
    for eng in (eng_g, eng_e):
        c = eng.classify_ids(torch.from_numpy(ids), torch.from_numpy(lens))
        assert torch.equal(c.idx, a.idx) and torch.equal(c.score, a.score)
    plain = _engines(gpu, None)[0]
    assert eng_g.memory_bytes() - plain.memory_bytes() == vocab.table_bytes


def test_engine_without_vocabulary_keeps_the_hash_tokenizer(gpu):
    texts = make_text_rows(36, words_per_row=30, seed=8) + ["", "abx quiz", "Hello, WORLD!!", "naïve café"]
    for eng in _engines(gpu, None):
        assert eng.vocab is None
        eng.classify_texts(texts)
        ids, lens = T.tokenize_rows([t.encode() for t in texts], 128, eng.cfg.vocab_size, eng.max_row_bytes)
        np.testing.assert_array_equal(eng.ids_s[0][:40].cpu().numpy(), ids)
        np.testing.assert_array_equal(eng.lens_s[0][:40].cpu().numpy(), lens)
