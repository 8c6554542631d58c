"""``atpu-wordpiece v1`` on the CPU: the pure-Python twin against HF ``BertTokenizer`` on the
corpus where the spec promises equality (printable ASCII plus ``\\t\\n\\r``), the host twin
against the Python twin on any bytes, the loader's errors, the model-spec options, and a
``texts`` job of ``map_classify`` on ``bert-tiny?vocab=...`` against the pre-tokenized form."""
import json

import numpy as np
import pytest
import torch

from agent_tpu_amd import tokenizer as T
from agent_tpu_amd.utils.synthetic import WP_MISSING, make_text_rows, make_wordpiece_vocab

PRINTABLE = [chr(c) for c in range(0x20, 0x7F)] + ["\t", "\n", "\r"]


def write_vocab(path, entries, newline="\n"):
    with open(path, "wb") as f:
        f.write(newline.join(entries).encode("utf-8") + newline.encode())
    return str(path)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    path = write_vocab(tmp_path_factory.mktemp("wp") / "vocab.txt", make_wordpiece_vocab(300, seed=1))
    return path, T.WordPieceVocab.load(path)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    path = write_vocab(tmp_path_factory.mktemp("wpbig") / "vocab.txt", make_wordpiece_vocab(30522, seed=2))
    return path, T.WordPieceVocab.load(path)


def ascii_rows(n=1100, seed=5):
    """Fixed edge rows, then seeded rows of 0-400 characters: half uniform over the printable
    set, half words (syllable words, random letters, upper case, some with a missing character)."""
    rng = np.random.default_rng(seed)
    rows = ["", "   ", " \t\r\n ", "a" * 99, "b" * 100, "c" * 101, "x" + "d" * 99, "e" * 99 + "x" + " ok",
            "abx", "kalox", "it's", "Hello, WORLD!! Ka-Lo", "KALOMI RATEN", "don't (stop) [now] {ok} <a@b.c> #1 $2 %3 ^4 &5 *6",
            " ".join("abcdefghij"[k % 10] for k in range(300)), "kalo" * 30, "lo" * 12 + "ka" * 12,
            "q", "z7", "a~b", "quiz"]
    words = make_text_rows(200, words_per_row=40, seed=seed)
    letters = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
    for r in range(n):
        L = int(rng.integers(0, 401))
        if r % 2 == 0:
            rows.append("".join(rng.choice(PRINTABLE, L)))
        else:
            parts = []
            while sum(map(len, parts)) + len(parts) < L:
                k = rng.random()
                if k < 0.5:
                    parts.append(words[int(rng.integers(0, len(words)))].split()[int(rng.integers(0, 20))])
                elif k < 0.9:
                    parts.append("".join(rng.choice(list(letters), int(rng.integers(1, 12)))))
                else:
                    parts.append(str(rng.choice(list(WP_MISSING))) + "ka")
            rows.append(" ".join(parts)[:L])
    return rows


def byte_rows(seed=9):
    rng = np.random.default_rng(seed)
    rows = ["naïve café — 東京 ok".encode(), "東京東 caféé é".encode(), b"a\tb\nc\x01d\x7fe\x00f\x1fg", b"\xff\xfe ka\x80\x80",
            b"\xc3" + b"\xa9" * 150, b"\xe6\x9d\xb1" * 100, b"\xe6\x9d\xb1" * 101, b"k" * 2048, b"k" * 2047 + b" lo",
            b" " * 2040 + b"kalokalo" + b"mi"]
    for _ in range(60):
        rows.append(bytes(rng.integers(0, 256, int(rng.integers(0, 3000)), dtype=np.uint8)))
    return rows


def test_python_twin_equals_hf_bert_tokenizer(small):
    transformers = pytest.importorskip("transformers")
    path, vocab = small
    hf = transformers.BertTokenizer(path, do_lower_case=True)
    rows = ascii_rows()
    assert len(rows) >= 1000
    for S in (8, 128):
        enc = hf(rows, truncation=True, max_length=S, padding="max_length")
        want = np.asarray(enc["input_ids"], dtype=np.int32)
        want_lens = np.asarray(enc["attention_mask"], dtype=np.int32).sum(1)
        ids, lens = vocab.tokenize_rows([r.encode() for r in rows], S, 2048)
        bad = [i for i in range(len(rows)) if not np.array_equal(ids[i], want[i])]
        assert not bad, (S, len(bad), rows[bad[0]], ids[bad[0]].tolist(), want[bad[0]].tolist())
        np.testing.assert_array_equal(lens, want_lens)
    assert (ids == vocab.unk_id).any()  # the corpus does reach [UNK]


def _host(nat, vocab, rows, S, max_row_bytes=2048):
    text, offs = T.pack_rows(rows)
    return nat.wordpiece_host(text, offs, S, vocab.table, max_row_bytes)


def test_host_twin_equals_python_twin(nat, small, big):
    rows = [r.encode() for r in ascii_rows(300)] + byte_rows()
    for vocab in (small[1], big[1]):
        for S in (8, 128):
            ids, lens = vocab.tokenize_rows(rows, S, 2048)
            ids_h, lens_h = _host(nat, vocab, rows, S)
            np.testing.assert_array_equal(ids_h, ids)
            np.testing.assert_array_equal(lens_h, lens)
    # the rows are cut at max_row_bytes first
    ids, lens = small[1].tokenize_rows(rows, 128, 100)
    ids_h, lens_h = _host(nat, small[1], rows, 128, 100)
    np.testing.assert_array_equal(ids_h, ids)
    np.testing.assert_array_equal(lens_h, lens)


def test_table_shape_and_probing_at_real_size(big):
    vocab = big[1]
    hdr = vocab.header
    slots, stored = int(hdr[1]), int(hdr[9])
    assert slots & (slots - 1) == 0 and stored <= slots // 2 and stored >= 30000
    assert vocab.table_bytes == 64 + 16 * slots + int(hdr[3]) < 2 << 20  # well inside one XCD's 4 MiB L2
    assert [int(x) for x in hdr[4:8]] == [vocab.pad_id, vocab.unk_id, vocab.cls_id, vocab.sep_id]
    assert not vocab.table[-32:].any()  # the blob's zero padding


def test_specials_read_from_the_file_and_last_duplicate_wins(small):
    vocab = small[1]
    assert (vocab.pad_id, vocab.unk_id, vocab.cls_id, vocab.sep_id) == (0, 6, 7, 8)
    ka = [i for i, e in enumerate(vocab.entries) if e == b"ka"]
    assert len(ka) == 2
    assert vocab.token_ids(b"ka", 8) == [ka[1]]
    assert vocab.token_ids(b"abx quiz KA", 8) == [vocab.unk_id, vocab.unk_id, ka[1]]


def test_cased_vocabulary(nat, tmp_path):
    path = write_vocab(tmp_path / "vocab.txt", make_wordpiece_vocab(300, seed=1), newline="\r\n")
    cased = T.WordPieceVocab.load(path, lowercase=False)
    uncased = T.WordPieceVocab.load(path)
    assert cased.entries == uncased.entries  # \r\n line ends are stripped
    assert cased.token_ids(b"ABC", 8) == [cased.first[b"A"], cased.cont[b"B"], cased.cont[b"C"]]
    assert cased.token_ids(b"Gab", 8) == [cased.unk_id]
    assert uncased.token_ids(b"ABC", 8) == uncased.token_ids(b"abc", 8) != cased.token_ids(b"ABC", 8)
    rows = [r.encode() for r in ascii_rows(200)] + byte_rows()
    ids, lens = cased.tokenize_rows(rows, 128, 2048)
    ids_h, lens_h = _host(nat, cased, rows, 128)
    np.testing.assert_array_equal(ids_h, ids)
    np.testing.assert_array_equal(lens_h, lens)


def test_loader_errors(nat, tmp_path):
    from agent_tpu_amd.models.bert import config_for

    entries = make_wordpiece_vocab(300, seed=1)
    with pytest.raises(ValueError, match=r"\[UNK\]"):
        T.WordPieceVocab.load(write_vocab(tmp_path / "nounk.txt", [e for e in entries if e != "[UNK]"]))
    empty = tmp_path / "empty.txt"
    empty.write_bytes(b"")
    with pytest.raises(ValueError, match="empty"):
        T.WordPieceVocab.load(str(empty))
    cfg = config_for("bert-tiny", num_labels=2)
    ok = write_vocab(tmp_path / "fits.txt", make_wordpiece_vocab(cfg.vocab_size, seed=3))
    assert len(T.WordPieceVocab.load(ok, vocab_size=cfg.vocab_size)) == cfg.vocab_size
    with pytest.raises(ValueError, match="vocab_size"):
        T.WordPieceVocab.load(write_vocab(tmp_path / "big.txt", make_wordpiece_vocab(cfg.vocab_size + 1, seed=3)),
                              vocab_size=cfg.vocab_size)
    # the native builder refuses the same inputs
    with pytest.raises(ValueError, match=r"\[SEP\]"):
        nat.wordpiece_build_table([e.encode() for e in entries if e != "[SEP]"], True)
    with pytest.raises(ValueError):
        nat.wordpiece_build_table([], True)
    with pytest.raises(ValueError, match="bad table"):
        nat.wordpiece_host(np.zeros(4, np.uint8), np.array([0, 4], np.int32), 8, np.zeros(128, np.uint8), 2048)


def test_parse_spec_vocab_options(tmp_path):
    from ops._gpu_runtime import parse_spec

    spec = parse_spec("bert-tiny?labels=5")
    assert spec.vocab is None and spec.lowercase is True
    spec = parse_spec("bert-tiny?vocab=/abs/vocab.txt&labels=5")
    assert spec.vocab == "/abs/vocab.txt" and spec.lowercase is True and spec.labels == 5
    assert parse_spec("bert-tiny?vocab=/abs/vocab.txt&lowercase=0").lowercase is False
    model = tmp_path / "m.safetensors"
    model.write_bytes(b"")
    meta = tmp_path / "m.safetensors.json"
    meta.write_text(json.dumps({"preset": "bert-tiny", "num_labels": 3}))
    assert parse_spec(str(model)).vocab is None
    meta.write_text(json.dumps({"preset": "bert-tiny", "num_labels": 3, "vocab": "sub/vocab.txt", "lowercase": False}))
    spec = parse_spec(str(model))
    assert spec.vocab == str(tmp_path / "sub" / "vocab.txt") and spec.lowercase is False and spec.labels == 3
    spec = parse_spec(f"{model}?vocab=/other/v.txt&lowercase=1")  # the query wins over the json
    assert spec.vocab == "/other/v.txt" and spec.lowercase is True and spec.file == str(model)


def test_map_classify_texts_with_vocab_equals_input_form(monkeypatch, tmp_path):
    transformers = pytest.importorskip("transformers")
    from ops import _gpu_runtime as rt
    from ops import map_classify as mc

    monkeypatch.setenv("CLASSIFY_DEVICE", "cpu")
    monkeypatch.delenv("CLASSIFY_QUANT", raising=False)
    vf = write_vocab(tmp_path / "vocab.txt", make_wordpiece_vocab(300, seed=1))
    hf = transformers.BertTokenizer(vf, do_lower_case=True)
    texts = ["Kalomi raten, voqua zi!", "it's a quiz", "", "lo ka mi ra ten vo " * 40, "Ber-nox (al) pe dru"]
    path = f"bert-tiny?vocab={vf}&labels=5"
    out = mc.map_classify({"texts": texts, "model_path": path, "topk": 3, "allow_fallback": False})
    assert out["ok"] is True and out["model_path"] == path and out["row_count"] == len(texts)
    eng = rt._cache[(path, "cpu")].engine
    S = eng.S
    assert eng.vocab is not None
    enc = hf(texts, truncation=True, max_length=S, padding="max_length")["input_ids"]

    def close(got, ref, what):
        err = max([abs(a["score"] - b["score"]) for a, b in zip(got, ref)], default=0.0)
        print(f"{what}: max |score - ref| = {err:.3g}")
        assert [t["index"] for t in got] == [t["index"] for t in ref], what
        assert err < 1e-5, (what, err)

    # The CPU engine stores activations in bf16, so its scores depend on the batch shape in the
    # last bf16 digit wherever the BLAS blocks M differently. Each comparison is therefore between
    # runs of the same shape: one text per job against the one-row ``input`` job of its HF ids,
    # and the five-row job against the engine's pre-tokenized path on the five HF rows.
    for i, (text, ids) in enumerate(zip(texts, enc)):
        one = mc.map_classify({"texts": [text], "model_path": path, "topk": 3, "allow_fallback": False})
        ref = mc.map_classify({"input": ids, "model_path": path, "topk": 3, "allow_fallback": False})
        close(one["rows"][0]["topk"], ref["topk"], f"row {i}, one-row jobs")
    hf_ids = torch.tensor(enc, dtype=torch.int32)
    res = eng.classify_ids(hf_ids, (hf_ids != eng.vocab.pad_id).sum(1).to(torch.int32), 3)
    for i, row in enumerate(out["rows"]):
        ref = [{"index": int(j), "score": float(s)} for j, s in zip(res.idx[i], res.score[i])]
        close(row["topk"], ref, f"row {i}, five-row job")
    plain = mc.map_classify({"texts": texts, "model_path": "bert-tiny?labels=5", "topk": 3, "allow_fallback": False})
    assert rt._cache[("bert-tiny?labels=5", "cpu")].engine.vocab is None
    assert [r["topk"] for r in plain["rows"]] != [r["topk"] for r in out["rows"]]
    # a load error follows the existing rule: the stub with the reason, or raised
    bad = f"bert-tiny?vocab={tmp_path / 'missing.txt'}&labels=5"
    stub = mc.map_classify({"texts": texts, "model_path": bad})
    assert stub["fallback"] == "cpu" and stub["topk"] == [] and "missing.txt" in stub["reason"]
    with pytest.raises(FileNotFoundError, match="missing.txt"):
        mc.map_classify({"texts": texts, "model_path": bad, "allow_fallback": False})
