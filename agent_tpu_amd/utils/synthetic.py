"""Synthetic CSV shards for benchmarks and tests (no datasets are downloadable).

Rows look like ``id,text,risk`` (the column set of the reference's csv_shard
probes). ``text`` is a sentence of random words from a
fixed synthetic vocabulary, with punctuation and some quoting, long enough by
default to fill a 128-token BERT window.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

_SYLL = ["ka", "lo", "mi", "ra", "ten", "vo", "qua", "zi", "ber", "nox", "al", "pe", "dru", "sim", "ox", "ul"]
_PUNCT = [",", ".", ";", "!", "?", "-", "(", ")"]


def _vocab(rng: np.random.Generator, size: int = 4096):
    words = set()
    while len(words) < size:
        n = int(rng.integers(1, 5))
        words.add("".join(rng.choice(_SYLL, n)))
    return sorted(words)


def make_text_rows(n: int, words_per_row: int = 150, seed: int = 0):
    rng = np.random.default_rng(seed)
    vocab = np.array(_vocab(rng), dtype=object)
    out = []
    for _ in range(n):
        w = vocab[rng.integers(0, len(vocab), words_per_row)]
        toks = []
        for j, word in enumerate(w):
            toks.append(word.capitalize() if j == 0 else word)
            if rng.random() < 0.06:
                toks.append(_PUNCT[int(rng.integers(0, len(_PUNCT)))])
        out.append(" ".join(toks))
    return out


# characters a generated vocabulary has no single-character entry for (they occur only inside the
# syllables "qua" and "zi"): a word that needs one of them on its own becomes [UNK]
WP_MISSING = "qz7~"


def make_wordpiece_vocab(n: int = 300, seed: int = 0):
    """A deterministic ``n``-entry (>= 300) uncased WordPiece vocabulary, as the lines of a
    ``vocab.txt``: the specials at ids that are NOT BERT's 0/100/101/102 (``[unusedN]`` fillers
    in between), single characters and ``##`` characters (none of :data:`WP_MISSING`; no
    ``##x``, so a word ending in an unmatched ``x`` is ``[UNK]``), a few upper-case and
    non-ASCII entries, the syllables :func:`make_text_rows` builds its words from, one long
    entry, one entry listed twice (the last id wins), then random lower-case pieces."""
    rng = np.random.default_rng(seed)
    out = ["[PAD]"] + [f"[unused{i}]" for i in range(5)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    chars = [chr(c) for c in range(0x21, 0x7F) if not ("A" <= chr(c) <= "Z") and chr(c) not in WP_MISSING]
    out += chars
    out += ["##" + c for c in chars if c.isalnum() and c != "x"]
    out += list("ABCDEF") + ["##" + c for c in "ABCDEF"]
    out += ["é", "##é", "東", "##京", "caf", "naï", "##ve"]
    out += _SYLL + ["##" + s for s in _SYLL]
    out += ["lo" * 12, "##" + "ka" * 11, "ka"]  # "ka" again: this id wins over the syllable's
    seen = set(out)
    letters = [c for c in "abcdefghijklmnopqrstuvwxyz0123456789" if c not in WP_MISSING]
    assert n >= len(out), f"make_wordpiece_vocab: n must be at least {len(out)}"
    while len(out) < n:
        k = int(rng.integers(1, 4)) if rng.random() < 0.5 else 0
        piece = "".join(rng.choice(_SYLL, k)) if k else "".join(rng.choice(letters, int(rng.integers(2, 10))))
        if rng.random() < 0.4:
            piece = "##" + piece
        if piece not in seen:
            seen.add(piece)
            out.append(piece)
    return out


def write_csv(path: str, n: int, words_per_row: int = 150, seed: int = 0, quote_every: int = 7,
              unique_rows: Optional[int] = None) -> str:
    """Write ``n`` rows; every ``quote_every``-th text is quoted with an embedded comma/quote/newline.

    With ``unique_rows`` < ``n`` only that many texts are generated and the file repeats them
    in order (a long file at a bounded generation cost); the first ``unique_rows`` rows are
    the same either way."""
    import csv

    u = n if unique_rows is None else max(1, min(n, int(unique_rows)))
    rows = make_text_rows(u, words_per_row, seed)
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f, lineterminator="\n")  # excel dialect, QUOTE_MINIMAL
        w.writerow(["id", "text", "risk"])
        for i in range(n):
            t = rows[i % u]
            if quote_every and i % quote_every == 3:
                t = t + ', said "x"\nend'
            w.writerow([i, t, (i % 1000) / 1000.0])
    os.replace(tmp, path)
    return path


def ensure_csv(path: str, n: int, words_per_row: int = 150, seed: int = 0) -> str:
    if not os.path.exists(path):
        write_csv(path, n, words_per_row, seed)
    return path
