"""atpu-hash-wordpiece v1 — the tokenizer the GPU K1 kernel implements.

There is no subword vocabulary in the reference: ``map_tokenize`` is character
chunking (``/root/reference/ops/map_tokenize.py:6-9``) and ``map_classify_tpu``
consumes pre-tokenized ids (``map_classify_tpu.CONTRACT.md:7-8,23``). With
random-init weights a deterministic hash tokenizer is the contractually
honest choice. Spec:

* bytes 0x09-0x0D and 0x20 separate tokens; other control bytes (<0x20, 0x7F)
  are dropped and also separate;
* each ASCII punctuation byte is a token of its own (BERT BasicTokenizer);
* every other byte (ASCII alnum, UTF-8 >= 0x80) is a word byte, A-Z folded
  to lower case;
* a word is cut into pieces of at most 24 bytes; piece 0 hashes from the
  FNV-1a-32 offset basis, later pieces from the FNV state after "##";
* ``id = 1000 + fnv % (vocab - 1000)``; ``[CLS]=101 … [SEP]=102`` then
  ``[PAD]=0`` up to ``seq_len``; ``len = tokens + 2``.

Three implementations must agree bit-for-bit: :func:`tokenize_rows` (pure
Python, this file), ``_atpu.tokenize_host`` (C++) and the HIP kernel.

atpu-wordpiece v1 — the tokenizer of a model that comes with a ``vocab.txt``
(:class:`WordPieceVocab`; host twin ``_atpu.wordpiece_host``, HIP kernel
``csrc/kernels/tokenize_wp.hip``, again bit-for-bit on any byte string). Spec:

* vocabulary file: one token per line, id = line index, the trailing ``\\n`` /
  ``\\r\\n`` stripped, the last occurrence of a repeated token wins; ``[PAD]``,
  ``[UNK]``, ``[CLS]`` and ``[SEP]`` must be present and their ids are read
  from the file; an entry of more than 4096 bytes cannot match (rows are cut
  at 4096 bytes at most) and is ignored;
* byte classes are those of the hash tokenizer: separators, one-byte
  punctuation words, word bytes (ASCII alnum and every byte >= 0x80); with
  ``lowercase`` (the default, for uncased models) ASCII ``A-Z`` are folded
  before matching;
* each word is matched greedily, longest match first, on bytes: at position
  ``s`` the longest ``e`` such that bytes ``[s, e)`` are an entry (for
  ``s > 0``: those bytes prefixed by ``##``); a position that matches nothing
  makes the whole word one ``[UNK]``, and so does a word of more than 100
  characters (bytes that are not UTF-8 continuation bytes 0x80-0xBF);
* ``[CLS]`` + the first ``seq_len - 2`` tokens + ``[SEP]``, then ``[PAD]``;
  ``len = tokens + 2``; rows are cut at ``max_row_bytes`` first.

Deviations from HF ``BertTokenizer``: no Unicode normalisation (no accent
stripping, no Unicode lower-casing, no CJK splitting, no Unicode whitespace or
punctuation classes -- every byte >= 0x80 is a word byte); control bytes
separate instead of being deleted; a literal special-token string in the text
(``[SEP]``) is punctuation plus a word. On rows of printable ASCII plus
``\\t \\n \\r`` without special-token strings the output equals
``BertTokenizer(vocab_file, do_lower_case=True)`` exactly (tested).

atpu-pair v1 — cross-encoder rows ``[CLS] query [SEP] passage [SEP]`` with their
``token_type_ids``, assembled from the single-segment rows of either tokenizer
(:func:`pair_rows`; HIP kernel ``csrc/kernels/rerank.hip``, bit-for-bit). The spec is
the docstring of :func:`pair_rows`.

atpu-window v1 — overlapping windows over a passage too long for one pair row (``doc_stride``):
the window geometry with the start positions each window owns (:func:`window_table`) and the
window rows (:func:`window_rows`; HIP kernel ``csrc/kernels/window.hip``, bit-for-bit). The spec is
the docstrings of the two.

atpu-fill v1 — rows with ``[MASK]`` tokens for masked-token prediction: the text is split at every
literal mask token (:func:`split_masks`), the pieces are tokenized as ordinary rows and joined with
the mask id between them (:func:`fill_rows`; HIP kernel ``csrc/kernels/fill.hip``, bit-for-bit). The
spec is the docstring of :func:`fill_rows`.

Token byte offsets — the tokenizers return ids only; :func:`token_spans` (hash) and
:meth:`WordPieceVocab.token_spans` give, host side only, the ``(byte_start, byte_end)`` of every id
that ``token_ids`` returns for the same row and cap: a hash piece or a matched WordPiece piece gets
its own bytes, a word that becomes ``[UNK]`` the whole word. ``map_answer`` maps answer token spans
to characters with them.
"""
from __future__ import annotations

import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

CLS_ID, SEP_ID, PAD_ID = 101, 102, 0
FIRST_HASH_ID = 1000
PIECE_BYTES = 24
DEFAULT_MAX_ROW_BYTES = 2048
_BASIS, _PRIME = 2166136261, 16777619


def _byte_class(c: int) -> int:
    if c == 0x20 or 0x09 <= c <= 0x0D or c < 0x20 or c == 0x7F:
        return 0
    if 0x21 <= c <= 0x2F or 0x3A <= c <= 0x40 or 0x5B <= c <= 0x60 or 0x7B <= c <= 0x7E:
        return 1
    return 2


_CLASS = bytes(_byte_class(c) for c in range(256))
_WORDS = re.compile(b"\x01|\x02+")  # on a row translated by _CLASS: one punctuation byte, or a run of word bytes


def _fnv(h: int, data: bytes) -> int:
    for c in data:
        if 0x41 <= c <= 0x5A:
            c += 32
        h = ((h ^ c) * _PRIME) & 0xFFFFFFFF
    return h


_CONT = _fnv(_BASIS, b"##")


def token_ids(row: bytes, vocab: int, cap: int) -> List[int]:
    """Hash-token ids of one row (no specials), at most ``cap`` of them."""
    mod = vocab - FIRST_HASH_ID
    out: List[int] = []
    i, n = 0, len(row)
    while i < n and len(out) < cap:
        k = _CLASS[row[i]]
        if k == 0:
            i += 1
            continue
        if k == 1:
            out.append(FIRST_HASH_ID + _fnv(_BASIS, row[i:i + 1]) % mod)
            i += 1
            continue
        j = i
        while j < n and _CLASS[row[j]] == 2:
            j += 1
        for p, b0 in enumerate(range(i, j, PIECE_BYTES)):
            if len(out) >= cap:
                break
            h = _fnv(_BASIS if p == 0 else _CONT, row[b0:min(j, b0 + PIECE_BYTES)])
            out.append(FIRST_HASH_ID + h % mod)
        i = j
    return out


def token_spans(row: bytes, vocab: int, cap: int) -> List[Tuple[int, int]]:
    """``(byte_start, byte_end)`` in ``row`` of every id :func:`token_ids` returns for the same ``row``
    and ``cap`` (``vocab`` only keeps the signatures alike): a punctuation byte, or a piece of at
    most 24 bytes of a word."""
    out: List[Tuple[int, int]] = []
    for m in _WORDS.finditer(bytes(row).translate(_CLASS)):  # the words, found on the row's byte classes
        i, j = m.span()
        for b0 in range(i, j, PIECE_BYTES):
            if len(out) >= cap:
                return out
            out.append((b0, min(j, b0 + PIECE_BYTES)))
    return out[:cap]


def tokenize_rows(rows: Sequence[bytes], seq_len: int, vocab: int,
                  max_row_bytes: int = DEFAULT_MAX_ROW_BYTES) -> Tuple[np.ndarray, np.ndarray]:
    """Pure-Python reference: returns ``ids[B, seq_len]`` and ``lens[B]`` (int32)."""
    ids = np.zeros((len(rows), seq_len), dtype=np.int32)
    lens = np.zeros(len(rows), dtype=np.int32)
    for r, row in enumerate(rows):
        toks = token_ids(bytes(row[:max_row_bytes]), vocab, seq_len - 2)
        ids[r, 0] = CLS_ID
        ids[r, 1:1 + len(toks)] = toks
        ids[r, 1 + len(toks)] = SEP_ID
        lens[r] = len(toks) + 2
    return ids, lens


def pack_rows(rows: Iterable) -> Tuple[np.ndarray, np.ndarray]:
    """Pack str/bytes rows into (uint8 text, int32 offsets[B+1])."""
    blobs = [r.encode("utf-8") if isinstance(r, str) else bytes(r) for r in rows]
    offsets = np.zeros(len(blobs) + 1, dtype=np.int32)
    if blobs:
        offsets[1:] = np.cumsum([len(b) for b in blobs])
    text = np.frombuffer(b"".join(blobs), dtype=np.uint8).copy() if blobs else np.zeros(0, np.uint8)
    return text, offsets


# ------------------------------------------------------------ atpu-wordpiece v1
MAX_WORD_CHARS = 100
MAX_ENTRY_BYTES = 4096
SPECIAL_TOKENS = (b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]")
_NOT_CONT = bytes(0 if 0x80 <= c <= 0xBF else 1 for c in range(256))


class WordPieceVocab:
    """A BERT ``vocab.txt`` and the three forms it is used in: the dicts of the pure-Python
    twin (:meth:`tokenize_rows`, the oracle of the other two), the packed host table
    (:attr:`table`, built once by ``_atpu.wordpiece_build_table``) and its per-device copy
    (:meth:`device_table`, uploaded once per device)."""

    def __init__(self, entries: Sequence[bytes], lowercase: bool = True, source: str = "<entries>"):
        self.entries = [bytes(e) for e in entries]
        self.lowercase = bool(lowercase)
        self.source = source
        if not self.entries:
            raise ValueError(f"{source}: empty vocabulary")
        self.first: Dict[bytes, int] = {}
        self.cont: Dict[bytes, int] = {}
        index: Dict[bytes, int] = {}
        for i, e in enumerate(self.entries):
            index[e] = i  # the last occurrence wins
            is_cont = len(e) > 2 and e.startswith(b"##")
            piece = e[2:] if is_cont else e
            if piece and len(piece) <= MAX_ENTRY_BYTES:
                (self.cont if is_cont else self.first)[piece] = i
        missing = [s.decode() for s in SPECIAL_TOKENS if s not in index]
        if missing:
            raise ValueError(f"{source}: vocabulary has no {', '.join(missing)}")
        self.pad_id, self.unk_id, self.cls_id, self.sep_id = (index[s] for s in SPECIAL_TOKENS)
        self.mask_id: Optional[int] = index.get(b"[MASK]")  # None: the vocabulary cannot fill masks
        self.index = index
        self.max_len = max([1] + [len(p) for d in (self.first, self.cont) for p in d])
        self._table: Optional[np.ndarray] = None
        self._device: Dict[str, object] = {}

    @classmethod
    def load(cls, path: str, lowercase: bool = True, vocab_size: Optional[int] = None) -> "WordPieceVocab":
        """Read ``path``; ``vocab_size``: the model's embedding rows, which the ids index."""
        with open(path, "rb") as f:
            data = f.read()
        lines = data.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()  # the file ends with a newline
        entries = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]
        if not entries:
            raise ValueError(f"{path}: empty vocabulary file")
        if vocab_size is not None and len(entries) > int(vocab_size):
            raise ValueError(f"{path}: {len(entries)} vocabulary entries exceed the model's vocab_size {vocab_size}")
        return cls(entries, lowercase, source=str(path))

    def __len__(self) -> int:
        return len(self.entries)

    # -------------------------------------------------------------- Python twin
    def _match(self, word: bytes, ends: Optional[List[int]] = None) -> Optional[List[int]]:
        """Greedy longest-match ids of ``word``; ``ends``, when given, receives each piece's end byte."""
        out: List[int] = []
        s, n = 0, len(word)
        while s < n:
            d = self.first if s == 0 else self.cont
            e = min(n, s + self.max_len)
            hit = None
            while e > s:
                hit = d.get(word[s:e])
                if hit is not None:
                    break
                e -= 1
            if hit is None:
                return None
            out.append(hit)
            if ends is not None:
                ends.append(e)
            s = e
        return out

    def word_ids(self, word: bytes) -> List[int]:
        """Ids of one word (word bytes only, or one punctuation byte)."""
        if len(word) > MAX_WORD_CHARS and sum(word.translate(_NOT_CONT)) > MAX_WORD_CHARS:
            return [self.unk_id]
        got = self._match(word.lower() if self.lowercase else word)  # bytes.lower() folds ASCII only
        return [self.unk_id] if got is None else got

    def word_spans(self, word: bytes) -> List[Tuple[int, int]]:
        """``(start, end)`` within ``word`` of every id :meth:`word_ids` returns: a matched piece gets its
        own bytes, a word that becomes ``[UNK]`` the whole word."""
        if len(word) > MAX_WORD_CHARS and sum(word.translate(_NOT_CONT)) > MAX_WORD_CHARS:
            return [(0, len(word))]
        ends: List[int] = []
        if self._match(word.lower() if self.lowercase else word, ends) is None:  # lower() keeps byte positions
            return [(0, len(word))]
        return list(zip([0] + ends[:-1], ends))

    def token_spans(self, row: bytes, cap: int) -> List[Tuple[int, int]]:
        """``(byte_start, byte_end)`` in ``row`` of every id :meth:`token_ids` returns for the same ``row``
        and ``cap``."""
        out: List[Tuple[int, int]] = []
        row = bytes(row)
        for m in _WORDS.finditer(row.translate(_CLASS)):
            if len(out) >= cap:
                break
            i, j = m.span()
            out.extend((i + a, i + b) for a, b in self.word_spans(row[i:j]))
        return out[:cap]

    def token_ids(self, row: bytes, cap: int) -> List[int]:
        """Token ids of one row (no specials), at most ``cap`` of them."""
        out: List[int] = []
        i, n = 0, len(row)
        while i < n and len(out) < cap:
            k = _CLASS[row[i]]
            if k == 0:
                i += 1
                continue
            j = i + 1
            if k == 2:
                while j < n and _CLASS[row[j]] == 2:
                    j += 1
            out.extend(self.word_ids(row[i:j]))
            i = j
        return out[:cap]

    def tokenize_rows(self, rows: Sequence[bytes], seq_len: int,
                      max_row_bytes: int = DEFAULT_MAX_ROW_BYTES) -> Tuple[np.ndarray, np.ndarray]:
        """Pure-Python reference: returns ``ids[B, seq_len]`` and ``lens[B]`` (int32)."""
        ids = np.full((len(rows), seq_len), self.pad_id, dtype=np.int32)
        lens = np.zeros(len(rows), dtype=np.int32)
        for r, row in enumerate(rows):
            toks = self.token_ids(bytes(row[:max_row_bytes]), seq_len - 2)
            ids[r, 0] = self.cls_id
            ids[r, 1:1 + len(toks)] = toks
            ids[r, 1 + len(toks)] = self.sep_id
            lens[r] = len(toks) + 2
        return ids, lens

    # ------------------------------------------------------- packed table forms
    @property
    def table(self) -> np.ndarray:
        """The packed table (uint8) that the host twin and the kernel read."""
        if self._table is None:
            from ._native import native

            self._table = native().wordpiece_build_table(self.entries, self.lowercase)
        return self._table

    @property
    def header(self) -> np.ndarray:
        return self.table[:64].view(np.int32)

    @property
    def table_bytes(self) -> int:
        return int(self.table.size)

    def device_table(self, device):
        """The table on ``device``: uploaded on first use, then cached (stable pointer)."""
        import torch

        key = str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            t = torch.from_numpy(self.table).to(device)
            self._device[key] = t
        return t


# ------------------------------------------------------------------ atpu-pair v1
def default_max_query_tokens(seq_len: int) -> int:
    """The query budget of a pair row when the caller names none: ``min(32, (S - 3) // 2)``."""
    return min(32, (int(seq_len) - 3) // 2)


def pair_rows(ids_q: np.ndarray, lens_q: np.ndarray, ids_p: np.ndarray, lens_p: np.ndarray, qidx: np.ndarray,
              max_query_tokens: int, cls_id: int = CLS_ID, sep_id: int = SEP_ID,
              pad_id: int = PAD_ID) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """atpu-pair v1: cross-encoder rows ``[CLS] query [SEP] passage [SEP]`` assembled from the
    single-segment rows either tokenizer emits (``[CLS] t... [SEP] [PAD]...``, ``len = n + 2``);
    pure-Python twin of ``csrc/kernels/rerank.hip`` ``pair_assemble_kernel``, bit-for-bit.

    For passage row ``r`` with ``q = clamp(qidx[r], 0, Q - 1)``, ``S`` the row width (>= 4):

    * ``nq = min(clamp(lens_q[q], 2, S) - 2, max_query_tokens, S - 3)``;
    * ``np = min(clamp(lens_p[r], 2, S) - 2, S - 3 - nq)``;
    * ``ids = [CLS] q_tok[0:nq] [SEP] p_tok[0:np] [SEP]`` then ``[PAD]``;
    * ``type_ids`` 0 on the first ``nq + 2`` positions, 1 on the next ``np + 1``, 0 on padding;
    * ``len = nq + np + 3``.

    Where ``max_query_tokens`` does not cut the query this is HF ``BertTokenizer(q, p,
    truncation="only_second", max_length=S, padding="max_length")`` (``input_ids``,
    ``token_type_ids``, attention length), under the caveats of atpu-wordpiece v1.
    Returns ``(ids[P, S], type_ids[P, S], lens[P])``, all int32."""
    ids_q, ids_p = np.asarray(ids_q, dtype=np.int32), np.asarray(ids_p, dtype=np.int32)
    lens_q, lens_p = np.asarray(lens_q, dtype=np.int32), np.asarray(lens_p, dtype=np.int32)
    qidx = np.asarray(qidx, dtype=np.int32)
    if ids_q.ndim != 2 or ids_p.ndim != 2 or ids_q.shape[1] != ids_p.shape[1]:
        raise ValueError("pair_rows: ids_q [Q, S] and ids_p [P, S]")
    Q, S = ids_q.shape
    P = ids_p.shape[0]
    mq = int(max_query_tokens)
    if S < 4 or Q < 1 or mq < 0:
        raise ValueError("pair_rows: S >= 4, Q >= 1 and max_query_tokens >= 0")
    if lens_q.shape != (Q,) or lens_p.shape != (P,) or qidx.shape != (P,):
        raise ValueError("pair_rows: lens_q [Q], lens_p [P] and qidx [P]")
    ids = np.full((P, S), pad_id, dtype=np.int32)
    types = np.zeros((P, S), dtype=np.int32)
    lens = np.zeros(P, dtype=np.int32)
    for r in range(P):
        q = min(max(int(qidx[r]), 0), Q - 1)
        nq = min(min(max(int(lens_q[q]), 2), S) - 2, mq, S - 3)
        n_p = min(min(max(int(lens_p[r]), 2), S) - 2, S - 3 - nq)
        ids[r, 0] = cls_id
        ids[r, 1:1 + nq] = ids_q[q, 1:1 + nq]
        ids[r, 1 + nq] = sep_id
        ids[r, 2 + nq:2 + nq + n_p] = ids_p[r, 1:1 + n_p]
        ids[r, 2 + nq + n_p] = sep_id
        types[r, 2 + nq:3 + nq + n_p] = 1
        lens[r] = nq + n_p + 3
    return ids, types, lens


def premise_rows(ids_t: np.ndarray, lens_t: np.ndarray, ids_h: np.ndarray, lens_h: np.ndarray, tidx: np.ndarray,
                 hidx: np.ndarray, max_hypothesis_tokens: int, cls_id: int = CLS_ID, sep_id: int = SEP_ID,
                 pad_id: int = PAD_ID) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """atpu-premise v1: NLI rows ``[CLS] text [SEP] hypothesis [SEP]`` assembled from the single-segment
    rows either tokenizer emits; pure-Python twin of ``csrc/kernels/zeroshot.hip``
    ``premise_assemble_kernel``, bit-for-bit. The opposite of :func:`pair_rows`: the long first segment
    gives way, the short second one is kept, and neither is one row per pair.

    For row ``r`` with ``t = clamp(tidx[r], 0, T - 1)``, ``h = clamp(hidx[r], 0, Hn - 1)``, ``S`` the row
    width (>= 4):

    * ``nh = min(clamp(lens_h[h], 2, S) - 2, max_hypothesis_tokens, S - 3)``;
    * ``nt = min(clamp(lens_t[t], 2, S) - 2, S - 3 - nh)``;
    * ``ids = [CLS] t_tok[0:nt] [SEP] h_tok[0:nh] [SEP]`` then ``[PAD]``;
    * ``type_ids`` 1 on positions ``nt + 2 .. nt + nh + 2``, 0 elsewhere;
    * ``len = nt + nh + 3``.

    Where ``max_hypothesis_tokens`` does not cut the hypothesis this is HF ``BertTokenizer(text,
    hypothesis, truncation="only_first", max_length=S, padding="max_length")``, under the caveats of
    atpu-wordpiece v1. Returns ``(ids[P, S], type_ids[P, S], lens[P])``, all int32."""
    ids_t, ids_h = np.asarray(ids_t, dtype=np.int32), np.asarray(ids_h, dtype=np.int32)
    lens_t, lens_h = np.asarray(lens_t, dtype=np.int32), np.asarray(lens_h, dtype=np.int32)
    tidx, hidx = np.asarray(tidx, dtype=np.int32), np.asarray(hidx, dtype=np.int32)
    if ids_t.ndim != 2 or ids_h.ndim != 2 or ids_t.shape[1] != ids_h.shape[1]:
        raise ValueError("premise_rows: ids_t [T, S] and ids_h [Hn, S]")
    Tn, S = ids_t.shape
    Hn = ids_h.shape[0]
    mh = int(max_hypothesis_tokens)
    if S < 4 or Tn < 1 or Hn < 1 or mh < 0:
        raise ValueError("premise_rows: S >= 4, T >= 1, Hn >= 1 and max_hypothesis_tokens >= 0")
    if lens_t.shape != (Tn,) or lens_h.shape != (Hn,) or tidx.ndim != 1 or hidx.shape != tidx.shape:
        raise ValueError("premise_rows: lens_t [T], lens_h [Hn], tidx [P] and hidx [P]")
    P = tidx.shape[0]
    ids = np.full((P, S), pad_id, dtype=np.int32)
    types = np.zeros((P, S), dtype=np.int32)
    lens = np.zeros(P, dtype=np.int32)
    for r in range(P):
        t = min(max(int(tidx[r]), 0), Tn - 1)
        h = min(max(int(hidx[r]), 0), Hn - 1)
        nh = min(min(max(int(lens_h[h]), 2), S) - 2, mh, S - 3)
        nt = min(min(max(int(lens_t[t]), 2), S) - 2, S - 3 - nh)
        ids[r, 0] = cls_id
        ids[r, 1:1 + nt] = ids_t[t, 1:1 + nt]
        ids[r, 1 + nt] = sep_id
        ids[r, 2 + nt:2 + nt + nh] = ids_h[h, 1:1 + nh]
        ids[r, 2 + nt + nh] = sep_id
        types[r, 2 + nt:3 + nt + nh] = 1
        lens[r] = nt + nh + 3
    return ids, types, lens


# ---------------------------------------------------------------- atpu-window v1
def window_table(T: int, nq: int, S: int, doc_stride: int) -> List[Tuple[int, int, int, int]]:
    """atpu-window v1: the windows ``(start, len, own_lo, own_hi)`` of a passage of ``T`` tokens read
    behind a question of ``nq`` tokens (already cut: ``nq <= S - 3``) in rows of width ``S``. All
    quantities are passage tokens without specials.

    * ``cap = S - 3 - nq``; ``cap < 1``: one window with an empty passage, ``(0, 0, 0, 0)``;
    * ``step = min(doc_stride, cap)``, ``h = (cap - step) // 2``;
    * ``W = 1`` if ``T <= cap`` else ``ceil((T - cap) / step) + 1`` windows, window ``w`` starting at
      ``a_w = w * step`` with ``len_w = min(cap, T - a_w)`` tokens (0 only when ``T == 0``);
    * window ``w`` owns the window-relative start positions ``[own_lo, own_hi)``: ``own_lo = 0`` for
      ``w == 0`` else ``h``; ``own_hi = len_w`` for ``w == W - 1`` else ``step + h``.

    The owned ranges ``[a_w + own_lo, a_w + own_hi)`` partition ``[0, T)`` and each lies inside its
    window, so a span is a candidate of the one window that owns its start, if it ends inside that
    window: every span of at most ``ceil((cap - step) / 2) + 1`` tokens does (tested by brute force)."""
    T, nq, S, doc_stride = int(T), int(nq), int(S), int(doc_stride)
    if S < 4 or not 0 <= nq <= S - 3 or T < 0 or doc_stride < 1:
        raise ValueError("window_table: S >= 4, 0 <= nq <= S - 3, T >= 0 and doc_stride >= 1")
    cap = S - 3 - nq
    if cap < 1:
        return [(0, 0, 0, 0)]
    step = min(doc_stride, cap)
    h = (cap - step) // 2
    W = 1 if T <= cap else -(-(T - cap) // step) + 1
    out = []
    for w in range(W):
        a = w * step
        n = min(cap, T - a)
        out.append((a, n, 0 if w == 0 else h, n if w == W - 1 else step + h))
    return out


def window_rows(ids_q: np.ndarray, lens_q: np.ndarray, ids_p: np.ndarray, lens_p: np.ndarray, qidx: np.ndarray,
                win_pair: np.ndarray, win_start: np.ndarray, max_query_tokens: int, doc_stride: int,
                cls_id: int = CLS_ID, sep_id: int = SEP_ID, pad_id: int = PAD_ID
                ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """atpu-window v1: the window rows of long passages; pure-Python twin of ``csrc/kernels/window.hip``
    ``window_assemble_kernel``, bit-for-bit. ``ids_q [Q, S]`` / ``lens_q [Q]`` are question rows,
    ``ids_p [Pp, L]`` / ``lens_p [Pp]`` the long passage rows (tokenizer output at width ``L``) with their
    question ``qidx [Pp]``; window row ``r`` reads pair ``p = clamp(win_pair[r], 0, Pp - 1)`` from passage
    token ``a = clamp(win_start[r], 0, max(T - 1, 0))``:

    * ``nq`` as in :func:`pair_rows`, ``cap = S - 3 - nq``, ``T = clamp(lens_p[p], 2, L) - 2``,
      ``nw = min(cap, T - a)``;
    * ``ids = [CLS] q_tok[0:nq] [SEP] p_tok[a:a + nw] [SEP]`` then ``[PAD]``; ``type_ids`` and ``len`` as
      in :func:`pair_rows`;
    * ``own = (0 if a == 0 else h, nw if a + cap >= T else step + h)`` with ``step = min(doc_stride,
      cap)``, ``h = (cap - step) // 2``: on the starts of :func:`window_table` its ``(own_lo, own_hi)``.

    With ``T <= cap`` (one window at 0) ids, type_ids and lens are those of :func:`pair_rows`.
    Returns ``(ids [R, S], type_ids [R, S], lens [R], own [R, 2])``, all int32."""
    ids_q, ids_p = np.asarray(ids_q, dtype=np.int32), np.asarray(ids_p, dtype=np.int32)
    lens_q, lens_p = np.asarray(lens_q, dtype=np.int32), np.asarray(lens_p, dtype=np.int32)
    qidx = np.asarray(qidx, dtype=np.int32)
    win_pair, win_start = np.asarray(win_pair, dtype=np.int32), np.asarray(win_start, dtype=np.int32)
    if ids_q.ndim != 2 or ids_p.ndim != 2:
        raise ValueError("window_rows: ids_q [Q, S] and ids_p [Pp, L]")
    (Q, S), (Pp, L) = ids_q.shape, ids_p.shape
    mq, stride = int(max_query_tokens), int(doc_stride)
    if S < 4 or L < 2 or Q < 1 or Pp < 1 or mq < 0 or stride < 1:
        raise ValueError("window_rows: S >= 4, L >= 2, Q >= 1, Pp >= 1, max_query_tokens >= 0 and doc_stride >= 1")
    if lens_q.shape != (Q,) or lens_p.shape != (Pp,) or qidx.shape != (Pp,):
        raise ValueError("window_rows: lens_q [Q], lens_p [Pp] and qidx [Pp]")
    if win_pair.ndim != 1 or win_start.shape != win_pair.shape:
        raise ValueError("window_rows: win_pair [R] and win_start [R]")
    R = win_pair.shape[0]
    ids = np.full((R, S), pad_id, dtype=np.int32)
    types = np.zeros((R, S), dtype=np.int32)
    lens = np.zeros(R, dtype=np.int32)
    own = np.zeros((R, 2), dtype=np.int32)
    for r in range(R):
        p = min(max(int(win_pair[r]), 0), Pp - 1)
        q = min(max(int(qidx[p]), 0), Q - 1)
        nq = min(min(max(int(lens_q[q]), 2), S) - 2, mq, S - 3)
        cap = S - 3 - nq
        T = min(max(int(lens_p[p]), 2), L) - 2
        a = min(max(int(win_start[r]), 0), max(T - 1, 0))
        step = min(stride, cap)
        h = (cap - step) // 2
        nw = min(cap, T - a)
        ids[r, 0] = cls_id
        ids[r, 1:1 + nq] = ids_q[q, 1:1 + nq]
        ids[r, 1 + nq] = sep_id
        ids[r, 2 + nq:2 + nq + nw] = ids_p[p, 1 + a:1 + a + nw]
        ids[r, 2 + nq + nw] = sep_id
        types[r, 2 + nq:3 + nq + nw] = 1
        lens[r] = nq + nw + 3
        own[r] = (0 if a == 0 else h, nw if a + cap >= T else step + h)
    return ids, types, lens, own


MASK_ID = 103  # [MASK] of the hash tokenizer (the id bert-base-uncased gives it)
MAX_MASKS = 16


def split_masks(text: str, mask_token: str = "[MASK]") -> Tuple[List[str], List[Tuple[int, int]]]:
    """The pieces of ``text`` between the literal, case-sensitive occurrences of ``mask_token`` (``m + 1``
    pieces for ``m`` masks, empty ones included) and the ``(start, end)`` character offsets of the masks."""
    if not mask_token:
        raise ValueError("mask_token must be a non-empty string")
    pieces, spans, at = [], [], 0
    while True:
        i = text.find(mask_token, at)
        if i < 0:
            pieces.append(text[at:])
            return pieces, spans
        pieces.append(text[at:i])
        spans.append((i, i + len(mask_token)))
        at = i + len(mask_token)


def fill_rows(ids_s: np.ndarray, lens_s: np.ndarray, segoff: np.ndarray, max_masks: int, cls_id: int = CLS_ID,
              sep_id: int = SEP_ID, pad_id: int = PAD_ID, mask_id: int = MASK_ID
              ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """atpu-fill v1: rows with mask tokens; pure-Python twin of ``csrc/kernels/fill.hip``
    ``fill_assemble_kernel``, bit-for-bit. Both tokenizers turn a literal ``[MASK]`` into punctuation plus
    a word, so (as HF does) the host splits each text at every literal mask token (:func:`split_masks`)
    and the pieces are tokenized as ordinary single-segment rows ``ids_s [Ns, S]`` / ``lens_s [Ns]``; the
    pieces of row ``b`` are ``segoff[b] .. segoff[b + 1] - 1``. With ``a = clamp(segoff[b], 0, Ns)``,
    ``nseg = clamp(clamp(segoff[b + 1], 0, Ns) - a, 0, M + 1)``, piece ``i`` the row ``min(a + i, Ns - 1)`` and
    ``n_i = clamp(lens_s, 2, S) - 2`` its tokens without ``[CLS]`` / ``[SEP]``:

    * the concatenation ``c = seg_0 [MASK] seg_1 [MASK] ... seg_{nseg-1}`` has ``T`` tokens, of which the
      first ``kept = min(T, S - 2)`` stay;
    * ``ids = [CLS] c[0:kept] [SEP]`` then ``[PAD]``; ``len = kept + 2``; every ``type_id`` is 0;
    * ``pos[b, j]`` = the row position of mask ``j`` (``1 +`` its index in ``c``), or ``-1`` where the row has
      fewer masks or the mask fell at or beyond position ``S - 1``.

    ``S >= 3``, ``M = max_masks`` in ``[1, 16]``. Returns ``(ids [B, S], lens [B], pos [B, M])``, all int32."""
    ids_s = np.asarray(ids_s, dtype=np.int32)
    lens_s, segoff = np.asarray(lens_s, dtype=np.int32), np.asarray(segoff, dtype=np.int32)
    M = int(max_masks)
    if ids_s.ndim != 2 or lens_s.shape != (ids_s.shape[0],):
        raise ValueError("fill_rows: ids_s [Ns, S] and lens_s [Ns]")
    Ns, S = ids_s.shape
    if S < 3 or not 1 <= M <= MAX_MASKS or segoff.ndim != 1 or segoff.shape[0] < 1:
        raise ValueError("fill_rows: S >= 3, max_masks in [1, 16] and segoff [B + 1]")
    B = segoff.shape[0] - 1
    if B > 0 and Ns < 1:
        raise ValueError("fill_rows: Ns >= 1")
    ids = np.full((B, S), pad_id, dtype=np.int32)
    lens = np.zeros(B, dtype=np.int32)
    pos = np.full((B, M), -1, dtype=np.int32)
    for b in range(B):
        a = min(max(int(segoff[b]), 0), Ns)
        nseg = min(max(min(max(int(segoff[b + 1]), 0), Ns) - a, 0), M + 1)
        c: List[int] = []
        for i in range(nseg):
            s = min(a + i, Ns - 1)
            n = min(max(int(lens_s[s]), 2), S) - 2
            c.extend(int(t) for t in ids_s[s, 1:1 + n])
            if i + 1 < nseg:
                if len(c) < S - 2:
                    pos[b, i] = len(c) + 1
                c.append(mask_id)
        kept = min(len(c), S - 2)
        ids[b, 0] = cls_id
        ids[b, 1:1 + kept] = c[:kept]
        ids[b, 1 + kept] = sep_id
        lens[b] = kept + 2
    return ids, lens, pos
