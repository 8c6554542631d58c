"""ClassifyEngine: rows of text -> top-k classes on one MI355X.

The device-side replacement for the reference's single-tensor
``set_tensor / invoke / get_tensor`` (``/root/reference/ops/map_classify_tpu.py:71-74``),
batched and pipelined:

  host (C++ HostStager thread)        copy stream              compute stream
  CSV rows -> pinned slot s   ──►  hipMemcpyAsync(slot s) ──►  tokenize (K1)
                                                                BERT encoder (K2-K6)
                                                                pooler + head/top-k (K7)
                                                                D2H top-k (pinned)

Two staging slots alternate, so extraction of batch i+1 (host threads), its
H2D copy (side stream) and the encoder of batch i (compute stream) overlap.
The whole device step for a full batch (tokenize -> top-k) is captured once per
slot into a hipGraph (``torch.cuda.CUDAGraph``) and replayed: one launch per
batch instead of ~100.
"""
from __future__ import annotations

import os
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from .._native import native
from ..models.bert import BertClassifier, BertConfig
from ..models.params import ParamPack
from ..tokenizer import (CLS_ID, DEFAULT_MAX_ROW_BYTES, MASK_ID, MAX_MASKS, PAD_ID, SEP_ID, WordPieceVocab,
                         default_max_query_tokens, pack_rows, split_masks, token_spans, window_table)
from ..utils.trace import DeviceStages, span
from .graphs import capture_graph


def i32(*shape, **kw) -> torch.Tensor:
    return torch.zeros(shape, dtype=torch.int32, **kw)


@dataclass
class BatchResult:
    rows: int
    idx: torch.Tensor    # [rows, k] int32 (host)
    score: torch.Tensor  # [rows, k] fp32 (host)


@dataclass
class EmbedResult:
    rows: int
    emb: torch.Tensor    # [rows, H] fp32 (host)


@dataclass
class RerankResult:
    queries: int
    pairs: int
    idx: torch.Tensor     # [queries, k] int32 (host): index within the query's passages, -1 past its end
    score: torch.Tensor   # [queries, k] fp32 (host): the ranked scores (after ``activation``)
    scores: torch.Tensor  # [pairs] fp32 (host): every pair's raw score, in input order


@dataclass
class AnswerResult:
    questions: int
    pairs: int
    # per question, best first: {"passage": index within the question's passages, "start" / "end": character
    # offsets into that passage, "text", "score": the span's logit sum, "null_score": its pair's no-answer
    # score, "tokens": the passage-relative token span}
    answers: List[List[Dict[str, object]]]
    span: torch.Tensor   # [pairs, n, 2] int32 (host): every pair's n best token spans, (-1, -1) past the last
    score: torch.Tensor  # [pairs, n] fp32 (host)
    null: torch.Tensor   # [pairs] fp32 (host)
    window_count: Optional[int] = None  # with doc_stride: the window rows this call read


@dataclass
class TagResult:
    rows: int
    # per row, in token order. Grouped modes: {"entity_group", "score", "word", "start", "end"}; mode "none":
    # {"entity", "score", "index", "word", "start", "end"} with index = the token's position in the row,
    # [CLS] being 0. start / end are character offsets into the row's text; score = ent_sum / n in fp64
    entities: List[List[Dict[str, object]]]
    counts: List[int]        # per row: the true number of groups
    truncated: List[int]     # the rows whose count exceeded max_entities
    ent: torch.Tensor        # [rows, E, 4] int32 (host): (first, last, type, n), (-1, -1, -1, 0) past the last
    ent_sum: torch.Tensor    # [rows, E] fp32 (host)


@dataclass
class FillResult:
    rows: int
    # per row, one record per mask in text order: {"start", "end": character offsets of the literal mask
    # token in the row's text, "candidates": [{"token_id", "token": the vocabulary string (None for the hash
    # tokenizer), "score": the probability}], best first}; a truncated mask has no candidates
    fills: List[List[Dict[str, object]]]
    truncated: List[Tuple[int, int]]  # the (row, mask) pairs that fell beyond the row
    tok: torch.Tensor    # [rows, M, k] int32 (host): -1 past a row's masks, for a truncated mask, past the targets
    prob: torch.Tensor   # [rows, M, k] fp32 (host)
    pos: torch.Tensor    # [rows, M] int32 (host): the row position of every mask, -1 as tok


@dataclass
class ZeroShotResult:
    texts: int
    pairs: int
    goff: List[int]       # text t owns positions goff[t] .. goff[t + 1] - 1 of the rows below
    order: torch.Tensor   # [pairs] int32 (host): position goff[t] + r = the index, within the text's labels, of its r-th
    score: torch.Tensor   # [pairs] fp32 (host): ... and that label's score
    logits: torch.Tensor  # [pairs, 2] fp32 (host): every pair's (entailment, contradiction) logits, in input order

    def ranked(self, t: int) -> Tuple[List[int], List[float]]:
        """``(label indices, scores)`` of text ``t``, best first."""
        a, b = self.goff[t], self.goff[t + 1]
        return self.order[a:b].tolist(), self.score[a:b].tolist()


def _offsets(counts: Sequence[int]) -> List[int]:
    off = [0]
    for c in counts:
        off.append(off[-1] + int(c))
    return off


@dataclass
class RunStats:
    rows: int = 0
    batches: int = 0
    wall_s: float = 0.0
    timing_ms: Dict[str, float] = field(default_factory=dict)

    @property
    def rows_per_sec(self) -> float:
        return self.rows / self.wall_s if self.wall_s > 0 else 0.0


class ClassifyEngine:
    def __init__(self, cfg: BertConfig, pack: ParamPack, device: torch.device, batch_rows: int = 512,
                 seq_len: int = 128, topk: int = 5, max_row_bytes: int = DEFAULT_MAX_ROW_BYTES,
                 use_graph: bool = True, slots: int = 2, concurrent: Optional[bool] = None,
                 quant: Optional[str] = None, vocab: Optional[WordPieceVocab] = None):
        if pack.buffer.device != device:
            pack = pack.to(device)
        self.cfg, self.pack, self.device = cfg, pack, device
        # a model with a vocabulary: K1 is the WordPiece kernel on its table; None: the hash tokenizer
        self.vocab = vocab
        if vocab is not None:
            if len(vocab) > cfg.vocab_size:
                raise ValueError(f"{vocab.source}: {len(vocab)} vocabulary entries exceed the model's "
                                 f"vocab_size {cfg.vocab_size}")
            if device.type == "cuda":
                vocab.device_table(device)  # uploaded now: the launches inside a graph capture allocate nothing
        self.model = BertClassifier(cfg, pack, quant=quant)  # quant None: the CLASSIFY_QUANT default
        self.B, self.S = int(batch_rows), int(seq_len)
        self.k = max(1, min(int(topk), cfg.num_labels))
        self.max_row_bytes = int(max_row_bytes)
        self.use_graph = use_graph and device.type == "cuda"
        self.n_slots = slots
        cap = self.B * self.max_row_bytes
        self.text = [torch.empty(cap, dtype=torch.uint8, device=device) for _ in range(slots)]
        self.offs = [torch.zeros(self.B + 1, dtype=torch.int32, device=device) for _ in range(slots)]
        # per-slot token buffers: with concurrent slots two batches are in flight at once
        self.ids_s = [torch.zeros((self.B, self.S), dtype=torch.int32, device=device) for _ in range(slots)]
        self.lens_s = [torch.zeros(self.B, dtype=torch.int32, device=device) for _ in range(slots)]
        self.ids, self.lens = self.ids_s[0], self.lens_s[0]
        self.copy_stream = torch.cuda.Stream(device) if device.type == "cuda" else None
        # Concurrent slots: batch i runs on compute stream i % slots, so the
        # encoders of two consecutive batches overlap on the GPU. A GEMM block
        # fills a CU (128 KiB LDS, full register file), so overlap happens at CU
        # granularity: the memory-bound kernels (attention, LayerNorm, GEMM store
        # tails) of one batch run on some CUs while the other batch's GEMM main
        # loops run on the rest, instead of every CU alternating between regimes.
        if concurrent is None:
            concurrent = os.getenv("ATPU_CONCURRENT_SLOTS", "1") not in ("0", "false", "no")
        self.concurrent = bool(concurrent) and device.type == "cuda" and slots > 1
        self.compute_streams = [torch.cuda.Stream(device) for _ in range(slots)] if self.concurrent else None
        # CU split (ATPU_CU_SPLIT=1): slot i's stream is CU-masked to an even 1/slots share of every
        # XCD, and persistent grids are sized for that share (process-wide cu_budget). Without it a
        # persistent GEMM holds every CU (146 KiB LDS per workgroup) and the other batch's kernels
        # only slot in at kernel boundaries.
        self.cu_split = self.concurrent and os.getenv("ATPU_CU_SPLIT", "0") not in ("0", "false", "no")
        if self.cu_split:
            nat = native()
            nat.cu_budget(0)
            share = (nat.num_cus() // slots) // 8 * 8
            self.compute_streams = [torch.cuda.ExternalStream(nat.make_cu_mask_stream(i * share, share), device=device)
                                    for i in range(slots)]
            nat.cu_budget(share)
        if device.type == "cuda" and self.model.can_fold(self.B, self.S):
            self.model.folded()  # build the LN-folded weights now, so memory_bytes() counts them
        if self.model.quant:
            self.model.quantized()  # likewise the int8 weights (and not inside a graph capture)
        self._graphs: Dict[int, Tuple["torch.cuda.CUDAGraph", Tuple[torch.Tensor, ...]]] = {}
        # stage-timed replay: the same step as three graphs (tokenize | encoder | head) with
        # hipEvents between them, so timing_ms carries device time per stage
        self._staged: Dict[int, Tuple[Tuple["torch.cuda.CUDAGraph", ...], Tuple[torch.Tensor, ...]]] = {}
        self._stager = None
        # embed graphs, keyed by (pooling, normalize): built on first use (an engine that never
        # embeds allocates nothing for them), from the graph pools of the classify graphs
        self._egraphs: Dict[Tuple[int, str, bool], Tuple["torch.cuda.CUDAGraph", torch.Tensor]] = {}
        self._epools: Dict[int, Tuple[int, int]] = {}
        # bucket graphs of the small-job forms (:meth:`_replay`), keyed by kind, bucket and whatever else
        # the step was captured with; they replay in order on one stream, so one pool, made on first
        # use, serves them all
        self._bgraphs: Dict[tuple, Tuple["torch.cuda.CUDAGraph", object]] = {}
        self._bpool: Optional[Tuple[int, int]] = None

    # ------------------------------------------------------------ device step
    def _tokenize(self, text: torch.Tensor, offs: torch.Tensor, ids: Optional[torch.Tensor] = None,
                  lens: Optional[torch.Tensor] = None, rows: Optional[int] = None, seq_len: Optional[int] = None):
        """K1 of this engine: the model's WordPiece vocabulary when it has one, else the hash tokenizer.
        ``seq_len``: the row width (default: the engine's ``S``)."""
        S = self.S if seq_len is None else seq_len
        if self.vocab is not None:
            return ops.tokenize_wordpiece(text, offs, S, self.vocab, self.max_row_bytes,
                                          ids=ids, lens=lens, rows=rows)
        return ops.tokenize(text, offs, S, self.cfg.vocab_size, self.max_row_bytes,
                            ids=ids, lens=lens, rows=rows)

    def _step(self, slot: int, rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        ids, lens = self.ids_s[slot], self.lens_s[slot]
        self._tokenize(self.text[slot], self.offs[slot], ids=ids, lens=lens, rows=rows)
        return self.model.forward(ids[:rows], lens[:rows], self.k)

    def _warm(self, fn) -> None:
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):  # warm up allocator + code objects off-graph
            fn()
        torch.cuda.current_stream(self.device).wait_stream(s)

    def _graph_step(self, slot: int):
        if slot not in self._graphs:
            if not self._graphs:  # once per engine: the other slots' steps take the same kernels
                self._warm(lambda: self._step(slot, self.B))
            g, outs = capture_graph(lambda: self._step(slot, self.B))
            self._graphs[slot] = (g, outs)
        g, outs = self._graphs[slot]
        g.replay()
        return outs

    def _stage_fns(self, slot: int, rows: int):
        ids, lens = self.ids_s[slot], self.lens_s[slot]
        box = {}

        def tok():
            self._tokenize(self.text[slot], self.offs[slot], ids=ids, lens=lens, rows=rows)

        def enc():
            box["h"] = self.model.encoder(ids[:rows], lens[:rows])

        def head():
            box["out"] = self.model.head(box["h"], rows, self.S, self.k)
            return box["out"]

        return tok, enc, head

    def _staged_graphs(self, slot: int):
        if slot not in self._staged:
            tok, enc, head = self._stage_fns(slot, self.B)
            self._warm(lambda: (tok(), enc(), head()))
            pool = torch.cuda.graph_pool_handle()
            gs = []
            outs = None
            for fn in (tok, enc, head):
                g, r = capture_graph(fn, pool=pool)
                gs.append(g)
                outs = r if r is not None else outs
            self._staged[slot] = (tuple(gs), outs)
        return self._staged[slot]

    def run_slot(self, slot: int, rows: int, stages: Optional[DeviceStages] = None, stream=None):
        if rows < self.B and ops.batch_invariant():
            # batch invariance: a partial batch (a shard's tail) runs the full-batch step like every
            # other batch -- an M-sized eager step could take other kernels (the folded encoder needs
            # M >= 2048 and whole 256-row tiles) -- its extra rows empty strings, their results unused
            offs = self.offs[slot]
            offs[rows + 1:].copy_(offs[rows:rows + 1].expand(self.B - rows))
            rows = self.B
        if stages is None:
            if self.use_graph and rows == self.B:
                return self._graph_step(slot)
            return self._step(slot, rows)
        ev = DeviceStages.event
        if self.use_graph and rows == self.B:
            gs, outs = self._staged_graphs(slot)
            fns = [g.replay for g in gs]
        else:
            fns, outs = list(self._stage_fns(slot, rows)), None
        marks = [ev(stream)]
        res = None
        for fn in fns:
            r = fn()
            res = r if r is not None else res
            marks.append(ev(stream))
        for name, a, b in zip(("tokenize", "encoder", "head"), marks, marks[1:]):
            stages.add(name, a, b)
        return outs if outs is not None else res

    # -------------------------------------------------------------- host APIs
    # ------------------------------------------------- small jobs (texts / input)
    # The per-job forms (the reference's one-row ``input`` job, short ``texts`` lists)
    # replay a captured graph too: rows are padded up to a power-of-two bucket (8 .. B),
    # so a job costs one H2D from pinned staging, one graph launch and one D2H instead
    # of ~100 eager launches (padding rows are empty and their results dropped).
    def _bucket(self, n: int) -> int:
        # batch invariance: at least 16 rows (2048 tokens), so every bucket takes the LayerNorm-
        # folded encoder (ops.fold_ok: M >= 2048, whole 256-row tiles) that the big batches take
        b = 16 if ops.batch_invariant() else 8
        while b < n:
            b *= 2
        return min(b, self.B)

    def _pinned(self):
        if getattr(self, "_pin", None) is None:
            self._pin = {
                "ids": torch.zeros((self.B, self.S), dtype=torch.int32, pin_memory=True),
                "lens": torch.ones(self.B, dtype=torch.int32, pin_memory=True),
                "text": torch.zeros(self.B * self.max_row_bytes, dtype=torch.uint8, pin_memory=True),
                "offs": torch.zeros(self.B + 1, dtype=torch.int32, pin_memory=True),
            }
        return self._pin

    def _replay(self, key: tuple, fn, prepare=None):
        """``fn()`` of a small-job step on ``bucket`` rows staged in slot 0. A graph engine captures it once
        per ``key`` and replays it, returning the capture's static outputs; on a miss ``prepare()`` (inputs
        built lazily, which must not be built inside a capture) and a warm-up run come first."""
        if not self.use_graph:
            return fn()
        if key not in self._bgraphs:
            if self._bpool is None:
                self._bpool = torch.cuda.graph_pool_handle()
            if prepare is not None:
                prepare()
            self._warm(fn)
            self._bgraphs[key] = capture_graph(fn, pool=self._bpool)
        g, outs = self._bgraphs[key]
        g.replay()
        return outs

    def _stage_texts(self, chunk: Tuple[np.ndarray, np.ndarray], n: int, rows: Optional[int] = None) -> int:
        """The packed ``(text, offs)`` of ``n`` rows, through the pinned rows into slot 0, padded with empty
        strings up to the bucket of ``n`` (of ``rows >= n`` when given: a step that runs more rows than it
        has texts), which is returned. The copies are asynchronous: the caller does not overwrite the pinned
        rows (the next call) before something it waits for is ordered after them."""
        text, offs = chunk
        pin = self._pinned()
        bk = self._bucket(n if rows is None else rows)
        pin["text"][:text.size].copy_(torch.from_numpy(text))
        pin["offs"][:n + 1].copy_(torch.from_numpy(offs))
        pin["offs"][n + 1:bk + 1].fill_(int(offs[-1]))  # padding rows: empty strings
        if text.size:
            self.text[0][:text.size].copy_(pin["text"][:text.size], non_blocking=True)
        self.offs[0][:bk + 1].copy_(pin["offs"][:bk + 1], non_blocking=True)
        return bk

    def _result_rows(self, name: str, rows: int, floor: int, *specs) -> Tuple[torch.Tensor, ...]:
        """The first ``rows`` rows of the engine's result buffers ``self.<name>``, one ``[cap, *shape]`` tensor
        per ``(shape, dtype)`` of ``specs``: allocated at ``max(rows, floor)`` rows on first use, again when
        ``rows`` outgrows them or the row shape changes. Views, valid until the next call."""
        bufs = getattr(self, name, None)
        if bufs is None or bufs[0].shape[0] < rows or tuple(bufs[0].shape[1:]) != specs[0][0]:
            cap = max(rows, floor)
            bufs = tuple(torch.empty((cap,) + shape, dtype=dtype, device=self.device) for shape, dtype in specs)
            setattr(self, name, bufs)
        return tuple(t[:rows] for t in bufs)

    def _run_bucket(self, kind: str, m: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        bk = self._bucket(m)

        def fn():
            if kind == "text":
                self._tokenize(self.text[0], self.offs[0], ids=self.ids_s[0], lens=self.lens_s[0], rows=bk)
            return self.model.forward(self.ids_s[0][:bk], self.lens_s[0][:bk], self.k)

        _, idx, sc = self._replay((kind, bk), fn)
        both = torch.cat([idx[:m, :k].view(torch.float32), sc[:m, :k]], 1).cpu()  # one D2H, one sync
        return both[:, :k].contiguous().view(torch.int32), both[:, k:].contiguous()

    def classify_ids(self, ids: torch.Tensor, lens: torch.Tensor, k: Optional[int] = None) -> BatchResult:
        """Pre-tokenized rows ``ids [n, S]`` / ``lens [n]`` (host tensors) -> top-k on the host."""
        k = self.k if k is None else max(1, min(int(k), self.k))
        n = int(ids.shape[0])
        if self.device.type != "cuda":
            _, idx, sc = self.model.forward(ids.to(torch.int32), lens.to(torch.int32), k)
            return BatchResult(n, idx[:, :k].cpu(), sc[:, :k].cpu())
        pin = self._pinned()
        idx_all, sc_all = [], []
        for c0 in range(0, n, self.B):
            m = min(self.B, n - c0)
            bk = self._bucket(m)
            pin["ids"][:m].copy_(ids[c0:c0 + m])
            pin["ids"][m:bk].zero_()
            pin["lens"][:m].copy_(lens[c0:c0 + m])
            pin["lens"][m:bk].fill_(1)
            self.ids_s[0][:bk].copy_(pin["ids"][:bk], non_blocking=True)
            self.lens_s[0][:bk].copy_(pin["lens"][:bk], non_blocking=True)
            i, s_ = self._run_bucket("ids", m, k)  # its D2H synchronizes: the pinned rows are free again
            idx_all.append(i)
            sc_all.append(s_)
        if not idx_all:
            return BatchResult(0, torch.zeros((0, k), dtype=torch.int32), torch.zeros((0, k)))
        return BatchResult(n, torch.cat(idx_all), torch.cat(sc_all))

    def classify_texts(self, rows: Sequence, k: Optional[int] = None) -> BatchResult:
        """Classify an in-memory list of strings (small jobs; no CSV)."""
        k = self.k if k is None else max(1, min(int(k), self.cfg.num_labels))
        idx_all, sc_all = [], []
        for b0 in range(0, len(rows), self.B):
            chunk = rows[b0:b0 + self.B]
            text, offs = pack_rows(r[:self.max_row_bytes] if isinstance(r, (bytes, bytearray)) else
                                   r.encode("utf-8")[:self.max_row_bytes] for r in chunk)
            n = len(chunk)
            if self.device.type == "cuda":
                self._stage_texts((text, offs), n)
                i, s_ = self._run_bucket("text", n, min(k, self.k))  # its D2H synchronizes: pinned rows free again
                idx_all.append(i)
                sc_all.append(s_)
            else:
                ids, lens = self._tokenize(torch.from_numpy(text), torch.from_numpy(offs))
                logits, idx, sc = self.model.forward(ids, lens, k)
                idx_all.append(idx.cpu())
                sc_all.append(sc.cpu())
        if not idx_all:
            return BatchResult(0, torch.zeros((0, k), dtype=torch.int32), torch.zeros((0, k)))
        return BatchResult(len(rows), torch.cat(idx_all), torch.cat(sc_all))

    def _get_stager(self):
        if self._stager is None:
            self._stager = native().HostStager(self.n_slots, self.B * self.max_row_bytes, self.B)
        return self._stager

    def classify_table(self, table, start: int, n: int, col: int, host_threads: Optional[int] = None,
                       out_idx: Optional[torch.Tensor] = None, out_score: Optional[torch.Tensor] = None,
                       stage_timing: bool = False) -> Tuple[torch.Tensor, torch.Tensor, RunStats]:
        """Pipelined classification of CSV rows ``[start, start+n)``.

        Returns device tensors ``idx[n,k]`` / ``score[n,k]`` (left on the GPU
        so a DP caller can all-gather them without a host round trip).
        ``stats.timing_ms``: ``host_*_ms`` host-side spans (stager waits, launch
        enqueue, the final drain); with ``stage_timing`` also ``device_*_ms``, GPU
        time per stage from hipEvent pairs (h2d: the copies on the copy stream,
        timed by the native stager after its wait for the slot's consumer;
        tokenize / encoder / head replayed as three graphs; the top-k copy-out),
        and ``device_span_ms`` (see :class:`DeviceStages`).
        """
        assert self.device.type == "cuda", "classify_table needs a ROCm device"
        if host_threads is None:
            from ..parallel.placement import host_threads as budget

            host_threads = budget(8)  # this rank's NUMA share (placement.py), at most the tuned 8
        n = max(0, min(int(n), table.num_rows - int(start)))
        dev = self.device
        out_idx = torch.empty((n, self.k), dtype=torch.int32, device=dev) if out_idx is None else out_idx
        out_score = torch.empty((n, self.k), dtype=torch.float32, device=dev) if out_score is None else out_score
        stats = RunStats()
        if n == 0:
            return out_idx, out_score, stats
        st = self._get_stager()
        caller = torch.cuda.current_stream(dev)
        streams = self.compute_streams or [caller] * self.n_slots
        for s in streams:
            if s is not caller:
                s.wait_stream(caller)  # out_* and earlier work were enqueued on the caller's stream
        cs = int(self.copy_stream.cuda_stream)
        nb = (n + self.B - 1) // self.B
        t0 = time.perf_counter()
        tm = stats.timing_ms  # host_* spans (+ roctx ranges under MI355X_TRACE=1); device_* from hipEvents
        dst = DeviceStages() if stage_timing else None
        ev = DeviceStages.event
        if dst and self.use_graph:
            # capture the stage graphs of every slot this run replays before the first event: a lazy
            # capture inside the loop is host time that device_span_ms would count as a pipeline gap
            graphed = nb if ops.batch_invariant() else n // self.B  # batches that run the full-batch step
            for slot in range(min(self.n_slots, graphed)):
                with torch.cuda.stream(streams[slot]):
                    self._staged_graphs(slot)
        with span("host_csv_stage_ms", tm):
            st.submit(0, table, start, min(self.B, n), col, self.max_row_bytes, host_threads)
        def stage_next(i: int) -> None:
            if i + 1 < nb:
                b1 = start + (i + 1) * self.B
                with span("host_csv_stage_ms", tm):
                    st.submit((i + 1) % self.n_slots, table, b1, min(self.B, start + n - b1), col,
                              self.max_row_bytes, host_threads)

        for i in range(nb):
            slot = i % self.n_slots
            if self.n_slots > 1:  # batch i+1 stages into the other slot while batch i runs
                stage_next(i)
            stream = streams[slot]
            ks = int(stream.cuda_stream)
            with torch.cuda.stream(stream):
                with span("host_stager_wait_ms", tm):
                    rows, _ = st.upload(slot, self.text[slot].data_ptr(), self.text[slot].numel(),
                                        self.offs[slot].data_ptr(), cs, ks)
                with span("host_launch_ms", tm):
                    _, idx, sc = self.run_slot(slot, int(rows), dst, stream)
                st.release(slot, ks)
                if self.n_slots == 1:  # one slot: the next batch stages once this one released it
                    stage_next(i)
                r0 = i * self.B
                c0 = ev(stream) if dst else None
                out_idx[r0:r0 + rows].copy_(idx[:rows], non_blocking=True)
                out_score[r0:r0 + rows].copy_(sc[:rows], non_blocking=True)
                if dst:
                    dst.add("copy_out", c0, ev(stream))
            stats.batches += 1
        for s in streams:
            if s is not caller:
                caller.wait_stream(s)
        with span("host_drain_ms", tm):
            torch.cuda.synchronize(dev)
        h2d_ms, _ = st.take_h2d_ms()  # hipEvent pairs around the copies (native stager)
        if dst:
            dst.resolve(tm)
            tm["device_h2d_ms"] = round(h2d_ms, 3)
        stats.rows = n
        stats.wall_s = time.perf_counter() - t0
        return out_idx, out_score, stats

    # ------------------------------------------------------------------ embed
    # Sentence embeddings [rows, H] instead of top-k, on the machinery of the classify forms:
    # the stager, the two slots and their streams, one graph per slot for full batches, the
    # power-of-two bucket graphs for small jobs, the full-batch step for a partial batch under
    # batch invariance. The classify paths and their graphs are not touched.
    @staticmethod
    def _embed_key(pooling: str, normalize: bool) -> Tuple[str, bool]:
        if pooling not in ("mean", "cls"):
            raise ValueError("pooling must be 'mean' or 'cls'")
        return str(pooling), bool(normalize)

    def _embed_step(self, slot: int, rows: int, key: Tuple[str, bool]) -> torch.Tensor:
        ids, lens = self.ids_s[slot], self.lens_s[slot]
        self._tokenize(self.text[slot], self.offs[slot], ids=ids, lens=lens, rows=rows)
        return self.model.embed(ids[:rows], lens[:rows], key[0], key[1])

    def _embed_graph_step(self, slot: int, key: Tuple[str, bool]) -> torch.Tensor:
        gk = (slot,) + key
        if gk not in self._egraphs:
            if not any(k[1:] == key for k in self._egraphs):  # the other slots' steps take the same kernels
                self._warm(lambda: self._embed_step(slot, self.B, key))
            # the slot's graphs replay in order on the slot's stream: one pool serves them all
            if slot in self._graphs:
                pool = self._graphs[slot][0].pool()
            else:
                pool = self._epools.setdefault(slot, torch.cuda.graph_pool_handle())
            self._egraphs[gk] = capture_graph(lambda: self._embed_step(slot, self.B, key), pool=pool)
        g, out = self._egraphs[gk]
        g.replay()
        return out

    def _embed_slot(self, slot: int, rows: int, key: Tuple[str, bool]) -> torch.Tensor:
        if rows < self.B and ops.batch_invariant():  # as run_slot: a partial batch runs the full-batch step
            offs = self.offs[slot]
            offs[rows + 1:].copy_(offs[rows:rows + 1].expand(self.B - rows))
            rows = self.B
        if self.use_graph and rows == self.B:
            return self._embed_graph_step(slot, key)
        return self._embed_step(slot, rows, key)

    def _embed_bucket(self, bucket: int, key: Tuple[str, bool]) -> torch.Tensor:
        def fn():
            self._tokenize(self.text[0], self.offs[0], ids=self.ids_s[0], lens=self.lens_s[0], rows=bucket)
            return self.model.embed(self.ids_s[0][:bucket], self.lens_s[0][:bucket], key[0], key[1])

        return self._replay(("embed", bucket) + key, fn)

    def embed_texts(self, rows: Sequence, pooling: str = "mean", normalize: bool = True) -> EmbedResult:
        """Embed an in-memory list of strings (small jobs; no CSV) -> host fp32 ``[n, H]``."""
        key = self._embed_key(pooling, normalize)
        out = []
        for b0 in range(0, len(rows), self.B):
            chunk = rows[b0:b0 + self.B]
            text, offs = pack_rows(r[:self.max_row_bytes] if isinstance(r, (bytes, bytearray)) else
                                   r.encode("utf-8")[:self.max_row_bytes] for r in chunk)
            n = len(chunk)
            if self.device.type == "cuda":
                bk = self._stage_texts((text, offs), n)
                out.append(self._embed_bucket(bk, key)[:n].cpu())  # the D2H synchronizes: pinned rows free again
            else:
                ids, lens = self._tokenize(torch.from_numpy(text), torch.from_numpy(offs))
                out.append(self.model.embed(ids, lens, key[0], key[1]).float().cpu())
        if not out:
            return EmbedResult(0, torch.zeros((0, self.cfg.hidden), dtype=torch.float32))
        return EmbedResult(len(rows), torch.cat(out))

    def embed_table(self, table, start: int, n: int, col: int, pooling: str = "mean", normalize: bool = True,
                    out: Optional[torch.Tensor] = None, stage_timing: bool = False,
                    host_threads: Optional[int] = None) -> Tuple[torch.Tensor, RunStats]:
        """Pipelined embedding of CSV rows ``[start, start+n)`` -> device fp32 ``emb[n, H]`` (left on
        the GPU for a DP all-gather) and the run's stats; the pipeline of :meth:`classify_table`.
        With ``stage_timing``, ``stats.timing_ms`` carries ``device_embed_ms`` (tokenize, encoder and
        pooling, one graph), ``device_copy_out_ms`` and ``device_h2d_ms`` from hipEvent pairs."""
        assert self.device.type == "cuda", "embed_table needs a ROCm device"
        key = self._embed_key(pooling, normalize)
        if host_threads is None:
            from ..parallel.placement import host_threads as budget

            host_threads = budget(8)
        n = max(0, min(int(n), table.num_rows - int(start)))
        dev = self.device
        out = torch.empty((n, self.cfg.hidden), dtype=torch.float32, device=dev) if out is None else out
        stats = RunStats()
        if n == 0:
            return out, stats
        st = self._get_stager()
        caller = torch.cuda.current_stream(dev)
        streams = self.compute_streams or [caller] * self.n_slots
        for s in streams:
            if s is not caller:
                s.wait_stream(caller)  # out and earlier work were enqueued on the caller's stream
        cs = int(self.copy_stream.cuda_stream)
        nb = (n + self.B - 1) // self.B
        t0 = time.perf_counter()
        tm = stats.timing_ms
        dst = DeviceStages() if stage_timing else None
        ev = DeviceStages.event

        def stage(i: int) -> None:
            if i < nb:
                b1 = start + i * self.B
                with span("host_csv_stage_ms", tm):
                    st.submit(i % self.n_slots, table, b1, min(self.B, start + n - b1), col, self.max_row_bytes,
                              host_threads)

        stage(0)
        for i in range(nb):
            slot = i % self.n_slots
            if self.n_slots > 1:  # batch i+1 stages into the other slot while batch i runs
                stage(i + 1)
            stream = streams[slot]
            ks = int(stream.cuda_stream)
            with torch.cuda.stream(stream):
                with span("host_stager_wait_ms", tm):
                    rows, _ = st.upload(slot, self.text[slot].data_ptr(), self.text[slot].numel(),
                                        self.offs[slot].data_ptr(), cs, ks)
                e0 = ev(stream) if dst else None
                with span("host_launch_ms", tm):
                    emb = self._embed_slot(slot, int(rows), key)
                st.release(slot, ks)
                if self.n_slots == 1:  # one slot: the next batch stages once this one released it
                    stage(i + 1)
                c0 = ev(stream) if dst else None
                out[i * self.B:i * self.B + rows].copy_(emb[:rows], non_blocking=True)
                if dst:
                    dst.add("embed", e0, c0)
                    dst.add("copy_out", c0, ev(stream))
            stats.batches += 1
        for s in streams:
            if s is not caller:
                caller.wait_stream(s)
        with span("host_drain_ms", tm):
            torch.cuda.synchronize(dev)
        h2d_ms, _ = st.take_h2d_ms()
        if dst:
            dst.resolve(tm)
            tm["device_h2d_ms"] = round(h2d_ms, 3)
        stats.rows = n
        stats.wall_s = time.perf_counter() - t0
        return out, stats

    # ----------------------------------------------------------------- rerank
    # Cross-encoder scoring of (query, passage) pairs on the bucket machinery of the small-job
    # forms: per chunk of at most B pairs one H2D of the packed texts, one graph (tokenize the
    # chunk's queries, tokenize its passages, pair_assemble, model.score) and one D2D of the
    # scores; after the last chunk one group_topk launch and one D2H.
    def _special_ids(self) -> Tuple[int, int, int]:
        if self.vocab is not None:
            return self.vocab.cls_id, self.vocab.sep_id, self.vocab.pad_id
        return CLS_ID, SEP_ID, PAD_ID

    def _rerank_bufs(self) -> Dict[str, torch.Tensor]:
        """The re-ranker's extra buffers, allocated on first use: a text / offsets slot and token rows
        for the queries, the pair rows with their type ids, and the rows' query index."""
        if getattr(self, "_rr", None) is None:
            dev, B, S = self.device, self.B, self.S
            rr = {"text_q": torch.empty(B * self.max_row_bytes, dtype=torch.uint8, device=dev),
                  "offs_q": i32(B + 1, device=dev), "ids_q": i32(B, S, device=dev), "lens_q": i32(B, device=dev),
                  "ids": i32(B, S, device=dev), "type_ids": i32(B, S, device=dev), "lens": i32(B, device=dev),
                  "qidx": i32(B, device=dev)}
            if dev.type == "cuda":
                rr.update(pin_text_q=torch.zeros(B * self.max_row_bytes, dtype=torch.uint8, pin_memory=True),
                          pin_offs_q=i32(B + 1, pin_memory=True), pin_qidx=i32(B, pin_memory=True))
            self._rr = rr
        return self._rr

    def _assemble_pairs(self, bucket: int, mq: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The pair rows ``(ids, lens, type_ids)`` of the pairs staged in slot 0 (passages) and the query slot."""
        r = self._rerank_bufs()
        cls_id, sep_id, pad_id = self._special_ids()
        self._tokenize(r["text_q"], r["offs_q"], ids=r["ids_q"], lens=r["lens_q"], rows=bucket)
        self._tokenize(self.text[0], self.offs[0], ids=self.ids_s[0], lens=self.lens_s[0], rows=bucket)
        ops.pair_assemble(r["ids_q"][:bucket], r["lens_q"][:bucket], self.ids_s[0], self.lens_s[0], r["qidx"], mq,
                          cls_id, sep_id, pad_id, ids=r["ids"], type_ids=r["type_ids"], lens=r["lens"], rows=bucket)
        return r["ids"][:bucket], r["lens"][:bucket], r["type_ids"][:bucket]

    def _rerank_step(self, bucket: int, mq: int, label: int) -> torch.Tensor:
        """Raw scores ``[bucket]`` of the staged pairs."""
        ids, lens, types = self._assemble_pairs(bucket, mq)
        return self.model.score(ids, lens, types, label)

    def _encode_rows(self, rows: Sequence) -> List[bytes]:
        return [(r if isinstance(r, (bytes, bytearray)) else r.encode("utf-8"))[:self.max_row_bytes] for r in rows]

    @staticmethod
    def _check_goff(goff: Sequence[int], Q: int, P: int) -> List[int]:
        goff = [int(g) for g in goff]
        if len(goff) != Q + 1 or goff[0] != 0 or goff[-1] != P or any(a > b for a, b in zip(goff, goff[1:])):
            raise ValueError("goff must be Q + 1 non-decreasing offsets from 0 to len(passages)")
        return goff

    def score_pairs(self, queries: Sequence, passages: Sequence, goff: Sequence[int],
                    max_query_tokens: Optional[int] = None, label: int = 0) -> torch.Tensor:
        """Raw cross-encoder scores ``[P]`` fp32, left on the engine's device (a DP caller all-gathers
        them): ``passages`` is the flat list of all candidates, query ``q`` owning rows
        ``goff[q] .. goff[q + 1] - 1``; the score of a pair is the logit of class ``label`` of the row
        ``[CLS] query [SEP] passage [SEP]`` (``ops.pair_assemble``, the query cut at
        ``max_query_tokens``, default ``min(32, (S - 3) // 2)``)."""
        Q, P = len(queries), len(passages)
        goff = self._check_goff(goff, Q, P)
        if self.S < 4:
            raise ValueError("rerank_pairs needs seq_len >= 4")
        mq = default_max_query_tokens(self.S) if max_query_tokens is None else max_query_tokens
        if isinstance(mq, bool) or not isinstance(mq, int) or mq < 0:
            raise ValueError("max_query_tokens must be an int >= 0")
        if isinstance(label, bool) or not isinstance(label, int) or not 0 <= label < self.cfg.num_labels:
            raise ValueError("label must be in [0, num_labels)")
        scores = torch.empty(P, dtype=torch.float32, device=self.device)
        for c0, m, bk, rows in self._pair_chunks(queries, passages, goff, mq):
            if rows is not None:
                ids, types, lens = rows
                scores[c0:c0 + m] = self.model.score(ids, lens, types, label)
            else:
                # the WordPiece table is on the device since __init__; the warm-up run loads the code objects
                out = self._replay(("rerank", bk, mq, label), lambda: self._rerank_step(bk, mq, label))
                scores[c0:c0 + m].copy_(out[:m])
        return scores

    def _pair_chunks(self, queries: Sequence, passages: Sequence, goff: List[int], mq: int, wide: bool = False):
        """The chunk staging of the pair jobs (:meth:`score_pairs`, :meth:`span_pairs`): yields
        ``(c0, m, bucket, rows)`` per chunk of at most ``B`` pairs. On the GPU the chunk's packed texts,
        offsets (padding rows: empty passages of query 0) and query indices are copied through the
        pinned rows into slot 0 and the query slot, ``rows`` is None and the caller runs its step on
        ``bucket`` rows; on the CPU ``rows`` is the assembled ``(ids, type_ids, lens)``. Before a
        chunk's pinned rows are overwritten the copies of the previous one have completed (``free``).
        ``wide`` (the windowed reader): on the CPU ``rows`` is ``(ids_q, lens_q, ids_p, lens_p, qidx)`` with
        the passages tokenized whole, at ``L = max_row_bytes + 2``, and not assembled."""
        Q, P = len(queries), len(passages)
        cuda = self.device.type == "cuda"
        if P == 0:
            return
        qid = np.repeat(np.arange(Q, dtype=np.int64), np.diff(np.asarray(goff, dtype=np.int64)))  # row -> query
        r = self._rerank_bufs()
        free = None  # the event after which the pinned rows of the previous chunk may be overwritten
        for c0 in range(0, P, self.B):
            m = min(self.B, P - c0)
            used, local = np.unique(qid[c0:c0 + m], return_inverse=True)  # the chunk's queries: at most m
            text_p, offs_p = pack_rows(self._encode_rows(passages[c0:c0 + m]))
            text_q, offs_q = pack_rows(self._encode_rows([queries[int(q)] for q in used]))
            local = local.astype(np.int32)
            if not cuda:
                ids_q, lens_q = self._tokenize(torch.from_numpy(text_q), torch.from_numpy(offs_q))
                if wide:
                    ids_p, lens_p = self._tokenize(torch.from_numpy(text_p), torch.from_numpy(offs_p),
                                                   seq_len=self.max_row_bytes + 2)
                    yield c0, m, None, (ids_q, lens_q, ids_p, lens_p, torch.from_numpy(local))
                    continue
                ids_p, lens_p = self._tokenize(torch.from_numpy(text_p), torch.from_numpy(offs_p))
                yield c0, m, None, ops.pair_assemble(ids_q, lens_q, ids_p, lens_p, torch.from_numpy(local), mq,
                                                     *self._special_ids())
                continue
            if free is not None:
                free.synchronize()
            bk, nq = self._stage_texts((text_p, offs_p), m), len(used)  # padding rows: an empty passage ...
            r["pin_text_q"][:text_q.size].copy_(torch.from_numpy(text_q))
            r["pin_offs_q"][:nq + 1].copy_(torch.from_numpy(offs_q))
            r["pin_offs_q"][nq + 1:bk + 1].fill_(int(offs_q[-1]))
            r["pin_qidx"][:m].copy_(torch.from_numpy(local))
            r["pin_qidx"][m:bk].zero_()  # ... of query 0, their scores dropped
            if text_q.size:
                r["text_q"][:text_q.size].copy_(r["pin_text_q"][:text_q.size], non_blocking=True)
            r["offs_q"][:bk + 1].copy_(r["pin_offs_q"][:bk + 1], non_blocking=True)
            r["qidx"][:bk].copy_(r["pin_qidx"][:bk], non_blocking=True)
            free = torch.cuda.Event()
            free.record()
            yield c0, m, bk, None
        if free is not None:
            free.synchronize()  # the pinned rows are free for the next call, whichever form it is

    # ----------------------------------------------------------------- answer
    # Extractive question answering on the pair rows of the re-ranker: per chunk one graph (tokenize
    # the chunk's questions, tokenize its passages, pair_assemble, model.spans) and D2D copies of the
    # spans into [P, n] buffers; after the last chunk one group_topk launch over the flattened
    # [P * n] scores and one D2H. The host maps the returned token spans to character offsets.
    def _answer_step(self, bucket: int, mq: int, max_len: int, n: int):
        ids, lens, types = self._assemble_pairs(bucket, mq)
        return self.model.spans(ids, lens, types, max_len, n)

    def _check_answer_args(self, top_k, max_answer_tokens, max_query_tokens) -> Tuple[int, int, int]:
        if self.S < 4:
            raise ValueError("answer_pairs needs seq_len >= 4")
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= ops.span.MAX_N:
            raise ValueError("top_k must be an int in [1, 32]")
        ma = max_answer_tokens
        if isinstance(ma, bool) or not isinstance(ma, int) or not 1 <= ma <= self.S - 3:
            raise ValueError("max_answer_tokens must be an int in [1, seq_len - 3]")
        mq = default_max_query_tokens(self.S) if max_query_tokens is None else max_query_tokens
        if isinstance(mq, bool) or not isinstance(mq, int) or mq < 0:
            raise ValueError("max_query_tokens must be an int >= 0")
        return top_k, ma, mq

    def span_pairs(self, questions: Sequence, passages: Sequence, goff: Sequence[int], n_best: int = 3,
                   max_answer_tokens: int = 30, max_query_tokens: Optional[int] = None,
                   doc_stride: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The ``n_best`` answer spans of every (question, passage) pair: ``(span [P, n, 2] int32
        passage-relative token spans, score [P, n] fp32, null [P] fp32)`` of ``ops.span_topk``, left on the
        engine's device (a DP caller all-gathers them): views of the engine's ``[P, n]`` buffers, valid until
        the next call. The pair layout is that of :meth:`score_pairs`.

        ``doc_stride`` (an int in ``[1, S - 3]``): a passage too long for its row is read in overlapping
        windows ("atpu-window v1", ``tokenizer.window_table``) that advance by ``min(doc_stride, cap)``
        tokens; the windows' spans are folded back per pair (``ops.window_best``), ``span`` then being
        passage-absolute tokens of the passage cut at ``max_row_bytes`` and ``null`` the minimum over the
        pair's windows. ``self.window_counts`` holds every pair's window count, ``[P]`` int32."""
        Q, P = len(questions), len(passages)
        goff = self._check_goff(goff, Q, P)
        n, ma, mq = self._check_answer_args(n_best, max_answer_tokens, max_query_tokens)
        if doc_stride is not None and (isinstance(doc_stride, bool) or not isinstance(doc_stride, int)
                                       or not 1 <= doc_stride <= self.S - 3):
            raise ValueError("doc_stride must be an int in [1, seq_len - 3]")
        # one allocation serves every job of up to B pairs
        span, score, null = self._result_rows("_an", P, self.B, ((n, 2), torch.int32), ((n,), torch.float32),
                                              ((), torch.float32))
        if doc_stride is not None:
            self._span_windows(questions, passages, goff, n, ma, mq, doc_stride, span, score, null)
            return span, score, null
        for c0, m, bk, rows in self._pair_chunks(questions, passages, goff, mq):
            if rows is not None:
                ids, types, lens = rows
                sp, sc, nl = self.model.spans(ids, lens, types, ma, n)
            else:
                sp, sc, nl = self._replay(("answer", bk, mq, ma, n), lambda: self._answer_step(bk, mq, ma, n),
                                          prepare=self.model.span_inputs)
            span[c0:c0 + m].copy_(sp[:m]), score[c0:c0 + m].copy_(sc[:m]), null[c0:c0 + m].copy_(nl[:m])
        return span, score, null

    # ------------------------------------------------------- answer: windows over long passages
    # With doc_stride a pair chunk takes two kinds of graph. ("wtok", bucket) tokenizes the chunk's
    # questions at S and its passages whole, at L = max_row_bytes + 2 (a token covers at least one
    # byte, so only the byte cut truncates). The two length vectors come back in one D2H (the call's
    # one sync per pair chunk), the host lays out the window table, and per chunk of at most B window
    # rows ("wanswer", bucket, mq, max_len, n, doc_stride) runs window_assemble and model.spans(own=)
    # on the table's rows; their spans are copied D2D into [R, n] buffers and one window_best launch
    # folds them into the chunk's slice of the per-pair buffers. Padding window rows are windows of
    # pair 0 at start 0; they lie outside every pair's row range.
    def _window_bufs(self) -> Dict[str, torch.Tensor]:
        if getattr(self, "_wn", None) is None:
            dev, B = self.device, self.B
            L = self.max_row_bytes + 2
            w = {"ids_p": i32(B, L, device=dev), "lens_p": i32(B, device=dev), "win_pair": i32(B, device=dev),
                 "win_start": i32(B, device=dev), "own": i32(B, 2, device=dev), "wrow": i32(B + 1, device=dev)}
            if dev.type == "cuda":
                w.update(pin_pair=i32(B, pin_memory=True), pin_start=i32(B, pin_memory=True),
                         pin_wrow=i32(B + 1, pin_memory=True))
            self._wn = w
        return self._wn

    def _wtok_step(self, bucket: int) -> None:
        r, w = self._rerank_bufs(), self._window_bufs()
        self._tokenize(r["text_q"], r["offs_q"], ids=r["ids_q"], lens=r["lens_q"], rows=bucket)
        self._tokenize(self.text[0], self.offs[0], ids=w["ids_p"], lens=w["lens_p"], rows=bucket,
                       seq_len=self.max_row_bytes + 2)

    def _wanswer_step(self, bucket: int, mq: int, max_len: int, n: int, doc_stride: int):
        r, w = self._rerank_bufs(), self._window_bufs()
        cls_id, sep_id, pad_id = self._special_ids()
        ops.window_assemble(r["ids_q"], r["lens_q"], w["ids_p"], w["lens_p"], r["qidx"], w["win_pair"],
                            w["win_start"], mq, doc_stride, cls_id, sep_id, pad_id, ids=r["ids"],
                            type_ids=r["type_ids"], lens=r["lens"], own=w["own"], rows=bucket)
        return self.model.spans(r["ids"][:bucket], r["lens"][:bucket], r["type_ids"][:bucket], max_len, n,
                                own=w["own"])

    def _span_windows(self, questions: Sequence, passages: Sequence, goff: List[int], n: int, ma: int, mq: int,
                      doc_stride: int, span: torch.Tensor, score: torch.Tensor, null: torch.Tensor) -> None:
        """The windowed form of :meth:`span_pairs`: fills the per-pair ``span / score / null [P]`` views."""
        S, B, L = self.S, self.B, self.max_row_bytes + 2
        P = len(passages)
        counts = np.zeros(P, dtype=np.int32)
        r, w = self._rerank_bufs(), self._window_bufs()
        wfree = None  # the event after which the pinned table rows may be overwritten
        for c0, m, bk, rows in self._pair_chunks(questions, passages, goff, mq, wide=True):
            if rows is not None:
                ids_q, lens_q, ids_p, lens_p, qidx = rows
                lq, lp, qi = lens_q.tolist(), lens_p.tolist(), qidx.tolist()
            else:
                self._replay(("wtok", bk), lambda: self._wtok_step(bk))
                host = torch.cat([r["lens_q"][:bk], w["lens_p"][:bk], r["qidx"][:bk]]).cpu()  # one D2H, one sync
                lq, lp, qi = (host[i * bk:(i + 1) * bk].tolist() for i in range(3))
            pair_l, start_l, wrow = [], [], [0]
            for i in range(m):
                nq = min(min(max(lq[qi[i]], 2), S) - 2, mq, S - 3)
                table = window_table(min(max(lp[i], 2), L) - 2, nq, S, doc_stride)
                pair_l += [i] * len(table)
                start_l += [t[0] for t in table]
                wrow.append(len(pair_l))
            R = len(pair_l)
            counts[c0:c0 + m] = np.diff(np.asarray(wrow))
            win_pair = torch.tensor(pair_l, dtype=torch.int32)
            win_start = torch.tensor(start_l, dtype=torch.int32)
            wrow_t = torch.tensor(wrow, dtype=torch.int32)
            if rows is not None:
                ids, types, lens, own = ops.window_assemble(ids_q, lens_q, ids_p, lens_p, qidx, win_pair, win_start,
                                                            mq, doc_stride, *self._special_ids())
                sp, sc, nl = self.model.spans(ids, lens, types, ma, n, own=own)
                ops.window_best(sp, sc, nl, win_start, wrow_t, span=span[c0:], score=score[c0:], null=null[c0:])
                continue
            # the chunk's window rows: grown here, outside any capture
            span_w, score_w, null_w, start_w = self._result_rows(
                "_wr", R, 2 * B, ((n, 2), torch.int32), ((n,), torch.float32), ((), torch.float32), ((), torch.int32))
            for r0 in range(0, R, B):
                mw = min(B, R - r0)
                bkw = self._bucket(mw)
                if wfree is not None:
                    wfree.synchronize()
                w["pin_pair"][:mw].copy_(win_pair[r0:r0 + mw])
                w["pin_pair"][mw:bkw].zero_()  # padding rows: windows of pair 0 ...
                w["pin_start"][:mw].copy_(win_start[r0:r0 + mw])
                w["pin_start"][mw:bkw].zero_()  # ... at start 0, their spans dropped
                if r0 == 0:
                    w["pin_wrow"][:m + 1].copy_(wrow_t)
                    w["wrow"][:m + 1].copy_(w["pin_wrow"][:m + 1], non_blocking=True)
                w["win_pair"][:bkw].copy_(w["pin_pair"][:bkw], non_blocking=True)
                w["win_start"][:bkw].copy_(w["pin_start"][:bkw], non_blocking=True)
                wfree = torch.cuda.Event()
                wfree.record()
                sp, sc, nl = self._replay(("wanswer", bkw, mq, ma, n, doc_stride),
                                          lambda: self._wanswer_step(bkw, mq, ma, n, doc_stride),
                                          prepare=self.model.span_inputs)
                span_w[r0:r0 + mw].copy_(sp[:mw]), score_w[r0:r0 + mw].copy_(sc[:mw])
                null_w[r0:r0 + mw].copy_(nl[:mw]), start_w[r0:r0 + mw].copy_(w["win_start"][:mw])
            ops.window_best(span_w, score_w, null_w, start_w, w["wrow"][:m + 1], span=span[c0:], score=score[c0:],
                            null=null[c0:])
        if wfree is not None:
            wfree.synchronize()
        self.window_counts = torch.from_numpy(counts).to(self.device)

    @staticmethod
    def _char_span(full: bytes, a: int, b: int) -> Tuple[int, int, str]:
        """The byte range ``[a, b)`` of ``full`` widened outward to UTF-8 character boundaries, as
        ``(start, end, text)`` in characters of the decoded string."""
        while a > 0 and 0x80 <= full[a] <= 0xBF:
            a -= 1
        while b < len(full) and 0x80 <= full[b] <= 0xBF:
            b += 1
        start = len(full[:a].decode("utf-8", "replace"))
        text = full[a:b].decode("utf-8", "replace")
        return start, start + len(text), text

    def rank_spans(self, span: torch.Tensor, score: torch.Tensor, null: torch.Tensor, passages: Sequence,
                   goff: Sequence[int], top_k: int = 3, token_cap: Optional[int] = None) -> "AnswerResult":
        """Every question's ``top_k`` best spans over all of its pairs: one ``ops.group_topk`` launch over the
        flattened ``[P * n]`` scores (offsets ``goff * n``; score descending, then pair and slot ascending)
        and one D2H; the token spans of the returned answers are mapped to character offsets of their
        passage on the host (``token_spans``, the row cut at ``max_row_bytes`` as the device cut it).
        ``-inf`` entries are dropped. ``token_cap``: the most tokens of a passage a span can refer to,
        ``S - 2`` by default; windowed spans (``doc_stride``) are passage-absolute: pass ``max_row_bytes``."""
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= ops.rerank.MAX_K:
            raise ValueError("top_k must be an int in [1, 32]")
        P, n = int(score.shape[0]), int(score.shape[1])
        Q = len(goff) - 1
        goff = self._check_goff(goff, Q, P)
        if len(passages) != P:
            raise ValueError("rank_spans: one passage per span row")
        k = top_k
        if P == 0 or Q == 0:
            return AnswerResult(Q, P, [[] for _ in range(Q)], span.cpu(), score.cpu(), null.cpu())
        idx, val = ops.group_topk(score.reshape(-1), torch.tensor([g * n for g in goff], dtype=torch.int32)
                                  .to(score.device), k)
        both = torch.cat([idx.view(torch.float32).reshape(-1), val.reshape(-1), span.view(torch.float32).reshape(-1),
                          score.reshape(-1), null]).cpu()  # one D2H, one sync
        cut = np.cumsum([0, Q * k, Q * k, P * n * 2, P * n, P]).tolist()
        idx_h = both[cut[0]:cut[1]].clone().view(torch.int32).view(Q, k)
        val_h = both[cut[1]:cut[2]].clone().view(Q, k)
        span_h = both[cut[2]:cut[3]].clone().view(torch.int32).view(P, n, 2)
        score_h = both[cut[3]:cut[4]].clone().view(P, n)
        null_h = both[cut[4]:cut[5]].clone()
        cap = self.S - 2 if token_cap is None else int(token_cap)
        answers: List[List[Dict[str, object]]] = []
        tok_cache: Dict[int, Tuple[bytes, list]] = {}
        for q in range(Q):
            row = []
            for f, s in zip(idx_h[q].tolist(), val_h[q].tolist()):
                if f < 0 or s == float("-inf"):
                    break  # sorted: nothing after a padding entry or a -inf score
                pair, slot = goff[q] + f // n, f % n
                t0, t1 = span_h[pair, slot].tolist()
                if pair not in tok_cache or len(tok_cache[pair][1]) <= t1:
                    p = passages[pair]
                    full = bytes(p) if isinstance(p, (bytes, bytearray)) else p.encode("utf-8")
                    cutrow = full[:self.max_row_bytes]
                    need = min(cap, t1 + 1)  # the row is tokenized only as far as the span's last token
                    toks = (self.vocab.token_spans(cutrow, need) if self.vocab is not None
                            else token_spans(cutrow, self.cfg.vocab_size, need))
                    tok_cache[pair] = (full, toks)
                full, toks = tok_cache[pair]
                a, b = toks[t0][0], toks[t1][1]
                start, end, text = self._char_span(full, a, b)
                row.append({"passage": pair - goff[q], "start": start, "end": end, "text": text, "score": float(s),
                            "null_score": float(null_h[pair]), "tokens": (int(t0), int(t1))})
            answers.append(row)
        return AnswerResult(Q, P, answers, span_h, score_h, null_h)

    def answer_pairs(self, questions: Sequence, passages: Sequence, goff: Sequence[int], top_k: int = 3,
                     max_answer_tokens: int = 30, max_query_tokens: Optional[int] = None,
                     doc_stride: Optional[int] = None) -> "AnswerResult":
        """:meth:`span_pairs` with ``n_best = top_k``, then :meth:`rank_spans`: a reader over every
        (question, passage) pair, each question's best ``top_k`` answer spans over all of its passages (a
        question's top-k holds at most ``top_k`` spans of one pair). ``doc_stride``: long passages are read
        in overlapping windows, see :meth:`span_pairs`."""
        span, score, null = self.span_pairs(questions, passages, goff, top_k, max_answer_tokens, max_query_tokens,
                                            doc_stride)
        if doc_stride is None:
            return self.rank_spans(span, score, null, passages, goff, top_k)
        res = self.rank_spans(span, score, null, passages, goff, top_k, token_cap=self.max_row_bytes)
        res.window_count = int(self.window_counts.sum())
        return res

    # ------------------------------------------------------------ token classification (map_tag)
    # Single-segment rows [CLS] text [SEP] on the machinery of embed_texts: per chunk of at most B rows
    # one H2D through the pinned rows, one captured graph per ("tag", bucket, mode, E) (tokenize,
    # model.tags) and D2D copies of the records into [N, E] buffers; one D2H per call. The host maps
    # the token positions to character offsets. Text past seq_len - 2 tokens is not tagged.
    TAG_NEEDS_VOCAB = "aggregation 'first' needs a WordPiece vocabulary (the hash tokenizer has no word pieces)"

    def set_tag_labels(self, names: Optional[Sequence[str]] = None, outside: Sequence[str] = ("O",)) -> None:
        """Name the tag head's labels (default: ``ops.default_tag_names``) and build the label tables."""
        L = self.cfg.tag_labels
        if L <= 0:
            raise ValueError("model has no tag head")
        names = ops.default_tag_names(L) if names is None else [str(n) for n in names]
        if len(names) != L:
            raise ValueError(f"tag_labels: {len(names)} names for a head of {L} labels")
        types, lt, lb = ops.tag_tables(names, outside)
        self._tag = {"names": names, "types": types, "label_type": lt.to(self.device),
                     "label_begin": lb.to(self.device)}

    def _tag_state(self) -> Dict[str, object]:
        if getattr(self, "_tag", None) is None:
            self.set_tag_labels()
        return self._tag

    def _tag_cont(self) -> Optional[torch.Tensor]:
        """``cont [V]`` uint8: 1 where the vocabulary's entry is a ``##`` piece (built once per engine)."""
        if self.vocab is None:
            raise ValueError(self.TAG_NEEDS_VOCAB)
        if getattr(self, "_tagcont", None) is None:
            flags = np.fromiter((len(e) > 2 and e.startswith(b"##") for e in self.vocab.entries), dtype=np.uint8,
                                count=len(self.vocab))
            self._tagcont = torch.from_numpy(flags).to(self.device)
        return self._tagcont

    @staticmethod
    def _check_tag_args(mode, max_entities) -> Tuple[int, int]:
        if isinstance(mode, str):
            if mode not in ops.tag.MODES:
                raise ValueError("aggregation must be 'simple', 'first' or 'none'")
            mode = ops.tag.MODES[mode]
        if isinstance(mode, bool) or not isinstance(mode, int) or mode not in (0, 1, 2):
            raise ValueError("aggregation must be 'simple', 'first' or 'none'")
        E = max_entities
        if isinstance(E, bool) or not isinstance(E, int) or not 1 <= E <= ops.tag.MAX_ENTITIES:
            raise ValueError("max_entities must be an int in [1, 512]")
        return mode, E

    def _tag_step(self, bucket: int, mode: int, E: int):
        st = self._tag_state()
        self._tokenize(self.text[0], self.offs[0], ids=self.ids_s[0], lens=self.lens_s[0], rows=bucket)
        return self.model.tags(self.ids_s[0][:bucket], self.lens_s[0][:bucket], st["label_type"], st["label_begin"],
                               mode, E, cont=self._tag_cont() if mode == 2 else None)

    def tag_rows(self, rows: Sequence, mode="simple", max_entities: int = 64
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The entity records of every row: ``(ent [N, E, 4] int32, ent_sum [N, E] fp32, count [N] int32)`` of
        ``ops.tag_entities``, left on the engine's device (a DP caller all-gathers them): views of the
        engine's ``[N, E]`` buffers, valid until the next call."""
        mode, E = self._check_tag_args(mode, max_entities)
        if self.S < 3:
            raise ValueError("tag_texts needs seq_len >= 3")
        self._tag_state()
        if mode == 2:
            self._tag_cont()
        N, dev = len(rows), self.device
        # one allocation serves every job of up to B rows
        ent, ent_sum, count = self._result_rows("_tg", N, self.B, ((E, 4), torch.int32), ((E,), torch.float32),
                                                ((), torch.int32))
        for b0 in range(0, N, self.B):
            chunk = self._encode_rows(rows[b0:b0 + self.B])
            text, offs = pack_rows(chunk)
            n = len(chunk)
            if dev.type == "cuda":
                bk = self._stage_texts((text, offs), n)
                e, s_, c = self._replay(("tag", bk, mode, E), lambda: self._tag_step(bk, mode, E),
                                        prepare=self.model.tag_inputs)
                ent[b0:b0 + n].copy_(e[:n]), ent_sum[b0:b0 + n].copy_(s_[:n]), count[b0:b0 + n].copy_(c[:n])
                torch.cuda.current_stream(dev).synchronize()  # the pinned rows are free again
            else:
                ids, lens = self._tokenize(torch.from_numpy(text), torch.from_numpy(offs))
                st = self._tag_state()
                e, s_, c = self.model.tags(ids, lens, st["label_type"], st["label_begin"], mode, E,
                                           cont=self._tag_cont() if mode == 2 else None)
                ent[b0:b0 + n].copy_(e), ent_sum[b0:b0 + n].copy_(s_), count[b0:b0 + n].copy_(c)
        return ent, ent_sum, count

    def map_tags(self, ent: torch.Tensor, ent_sum: torch.Tensor, count: torch.Tensor, rows: Sequence,
                 mode="simple") -> "TagResult":
        """Records -> entities on the host: one D2H, then the token positions of every record are mapped to
        character offsets of its row (``token_spans``, the row cut at ``max_row_bytes`` as the device cut it,
        tokenized only as far as the row's last record) and ``score = ent_sum / n`` in fp64."""
        mode, _ = self._check_tag_args(mode, 1)
        st = self._tag_state()
        N, E = int(ent.shape[0]), int(ent.shape[1])
        if len(rows) != N:
            raise ValueError("map_tags: one row of text per record row")
        if N == 0:
            return TagResult(0, [], [], [], ent.cpu(), ent_sum.cpu())
        both = torch.cat([ent.view(torch.float32).reshape(-1), ent_sum.reshape(-1),
                          count.view(torch.float32).reshape(-1)]).cpu()  # one D2H, one sync
        ent_h = both[:N * E * 4].clone().view(torch.int32).view(N, E, 4)
        sum_h = both[N * E * 4:N * E * 5].clone().view(N, E)
        counts = both[N * E * 5:].clone().view(torch.int32).tolist()
        cap = self.S - 2
        entities: List[List[Dict[str, object]]] = []
        for i in range(N):
            k = min(counts[i], E)
            recs, sums = ent_h[i, :k].tolist(), sum_h[i, :k].tolist()
            row: List[Dict[str, object]] = []
            if k:
                r = rows[i]
                full = bytes(r) if isinstance(r, (bytes, bytearray)) else r.encode("utf-8")
                cutrow = full[:self.max_row_bytes]
                need = min(cap, recs[-1][1] + 1)  # records are in token order: the last one ends last
                toks = (self.vocab.token_spans(cutrow, need) if self.vocab is not None
                        else token_spans(cutrow, self.cfg.vocab_size, need))
                ascii_row = full.isascii()  # bytes are characters: nothing to widen, no prefix to decode
                for (first, last, third, n), s in zip(recs, sums):
                    if ascii_row:
                        start, end = toks[first][0], toks[last][1]
                        word = full[start:end].decode("ascii")
                    else:
                        start, end, word = self._char_span(full, toks[first][0], toks[last][1])
                    score = float(np.float64(s) / np.float64(n)) if n > 0 else 0.0
                    if mode == 0:
                        row.append({"entity": st["names"][third], "score": score, "index": first + 1, "word": word,
                                    "start": start, "end": end})
                    else:
                        row.append({"entity_group": st["types"][third], "score": score, "word": word,
                                    "start": start, "end": end})
            entities.append(row)
        return TagResult(N, entities, counts, [i for i in range(N) if counts[i] > E], ent_h, sum_h)

    def tag_texts(self, rows: Sequence, mode="simple", max_entities: int = 64) -> "TagResult":
        """:meth:`tag_rows`, then :meth:`map_tags`: the entities of an in-memory list of strings."""
        ent, ent_sum, count = self.tag_rows(rows, mode, max_entities)
        return self.map_tags(ent, ent_sum, count, rows, mode)

    # ------------------------------------------------------------ masked-token prediction (map_fill)
    # The staging of embed_texts with the text split at its mask tokens on the host: per chunk of at most B
    # texts one H2D of the packed pieces, their offsets and the compact slot lists (the host knows every
    # text's mask count), one captured graph per ("fill", row bucket, slot bucket, k, targets) (tokenize the
    # pieces, fill_assemble, model.fills) and D2D scatters of the slots into per-text [N, M, k] buffers; one
    # D2H per call. The slot count is padded to 16 * 2^i with invalid slots.
    FILL_NO_HEAD = "model has no MLM head"
    FILL_NO_MASK_ID = "vocabulary has no [MASK] token"
    FILL_TOO_MANY = "a text has more than 16 mask tokens"

    def _mask_id(self) -> int:
        if self.vocab is None:
            return MASK_ID
        if self.vocab.mask_id is None:
            raise ValueError(self.FILL_NO_MASK_ID)
        return int(self.vocab.mask_id)

    def _fill_bufs(self) -> Dict[str, torch.Tensor]:
        """The fill buffers, allocated once on first use (captured graphs keep their addresses): token rows and
        offsets for up to 17 B pieces, the rows' segment offsets, the mask positions and the slot lists."""
        if getattr(self, "_fl", None) is None:
            dev, B, S = self.device, self.B, self.S
            segcap, rcap = (MAX_MASKS + 1) * B, MAX_MASKS * B
            fl = {"offs": i32(segcap + 1, device=dev), "ids_s": i32(segcap, S, device=dev),
                  "lens_s": i32(segcap, device=dev), "segoff": i32(B + 1, device=dev), "ids": i32(B, S, device=dev),
                  "lens": i32(B, device=dev), "pos": i32(B, MAX_MASKS, device=dev), "mrow": i32(rcap, device=dev),
                  "mord": i32(rcap, device=dev), "tids": torch.zeros(ops.fill.MAX_K, dtype=torch.int64, device=dev)}
            if dev.type == "cuda":
                fl.update(pin_offs=i32(segcap + 1, pin_memory=True), pin_segoff=i32(B + 1, pin_memory=True),
                          pin_mrow=i32(rcap, pin_memory=True), pin_mord=i32(rcap, pin_memory=True))
            self._fl = fl
        return self._fl

    def _fill_step(self, bucket: int, segs: int, slots: int, k: int, T: int):
        f = self._fl
        cls_id, sep_id, pad_id = self._special_ids()
        self._tokenize(self.text[0], f["offs"], ids=f["ids_s"], lens=f["lens_s"], rows=segs)
        ops.fill_assemble(f["ids_s"][:segs], f["lens_s"][:segs], f["segoff"], MAX_MASKS, cls_id, sep_id, pad_id,
                          self._mask_id(), ids=f["ids"], lens=f["lens"], pos=f["pos"], rows=bucket)
        tok, _, prob, _ = self.model.fills(f["ids"][:bucket], f["lens"][:bucket], f["pos"][:bucket], f["mrow"][:slots],
                                           f["mord"][:slots], k, tids=f["tids"][:T] if T else None)
        return tok, prob, f["pos"]

    def _slot_bucket(self, R: int) -> int:
        b = 16
        while b < R:
            b *= 2
        return min(b, MAX_MASKS * self.B)  # the slot buffers' size (R never exceeds it)

    def _check_fill_args(self, top_k, mask_token, tids) -> Tuple[int, Optional[List[int]]]:
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= ops.fill.MAX_K:
            raise ValueError("top_k must be an int in [1, 32]")
        if not isinstance(mask_token, str) or not mask_token:
            raise ValueError("mask_token must be a non-empty string")
        if not self.cfg.mlm_head:
            raise ValueError(self.FILL_NO_HEAD)
        self._mask_id()
        if tids is not None:
            tids = [int(t) for t in tids]
            if not 1 <= len(tids) <= ops.fill.MAX_K or len(set(tids)) != len(tids) or any(
                    not 0 <= t < self.cfg.vocab_size for t in tids):
                raise ValueError("targets must be 1 to 32 distinct token ids of the vocabulary")
        return top_k, tids

    def fill_rows(self, rows: Sequence[str], top_k: int = 5, mask_token: str = "[MASK]",
                  tids: Optional[Sequence[int]] = None, max_masks: Optional[int] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The mask predictions of every text: ``(tok [N, M, k] int32, prob [N, M, k] fp32, pos [N, M] int32)``
        left on the engine's device (a DP caller all-gathers them), ``M`` = ``max_masks`` (default: the largest
        mask count of ``rows``, at least 1), ``k = min(top_k, len(tids))`` with targets. Slots past a text's
        masks are ``(-1, 0, -1)``. The pieces of a text are cut to ``max_row_bytes`` bytes in total, in text order
        (the mask tokens do not count): the cut depends on the text alone, and a chunk always fits the text slot.
        Masks after the cut follow the cut text directly."""
        k, tids = self._check_fill_args(top_k, mask_token, tids)
        if self.S < 3:
            raise ValueError("fill_texts needs seq_len >= 3")
        T = len(tids) if tids is not None else 0
        kk = min(k, T) if T else k
        split = [split_masks(r if isinstance(r, str) else bytes(r).decode("utf-8"), mask_token)[0] for r in rows]
        counts = [len(p) - 1 for p in split]
        if counts and max(counts) > MAX_MASKS:
            raise ValueError(self.FILL_TOO_MANY)
        M = max([1] + counts) if max_masks is None else int(max_masks)
        if not max([1] + counts) <= M <= MAX_MASKS:
            raise ValueError("max_masks must cover every text's masks and be at most 16")
        N, dev = len(rows), self.device
        tok = torch.full((N, M, kk), -1, dtype=torch.int32, device=dev)
        prob = torch.zeros((N, M, kk), dtype=torch.float32, device=dev)
        pos = torch.full((N, M), -1, dtype=torch.int32, device=dev)
        f = self._fill_bufs()
        if T:
            f["tids"][:T].copy_(torch.tensor(tids, dtype=torch.int64))
        for b0 in range(0, N, self.B):
            parts = split[b0:b0 + self.B]
            n = len(parts)
            pieces: List[bytes] = []
            for ps in parts:  # per text: max_row_bytes in all, so B texts fit the B * max_row_bytes text slot
                budget = self.max_row_bytes
                for p in ps:
                    pieces.append(p.encode("utf-8")[:budget])
                    budget -= len(pieces[-1])
            text, offs = pack_rows(pieces)
            segoff = np.zeros(n + 1, dtype=np.int32)
            segoff[1:] = np.cumsum([len(ps) for ps in parts])
            mrow = np.array([i for i, ps in enumerate(parts) for _ in range(len(ps) - 1)], dtype=np.int32)
            mord = np.array([j for ps in parts for j in range(len(ps) - 1)], dtype=np.int32)
            R = int(mrow.size)
            if dev.type == "cuda":
                pin = self._pinned()
                bk = self._bucket(n)
                segs = 2 * bk if len(pieces) <= 2 * bk else (MAX_MASKS + 1) * bk
                Rb = self._slot_bucket(R)
                pin["text"][:text.size].copy_(torch.from_numpy(text))
                f["pin_offs"][:len(pieces) + 1].copy_(torch.from_numpy(offs))
                f["pin_offs"][len(pieces) + 1:segs + 1].fill_(int(offs[-1]))  # padding pieces: empty strings
                f["pin_segoff"][:n + 1].copy_(torch.from_numpy(segoff))
                f["pin_segoff"][n + 1:bk + 1].fill_(int(segoff[-1]))  # padding rows: no pieces, [CLS] [SEP]
                f["pin_mrow"][:R].copy_(torch.from_numpy(mrow))
                f["pin_mrow"][R:Rb].fill_(-1)  # padding slots: invalid
                f["pin_mord"][:R].copy_(torch.from_numpy(mord))
                f["pin_mord"][R:Rb].fill_(0)
                if text.size:
                    self.text[0][:text.size].copy_(pin["text"][:text.size], non_blocking=True)
                f["offs"][:segs + 1].copy_(f["pin_offs"][:segs + 1], non_blocking=True)
                f["segoff"][:bk + 1].copy_(f["pin_segoff"][:bk + 1], non_blocking=True)
                f["mrow"][:Rb].copy_(f["pin_mrow"][:Rb], non_blocking=True)
                f["mord"][:Rb].copy_(f["pin_mord"][:Rb], non_blocking=True)
                t_, p_, ps_ = self._replay(("fill", bk, segs, Rb, k, T), lambda: self._fill_step(bk, segs, Rb, k, T),
                                           prepare=self.model.fill_inputs)
                if R:
                    dst = (f["mrow"][:R].long() + b0) * M + f["mord"][:R].long()
                    tok.view(N * M, kk).index_copy_(0, dst, t_[:R])
                    prob.view(N * M, kk).index_copy_(0, dst, p_[:R])
                pos[b0:b0 + n].copy_(ps_[:n, :M])
                torch.cuda.current_stream(dev).synchronize()  # the pinned rows are free again
            else:
                cls_id, sep_id, pad_id = self._special_ids()
                ids_s, lens_s = self._tokenize(torch.from_numpy(text), torch.from_numpy(offs))
                ids, lens, ps_ = ops.fill_assemble(ids_s, lens_s, torch.from_numpy(segoff), MAX_MASKS, cls_id, sep_id,
                                                   pad_id, self._mask_id())
                t_, _, p_, _ = self.model.fills(ids, lens, ps_, torch.from_numpy(mrow), torch.from_numpy(mord), k,
                                                tids=f["tids"][:T] if T else None)
                if R:
                    dst = (torch.from_numpy(mrow).long() + b0) * M + torch.from_numpy(mord).long()
                    tok.view(N * M, kk).index_copy_(0, dst, t_)
                    prob.view(N * M, kk).index_copy_(0, dst, p_.float())
                pos[b0:b0 + n].copy_(ps_[:, :M])
        return tok, prob, pos

    def map_fills(self, tok: torch.Tensor, prob: torch.Tensor, pos: torch.Tensor, rows: Sequence[str],
                  mask_token: str = "[MASK]") -> "FillResult":
        """Slots -> candidates on the host: one D2H, then every mask's candidates with the character offsets
        of its literal mask token. A mask with ``pos == -1`` fell beyond the row: no candidates, listed in
        ``truncated``."""
        N, M, k = (int(v) for v in tok.shape)
        if len(rows) != N:
            raise ValueError("map_fills: one row of text per record row")
        both = torch.cat([tok.view(torch.float32).reshape(-1), prob.reshape(-1),
                          pos.view(torch.float32).reshape(-1)]).cpu()  # one D2H, one sync
        tok_h = both[:N * M * k].clone().view(torch.int32).view(N, M, k)
        prob_h = both[N * M * k:2 * N * M * k].clone().view(N, M, k)
        pos_h = both[2 * N * M * k:].clone().view(torch.int32).view(N, M)
        names = self.vocab.entries if self.vocab is not None else None
        fills: List[List[Dict[str, object]]] = []
        truncated: List[Tuple[int, int]] = []
        for i in range(N):
            r = rows[i]
            spans = split_masks(r if isinstance(r, str) else bytes(r).decode("utf-8"), mask_token)[1]
            row: List[Dict[str, object]] = []
            for j, (a, b) in enumerate(spans):
                cands: List[Dict[str, object]] = []
                if pos_h[i, j] < 0:
                    truncated.append((i, j))
                else:
                    for t, p in zip(tok_h[i, j].tolist(), prob_h[i, j].tolist()):
                        if t >= 0:
                            name = names[t].decode("utf-8", "replace") if names is not None and t < len(names) else None
                            cands.append({"token_id": t, "token": name, "score": p})
                row.append({"start": a, "end": b, "candidates": cands})
            fills.append(row)
        return FillResult(N, fills, truncated, tok_h, prob_h, pos_h)

    def fill_texts(self, rows: Sequence[str], top_k: int = 5, mask_token: str = "[MASK]",
                   tids: Optional[Sequence[int]] = None) -> "FillResult":
        """:meth:`fill_rows`, then :meth:`map_fills`: the mask candidates of an in-memory list of strings."""
        tok, prob, pos = self.fill_rows(rows, top_k, mask_token, tids)
        return self.map_fills(tok, prob, pos, rows, mask_token)

    def rank_scores(self, scores: torch.Tensor, goff: Sequence[int], top_k: int = 10,
                    activation: str = "none") -> RerankResult:
        """The top ``top_k`` (1..32) of every query's own scores, in the total order (score descending,
        index ascending) of ``ops.group_topk``: one launch and one D2H, which also brings every raw
        score to the host. ``activation="sigmoid"`` maps the returned top-k values on the host, in
        fp32, after the ranking on raw logits (monotone: the order is the same)."""
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= ops.rerank.MAX_K:
            raise ValueError("top_k must be an int in [1, 32]")
        if activation not in ("none", "sigmoid"):
            raise ValueError("activation must be 'none' or 'sigmoid'")
        k, P = top_k, int(scores.numel())
        Q = len(goff) - 1
        goff = self._check_goff(goff, Q, P)
        if P == 0 or Q == 0:
            return RerankResult(Q, P, torch.full((Q, k), -1, dtype=torch.int32),
                                torch.full((Q, k), float("-inf")), scores.cpu())
        idx, val = ops.group_topk(scores, torch.tensor(goff, dtype=torch.int32).to(scores.device), k)
        both = torch.cat([idx.view(torch.float32).reshape(-1), val.reshape(-1), scores]).cpu()  # one D2H, one sync
        idx_h = both[:Q * k].clone().view(torch.int32).view(Q, k)
        val_h = both[Q * k:2 * Q * k].clone().view(Q, k)
        if activation == "sigmoid":
            val_h = torch.where(idx_h >= 0, torch.sigmoid(val_h), val_h)
        return RerankResult(Q, P, idx_h, val_h, both[2 * Q * k:].clone())

    def rerank_pairs(self, queries: Sequence, passages: Sequence, goff: Sequence[int], top_k: int = 10,
                     max_query_tokens: Optional[int] = None, label: int = 0,
                     activation: str = "none") -> RerankResult:
        """:meth:`score_pairs`, then :meth:`rank_scores`: every (query, passage) pair scored by the model
        as a cross-encoder, each query's own passages ranked."""
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= ops.rerank.MAX_K:
            raise ValueError("top_k must be an int in [1, 32]")
        if activation not in ("none", "sigmoid"):
            raise ValueError("activation must be 'none' or 'sigmoid'")
        scores = self.score_pairs(queries, passages, goff, max_query_tokens, label)
        return self.rank_scores(scores, goff, top_k, activation)

    # ------------------------------------------------------ late interaction (map_maxsim)
    # ColBERT scoring: the encoder reads every query and every passage once, alone, and keeps one unit
    # vector per token (model.token_vectors); a pair's score is ops.maxsim of its two rows. All queries
    # are encoded first, in chunks of at most B rows through the ("maxsim", bucket) graphs (tokenize,
    # token_vectors), and stay resident as qv [Q, S, P] with their lengths. The passages then stream in
    # chunks of at most B through the same graphs (the bucket is that of the rows staged, so 32 queries
    # cost a 32-row step whatever the passage chunks are), and one maxsim launch per chunk scores the
    # chunk's pairs into the result. Pair form: pair p is passage p with its own query (qidx through
    # the re-ranker's pinned index row, didx = arange). Shared form: every query against every passage
    # of the chunk, Q * bucket pairs whose index rows are built on the device once per (Q, bucket).
    @property
    def late_dim(self) -> int:
        """The width ``P`` of the token vectors: the late head's, or the hidden size without one."""
        return self.cfg.late_dim or self.cfg.hidden

    def _token_vector_step(self, bucket: int) -> Tuple[torch.Tensor, torch.Tensor]:
        self._tokenize(self.text[0], self.offs[0], ids=self.ids_s[0], lens=self.lens_s[0], rows=bucket)
        return self.model.token_vectors(self.ids_s[0][:bucket], self.lens_s[0][:bucket]), self.lens_s[0][:bucket]

    def _token_vector_chunks(self, rows: Sequence):
        """Yields ``(c0, m, bucket, tv [bucket * S, P] fp32, lens [bucket] int32)`` per chunk of at most ``B``
        rows; rows ``m .. bucket - 1`` are empty strings. On the GPU ``tv`` / ``lens`` are a graph's static
        outputs, valid until the next chunk: the consumer's work on them is ordered before the event after
        which the pinned rows (and the graph) are used again."""
        cuda = self.device.type == "cuda"
        free = None
        for c0 in range(0, len(rows), self.B):
            chunk = pack_rows(self._encode_rows(rows[c0:c0 + self.B]))
            m = min(self.B, len(rows) - c0)
            if not cuda:
                ids, lens = self._tokenize(torch.from_numpy(chunk[0]), torch.from_numpy(chunk[1]))
                # one row per call: the PyTorch reference's fp32 sums depend on the rows batched together,
                # and a row's vectors must not (the kernels' are batch-invariant by construction)
                tv = torch.cat([self.model.token_vectors(ids[i:i + 1], lens[i:i + 1]) for i in range(m)])
                yield c0, m, m, tv, lens
                continue
            if free is not None:
                free.synchronize()
            bk = self._stage_texts(chunk, m)
            tv, lens = self._replay(("maxsim", bk), lambda: self._token_vector_step(bk))
            yield c0, m, bk, tv, lens
            free = torch.cuda.Event()
            free.record()
        if free is not None:
            free.synchronize()  # the pinned rows are free for the next call, whichever form it is

    def _shared_index(self, Q: int, bucket: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(qidx, didx)`` int32 ``[Q * bucket]`` of every query against every row of a chunk, query-major."""
        cache = self.__dict__.setdefault("_ms_idx", {})
        if (Q, bucket) not in cache:
            if len(cache) >= 16:
                cache.clear()
            q = torch.arange(Q, dtype=torch.int32, device=self.device).repeat_interleave(bucket)
            d = torch.arange(bucket, dtype=torch.int32, device=self.device).repeat(Q)
            cache[(Q, bucket)] = (q.contiguous(), d.contiguous())
        return cache[(Q, bucket)]

    def _maxsim_queries(self, queries: Sequence) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(qv [Q, S, P] fp32, lens_q [Q] int32)`` of the queries, resident on the device; ``lens_q`` is also
        ``self.maxsim_lens_q``."""
        Q, S, P, dev = len(queries), self.S, self.late_dim, self.device
        qv = torch.empty((Q, S, P), dtype=torch.float32, device=dev)
        lens_q = torch.ones(Q, dtype=torch.int32, device=dev)
        self.maxsim_lens_q = lens_q
        for c0, m, _, tv, lens in self._token_vector_chunks(queries):
            qv[c0:c0 + m].copy_(tv.view(-1, S, P)[:m])
            lens_q[c0:c0 + m].copy_(lens[:m])
        return qv, lens_q

    def maxsim_scores(self, queries: Sequence, passages: Sequence, goff: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Late-interaction scores, fp32, left on the engine's device (a DP caller all-gathers them). With
        ``goff`` (pair form) ``[P]``: ``passages`` is the flat list of all candidates, query ``q`` owning rows
        ``goff[q] .. goff[q + 1] - 1``, as in :meth:`score_pairs`. With ``goff=None`` (shared form) ``[Q, N]``:
        every query against every passage. ``self.maxsim_lens_q`` holds the queries' token counts, ``[Q]``
        int32 on the device. A score depends on its own two texts only: not on the chunking or the form."""
        Q, N = len(queries), len(passages)
        S, P, dev = self.S, self.late_dim, self.device
        if goff is not None:
            goff = self._check_goff(goff, Q, N)
        if not ops.maxsim_ok(P):
            raise ValueError("token vectors must have a width that is a multiple of 64 in [64, 1024]")
        if Q * S * P * 4 > float(os.getenv("MAXSIM_QUERY_GB", "4")) * 2**30:
            raise ValueError("too many queries for the token-vector buffer")
        out = torch.empty((N,) if goff is not None else (Q, N), dtype=torch.float32, device=dev)
        qv, lens_q = self._maxsim_queries(queries)
        if Q == 0 or N == 0:
            return out
        cuda = dev.type == "cuda"
        if goff is not None:
            qid = np.repeat(np.arange(Q, dtype=np.int32), np.diff(np.asarray(goff, dtype=np.int64)))  # row -> query
            r = self._rerank_bufs()
            arange = torch.arange(self.B, dtype=torch.int32, device=dev)
        for c0, m, bk, tv, lens in self._token_vector_chunks(passages):
            dv = tv.view(-1, S, P)
            if goff is None:
                qidx, didx = self._shared_index(Q, bk)
                sc = ops.maxsim(qv, lens_q, dv, lens, qidx, didx)
                out[:, c0:c0 + m].copy_(sc.view(Q, bk)[:, :m])
                continue
            if cuda:  # the previous chunk's copy out of the pinned row completed before this chunk was staged
                r["pin_qidx"][:m].copy_(torch.from_numpy(qid[c0:c0 + m]))
                r["qidx"][:m].copy_(r["pin_qidx"][:m], non_blocking=True)
                qidx = r["qidx"][:m]
            else:
                qidx = torch.from_numpy(qid[c0:c0 + m].copy())
            ops.maxsim(qv, lens_q, dv, lens, qidx, arange[:m], out=out[c0:c0 + m])
        return out

    def maxsim_rank(self, queries: Sequence, passages: Sequence, goff: Optional[Sequence[int]] = None,
                    top_k: int = 10) -> RerankResult:
        """:meth:`maxsim_scores`, then :meth:`rank_scores`: each query's own passages (pair form) or all of
        them (shared form: ``goff = [0, N, 2N, ...]`` over the flattened ``[Q * N]``) ranked; ``index`` is the
        position in the query's list, or in ``passages``."""
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= ops.rerank.MAX_K:
            raise ValueError("top_k must be an int in [1, 32]")
        scores = self.maxsim_scores(queries, passages, goff)
        if goff is None:
            goff = [q * len(passages) for q in range(len(queries) + 1)]
        return self.rank_scores(scores.reshape(-1), goff, top_k)

    # ------------------------------------------- late interaction over a resident index (map_maxsim)
    # The passages' token vectors are computed once (maxsim_build: the ("maxsim", bucket) graphs in chunks,
    # the live rows of every chunk packed with plain PyTorch) and written as an index; a query call then
    # encodes only the queries and scores them against the resident rows with ops.maxsim_index: one
    # all-form launch over the rank's slice, or with per-query candidate lists one list-form launch over
    # the passage-major work list that PyTorch ops on the device build from them.
    def _check_late(self, Q: int = 0) -> None:
        if not ops.maxsim_ok(self.late_dim):
            raise ValueError("token vectors must have a width that is a multiple of 64 in [64, 1024]")
        if Q * self.S * self.late_dim * 4 > float(os.getenv("MAXSIM_QUERY_GB", "4")) * 2**30:
            raise ValueError("too many queries for the token-vector buffer")

    def maxsim_build(self, passages: Sequence) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(tok [T, P] fp32, lens [N] int32)`` on the engine's device: the unit token vectors of the live
        tokens of every passage back to back, the engine's own vectors (an index row has the bits of the
        on-the-fly path), and every passage's token count."""
        S, P, dev = self.S, self.late_dim, self.device
        self._check_late()
        pos = torch.arange(S, device=dev)
        parts, counts = [], []
        for _, m, _, tv, lens in self._token_vector_chunks(passages):
            ln = lens[:m].clamp(1, S)
            parts.append(tv.view(-1, S, P)[:m][pos[None, :] < ln[:, None]])  # a copy: the graph's output is reused
            counts.append(ln.to(torch.int32))
        if not parts:
            return torch.empty((0, P), dtype=torch.float32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev)
        return torch.cat(parts).contiguous(), torch.cat(counts).contiguous()

    def _candidate_entries(self, candidates: Sequence[Sequence[int]], index) -> Tuple[torch.Tensor, ...]:
        """The (query, passage) entries of the candidate lists that fall in the index's slice, passage-major:
        ``(pidx [M], qoff [M + 1], qsel [E], col [E])``, ``col`` the entry's position in its query's list."""
        dev = self.device
        n = [len(c) for c in candidates]
        pid = torch.tensor([int(p) for c in candidates for p in c], dtype=torch.int64).to(dev)
        qid = torch.repeat_interleave(torch.arange(len(n)), torch.tensor(n, dtype=torch.int64)).to(dev)
        col = torch.tensor([j for c in n for j in range(c)], dtype=torch.int64).to(dev)
        keep = (pid >= index.start) & (pid < index.start + index.count)
        pid, qid, col = pid[keep] - index.start, qid[keep], col[keep]
        order = torch.sort(pid, stable=True).indices  # by passage; a passage's queries in input order
        items, cnt = torch.unique_consecutive(pid[order], return_counts=True)
        qoff = torch.zeros(int(items.numel()) + 1, dtype=torch.int32, device=dev)
        qoff[1:] = torch.cumsum(cnt, 0).to(torch.int32)
        return items.to(torch.int32).contiguous(), qoff, qid[order].to(torch.int32).contiguous(), col[order]

    def maxsim_index_scores(self, queries: Sequence, index, candidates: Optional[Sequence[Sequence[int]]] = None
                            ) -> torch.Tensor:
        """Late-interaction scores of the queries against a resident index (``runtime.maxsim_index.TokenIndex``,
        a rank's slice), fp32 on the engine's device. Without ``candidates``: ``[Q, index.count]``, every query
        against every passage of the slice, one all-form launch. With ``candidates`` (one list of passage ids
        of the file per query): ``[Q, C]``, ``C`` the longest list, entry ``[q, j]`` the score of
        ``candidates[q][j]`` when that passage is in the slice and ``-inf`` when it is not (or past the list's
        end): one list-form launch. ``self.maxsim_lens_q`` as in :meth:`maxsim_scores`."""
        Q, P, dev = len(queries), self.late_dim, self.device
        self._check_late(Q)
        if int(index.tokens.shape[1]) != P:
            raise ValueError("index width is not the model's token-vector width")
        if candidates is not None and len(candidates) != Q:
            raise ValueError("candidates must be one list per query")
        qv, lens_q = self._maxsim_queries(queries)
        if candidates is None:
            if Q == 0 or index.count == 0:
                return torch.empty((Q, index.count), dtype=torch.float32, device=dev)
            return ops.maxsim_index(qv, lens_q, index.tokens, index.offsets)
        out = torch.full((Q, max([len(c) for c in candidates], default=0)), float("-inf"), dtype=torch.float32, device=dev)
        if Q == 0 or index.count == 0 or out.numel() == 0:
            return out
        pidx, qoff, qsel, col = self._candidate_entries(candidates, index)
        if qsel.numel():
            sc = ops.maxsim_index(qv, lens_q, index.tokens, index.offsets, pidx, qoff, qsel)
            out[qsel.to(torch.int64), col] = sc
        return out

    def maxsim_index_rank(self, queries: Sequence, index, candidates: Optional[Sequence[Sequence[int]]] = None,
                          top_k: int = 10) -> RerankResult:
        """:meth:`maxsim_index_scores`, then :meth:`rank_scores` (one ``group_topk`` launch, one copy back).
        Without ``candidates`` ``idx`` is the passage's position in the slice; with them its position in the
        query's candidate list (only the list's own entries are ranked; one outside the slice scores ``-inf``)."""
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= ops.rerank.MAX_K:
            raise ValueError("top_k must be an int in [1, 32]")
        scores = self.maxsim_index_scores(queries, index, candidates)
        Q, C = scores.shape
        if candidates is None or all(len(c) == C for c in candidates):
            return self.rank_scores(scores.reshape(-1), [q * C for q in range(Q + 1)], top_k)
        goff = [0]
        for c in candidates:
            goff.append(goff[-1] + len(c))
        flat = torch.cat([scores[q, :len(c)] for q, c in enumerate(candidates)])
        return self.rank_scores(flat, goff, top_k)

    # ------------------------------------------------------ zero-shot classification (map_zero_shot)
    # An NLI model reads every text with one hypothesis per candidate label as ``[CLS] text [SEP]
    # hypothesis [SEP]`` (``ops.premise_assemble``). Neither segment is one row per pair: per chunk of at
    # most B pairs the chunk's DISTINCT texts are staged and tokenized once in slot 0, its distinct
    # hypotheses in the query slot of the re-ranker, and two index rows name each pair's text and
    # hypothesis. One graph per bucket (two tokenizes, premise_assemble, model.nli_logits) and one D2D of
    # the [m, 2] logits; after the last chunk one nli_rank launch and one D2H.
    def _zero_shot_bufs(self) -> Dict[str, torch.Tensor]:
        if getattr(self, "_zs", None) is None:
            z = {"tidx": i32(self.B, device=self.device)}
            if self.device.type == "cuda":
                z["pin_tidx"] = i32(self.B, pin_memory=True)
            self._zs = z
        return self._zs

    def _zero_shot_step(self, bucket: int, mh: int, ent: int, con: int) -> torch.Tensor:
        """``(entailment, contradiction)`` logits ``[bucket, 2]`` of the staged pairs."""
        r, z = self._rerank_bufs(), self._zero_shot_bufs()
        cls_id, sep_id, pad_id = self._special_ids()
        self._tokenize(r["text_q"], r["offs_q"], ids=r["ids_q"], lens=r["lens_q"], rows=bucket)
        self._tokenize(self.text[0], self.offs[0], ids=self.ids_s[0], lens=self.lens_s[0], rows=bucket)
        ops.premise_assemble(self.ids_s[0][:bucket], self.lens_s[0][:bucket], r["ids_q"][:bucket], r["lens_q"][:bucket],
                             z["tidx"], r["qidx"], mh, cls_id, sep_id, pad_id, ids=r["ids"], type_ids=r["type_ids"],
                             lens=r["lens"], rows=bucket)
        return self.model.nli_logits(r["ids"][:bucket], r["lens"][:bucket], r["type_ids"][:bucket], ent, con)

    def _premise_chunks(self, texts: Sequence, hyps: Sequence, tid: np.ndarray, hid: np.ndarray, mh: int):
        """The chunk staging of the premise pairs ``(tid[p], hid[p])``, a sibling of :meth:`_pair_chunks`:
        yields ``(c0, m, bucket, rows)`` per chunk of at most ``B`` pairs. On the GPU the chunk's distinct
        texts go through the pinned rows into slot 0, its distinct hypotheses into the query slot, the
        pairs' local text / hypothesis indices into ``tidx`` / ``qidx`` (padding rows: text 0 with
        hypothesis 0), ``rows`` is None and the caller runs its step on ``bucket`` rows; on the CPU ``rows``
        is the assembled ``(ids, type_ids, lens)``."""
        P = int(tid.size)
        cuda = self.device.type == "cuda"
        if P == 0:
            return
        r, z = self._rerank_bufs(), self._zero_shot_bufs()
        free = None  # the event after which the pinned rows of the previous chunk may be overwritten
        for c0 in range(0, P, self.B):
            m = min(self.B, P - c0)
            used_t, local_t = np.unique(tid[c0:c0 + m], return_inverse=True)  # at most m of either
            used_h, local_h = np.unique(hid[c0:c0 + m], return_inverse=True)
            text_t, offs_t = pack_rows(self._encode_rows([texts[int(t)] for t in used_t]))
            text_h, offs_h = pack_rows(self._encode_rows([hyps[int(h)] for h in used_h]))
            local_t, local_h = local_t.astype(np.int32), local_h.astype(np.int32)
            if not cuda:
                ids_t, lens_t = self._tokenize(torch.from_numpy(text_t), torch.from_numpy(offs_t))
                ids_h, lens_h = self._tokenize(torch.from_numpy(text_h), torch.from_numpy(offs_h))
                yield c0, m, None, ops.premise_assemble(ids_t, lens_t, ids_h, lens_h, torch.from_numpy(local_t),
                                                        torch.from_numpy(local_h), mh, *self._special_ids())
                continue
            if free is not None:
                free.synchronize()
            bk, nh = self._stage_texts((text_t, offs_t), len(used_t), rows=m), len(used_h)
            r["pin_text_q"][:text_h.size].copy_(torch.from_numpy(text_h))
            r["pin_offs_q"][:nh + 1].copy_(torch.from_numpy(offs_h))
            r["pin_offs_q"][nh + 1:bk + 1].fill_(int(offs_h[-1]))
            r["pin_qidx"][:m].copy_(torch.from_numpy(local_h))
            r["pin_qidx"][m:bk].zero_()  # padding rows: text 0 with hypothesis 0, their logits dropped
            z["pin_tidx"][:m].copy_(torch.from_numpy(local_t))
            z["pin_tidx"][m:bk].zero_()
            if text_h.size:
                r["text_q"][:text_h.size].copy_(r["pin_text_q"][:text_h.size], non_blocking=True)
            r["offs_q"][:bk + 1].copy_(r["pin_offs_q"][:bk + 1], non_blocking=True)
            r["qidx"][:bk].copy_(r["pin_qidx"][:bk], non_blocking=True)
            z["tidx"][:bk].copy_(z["pin_tidx"][:bk], non_blocking=True)
            free = torch.cuda.Event()
            free.record()
            yield c0, m, bk, None
        if free is not None:
            free.synchronize()  # the pinned rows are free for the next call, whichever form it is

    def nli_ids(self, ent: Optional[int] = None, con: Optional[int] = None) -> Tuple[int, int]:
        """The checked ``(entailment, contradiction)`` label ids; None: ``(num_labels - 1, 0)``."""
        C = self.cfg.num_labels
        ent = C - 1 if ent is None else ent
        con = 0 if con is None else con
        for v in (ent, con):
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < C:
                raise ValueError("ent and con must be ints in [0, num_labels)")
        if ent == con:
            raise ValueError("ent and con must be distinct")
        return ent, con

    def score_premises(self, texts: Sequence, hyps: Sequence, ranges: Sequence[Tuple[int, int]],
                       max_hypothesis_tokens: Optional[int] = None, ent: Optional[int] = None,
                       con: Optional[int] = None) -> torch.Tensor:
        """NLI logits ``[P, 2]`` fp32 = (entailment, contradiction), left on the engine's device (a DP caller
        all-gathers them): text ``t`` is read with each of the hypotheses ``hyps[ranges[t][0]:ranges[t][1]]``,
        the pairs text-major. A pair's row is ``[CLS] text [SEP] hypothesis [SEP]`` (``ops.premise_assemble``):
        the text gives way (HF ``only_first``), the hypothesis is kept up to ``max_hypothesis_tokens``
        (default ``min(32, (S - 3) // 2)``; HF has no such cut)."""
        if len(ranges) != len(texts):
            raise ValueError("ranges must hold one (start, end) per text")
        ranges = [(int(a), int(b)) for a, b in ranges]
        if any(not 0 <= a <= b <= len(hyps) for a, b in ranges):
            raise ValueError("ranges must lie in [0, len(hyps)] with start <= end")
        if self.S < 4:
            raise ValueError("score_premises needs seq_len >= 4")
        mh = default_max_query_tokens(self.S) if max_hypothesis_tokens is None else max_hypothesis_tokens
        if isinstance(mh, bool) or not isinstance(mh, int) or mh < 0:
            raise ValueError("max_hypothesis_tokens must be an int >= 0")
        ent, con = self.nli_ids(ent, con)
        counts = np.asarray([b - a for a, b in ranges], dtype=np.int64)
        tid = np.repeat(np.arange(len(texts), dtype=np.int64), counts)
        hid = (np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in ranges]) if len(ranges)
               else np.zeros(0, dtype=np.int64))
        P = int(tid.size)
        pair = torch.empty((P, 2), dtype=torch.float32, device=self.device)
        for c0, m, bk, rows in self._premise_chunks(texts, hyps, tid, hid, mh):
            if rows is not None:
                ids, types, lens = rows
                pair[c0:c0 + m] = self.model.nli_logits(ids, lens, types, ent, con)
            else:
                out = self._replay(("zeroshot", bk, mh, ent, con), lambda: self._zero_shot_step(bk, mh, ent, con))
                pair[c0:c0 + m].copy_(out[:m])
        return pair

    def rank_labels(self, pair: torch.Tensor, goff: Sequence[int], multi_label: bool = False) -> ZeroShotResult:
        """Every text's labels scored and ranked in full from its NLI logits (``ops.nli_rank``): one launch
        and one D2H, which also brings the raw logits to the host."""
        if not isinstance(multi_label, bool):
            raise ValueError("multi_label must be a bool")
        P = int(pair.shape[0])
        T = len(goff) - 1
        goff = self._check_goff(goff, T, P)
        if P == 0 or T == 0:
            return ZeroShotResult(T, P, goff, torch.zeros(0, dtype=torch.int32), torch.zeros(0), pair.float().cpu())
        pair = pair.contiguous()
        order, score = ops.nli_rank(pair, torch.tensor(goff, dtype=torch.int32).to(pair.device), multi_label)
        both = torch.cat([order.view(torch.float32), score, pair.reshape(-1)]).cpu()  # one D2H, one sync
        return ZeroShotResult(T, P, goff, both[:P].clone().view(torch.int32), both[P:2 * P].clone(),
                              both[2 * P:].clone().view(P, 2))

    def zero_shot(self, texts: Sequence, hyps: Sequence, ranges: Sequence[Tuple[int, int]], multi_label: bool = False,
                  max_hypothesis_tokens: Optional[int] = None, ent: Optional[int] = None,
                  con: Optional[int] = None) -> ZeroShotResult:
        """:meth:`score_premises`, then :meth:`rank_labels`."""
        if not isinstance(multi_label, bool):
            raise ValueError("multi_label must be a bool")
        pair = self.score_premises(texts, hyps, ranges, max_hypothesis_tokens, ent, con)
        return self.rank_labels(pair, _offsets([b - a for a, b in ranges]), multi_label)

    def memory_bytes(self) -> int:
        """Resident device bytes: weights, the LayerNorm-folded weight copies once built
        (they are ~45 % of the encoder weights), staging and token buffers."""
        folded = getattr(self.model, "_folded", None) or {}
        folded = dict(folded, **(getattr(self.model, "_quantized", None) or {}))  # int8 weights + scales
        extra = sum(t.numel() * t.element_size() for t in folded.values())
        if self.vocab is not None and self.device.type == "cuda":
            extra += self.vocab.table_bytes  # the WordPiece table on this device
        # embed: the static [rows, H] fp32 outputs its graphs hold (nothing until the first embed call)
        egraphs = list(self._egraphs.values()) + [v for k, v in self._bgraphs.items()
                                                  if k[0] == "embed"]
        extra += sum(o.numel() * o.element_size() for _, o in egraphs)
        # rerank: its query slot, pair rows and type ids (nothing until the first rerank call)
        extra += sum(t.numel() * t.element_size() for t in (getattr(self, "_rr", None) or {}).values() if t.is_cuda)
        # answer: the [P, n] span buffers, the span head's fp32 forms and its graphs' static outputs
        extra += sum(t.numel() * t.element_size() for t in (getattr(self, "_an", None) or ()))
        extra += sum(t.numel() * t.element_size() for t in (getattr(self.model, "_span_inputs", None) or {}).values())
        extra += sum(o.numel() * o.element_size() for k, (_, outs) in self._bgraphs.items()
                     if k[0] in ("answer", "wanswer") for o in outs)
        # windowed answer: the long passage rows, the window table and the [R, n] window-row buffers
        extra += sum(t.numel() * t.element_size() for t in (getattr(self, "_wn", None) or {}).values() if t.is_cuda)
        extra += sum(t.numel() * t.element_size() for t in (getattr(self, "_wr", None) or ()))
        # zero-shot: the pairs' text index row (its other buffers are the re-ranker's)
        extra += sum(t.numel() * t.element_size() for t in (getattr(self, "_zs", None) or {}).values() if t.is_cuda)
        return (self.pack.nbytes + extra + sum(t.numel() for t in self.text)
                + sum(t.numel() * 4 for t in self.ids_s) + sum(t.numel() * 4 for t in self.offs))


def activation_bytes_per_row(cfg: BertConfig, seq_len: int) -> int:
    """Peak transient device bytes per batch row (bf16 activations, one layer live)."""
    H, I, S = cfg.hidden, cfg.intermediate, seq_len
    per_tok = 2 * (H * 4 + 3 * H + I)  # h, h1, ctx, h2 + qkv + ffn (bf16)
    return S * per_tok + DEFAULT_MAX_ROW_BYTES + 8 * S
