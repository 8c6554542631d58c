"""Device-resident model cache for accelerator ops.

MI355X counterpart of ``/root/reference/ops/_tpu_runtime.py``:

* :func:`get_model_path` keeps the reference's precedence (payload value, then
  env, then a default; ref ``:23-31``) with ``GPU_MODEL_PATH`` /
  ``CLASSIFY_MODEL`` in place of ``TPU_MODEL_PATH``.
* :func:`get_gpu_handle` replaces the single-slot, unlocked interpreter cache
  (ref ``:9-12,39-61``; switching models rebuilt it every time, SURVEY.md
  §2.4.13) with a mutex-guarded LRU of engines resident in HBM.

A "model path" is a BERT preset (``bert-base``, ``bert-large``, ``bert-tiny``),
optionally with query options ``bert-base?labels=5&seed=3&batch=512``, or a
``.safetensors`` file whose config sits next to it as ``<file>.json``.
``?vocab=/abs/vocab.txt[&lowercase=0]`` (any path) or ``"vocab": "vocab.txt"`` in
that json (relative to the model file; the query wins) gives the model a WordPiece
vocabulary: its texts are then tokenized by ``atpu-wordpiece v1`` instead of the
hash tokenizer.
``"head": "none"`` in that json marks an encoder without pooler and classifier (a plain
``BertModel`` export): the file need not hold ``pool_*`` / ``cls_*``, ``map_embed`` serves it
and ``map_classify`` refuses it. ``"head": "qa"`` marks a ``BertForQuestionAnswering`` export: the file
holds ``qa_w`` / ``qa_b`` (the span head ``map_answer`` needs), ``pool_*`` / ``cls_*`` are optional as for
``"none"``, and ``map_classify`` / ``map_rerank`` refuse it the same way. ``?qa=1`` on a preset adds a
random-init span head next to the pooler and classifier.
``"head": "token"`` marks a ``BertForTokenClassification`` export: the file holds ``tag_w`` / ``tag_b`` (the
tag head ``map_tag`` needs), the json names its labels in ``"tag_labels": [...]`` (``"outside": ["O"]`` by
default), ``pool_*`` / ``cls_*`` are optional, and ``map_classify`` / ``map_rerank`` / ``map_answer`` refuse it.
``?tags=N`` on a preset adds a random-init tag head of ``N`` labels named ``O, B-T0, I-T0, B-T1, ...``.
``"head": "mlm"`` marks a ``BertForMaskedLM`` export: the file holds ``mlm_w`` / ``mlm_b`` / ``mlm_ln_g`` /
``mlm_ln_b`` / ``mlm_out_b`` (the masked-LM head ``map_fill`` needs; the decoder is the word embeddings),
``pool_*`` / ``cls_*`` are optional, and the other head ops refuse it. ``?mlm=1`` on a preset adds a
random-init MLM head.
``"head": "late"`` with ``"late_dim": N`` marks a ColBERT export: the file holds the bias-free projection
``late_w [N, H]`` (the late-interaction head ``map_maxsim`` scores with), ``pool_*`` / ``cls_*`` are optional, and
the other head ops refuse it. ``?late=N`` (a multiple of 64) on a preset adds a random-init projection.
``?nli=1`` on a preset makes it an NLI classifier for ``map_zero_shot``: 3 labels unless ``labels=`` says otherwise,
entailment id 2 and contradiction id 0 (the MNLI order). A classifier json may name its labels in
``"nli_labels": [...]`` (one per label): the entailment id is the first name that starts with "entail", the
contradiction id the last label if that is label 0, else label 0 (HF's rule). No new weights: the NLI head is
the pooler and classifier.
Random-init weights are seeded, so every rank/host builds identical weights;
under DP rank 0 initialises and broadcasts them (RCCL).
"""
from __future__ import annotations

import json
import os
import threading
from collections import OrderedDict
from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple
from urllib.parse import parse_qs, urlsplit

DEFAULT_MODEL = "bert-base"


def get_model_path(requested: Optional[str] = None) -> str:
    return requested or os.environ.get("GPU_MODEL_PATH") or os.environ.get("CLASSIFY_MODEL") or DEFAULT_MODEL


@dataclass(frozen=True)
class ModelSpec:
    path: str
    preset: str
    labels: int
    seed: int
    batch_rows: int
    seq_len: int
    file: Optional[str] = None
    quant: Optional[str] = None  # "?quant=int8": INT8 encoder GEMMs; None: the CLASSIFY_QUANT default
    vocab: Optional[str] = None  # vocab.txt of the model: the WordPiece tokenizer; None: the hash tokenizer
    lowercase: bool = True  # uncased vocabulary: ASCII A-Z folded before matching
    head: bool = True  # False ("head": "none" in the json): an encoder without pooler / classifier (map_embed only)
    qa: bool = False  # a span head ("?qa=1", or "head": "qa" in the json, which also clears ``head``): map_answer
    tags: int = 0  # labels of a tag head ("?tags=N", or "head": "token" in the json, which clears ``head``): map_tag
    tag_names: Optional[Tuple[str, ...]] = None  # "tag_labels" of the json; None: ops.default_tag_names
    tag_outside: Tuple[str, ...] = ("O",)
    mlm: bool = False  # a masked-LM head ("?mlm=1", or "head": "mlm" in the json, which clears ``head``): map_fill
    # an NLI classifier: (entailment_id, contradiction_id) ("?nli=1": (2, 0), or "nli_labels" in the json); None:
    # map_zero_shot takes (num_labels - 1, 0) unless the payload names them
    nli: Optional[Tuple[int, int]] = None
    # the width of a late-interaction projection ("?late=N", or "head": "late" with "late_dim": N in the json,
    # which clears ``head``): map_maxsim scores with it; 0: map_maxsim takes the hidden states themselves
    late: int = 0


def _flag(value: Any) -> bool:
    if isinstance(value, str):
        return value.strip().lower() not in ("0", "false", "no", "")
    return bool(value)


def _tags(value: Any) -> int:
    n = int(value)
    if not 0 <= n <= 64:
        raise ValueError("a tag head has 1 to 64 labels")
    return n


def _late(value: Any) -> int:
    n = int(value)
    if n < 0 or n % 64 != 0 or n > 1024:
        raise ValueError("a late-interaction head has a width that is a multiple of 64, at most 1024")
    return n


def nli_ids_of(names: Any, num_labels: int, where: str) -> Tuple[int, int]:
    """``(entailment_id, contradiction_id)`` from a model's label names: the first name that starts with
    "entail" (any case) and, HF's own rule, the last label if that is label 0, else label 0."""
    if (not isinstance(names, list) or len(names) != num_labels or num_labels < 2
            or not all(isinstance(n, str) for n in names)):
        raise ValueError(f'{where}: "nli_labels" must name each of the num_labels (>= 2) labels')
    ent = next((i for i, n in enumerate(names) if n.strip().lower().startswith("entail")), None)
    if ent is None:
        raise ValueError(f'{where}: "nli_labels" has no label that starts with "entail"')
    return ent, (num_labels - 1 if ent == 0 else 0)


def parse_spec(path: str) -> ModelSpec:
    from agent_tpu_amd.models.bert import PRESETS, resolve_quant

    u = urlsplit(path)
    q = {k: v[-1] for k, v in parse_qs(u.query).items()}
    quant = resolve_quant(q["quant"]) if "quant" in q else None  # an unknown value raises ValueError
    base = u.path if u.scheme in ("", "file") else path
    seq = int(q.get("seq", os.getenv("CLASSIFY_SEQ_LEN", "128")))
    batch = int(q.get("batch", os.getenv("CLASSIFY_BATCH_ROWS", "0")) or 0)
    vocab = q.get("vocab") or None
    lowercase = _flag(q["lowercase"]) if "lowercase" in q else None
    if base in PRESETS:
        nli = _flag(q.get("nli", "0"))  # MNLI order: contradiction, neutral, entailment
        return ModelSpec(path, base, int(q.get("labels", "3" if nli else os.getenv("CLASSIFY_NUM_LABELS", "2"))),
                         int(q.get("seed", os.getenv("MODEL_SEED", "0"))), batch, seq, quant=quant,
                         vocab=vocab, lowercase=True if lowercase is None else lowercase,
                         qa=_flag(q.get("qa", "0")), tags=_tags(q.get("tags", "0")),
                         mlm=_flag(q.get("mlm", "0")), nli=(2, 0) if nli else None, late=_late(q.get("late", "0")))
    if base.endswith(".safetensors"):
        if not os.path.exists(base):
            raise FileNotFoundError(f"GPU model not found: {base}")
        with open(base + ".json") as f:
            meta = json.load(f)
        if vocab is None and meta.get("vocab"):  # the query wins over the json
            vocab = os.path.join(os.path.dirname(os.path.abspath(base)), str(meta["vocab"]))  # absolute stays
        if lowercase is None:
            lowercase = _flag(meta.get("lowercase", True))
        head = str(meta.get("head", "classifier")).strip().lower()
        names, outside = None, ("O",)
        if head == "token":
            names = meta.get("tag_labels")
            if not isinstance(names, list) or not names or not all(isinstance(n, str) for n in names):
                raise ValueError(f'{base}.json: "head": "token" needs "tag_labels": a list of label names')
            _tags(len(names))
            names = tuple(names)
            outside = tuple(str(n) for n in meta.get("outside", ["O"]))
        nli = None
        if meta.get("nli_labels") is not None:
            nli = nli_ids_of(meta["nli_labels"], int(meta.get("num_labels", 2)), base + ".json")
        late = 0
        if head == "late":
            late = _late(meta.get("late_dim", 0))
            if late <= 0:
                raise ValueError(f'{base}.json: "head": "late" needs "late_dim": a multiple of 64')
        return ModelSpec(path, meta.get("preset", DEFAULT_MODEL), int(meta.get("num_labels", 2)), 0, batch, seq,
                         file=base, quant=quant, vocab=vocab, lowercase=lowercase,
                         head=head not in ("none", "qa", "token", "mlm", "late"), qa=head == "qa",
                         tags=len(names) if names else 0, tag_names=names, tag_outside=outside, mlm=head == "mlm",
                         nli=nli, late=late)
    raise FileNotFoundError(f"GPU model not found: {path}")


class GpuHandle:
    """A loaded model: config + device engine."""

    def __init__(self, spec: ModelSpec, cfg, engine):
        self.spec = spec
        self.model_path = spec.path
        self.cfg = cfg
        self.engine = engine
        self.load_ms: Dict[str, Any] = {}  # cold-load phases (set by _build_handle)
        self.fresh = True  # built by this call (the first job reports load_ms as its cold load)


def _load_host_pack(spec: ModelSpec, cfg):
    from agent_tpu_amd.models.bert import init_random

    if spec.file:
        from safetensors.torch import load_file

        from agent_tpu_amd.models.bert import param_specs
        from agent_tpu_amd.models.params import ParamPack

        pack = ParamPack(param_specs(cfg))
        tensors = load_file(spec.file)
        # "head": "none": the file need not hold the pooler / classifier; what it lacks stays zero
        names = [n for n in pack.names() if spec.head or n in tensors or not n.startswith(("pool_", "cls_"))]
        missing = [n for n in names if n not in tensors]
        if missing:
            raise KeyError(f"{spec.file}: missing tensors {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        for name in names:
            pack[name].copy_(tensors[name])
        return pack
    return init_random(cfg, seed=spec.seed)


def _load_vocab(spec: ModelSpec, cfg):
    """The model's :class:`WordPieceVocab` with its packed table built, or None (hash tokenizer)."""
    if not spec.vocab:
        if spec.file:
            import logging

            logging.getLogger(__name__).warning(
                "%s has no vocabulary (\"vocab\" in %s.json or ?vocab=): texts are tokenized by the hash "
                "tokenizer, whose ids mean nothing to trained weights", spec.file, spec.file)
        return None
    from agent_tpu_amd.tokenizer import WordPieceVocab

    try:
        vocab = WordPieceVocab.load(spec.vocab, lowercase=spec.lowercase, vocab_size=cfg.vocab_size)
    except OSError as exc:
        raise FileNotFoundError(f"vocabulary file not readable: {spec.vocab} ({exc})") from None
    vocab.table  # built here, so a bad file fails the collective load and not the first job
    return vocab


def _build_handle(model_path: str, device) -> GpuHandle:
    """Load a model on this rank, or on every rank of the DP group together.

    Random-init specs are built on the device by every rank (``params.rand_fill``: the
    same bits everywhere, no host init, no H2D copy, no broadcast). A ``.safetensors``
    spec follows ``dp_ops.load_collectively``: rank 0 loads it on the host and copies it
    to its GPU, the other ranks allocate the destination, errors are exchanged, and only
    then does the C1 broadcast run (all ranks or none); the engine build is exchanged
    again. ``handle.load_ms`` records the phases (weights, engine).
    """
    from agent_tpu_amd.models.bert import config_for, param_specs
    from agent_tpu_amd.models.params import ParamPack
    from agent_tpu_amd.parallel.dp import broadcast_pack, is_dist, world
    from agent_tpu_amd.parallel.dp_ops import load_collectively
    from agent_tpu_amd.runtime.classify import ClassifyEngine

    import time

    from agent_tpu_amd.models.bert import init_random

    dist_on = is_dist()
    box = {"t0": time.perf_counter()}

    def sync():
        if getattr(device, "type", "cpu") == "cuda":
            import torch

            torch.cuda.synchronize(device)

    def local():
        spec = parse_spec(model_path)
        cfg = config_for(spec.preset, num_labels=spec.labels, qa_head=spec.qa, tag_labels=spec.tags,
                         mlm_head=spec.mlm, late_dim=spec.late)
        box.update(spec=spec, cfg=cfg)
        # the vocabulary is read and its table built on every rank (same file, same node: no
        # broadcast), before the weights, so a missing or bad file on any rank fails the load on all
        box["vocab"] = _load_vocab(spec, cfg)
        if not spec.file:
            return init_random(cfg, seed=spec.seed, device=device)
        if dist_on and world()[0] != 0:
            return ParamPack(param_specs(cfg), device=device)
        return _load_host_pack(spec, cfg).to(device)

    def collective(pack):
        out = broadcast_pack(pack, box["cfg"], device) if dist_on and box["spec"].file else pack
        sync()
        box["t1"] = time.perf_counter()
        return out

    def post(pack):
        spec, cfg = box["spec"], box["cfg"]
        batch = spec.batch_rows or _auto_batch_rows(spec.preset, spec.seq_len)
        eng = ClassifyEngine(cfg, pack, device, batch_rows=batch, seq_len=spec.seq_len,
                             topk=min(cfg.num_labels, 64), quant=spec.quant, vocab=box["vocab"])
        if spec.tags:
            eng.set_tag_labels(spec.tag_names, spec.tag_outside)
        sync()
        h = GpuHandle(spec, cfg, eng)
        t2 = time.perf_counter()
        h.load_ms = {"weights_ms": (box["t1"] - box["t0"]) * 1e3, "engine_ms": (t2 - box["t1"]) * 1e3,
                     "total_ms": (t2 - box["t0"]) * 1e3, "source": "file" if spec.file else "device_rand"}
        return h

    return load_collectively(local, collective, post)


def _auto_batch_rows(preset: str = "bert-base", seq_len: int = 128) -> int:
    """The engine batch of a served model: the SAME function the worker profile advertises
    (``worker_sizing.classify_batch_rows``, per model and sequence length)."""
    from worker_sizing import classify_batch_rows

    try:
        import torch

        total = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory
    except Exception:
        total = 288 * 1024 ** 3
    return classify_batch_rows(total, preset, seq_len)


_lock = threading.Lock()
_cache: "OrderedDict[Tuple[str, str], GpuHandle]" = OrderedDict()


def lru_capacity() -> int:
    return max(1, int(os.getenv("MODEL_LRU_SIZE", "4")))


def lru_budget_bytes(device) -> int:
    """HBM budget for resident models: ``MODEL_LRU_GB`` or
    25 % of the device's memory. Eviction is LRU and deterministic, so every DP
    rank (same request sequence, same configs) evicts the same models."""
    gb = os.getenv("MODEL_LRU_GB", "").strip()
    if gb:
        return int(float(gb) * 2**30)
    try:
        import torch

        return int(torch.cuda.get_device_properties(device).total_memory * 0.25)
    except Exception:
        return 64 * 2**30


def device_for_rank():
    import torch

    if os.getenv("CLASSIFY_DEVICE", "").strip().lower() == "cpu":
        return torch.device("cpu")  # fp32 PyTorch oracle path (CPU tests of the op forms)
    if not torch.cuda.is_available():
        raise RuntimeError("No ROCm GPU available (torch.cuda.is_available() is False)")
    # modulo: ranks may share a device in single-GPU rehearsals (gloo backend)
    local = int(os.getenv("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    return torch.device("cuda", local)


def get_gpu_handle(model_path: str, device=None) -> GpuHandle:
    """Cached handle for ``model_path``.

    Under a DP process group this is a collective: call it only from a
    dispatched DP task body (``dp_ops.dispatch``), where every rank asks for
    the same models in the same order. The caches of all ranks then hold the
    same keys, so they agree on hit or miss, and a miss broadcasts the
    weights from rank 0 (C1) with every rank taking part.
    """
    from agent_tpu_amd.parallel.dp import is_dist
    from agent_tpu_amd.parallel.dp_ops import in_task

    if is_dist() and not in_task():
        raise RuntimeError("get_gpu_handle under a DP process group must run inside a dispatched DP task "
                           "(dp_ops.dispatch), so that every rank loads the model together")
    device = device if device is not None else device_for_rank()
    key = (model_path, str(device))
    with _lock:
        h = _cache.get(key)
        if h is not None:
            _cache.move_to_end(key)
            return h
        h = _build_handle(model_path, device)
        _cache[key] = h
        budget = lru_budget_bytes(device)
        evicted = False
        while len(_cache) > 1 and (len(_cache) > lru_capacity() or _resident_bytes() > budget):
            _cache.popitem(last=False)
            evicted = True
        if evicted:
            import torch

            torch.cuda.empty_cache()  # hand the evicted packs/graph pools back to the device
        return h


def _resident_bytes() -> int:
    return sum(h.engine.memory_bytes() for h in _cache.values())


def cache_info() -> Dict[str, Any]:
    with _lock:
        return {"entries": [k[0] for k in _cache], "capacity": lru_capacity(), "resident_bytes": _resident_bytes()}
