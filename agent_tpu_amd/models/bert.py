"""BERT sequence classifier on the hand-written gfx950 kernels.

Replaces the reference's opaque Edge-TPU ``interpreter.invoke()``
(``/root/reference/ops/map_classify_tpu.py:71-74``) with an explicit encoder:

    ids --K2 embed+LN--> h
    repeat L: qkv = h·Wqkvᵀ+b (K3) -> ctx = attn(qkv, lens) (K4)
              h1  = LN(ctx·Woᵀ+b+h)  (K5 + K6b)
              h   = LN(gelu(h1·W1ᵀ+b1)·W2ᵀ+b2+h1)  (K6, K5 + K6b)
    pooled = tanh(h[:,0]·Wpᵀ+bp) (GEMM, tanh epilogue, strided CLS rows)
    logits/top-k = head (K7)

Parameter names/layouts mirror HF ``BertForSequenceClassification`` (Linear
weights are ``[out, in]``, exactly the GEMM's ``Bt`` operand), so
:func:`from_hf_state_dict` is a rename plus the Q/K/V concat — used by the
parity test against transformers with identical random weights.
"""
from __future__ import annotations

import dataclasses
import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from .. import ops
from .params import ParamPack, rand_fill


@dataclass(frozen=True)
class BertConfig:
    vocab_size: int = 30522
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    intermediate: int = 3072
    max_positions: int = 512
    type_vocab: int = 2
    num_labels: int = 2
    eps: float = 1e-12
    qa_head: bool = False  # a span head (HF BertForQuestionAnswering qa_outputs) after the classifier
    tag_labels: int = 0  # > 0: a token classification head of that many labels after the other heads
    mlm_head: bool = False  # a masked-LM head (HF BertForMaskedLM cls.predictions, decoder tied to emb.word) last
    late_dim: int = 0  # > 0: a bias-free late-interaction projection [late_dim, H] (ColBERT's linear) after every other head

    def __post_init__(self):
        if self.late_dim < 0 or self.late_dim % 64 != 0:
            raise ValueError("late_dim must be a multiple of 64")

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads

    def param_count(self) -> int:
        H, I, L = self.hidden, self.intermediate, self.layers
        emb = (self.vocab_size + self.max_positions + self.type_vocab) * H + 2 * H
        layer = 4 * H * H + 4 * H + 2 * H * I + I + H + 4 * H
        head = H * H + H + self.num_labels * H + self.num_labels
        if self.qa_head:
            head += 2 * H + 2
        if self.tag_labels > 0:
            head += self.tag_labels * H + self.tag_labels
        if self.mlm_head:
            head += H * H + 3 * H + self.vocab_size
        head += self.late_dim * H
        return emb + L * layer + head

    def flops_per_row_executed(self, seq_len: int, cls_only_last: bool = True,
                               cls_reassoc: Optional[bool] = None) -> float:
        """FLOPs actually executed per row when the last layer runs on [CLS] only.

        ``cls_reassoc`` (default: what :class:`BertClassifier` selects on the GPU for this
        shape): no K/V projection in that layer, but two GEMMs against the derived
        ``[heads*H, H]`` weights and the [CLS] attention over the raw rows."""
        if not cls_only_last:
            return self.flops_per_row(seq_len)
        H, I, S = self.hidden, self.intermediate, seq_len
        if cls_reassoc is None:
            cls_reassoc = (os.getenv("ATPU_CLS_REASSOC", "1") not in ("0", "false", "no")
                           and os.getenv("ATPU_LN_FOLD", "1") not in ("0", "false", "no")
                           and self.layers >= 2 and ops.cls_attend_ok(S, H, self.heads))
        full_layer = 2 * S * (4 * H * H + 2 * H * I) + 4 * S * S * H
        if cls_reassoc:
            last = 2 * (2 * self.heads * H * H) + 4 * S * self.heads * H + 2 * (2 * H * I)
        else:
            last = 2 * S * 2 * H * H + 2 * (2 * H * H + 2 * H * I) + 4 * S * H
        return self.flops_per_row(seq_len) - full_layer + last

    def flops_per_row(self, seq_len: int) -> float:
        """Forward FLOPs for one row of ``seq_len`` tokens (GEMMs + attention)."""
        H, I, L, S = self.hidden, self.intermediate, self.layers, seq_len
        gemm = 2 * S * (4 * H * H + 2 * H * I) * L
        attn = 4 * S * S * H * L
        head = 2 * (H * H + H * self.num_labels)
        return float(gemm + attn + head)


PRESETS: Dict[str, BertConfig] = {
    "bert-base": BertConfig(),
    "bert-large": BertConfig(hidden=1024, layers=24, heads=16, intermediate=4096),
    "bert-tiny": BertConfig(vocab_size=4096, hidden=256, layers=2, heads=4, intermediate=1024, max_positions=512),
}


def config_for(name: str, **overrides) -> BertConfig:
    if name not in PRESETS:
        raise ValueError(f"unknown BERT preset {name!r}; known: {sorted(PRESETS)}")
    return dataclasses.replace(PRESETS[name], **overrides)


def param_specs(cfg: BertConfig):
    H, I, C = cfg.hidden, cfg.intermediate, cfg.num_labels
    bf, f32 = torch.bfloat16, torch.float32
    yield "emb.word", (cfg.vocab_size, H), bf
    yield "emb.pos", (cfg.max_positions, H), bf
    yield "emb.type", (cfg.type_vocab, H), bf
    yield "emb.ln_g", (H,), f32
    yield "emb.ln_b", (H,), f32
    for i in range(cfg.layers):
        p = f"l{i}."
        yield p + "qkv_w", (3 * H, H), bf
        yield p + "qkv_b", (3 * H,), f32
        yield p + "o_w", (H, H), bf
        yield p + "o_b", (H,), f32
        yield p + "ln1_g", (H,), f32
        yield p + "ln1_b", (H,), f32
        yield p + "f1_w", (I, H), bf
        yield p + "f1_b", (I,), f32
        yield p + "f2_w", (H, I), bf
        yield p + "f2_b", (H,), f32
        yield p + "ln2_g", (H,), f32
        yield p + "ln2_b", (H,), f32
    yield "pool_w", (H, H), bf
    yield "pool_b", (H,), f32
    yield "cls_w", (C, H), bf
    yield "cls_b", (C,), f32
    if cfg.qa_head:
        yield "qa_w", (2, H), bf
        yield "qa_b", (2,), f32
    if cfg.tag_labels > 0:
        yield "tag_w", (cfg.tag_labels, H), bf
        yield "tag_b", (cfg.tag_labels,), f32
    if cfg.mlm_head:  # the decoder weight is emb.word (tied): no second [V, H] tensor
        yield "mlm_w", (H, H), bf
        yield "mlm_b", (H,), f32
        yield "mlm_ln_g", (H,), f32
        yield "mlm_ln_b", (H,), f32
        yield "mlm_out_b", (cfg.vocab_size,), f32
    if cfg.late_dim > 0:  # after every other head: packs without it keep their layout
        yield "late_w", (cfg.late_dim, H), bf


def init_random(cfg: BertConfig, seed: int = 0, std: float = 0.02, bias_std: float = 0.0,
                device="cpu") -> ParamPack:
    """Seeded random init, built where it will live: on a GPU by the ``rand_fill`` kernel
    (no host pass, no H2D copy), on the CPU by its native twin; the bits are the same on
    every device, host and rank (``params.rand_fill``).

    HF's BERT init scheme (N(0, 0.02)-like weights, LN γ=1/β=0, zero biases) unless
    ``bias_std`` > 0, which tests use to exercise the bias epilogues.
    """
    pack = ParamPack(param_specs(cfg), device=device)
    for name in pack.names():
        t = pack[name]
        if name.endswith("ln_g") or name.endswith("ln1_g") or name.endswith("ln2_g"):
            t.fill_(1.0)
        elif name.endswith("ln_b") or name.endswith("ln1_b") or name.endswith("ln2_b"):
            pass  # zeros
        elif name.endswith("_b"):
            if bias_std > 0:
                rand_fill(t, seed, name, bias_std)
        else:
            rand_fill(t, seed, name, std)
    return pack


def from_hf_state_dict(cfg: BertConfig, sd: Dict[str, torch.Tensor], head: str = "sequence") -> ParamPack:
    """Build a pack from a transformers ``BertForSequenceClassification`` state dict, from a
    ``BertForQuestionAnswering`` one (``qa_outputs``; no pooler, no classifier; ``cfg.qa_head``), or from
    a plain ``BertModel`` one (no ``bert.`` prefix, no classifier, the pooler optional): head
    tensors the dict does not have stay zero. ``head="token"``: a ``BertForTokenClassification`` dict
    (no pooler), whose ``classifier.*`` is the tag head (``cfg.tag_labels``), not the row classifier.
    ``head="mlm"``: a ``BertForMaskedLM`` dict (``cls.predictions.*``; ``cfg.mlm_head``); its decoder must be
    tied to the word embeddings. ``head="late"``: a ColBERT dict, a ``BertModel`` under ``bert.`` plus the
    bias-free projection ``linear.weight`` ``[late_dim, H]`` (``cfg.late_dim``)."""
    if head not in ("sequence", "token", "mlm", "late"):
        raise ValueError("head must be 'sequence', 'token', 'mlm' or 'late'")
    if head == "mlm" and not cfg.mlm_head:
        raise ValueError("head 'mlm' needs a config with mlm_head")
    if head == "late" and cfg.late_dim <= 0:
        raise ValueError("head 'late' needs a config with late_dim")
    pack = ParamPack(param_specs(cfg))
    if "embeddings.word_embeddings.weight" in sd and "bert.embeddings.word_embeddings.weight" not in sd:
        sd = {"bert." + k: v for k, v in sd.items()}

    def put(name, t):
        pack[name].copy_(t.to(pack[name].dtype).view(pack[name].shape))

    put("emb.word", sd["bert.embeddings.word_embeddings.weight"])
    put("emb.pos", sd["bert.embeddings.position_embeddings.weight"])
    put("emb.type", sd["bert.embeddings.token_type_embeddings.weight"])
    put("emb.ln_g", sd["bert.embeddings.LayerNorm.weight"])
    put("emb.ln_b", sd["bert.embeddings.LayerNorm.bias"])
    for i in range(cfg.layers):
        b = f"bert.encoder.layer.{i}."
        a = b + "attention."
        put(f"l{i}.qkv_w", torch.cat([sd[a + f"self.{n}.weight"] for n in ("query", "key", "value")], 0))
        put(f"l{i}.qkv_b", torch.cat([sd[a + f"self.{n}.bias"] for n in ("query", "key", "value")], 0))
        put(f"l{i}.o_w", sd[a + "output.dense.weight"])
        put(f"l{i}.o_b", sd[a + "output.dense.bias"])
        put(f"l{i}.ln1_g", sd[a + "output.LayerNorm.weight"])
        put(f"l{i}.ln1_b", sd[a + "output.LayerNorm.bias"])
        put(f"l{i}.f1_w", sd[b + "intermediate.dense.weight"])
        put(f"l{i}.f1_b", sd[b + "intermediate.dense.bias"])
        put(f"l{i}.f2_w", sd[b + "output.dense.weight"])
        put(f"l{i}.f2_b", sd[b + "output.dense.bias"])
        put(f"l{i}.ln2_g", sd[b + "output.LayerNorm.weight"])
        put(f"l{i}.ln2_b", sd[b + "output.LayerNorm.bias"])
    cls = ("tag_w", "tag_b") if head == "token" else ("cls_w", "cls_b")
    for name, key in (("pool_w", "bert.pooler.dense.weight"), ("pool_b", "bert.pooler.dense.bias"),
                      (cls[0], "classifier.weight"), (cls[1], "classifier.bias"),
                      ("qa_w", "qa_outputs.weight"), ("qa_b", "qa_outputs.bias")):
        if key in sd and name in pack:
            put(name, sd[key])
    if head == "mlm":
        dec = sd.get("cls.predictions.decoder.weight")
        if dec is not None and not torch.equal(dec, sd["bert.embeddings.word_embeddings.weight"]):
            raise ValueError("untied MLM decoder: cls.predictions.decoder.weight differs from the word embeddings")
        c = "cls.predictions."
        put("mlm_w", sd[c + "transform.dense.weight"])
        put("mlm_b", sd[c + "transform.dense.bias"])
        put("mlm_ln_g", sd[c + "transform.LayerNorm.weight"])
        put("mlm_ln_b", sd[c + "transform.LayerNorm.bias"])
        put("mlm_out_b", sd[c + "bias"])
    if head == "late":
        put("late_w", sd["linear.weight"])
    return pack


def resolve_quant(quant: Optional[str]) -> str:
    """Canonical quantisation mode, ``"none"`` or ``"int8"``; ``None`` reads env ``CLASSIFY_QUANT``
    (unset, ``""`` or ``none``: off)."""
    v = os.getenv("CLASSIFY_QUANT", "") if quant is None else quant
    v = str(v).strip().lower()
    if v in ("", "none"):
        return "none"
    if v == "int8":
        return "int8"
    raise ValueError(f"unknown quant {v!r}; known: none, int8")


class BertClassifier:
    """Encoder + pooler + classifier over a :class:`ParamPack`.

    ``params`` may live on a ROCm device (native kernels) or on the CPU (the
    PyTorch reference path of every op; pass ``fp32=True`` for an fp32 oracle).

    ``quant="int8"`` (default: env ``CLASSIFY_QUANT``): the encoder GEMMs over all ``B*S`` rows (QKV,
    out-projection, FFN1, FFN2, the K/V projection of a [CLS]-only last layer) run W8A8 on the i8
    MFMA (``ops/linear_i8.py``: per-row activation scales, per-output-channel weight scales), on
    the unfolded encoder structure; everything else stays bf16.
    """

    def __init__(self, cfg: BertConfig, pack: ParamPack, fp32: bool = False, cls_only_last: Optional[bool] = None,
                 quant: Optional[str] = None):
        self.cfg = cfg
        self.quant: Optional[str] = "int8" if resolve_quant(quant) == "int8" else None
        self._quantized: Optional[Dict[str, torch.Tensor]] = None
        self.pack = pack
        self.p = pack.with_dtype(torch.float32) if fp32 else {n: pack[n] for n in pack.names()}
        self.device = pack.buffer.device
        # The classifier reads only the [CLS] row of the last layer (pooler on
        # h[:, 0]). So in that layer only K/V need every token; Q, attention
        # output, O-proj, LN and the FFN run on the B [CLS] rows. The logits are
        # those of the full computation; only dead rows are skipped.
        if cls_only_last is None:
            cls_only_last = os.getenv("ATPU_CLS_ONLY_LAST", "1") not in ("0", "false", "no")
        self.cls_only_last = bool(cls_only_last)
        # LayerNorm folding (GPU): no LayerNorm pass inside the encoder; see encode_folded
        self.ln_fold = (self.device.type == "cuda" and not fp32
                        and os.getenv("ATPU_LN_FOLD", "1") not in ("0", "false", "no"))
        self._folded: Optional[Dict[str, torch.Tensor]] = None
        # activations between the folded encoder's GEMMs in K-tile image order (ops.to_image_order):
        # ATPU_ACT_LAYOUT=1 the FFN intermediate, 2 also the attention context, 3 also the hidden
        # states between full layers (layer 0's input and the last full layer's output stay
        # row-major); 4 (default) the FFN intermediate and those hidden states in fragment order
        # instead (ops.to_fragment_order; the context stays in image order); 0 everything
        # row-major. Logits are bit-identical at every level.
        self.act_layout = int(os.getenv("ATPU_ACT_LAYOUT", "4") or 0)
        # QKV projection + attention fused into one kernel (S = 128, LN-folded encoder):
        # ATPU_QKV_ATTN=0 runs the QKV GEMM and the packed attention kernel separately
        self.fused_qkv_attention = os.getenv("ATPU_QKV_ATTN", "1") not in ("0", "false", "no")
        # [CLS]-only last layer (S = 128, LN-folded encoder) without the all-token K/V projection:
        # the projection re-associated onto the query and the out-projection (ops/cls_attend.py);
        # ATPU_CLS_REASSOC=0 projects K/V for every token and runs _cls_layer
        self.cls_reassoc = (self.ln_fold and os.getenv("ATPU_CLS_REASSOC", "1") not in ("0", "false", "no")
                            and ops.cls_attend_ok(128, cfg.hidden, cfg.heads))
        # mean-pooled embeddings on the folded encoder: the last LayerNorm applied to the pooled
        # vector by pool_embed (ops/pool.py); ATPU_EMBED_FUSED=0 finishes every row with
        # ops.layernorm and pools the normalised rows
        self.embed_fused = os.getenv("ATPU_EMBED_FUSED", "1") not in ("0", "false", "no")
        # answer spans on the folded encoder: the last LayerNorm folded into the span head by
        # span_topk (ops/span.py); ATPU_ANSWER_FUSED=0 finishes every row with ops.layernorm and
        # runs the same kernel on the normalised rows
        self.answer_fused = os.getenv("ATPU_ANSWER_FUSED", "1") not in ("0", "false", "no")
        self._span_inputs: Optional[Dict[str, torch.Tensor]] = None
        # token labels on the folded encoder: the last LayerNorm folded into the tag head by
        # tag_entities (ops/tag.py); ATPU_TAG_FUSED=0 finishes every row with ops.layernorm and
        # runs the same kernel on the normalised rows
        self.tag_fused = os.getenv("ATPU_TAG_FUSED", "1") not in ("0", "false", "no")
        self._tag_inputs: Optional[Dict[str, torch.Tensor]] = None
        # mask predictions on the folded encoder: the last LayerNorm applied to the gathered mask
        # rows only by mask_gather (ops/fill.py); ATPU_FILL_FUSED=0 finishes every row with
        # ops.layernorm and gathers the normalised rows
        self.fill_fused = os.getenv("ATPU_FILL_FUSED", "1") not in ("0", "false", "no")
        self._fill_inputs: Optional[Dict[str, torch.Tensor]] = None

    # ------------------------------------------------------------ LN folding
    def folded(self) -> Dict[str, torch.Tensor]:
        """Weights with the preceding LayerNorm folded in (built once, on the device).

        QKV of layer i >= 1 consumes LN2 of layer i-1 and FFN1 of layer i consumes LN1
        of layer i: gamma goes into the weight, beta into the bias, plus the weight's
        column sums (:func:`ops.fold_ln_into_linear`). The out-proj / FFN2 residual is
        the same LayerNorm's output: its beta is added to their bias.
        """
        if self._folded is None:
            p, f = self.p, {}
            for i in range(self.cfg.layers):
                q = f"l{i}."
                if i > 0:
                    g2, b2 = p[f"l{i - 1}.ln2_g"], p[f"l{i - 1}.ln2_b"]
                    f[q + "qkv_w"], f[q + "qkv_c"], f[q + "qkv_b"] = ops.fold_ln_into_linear(
                        p[q + "qkv_w"], p[q + "qkv_b"], g2, b2)
                    f[q + "o_b"] = (p[q + "o_b"] + b2).contiguous()
                f[q + "f1_w"], f[q + "f1_c"], f[q + "f1_b"] = ops.fold_ln_into_linear(
                    p[q + "f1_w"], p[q + "f1_b"], p[q + "ln1_g"], p[q + "ln1_b"])
                f[q + "f2_b"] = (p[q + "f2_b"] + p[q + "ln1_b"]).contiguous()
                # head-ordered copies for the fused QKV + attention kernel ([h][Q|K|V] rows)
                perm = ops.qkv_head_order(self.cfg.heads, self.device)
                src = f if i > 0 else p
                f[q + "qkv_wh"] = src[q + "qkv_w"][perm].contiguous()
                f[q + "qkv_bh"] = src[q + "qkv_b"][perm].float().contiguous()
                if i > 0:
                    f[q + "qkv_ch"] = f[q + "qkv_c"][perm].contiguous()
            if self.cls_reassoc and self.cfg.layers >= 2:
                q, ln2 = f"l{self.cfg.layers - 1}.", f"l{self.cfg.layers - 2}."
                f.update(ops.cls_reassoc_weights(p[q + "qkv_w"], p[q + "qkv_b"], p[q + "o_w"], p[q + "o_b"],
                                                 p[ln2 + "ln2_g"], p[ln2 + "ln2_b"], self.cfg.heads))
            self._folded = f
        return self._folded

    def can_fold(self, B: int, S: int) -> bool:
        M, H, I = B * S, self.cfg.hidden, self.cfg.intermediate
        if self.quant:  # the int8 GEMM has no LayerNorm-folding epilogues: the unfolded structure
            return False
        return (self.ln_fold and self.cfg.layers >= 2 and ops.fold_ok(M, 3 * H, H) and ops.fold_ok(M, I, H)
                and ops.fold_ok(M, H, I))

    def encode_folded(self, ids: torch.Tensor, lens: torch.Tensor, type_ids: Optional[torch.Tensor] = None,
                      cls_only_last: bool = False, raw: bool = False):
        """:meth:`encode` with every encoder LayerNorm folded into the GEMMs around it.

        The post-LN residual stream stays raw (pre-LN sums). The out-proj / FFN2
        epilogues emit per-row partial (sum, sumsq) of their output; a finalize pass
        turns them into (rstd, rstd*mu), which FFN1 / the next QKV apply to the
        folded weights' product and FFN2 / the next out-proj apply to their residual.
        Removes 2 LayerNorm passes per layer (each a full read + write of the hidden
        states); the logits match the unfolded encoder to bf16 rounding.

        ``raw`` (all layers in full only): skip the final LayerNorm and return ``(g, fin, name)``,
        the last layer's raw rows ``[B*S, H]``, their ``(rstd, rstd*mu)`` and the parameter prefix
        of the LayerNorm that would finish them (``p[name + "ln2_g"]`` / ``"ln2_b"``)."""
        cfg, p, f = self.cfg, self.p, self.folded()
        B, S = ids.shape
        H, M, eps = cfg.hidden, B * S, cfg.eps
        dev = ids.device
        h0 = ops.embed_layernorm(ids, p["emb.word"], p["emb.pos"], p["emb.type"], p["emb.ln_g"], p["emb.ln_b"],
                                 eps, type_ids=type_ids)
        part = torch.empty((H // 256, M, 2), dtype=torch.float32, device=dev)  # raw rows' partials
        fin = torch.empty((M, 2), dtype=torch.float32, device=dev)             # (rstd, rstd*mu)
        last_full = cfg.layers - 1 if cls_only_last else cfg.layers
        fused = self.fused_qkv_attention and ops.qkv_attention_ok(M, 3 * H, H, S) and cfg.head_dim == 64
        g = h0
        # which tensors lie in K-tile image order (ops.to_image_order; see __init__): the FFN
        # intermediate, the attention context, the hidden states a / g between full layers
        lvl = self.act_layout if dev.type == "cuda" and ops.image_order_ok() else 0
        ffn_i, ctx_i, hid_i = lvl >= 1, lvl >= 2 and fused, lvl >= 3 and fused
        # level 4: a, the FFN intermediate and g between full layers in fragment order
        # (ops.to_fragment_order: written and read without an LDS transpose); the attention
        # context (written by the attention epilogue) stays in image order
        frag = lvl >= 4 and fused
        # per tensor: 0 row-major, 1 image order, 2 fragment order
        ffn_o, ctx_o, hid_o = ffn_i * (2 if frag else 1), int(ctx_i), hid_i * (2 if frag else 1)

        def lay(a=0, c=0, r=0):
            return ((0, ops.LAYOUT_A, ops.LAYOUT_A_FRAG)[a] | (0, ops.LAYOUT_C, ops.LAYOUT_C_FRAG)[c]
                    | (0, ops.LAYOUT_R, ops.LAYOUT_R_FRAG)[r])

        for i in range(last_full):
            q = f"l{i}."
            if fused:
                # QKV projection + attention in one kernel: the [M, 3H] QKV tensor never exists
                ctx = ops.qkv_attention(g, f[q + "qkv_wh"], f[q + "qkv_bh"], lens, cfg.heads,
                                        in_fin=fin if i > 0 else None, colsum_h=f.get(q + "qkv_ch") if i > 0 else None,
                                        layout=lay(a=hid_o if i > 0 else 0, c=ctx_o))
            else:
                if i == 0:
                    qkv = ops.linear(h0, p[q + "qkv_w"], p[q + "qkv_b"])
                else:  # consumes LN2_{i-1}(g); fin = its statistics (also the out-proj residual's)
                    qkv = ops.linear_ln(g, f[q + "qkv_w"], f[q + "qkv_b"], in_fin=fin, colsum=f[q + "qkv_c"])
                ctx = ops.attention_packed(qkv, lens, B, S, cfg.heads)
            if i == 0:  # the residual h0 is row-major
                a = ops.linear_ln(ctx, p[q + "o_w"], p[q + "o_b"], residual=h0, part_out=part,
                                  layout=lay(a=ctx_o, c=hid_o))
            else:
                a = ops.linear_ln(ctx, p[q + "o_w"], f[q + "o_b"], residual=g, res_fin=fin,
                                  res_gamma=p[f"l{i - 1}.ln2_g"], part_out=part,
                                  layout=lay(a=ctx_o, c=hid_o, r=hid_o))
            ops.ln_finalize(part, H, eps, out=fin)  # LN1 statistics of a
            ff = ops.linear_ln(a, f[q + "f1_w"], f[q + "f1_b"], act="gelu", in_fin=fin, colsum=f[q + "f1_c"],
                               layout=lay(a=hid_o, c=ffn_o))
            g = ops.linear_ln(ff, p[q + "f2_w"], f[q + "f2_b"], residual=a, res_fin=fin,
                              res_gamma=p[q + "ln1_g"], part_out=part,
                              layout=lay(a=ffn_o, c=hid_o if i + 1 < last_full else 0, r=hid_o))  # last g: row-major
            ops.ln_finalize(part, H, eps, out=fin)  # LN2 statistics of g
        ln2 = f"l{last_full - 1}."
        if raw:
            assert not cls_only_last, "encode_folded: raw rows are those of the full last layer"
            return g, fin, ln2
        if not cls_only_last:
            return ops.layernorm(g, p[ln2 + "ln2_g"], p[ln2 + "ln2_b"], eps)
        # last layer on the [CLS] rows (see encode): K/V over every token from the raw g
        q = f"l{cfg.layers - 1}."
        h_cls = ops.layernorm(g.view(B, S, H)[:, 0, :].contiguous(), p[ln2 + "ln2_g"], p[ln2 + "ln2_b"], eps)
        if self.cls_reassoc and S == 128 and "cls_wu" in f:
            # no K/V projection: one projected query per head against the raw rows, the value
            # and out-projection as one GEMM over the [B, heads*H] context (ops/cls_attend.py)
            u = ops.linear(h_cls, f["cls_wu"], f["cls_bu"])
            z = ops.cls_attend(g, fin, u, lens, cfg.heads)
            h1 = ops.linear(z, f["cls_wz"], f["cls_bz"], residual=h_cls)
            return self._cls_ffn(h1)
        kv = ops.linear_ln(g, f[q + "qkv_w"][H:], f[q + "qkv_b"][H:], in_fin=fin, colsum=f[q + "qkv_c"][H:])
        return self._cls_layer(h_cls, kv, lens, B, S)

    def _cls_layer(self, h_cls: torch.Tensor, kv: torch.Tensor, lens: torch.Tensor, B: int, S: int) -> torch.Tensor:
        """Last encoder layer on the [CLS] rows given their input and every token's K/V."""
        cfg, p, H = self.cfg, self.p, self.cfg.hidden
        q = f"l{cfg.layers - 1}."
        qc = ops.linear(h_cls, p[q + "qkv_w"][:H], p[q + "qkv_b"][:H])
        ctx = ops.decode_attention(qc, kv[:, :H], kv[:, H:], cfg.heads, S, 1, lens=lens,
                                   scale=1.0 / math.sqrt(cfg.head_dim))
        h1 = ops.linear(ctx, p[q + "o_w"], p[q + "o_b"], residual=h_cls.contiguous())
        return self._cls_ffn(h1)

    def _cls_ffn(self, h1: torch.Tensor) -> torch.Tensor:
        """LN1, FFN and LN2 of the last layer on the [CLS] rows' attention output + residual."""
        cfg, p = self.cfg, self.p
        q = f"l{cfg.layers - 1}."
        h1 = ops.layernorm(h1, p[q + "ln1_g"], p[q + "ln1_b"], cfg.eps)
        f = ops.linear(h1, p[q + "f1_w"], p[q + "f1_b"], act="gelu")
        h2 = ops.linear(f, p[q + "f2_w"], p[q + "f2_b"], residual=h1)
        return ops.layernorm(h2, p[q + "ln2_g"], p[q + "ln2_b"], cfg.eps)

    # ------------------------------------------------------------ INT8 encoder GEMMs
    _QUANT_WEIGHTS = ("qkv", "o", "f1", "f2")

    def quantized(self) -> Dict[str, torch.Tensor]:
        """Per-output-channel int8 weights ``l{i}.{w}_q`` and fp32 scales ``l{i}.{w}_s`` of the encoder
        GEMMs (built once, where the weights live, by the row quantiser the activations use)."""
        if self._quantized is None:
            z = {}
            for i in range(self.cfg.layers):
                for w in self._QUANT_WEIGHTS:
                    n = f"l{i}.{w}"
                    z[n + "_q"], z[n + "_s"] = ops.quantize_rows_i8(self.p[n + "_w"])
            self._quantized = z
        return self._quantized

    def _lin8(self, x: torch.Tensor, xq, name: str, rows: slice = slice(None), act: Optional[str] = None,
              residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``ops.linear`` of ``x`` against weight ``name`` (its output rows ``rows``) on the int8 GEMM;
        ``xq``: the ``(q, scale)`` of ``x`` when a producer already made it. A shape the int8 GEMM
        does not take stays on the bf16 GEMM."""
        z, p = self.quantized(), self.p
        wq, ws, b = z[name + "_q"][rows], z[name + "_s"][rows], p[name + "_b"][rows]
        if not ops.linear_i8_ok(x.shape[0], wq.shape[0], wq.shape[1]):
            return ops.linear(x, p[name + "_w"][rows], b, act=act, residual=residual)
        q, s = xq if xq is not None else ops.quantize_rows_i8(x)
        return ops.linear_i8(q, s, wq, ws, b, act=act, residual=residual, out_dtype=x.dtype)

    def encode_int8(self, ids: torch.Tensor, lens: torch.Tensor, type_ids: Optional[torch.Tensor] = None,
                    cls_only_last: bool = False) -> torch.Tensor:
        """:meth:`encode` (the unfolded structure) with the all-token GEMMs on the int8 GEMM. Each
        LayerNorm also emits the quantised rows its consumer GEMM reads (one pass)."""
        cfg, p = self.cfg, self.p
        B, S = ids.shape
        H = cfg.hidden
        h = ops.embed_layernorm(ids, p["emb.word"], p["emb.pos"], p["emb.type"], p["emb.ln_g"], p["emb.ln_b"],
                                cfg.eps, type_ids=type_ids)
        hq = None
        last_full = cfg.layers - 1 if cls_only_last else cfg.layers
        for i in range(last_full):
            q = f"l{i}."
            qkv = self._lin8(h, hq, q + "qkv")
            ctx = ops.attention_packed(qkv, lens, B, S, cfg.heads)
            h1 = self._lin8(ctx, None, q + "o", residual=h)
            h1, *h1q = ops.layernorm_quant_i8(h1, p[q + "ln1_g"], p[q + "ln1_b"], cfg.eps)
            f = self._lin8(h1, h1q, q + "f1", act="gelu")
            h2 = self._lin8(f, None, q + "f2", residual=h1)
            h, *hq = ops.layernorm_quant_i8(h2, p[q + "ln2_g"], p[q + "ln2_b"], cfg.eps)
        if not cls_only_last:
            return h
        q = f"l{cfg.layers - 1}."
        kv = self._lin8(h, hq, q + "qkv", rows=slice(H, None))
        h_cls = h.view(B, S, H)[:, 0, :]  # strided view: row stride S*H
        return self._cls_layer(h_cls, kv, lens, B, S)

    def encode(self, ids: torch.Tensor, lens: torch.Tensor, type_ids: Optional[torch.Tensor] = None,
               cls_only_last: bool = False) -> torch.Tensor:
        """Hidden states ``[B*S, H]``, or ``[B, H]`` [CLS] states with ``cls_only_last``."""
        cfg, p = self.cfg, self.p
        B, S = ids.shape
        if self.quant:
            return self.encode_int8(ids, lens, type_ids, cls_only_last)
        if ids.is_cuda and self.can_fold(B, S):
            return self.encode_folded(ids, lens, type_ids, cls_only_last)
        H = cfg.hidden
        h = ops.embed_layernorm(ids, p["emb.word"], p["emb.pos"], p["emb.type"], p["emb.ln_g"], p["emb.ln_b"],
                                cfg.eps, type_ids=type_ids)
        last_full = cfg.layers - 1 if cls_only_last else cfg.layers
        for i in range(last_full):
            q = f"l{i}."
            qkv = ops.linear(h, p[q + "qkv_w"], p[q + "qkv_b"])
            ctx = ops.attention_packed(qkv, lens, B, S, cfg.heads)
            h1 = ops.linear(ctx, p[q + "o_w"], p[q + "o_b"], residual=h)
            h1 = ops.layernorm(h1, p[q + "ln1_g"], p[q + "ln1_b"], cfg.eps)
            f = ops.linear(h1, p[q + "f1_w"], p[q + "f1_b"], act="gelu")
            h2 = ops.linear(f, p[q + "f2_w"], p[q + "f2_b"], residual=h1)
            h = ops.layernorm(h2, p[q + "ln2_g"], p[q + "ln2_b"], cfg.eps)
        if not cls_only_last:
            return h
        # last layer on the [CLS] rows: K/V GEMM over every token (rows H..3H of
        # the fused weight), Q GEMM over the B [CLS] rows, single-query attention
        q = f"l{cfg.layers - 1}."
        kv = ops.linear(h, p[q + "qkv_w"][H:], p[q + "qkv_b"][H:])
        h_cls = h.view(B, S, H)[:, 0, :]  # strided view: row stride S*H
        return self._cls_layer(h_cls, kv, lens, B, S)

    def pooled(self, h: torch.Tensor, B: int, S: int) -> torch.Tensor:
        cls_rows = h if h.shape[0] == B else h.view(B, S, self.cfg.hidden)[:, 0, :]  # strided: row stride S*H
        return ops.linear(cls_rows, self.p["pool_w"], self.p["pool_b"], act="tanh")

    def encoder(self, ids: torch.Tensor, lens: torch.Tensor,
                type_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The encoder stage of :meth:`forward` ([CLS] states when the last layer is pruned)."""
        return self.encode(ids, lens, type_ids, cls_only_last=self.cls_only_last and ids.shape[1] > 1)

    def embed(self, ids: torch.Tensor, lens: torch.Tensor, pooling: str = "mean", normalize: bool = True,
              type_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Sentence embeddings ``[B, H]`` fp32: the mean of the last hidden states over the real
        tokens (``pooling="mean"``) or the [CLS] state (``"cls"``), L2-normalised with ``normalize``.

        ``mean`` runs every layer in full; on the folded encoder the final LayerNorm is not run
        over the rows but applied to the pooled vector (:func:`ops.pool_embed` with ``fin``).
        ``cls`` takes :meth:`encoder`'s output (the pruned, re-associated last layer)."""
        if pooling not in ("mean", "cls"):
            raise ValueError("pooling must be 'mean' or 'cls'")
        B, S = ids.shape
        p = self.p
        if pooling == "cls":
            h = self.encoder(ids, lens, type_ids)  # [B, H] [CLS] states, or every row [B*S, H]
            return ops.pool_embed(h.contiguous(), lens, B, mode="cls", normalize=normalize)
        if ids.is_cuda and self.embed_fused and self.can_fold(B, S):
            g, fin, ln2 = self.encode_folded(ids, lens, type_ids, raw=True)
            return ops.pool_embed(g, lens, B, fin=fin, gamma=p[ln2 + "ln2_g"], beta=p[ln2 + "ln2_b"],
                                  normalize=normalize)
        h = self.encode(ids, lens, type_ids, cls_only_last=False)
        return ops.pool_embed(h, lens, B, normalize=normalize)

    # ------------------------------------------------------------ late interaction
    def token_vectors(self, ids: torch.Tensor, lens: torch.Tensor, type_ids: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Unit token vectors ``[B*S, P]`` fp32 for late-interaction scoring (``ops.maxsim``): the last hidden
        states (every layer in full, the final LayerNorm applied), through the bias-free ``late_w``
        projection when the model has one (``P = late_dim``, else ``P = H``), every row L2-normalised by
        ``ops.token_unit``. Rows of padding positions are normalised like any other; ``maxsim`` ignores them."""
        h = self.encode(ids, lens, type_ids, cls_only_last=False)
        if self.cfg.late_dim > 0:
            h = ops.linear(h, self.p["late_w"], out_f32=True)
        return ops.token_unit(h.contiguous(), out=out)

    # ------------------------------------------------------------ question answering
    def span_inputs(self) -> Dict[str, torch.Tensor]:
        """The span head as ``ops.span_topk`` takes it (fp32, built once, on the device). Fused with the
        last layer's LayerNorm: ``u [2, H] = ln2_g * qa_w``, ``su [2]`` = the row sums of ``u`` and
        ``c [2] = ln2_b . qa_w + qa_b``, both accumulated in fp64 and rounded once. Unfused: ``w`` =
        ``qa_w`` as fp32, ``z`` = zeros, ``b`` = ``qa_b``."""
        if not self.cfg.qa_head:
            raise ValueError("model has no QA head")
        if self._span_inputs is None:
            p = self.p
            ln2 = f"l{self.cfg.layers - 1}."
            w = p["qa_w"].float().contiguous()
            b = p["qa_b"].float().contiguous()
            u = (p[ln2 + "ln2_g"].float().view(1, -1) * w).contiguous()
            su = u.double().sum(1).float().contiguous()
            c = ((p[ln2 + "ln2_b"].double().view(1, -1) * w.double()).sum(1) + b.double()).float().contiguous()
            self._span_inputs = {"u": u, "su": su, "c": c, "w": w, "z": torch.zeros_like(b), "b": b}
        return self._span_inputs

    def spans(self, ids: torch.Tensor, lens: torch.Tensor, type_ids: torch.Tensor, max_answer_tokens: int,
              n_best: int, logits_out: Optional[torch.Tensor] = None, own: Optional[torch.Tensor] = None
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Answer spans of pair rows (``ops.pair_assemble``): ``(span [B, n_best, 2] int32 passage-relative
        token spans, score [B, n_best] fp32, null [B] fp32)`` of :func:`ops.span_topk`; ``logits_out
        [B, S, 2]`` fp32, when given, receives the start / end logits; ``own [B, 2]`` int32, when given
        (window rows, ``ops.window_assemble``), restricts every row's span starts to the range it owns.

        Every layer runs in full. On the folded encoder the final LayerNorm is not run over the rows
        but folded into the span head (``span_topk`` with ``fin``)."""
        B, S = ids.shape
        si = self.span_inputs()
        if ids.is_cuda and self.answer_fused and self.can_fold(B, S):
            g, fin, _ = self.encode_folded(ids, lens, type_ids, raw=True)
            return ops.span_topk(g, lens, type_ids, B, si["u"], si["su"], si["c"], max_answer_tokens, n_best,
                                 fin=fin, logits_out=logits_out, own=own)
        h = self.encode(ids, lens, type_ids, cls_only_last=False)
        return ops.span_topk(h, lens, type_ids, B, si["w"], si["z"], si["b"], max_answer_tokens, n_best,
                             logits_out=logits_out, own=own)

    # ------------------------------------------------------------ token classification
    def tag_inputs(self) -> Dict[str, torch.Tensor]:
        """The tag head as ``ops.tag_entities`` takes it (fp32, built once, on the device; build it
        outside graph capture). Fused with the last layer's LayerNorm: ``u [T, H] = ln2_g * tag_w``,
        ``su [T]`` = the row sums of ``u`` and ``c [T] = ln2_b . tag_w + tag_b``, both accumulated in fp64
        and rounded once. Unfused: ``w`` = ``tag_w`` as fp32, ``b`` = ``tag_b``."""
        if self.cfg.tag_labels <= 0:
            raise ValueError("model has no tag head")
        if self._tag_inputs is None:
            p = self.p
            ln2 = f"l{self.cfg.layers - 1}."
            w = p["tag_w"].float().contiguous()
            b = p["tag_b"].float().contiguous()
            u = (p[ln2 + "ln2_g"].float().view(1, -1) * w).contiguous()
            su = u.double().sum(1).float().contiguous()
            c = ((p[ln2 + "ln2_b"].double().view(1, -1) * w.double()).sum(1) + b.double()).float().contiguous()
            self._tag_inputs = {"u": u, "su": su, "c": c, "w": w, "b": b}
        return self._tag_inputs

    def tags(self, ids: torch.Tensor, lens: torch.Tensor, label_type: torch.Tensor, label_begin: torch.Tensor,
             mode: int, max_entities: int, type_ids: Optional[torch.Tensor] = None,
             cont: Optional[torch.Tensor] = None, **outs) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Entities of single-segment rows ``[CLS] text [SEP]``: ``(ent [B, E, 4] int32, ent_sum [B, E]
        fp32, count [B] int32)`` of :func:`ops.tag_entities` (``mode`` 0 / 1 / 2 = tokens / simple / first;
        mode 2 needs the vocabulary's continuation table ``cont``). ``outs``: the kernel's optional
        outputs (``ent``, ``ent_sum``, ``count``, ``label_out``, ``prob_out``, ``logits_out``).

        Every layer runs in full. On the folded encoder the final LayerNorm is not run over the rows
        but folded into the tag head (``tag_entities`` with ``fin``)."""
        B, S = ids.shape
        ti = self.tag_inputs()
        if ids.is_cuda and self.tag_fused and self.can_fold(B, S):
            g, fin, _ = self.encode_folded(ids, lens, type_ids, raw=True)
            return ops.tag_entities(g, lens, B, S, ti["u"], ti["su"], ti["c"], label_type, label_begin, mode,
                                    max_entities, fin=fin, ids=ids, cont=cont, **outs)
        h = self.encode(ids, lens, type_ids, cls_only_last=False)
        return ops.tag_entities(h, lens, B, S, ti["w"], None, ti["b"], label_type, label_begin, mode, max_entities,
                                ids=ids, cont=cont, **outs)

    # ------------------------------------------------------------ masked-token prediction
    def fill_inputs(self) -> Dict[str, torch.Tensor]:
        """The MLM head as :meth:`fills` takes it (built once, on the device; build it outside graph
        capture): ``E`` = ``emb.word`` (the tied decoder), ``bias`` = ``mlm_out_b`` and the last layer's
        ``gamma`` / ``beta``."""
        if not self.cfg.mlm_head:
            raise ValueError("model has no MLM head")
        if self._fill_inputs is None:
            p = self.p
            ln2 = f"l{self.cfg.layers - 1}."
            self._fill_inputs = {"E": p["emb.word"].contiguous(), "bias": p["mlm_out_b"].float().contiguous(),
                                 "gamma": p[ln2 + "ln2_g"].float().contiguous(),
                                 "beta": p[ln2 + "ln2_b"].float().contiguous()}
        return self._fill_inputs

    def fill_transform(self, xm: torch.Tensor) -> torch.Tensor:
        """The MLM transform of the gathered rows ``xm [R, H]`` -> ``t [R, H]`` fp32: dense + bias + erf-GELU,
        then the LayerNorm ``mlm_ln_*``. The LayerNorm's output has the rows' dtype (bf16 on the GPU) and is
        widened to fp32 for ``vocab_topk``; the fp32 CPU oracle keeps fp32 throughout."""
        p = self.p
        if xm.shape[0] == 0:
            return torch.zeros(xm.shape, dtype=torch.float32, device=xm.device)
        h = ops.linear(xm, p["mlm_w"], p["mlm_b"], act="gelu")
        return ops.layernorm(h, p["mlm_ln_g"], p["mlm_ln_b"], self.cfg.eps).float()

    def fills(self, ids: torch.Tensor, lens: torch.Tensor, pos: torch.Tensor, mrow: torch.Tensor,
              mord: torch.Tensor, k: int, type_ids: Optional[torch.Tensor] = None,
              tids: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Mask predictions of fill rows (``ops.fill_assemble``): ``(tok [R, k] int32, logit [R, k], prob [R, k],
        lse [R])`` of :func:`ops.vocab_topk` for the mask slots ``mrow [R]`` / ``mord [R]`` (slot ``r`` is mask
        ``mord[r]`` of row ``mrow[r]``, at ``pos [B, M]``). ``tids [T]`` int64 (``T <= 32``, distinct, in the
        vocabulary): score only those tokens (HF's ``targets``): the same kernel over the gathered table
        with the full vocabulary's ``lse``, ``tok`` mapped back through ``tids``, ``k`` capped at ``T``.
        ``logits_out [R, V]`` fp32, when given, receives the full logits.

        Every layer runs in full. On the folded encoder the final LayerNorm is not run over the rows but
        applied to the gathered mask rows (``mask_gather`` with ``fin``)."""
        B, S = ids.shape
        fi = self.fill_inputs()
        if ids.is_cuda and self.fill_fused and self.can_fold(B, S):
            g, fin, _ = self.encode_folded(ids, lens, type_ids, raw=True)
            xm, valid = ops.mask_gather(g, pos, mrow, mord, B, S, fin=fin, gamma=fi["gamma"], beta=fi["beta"])
        else:
            h = self.encode(ids, lens, type_ids, cls_only_last=False)
            xm, valid = ops.mask_gather(h, pos, mrow, mord, B, S)
        t = self.fill_transform(xm)
        if tids is None:
            return ops.vocab_topk(t, fi["E"], fi["bias"], k, valid=valid, logits_out=logits_out)
        full = ops.vocab_topk(t, fi["E"], fi["bias"], 1, valid=valid, logits_out=logits_out)
        kk = min(k, int(tids.numel()))
        tok, logit, prob, _ = ops.vocab_topk(t, fi["E"][tids].contiguous(), fi["bias"][tids].contiguous(), kk,
                                             valid=valid, lse_in=full[3])
        back = tids.to(torch.int32)[tok.clamp(min=0).long()]
        return torch.where(tok >= 0, back, tok), logit, prob, full[3]

    def head(self, h: torch.Tensor, B: int, S: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Pooler + classifier + softmax/top-k (K7) over encoder states ``h``."""
        pooled = self.pooled(h, B, S)
        return ops.classify_head_topk(pooled, self.p["cls_w"], self.p["cls_b"], k)

    def forward(self, ids: torch.Tensor, lens: torch.Tensor, k: int = 5,
                type_ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Returns ``(logits[B,C] fp32, topk_idx[B,k] int32, topk_prob[B,k] fp32)``."""
        B, S = ids.shape
        return self.head(self.encoder(ids, lens, type_ids), B, S, k)

    def score(self, ids: torch.Tensor, lens: torch.Tensor, type_ids: Optional[torch.Tensor],
              label: int = 0) -> torch.Tensor:
        """Cross-encoder relevance ``[B]`` fp32 of pair rows (``ops.pair_assemble``): the raw logit of
        class ``label`` of :meth:`forward` (no softmax: a one-logit head's probability is always 1)."""
        if not 0 <= int(label) < self.cfg.num_labels:
            raise ValueError("label must be in [0, num_labels)")
        logits, _, _ = self.forward(ids, lens, 1, type_ids=type_ids)
        return logits[:, int(label)]

    def nli_logits(self, ids: torch.Tensor, lens: torch.Tensor, type_ids: Optional[torch.Tensor], ent: int,
                   con: int) -> torch.Tensor:
        """``[B, 2]`` fp32 ``(entailment, contradiction)`` logits of premise rows (``ops.premise_assemble``): the
        raw logits of classes ``ent`` and ``con`` of :meth:`forward`. Integer slices and a stack: a list index
        would build an index tensor, which a graph capture must not."""
        C = self.cfg.num_labels
        if not (0 <= int(ent) < C and 0 <= int(con) < C) or int(ent) == int(con):
            raise ValueError("ent and con must be distinct labels in [0, num_labels)")
        logits, _, _ = self.forward(ids, lens, 1, type_ids=type_ids)
        return torch.stack([logits[:, int(ent)], logits[:, int(con)]], 1)
