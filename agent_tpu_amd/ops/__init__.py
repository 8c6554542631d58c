"""Device ops: thin, shape-checked wrappers over the gfx950 HIP kernels.

Every op runs the native kernel for CUDA (ROCm) tensors and a plain PyTorch
reference for CPU tensors; the reference doubles as the numerics oracle in
``tests/kernels``. There is no silent fallback for device tensors: if the
extension cannot load on a GPU, the call raises.
"""
from .linear import linear, fold_rms_into_linear, EPI_BIAS, EPI_GELU, EPI_TANH, EPI_RESIDUAL, EPI_RELU  # noqa: F401
from .linear import linear_ln, fold_ln_into_linear, fold_ok, ln_partials_ref, ln_finalize, row_parts_ref  # noqa: F401
from .linear import LAYOUT_A, LAYOUT_C, LAYOUT_R, to_image_order, from_image_order, image_order_ok  # noqa: F401
from .linear import LAYOUT_A_FRAG, LAYOUT_C_FRAG, LAYOUT_R_FRAG, to_fragment_order, from_fragment_order  # noqa: F401
from .linear import row_totals_parts_ref, batch_invariant, set_batch_invariant  # noqa: F401
from .linear_i8 import quantize_rows_i8, linear_i8, linear_i8_ok, quantize_rows_i8_ref, linear_i8_ref  # noqa: F401
from .linear_i8 import layernorm_quant_i8  # noqa: F401
from .decode import decode_attention, kv_append, gather_rows, beam_topk_rows, beam_reorder_hist, MAX_BANS  # noqa: F401
from .decode import DecEmbed, decode_advance, decode_advance_ok  # noqa: F401
from .decode import beam_select, beam_select_ref, ngram_bans, lm_head_topk, lm_head, LmHead, LM_HEAD_MAX_K  # noqa: F401
from .attention import attention_packed, attention  # noqa: F401
from .qkv_attention import qkv_attention, qkv_attention_ok, qkv_head_order  # noqa: F401
from .cls_attend import cls_attend, cls_attend_ok, cls_attend_ref, cls_reassoc_weights  # noqa: F401
from .pool import pool_embed, pool_embed_ok, pool_embed_ref  # noqa: F401
from .search import sim_topk, sim_topk_ok, sim_topk_ref  # noqa: F401
from .search import (RowMask, row_mask_from_ids, row_mask_from_ids_ref, row_mask_from_labels,  # noqa: F401
                     row_mask_from_labels_ref, row_mask_from_bits, row_mask_bits)
from .search import sim_topk_ivf, sim_topk_ivf_ref, ivf_labels, ivf_plan  # noqa: F401
from .pq import (pq_ok, pq_encode, pq_encode_ref, pq_lut, pq_lut_ref, pq_scan_topk, pq_scan_topk_ref,  # noqa: F401
                 sim_topk_pq, sim_topk_pq_ref, pq_bias, pq_interleave, pq_deinterleave, PqCodes)
from .pq import decode as pq_decode  # noqa: F401  (ops.decode stays the decode-attention module)
from .cluster import to_fixed  # noqa: F401
from .cluster import (kmeans_assign, kmeans_assign_ref, kmeans_update, kmeans_update_ref, kmeans_finalize,  # noqa: F401
                      kmeans_finalize_ref, fixed_shift, fixed_sum, fixed_sum_ref, kmeans_ok)
from .dedup import (sim_join, sim_join_ok, sim_join_ref, sort_pairs, cc_min_labels,  # noqa: F401
                    cc_min_labels_ref)
from .norm import layernorm, rmsnorm, embed_layernorm, embed_gather, embed_pos_layernorm  # noqa: F401
from .tokenize import tokenize, tokenize_wordpiece  # noqa: F401
from .rerank import pair_assemble, pair_assemble_ref, group_topk, group_topk_ref  # noqa: F401
from .maxsim import (token_unit, token_unit_ref, maxsim, maxsim_ref, maxsim_ok, maxsim_index,  # noqa: F401
                     maxsim_index_ref)
from .span import span_topk, span_topk_ok, span_topk_ref, span_logits_ref, span_select_ref  # noqa: F401
from .window import window_assemble, window_assemble_ref, window_best, window_best_ref  # noqa: F401
from .tag import (tag_entities, tag_ok, tag_logits_ref, tag_select_ref, tag_group_ref, tag_tables,  # noqa: F401
                  default_tag_names)
from .fill import (fill_assemble, fill_assemble_ref, mask_gather, mask_gather_ref, vocab_topk, vocab_topk_ok,  # noqa: F401
                   vocab_logits_ref, vocab_select_ref, vocab_topk_splits)
from .zeroshot import premise_assemble, premise_assemble_ref, nli_rank, nli_rank_ref  # noqa: F401
from .head import classify_head_topk  # noqa: F401
from .reduce import risk_stats, reduce_stats_tensor  # noqa: F401
