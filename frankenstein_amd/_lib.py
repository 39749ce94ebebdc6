"""ctypes binding of libfranken_hip.so (include/franken_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, a
RuntimeError is raised (with fk_last_error()).  Nothing here imports the oracle.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import os

# FRANKEN_HIP_LIB selects another build of the same ABI (A/B timing of kernel variants on one GPU box)
LIB_PATH = Path(os.environ.get("FRANKEN_HIP_LIB") or Path(__file__).resolve().parent / "libfranken_hip.so")

FK_F32, FK_BF16 = 0, 1
MASK_NONE, MASK_CAUSAL, MASK_BLOCK_CAUSAL, MASK_PREFIX, MASK_KEYPAD, MASK_DENSE = 0, 1, 2, 3, 4, 5
NORM_LAYER, NORM_RMS = 0, 1
ATTN_Q_PRESCALED = 1
GEMV_GELU = 1
NT_RING2, NT_RING192, NT_RING128, NT_BIG, NT_GLDS4, NT_GLDS, NT_STAGED = range(7)     # fk_gemm_nt_route
NT_LANE = 7                                                                           # fk_gemm_nt_rope_route / fk_gemm_nt_swiglu_route
MLP_BWD_HIPCC, MLP_BWD_ASM = 0, 1                                                     # fk_mlp_bwd_fused_route
NT_ROUTE_F32 = -2
ATTN_FWD_GENERIC, ATTN_FWD_FEWQ, ATTN_FWD_PS, ATTN_FWD_ASM = range(4)                 # fk_attn_route
ATTN_DQ_GENERIC, ATTN_DQ_FEWQ, ATTN_DQ_PS, ATTN_DQ_ASM = range(4)
ATTN_DKDV_GENERIC, ATTN_DKDV_PS, ATTN_DKDV_ASM, ATTN_DKDVW_ASM = range(4)

_p, _i64, _int, _f32, _f64, _sz, _u32 = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_uint32

# name -> (restype, argtypes); mirrors include/franken_hip.h one to one
SIGNATURES = {
    "fk_version": (_int, []),
    "fk_last_error": (C.c_char_p, []),
    "fk_gemm_nt": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _p, _p, _i64, _i64, _int, _int, _p]),
    "fk_gemv_nt": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _p, _p, _i64, _p, _p, _f32, _int, _int, _int, _p]),
    "fk_gemm_nt_rope": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_gemm_nt_swiglu": (_int, [_p, _i64, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_gemm_nt_dswiglu": (_int, [_p, _i64, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_mlp_bwd_fused": (_int, [_p, _i64, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_gemm_nt_route": (_int, [_i64, _i64, _i64, _int, _int, _int, _int]),
    "fk_gemm_nt_rope_route": (_int, [_i64] * 6 + [_int] + [_i64] * 5 + [_int, _int]),
    "fk_gemm_nt_swiglu_route": (_int, [_i64] * 7 + [_int, _int]),
    "fk_mlp_bwd_fused_route": (_int, [_i64, _i64]),
    "fk_gemm_tn_route": (_int, [_i64, _i64, _i64, _int, _p, _p]),
    "fk_gemm_tn_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "fk_gemm_tn": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _int, _int, _p, _sz, _p]),
    "fk_gemm_tn_swiglu": (_int, [_p, _i64, _p, _i64, _p, _p, _i64, _i64, _i64, _i64, _int, _p, _sz, _p]),
    "fk_colsum_workspace_bytes": (_sz, [_i64, _i64]),
    "fk_colsum": (_int, [_p, _i64, _p, _i64, _i64, _int, _int, _p, _sz, _p]),
    "fk_attn_fwd": (_int, [_p, _p, _p, _p, _p] + [_i64] * 13 + [_int, _i64, _i64, _i64, _p, _p, _f32, _int, _int, _p]),
    "fk_attn_bwd": (_int, [_p] * 10 + [_i64] * 13 + [_int, _i64, _i64, _i64, _p, _p, _f32, _p, _i64, _i64, _int, _int, _p]),
    "fk_attn_fwd_dropout": (_int, [_p, _p, _p, _p, _p] + [_i64] * 13 + [_int, _i64, _i64, _i64, _p, _p, _f32, _int, _f32, _p, _u32, _int, _p]),
    "fk_attn_bwd_dropout": (_int, [_p] * 10 + [_i64] * 13 + [_int, _i64, _i64, _i64, _p, _p, _f32, _p, _i64, _i64, _int, _f32, _p, _u32, _int, _p]),
    "fk_attn_route": (_int, [_i64, _i64, _i64, _int, _int, _i64, _i64, _i64, _int, _int, _int, _p, _p, _p]),
    "fk_dropout": (_int, [_p, _p, _p, _i64, _f32, _p, _u32, _int, _p]),
    "fk_norm_fwd": (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _f32, _int, _int, _p]),
    "fk_norm_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "fk_norm_bwd": (_int, [_p] * 9 + [_i64, _i64, _int, _int, _int, _p, _sz, _p]),
    "fk_rope": (_int, [_p, _i64, _i64, _i64, _i64, _i64, _p, _i64, _i64, _int, _int, _p]),
    "fk_patchify": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_swiglu_fwd": (_int, [_p, _p, _i64, _i64, _int, _p]),
    "fk_swiglu_bwd": (_int, [_p, _p, _p, _i64, _i64, _int, _p]),
    "fk_gelu_fwd": (_int, [_p, _p, _i64, _int, _p]),
    "fk_gelu_bwd": (_int, [_p, _p, _p, _i64, _int, _p]),
    "fk_cast_pack": (_int, [_p, _i64, _p, _i64, _i64, _i64, _int, _int, _p]),
    "fk_cast_pack_rows": (_int, [_p, _i64, _p, _i64, _i64, _i64, _int, _i64, _i64, _i64, _int, _p]),
    "fk_cast_pack_multi": (_int, [_p, _i64, _i64, _int, _p]),
    "fk_cast": (_int, [_p, _int, _p, _int, _i64, _p]),
    "fk_add": (_int, [_p, _p, _p, _i64, _int, _p]),
    "fk_gather_rows": (_int, [_p, _i64, _int, _p, _i64, _p, _i64, _int, _i64, _i64, _i64, _int, _p]),
    "fk_scatter_add_rows": (_int, [_p, _int, _p, _i64, _p, _i64, _i64, _p]),
    "fk_prefix_mask": (_int, [_p, _p, _i64, _p, _p, _i64, _i64, _i64, _p]),
    "fk_copy2d": (_int, [_p, _i64, _p, _i64, _i64, _i64, _int, _p]),
    "fk_attn_combine": (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_add2d": (_int, [_p, _i64, _p, _i64, _i64, _i64, _p]),
    "fk_gpt_embed_step": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _int, _p]),
    "fk_kv_append": (_int, [_p, _p, _p, _i64, _i64, _i64, _int, _p]),
    "fk_attn_decode": (_int, [_p, _i64, _p, _i64, _i64, _p, _i64, _p, _i64, _i64, _i64, _f32, _int, _p]),
    "fk_sample_topk": (_int, [_p, _i64, _i64, _i64, _f32, _i64, _p, _p, _p, _p, _p, _i64, _i64, _p, _p]),
    "fk_attn_decode_beam": (_int, [_p, _i64, _p, _i64, _i64, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _f32, _int, _p]),
    "fk_beam_topk": (_int, [_p, _i64, _i64, _i64, _f32, _i64, _p, _p, _p]),
    "fk_beam_select": (_int, [_p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _i64, _p]),
    "fk_attn_decode_beam_grouped": (_int, [_p, _i64, _p, _i64, _i64, _i64, _p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _f32, _int, _int, _p]),
    "fk_beam_select_grouped": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _i64, _p, _p]),
    "fk_beam_select_eos": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _i64, _p, _i64, _p, _p, _p, _i64, _p, _p, _p]),
    "fk_beam_backtrack": (_int, [_p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _p, _p, _p]),
    "fk_sample_topk_eos": (_int, [_p, _i64, _i64, _i64, _f32, _i64, _p, _p, _p, _p, _p, _i64, _i64, _p, _i64, _p, _p, _p, _p, _p]),
    "fk_sample_topp": (_int, [_p, _i64, _i64, _i64, _f32, _i64, _f32, _p, _p, _p, _p, _p, _i64, _i64, _p, _i64, _p, _p, _p, _p, _p]),
    "fk_logit_rules": (_int, [_p, _i64, _i64, _i64, _f32, _i64, _i64, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _p, _i64, _i64, _int, _p]),
    "fk_im2col1d": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_col2im1d": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_elu_fwd": (_int, [_p, _p, _i64, _int, _p]),
    "fk_elu_bwd": (_int, [_p, _p, _p, _i64, _int, _p]),
    "fk_argmax_rows": (_int, [_p, _i64, _p, _i64, _i64, _int, _p]),
    "fk_block_stats_workspace_bytes": (_sz, [_i64, _i64]),
    "fk_block_stats": (_int, [_p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _sz, _p]),
    "fk_zscore_smooth_pad": (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _f64, _p]),
    "fk_gpt_embed_fwd": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_gpt_embed_bwd_wte": (_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_loss_workspace_bytes": (_sz, [_i64]),
    "fk_l1_loss_fwd": (_int, [_p, _p, _p, _i64, _int, _p, _i64, _int, _p, _sz, _p]),
    "fk_l1_loss_bwd": (_int, [_p, _p, _p, _p, _i64, _int, _p, _i64, _p, _int, _p]),
    "fk_head_ce_workspace_bytes": (_sz, [_i64, _i64]),
    "fk_head_ce_fwd": (_int, [_p, _i64, _p, _i64, _i64, _p, _p, _p, _p, _p, _i64, _i64, _i64, _int, _p, _sz, _p]),
    "fk_head_ce_bwd": (_int, [_p, _i64, _p, _i64, _i64, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_transpose2d": (_int, [_p, _i64, _p, _i64, _i64, _i64, _int, _p]),
    "fk_ctc_route": (_int, [_i64]),
    "fk_ctc_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "fk_ctc_loss_fwd": (_int, [_p, _i64, _i64, _p, _i64, _p, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _p, _sz, _p]),
    "fk_ctc_loss_bwd": (_int, [_p, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _p, _sz, _p]),
    "fk_ctc_collapse": (_int, [_p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _p]),
    "fk_ctc_align_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "fk_ctc_align": (_int, [_p, _i64, _i64, _p, _i64, _p, _p, _i64] + [_i64] * 6 + [_p, _p, _i64, _p, _i64, _p, _p, _p, _i64, _int, _p, _sz, _p]),
    "fk_ctc_beam_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "fk_ctc_beam_search": (_int, [_p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _i64, _i64, _p, _p, _int, _p, _sz, _p]),
    "fk_ngram_hash": (_u32, [_u32, _u32]),
    "fk_ctc_beam_search_lm": (_int, [_p, _i64, _i64, _p] + [_i64] * 8 + [_p, _i64, _i64, _p, _p, _i64, _p, _p, _i64, _i64, _f32, _f32, _int, _p, _i64, _i64,
                                     _p, _p, _p, _p, _int, _p, _sz, _p]),
    "fk_ctc_beam_lex_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "fk_ctc_beam_search_lex": (_int, [_p, _i64, _i64, _p] + [_i64] * 9 + [_p, _i64, _i64, _p, _i64, _p, _i64, _i64, _p, _i64, _i64, _p, _p, _i64, _p, _p,
                                      _i64, _i64, _f32, _f32, _int, _p, _i64, _i64, _p, _p, _i64, _i64, _p, _p, _p, _p, _p, _int, _p, _sz, _p]),
    "fk_ctc_prefix_init": (_int, [_p, _i64, _i64, _p] + [_i64] * 5 + [_p, _i64, _i64, _p, _p, _p, _p, _int, _p]),
    "fk_ctc_prefix_score": (_int, [_p, _i64, _i64, _p, _p] + [_i64] * 6 + [_p, _p, _int, _f32, _i64, _p, _p, _p, _p, _i64, _p, _p, _p, _p, _int, _p]),
    "fk_nbest_trie": (_int, [_p, _i64, _i64, _p, _p] + [_i64] * 8 + [_p] * 8),
    "fk_nbest_trie_mask": (_int, [_p, _p, _p, _i64, _i64, _i64, _p]),
    "fk_gpt_embed_pos": (_int, [_p] * 6 + [_i64] * 6 + [_int, _p]),
    "fk_nbest_rescore": (_int, [_p] * 8 + [_i64, _i64, _p, _p] + [_i64] * 4 + [_int, _f32, _f32, _f32, _i64] + [_p] * 9),
    "fk_edit_distance_route": (_int, [_i64, _i64]),
    "fk_edit_distance": (_int, [_p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _p, _p, _p]),
    "fk_nbest_pairwise_distance": (_int, [_p, _i64, _i64, _p, _p, _i64, _i64, _i64, _p, _p]),
    "fk_mbr_rank": (_int, [_p, _p, _f32, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64] + [_p] * 8),
    "fk_mwer_combine": (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p]),
    "fk_mwer_reduce_rows": (_int, [_p, _p, _p, _i64, _i64, _i64, _int, _int, _p]),
    "fk_ce_workspace_bytes": (_sz, [_i64]),
    "fk_ce_loss_fwd": (_int, [_p, _i64, _p, _p, _p, _i64, _i64, _i64, _int, _p, _sz, _p]),
    "fk_ce_loss_bwd": (_int, [_p, _i64, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_ce_chunk_fwd": (_int, [_p, _i64, _p, _i64, _p, _p, _p, _i64, _i64, _int, _p]),
    "fk_ce_chunk_finish": (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _sz, _p]),
    "fk_ce_chunk_bwd": (_int, [_p, _i64, _p, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_adamw_step": (_int, [_p, _p, _p, _p, _i64, _f64, _f64, _f64, _f64, _f64, _i64, _f64, _f64, _int, _p]),
    "fk_grad_sumsq": (_int, [_p, _i64, _p, _i64, _p, _int, _p]),
    "fk_adamw_step_groups": (_int, [_p, _p, _p, _p, _i64, _p, _i64, _p, _int, _f64, _f64, _int, _f64, _p, _int, _p, _p]),
    "fk_vq_route": (_int, [_i64, _i64, _int]),
    "fk_vq_assign": (_int, [_p, _i64, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _f32, _p, _i64, _i64, _i64, _int, _p]),
    "fk_vq_bwd": (_int, [_p, _p, _p, _p, _f32, _p, _i64, _int, _p]),
    "fk_vq_codebook_update": (_int, [_p, _p, _p, _p, _i64, _p, _i64, _p, _p, _i64, _i64, _f32, _f32, _f32, _int, _p]),
    "fk_day_adapter_fwd": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _int, _p]),
    "fk_day_adapter_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "fk_day_adapter_bwd": (_int, [_p, _p, _p, _i64, _p, _p, _p, _sz, _i64, _i64, _i64, _i64, _i64, _p]),
    "fk_augment_patchify": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _p, _p, _int, _p]),
    "fk_lora_route": (_int, [_i64, _i64, _i64, _i64, _int]),
    "fk_lora_fwd": (_int, [_p, _i64, _p, _p, _i64, _i64, _i64, _i64, _f32, _i64, _f32, _p, _i64, _p, _p, _i64, _int, _p]),
    "fk_lora_wgrad_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "fk_lora_wgrad": (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _f32, _p, _p, _int, _int, _p, _sz, _p]),
    "fk_lora_merge": (_int, [_p, _p, _p, _i64, _i64, _i64, _f32, _p, _i64, _int, _p]),
}
LORA_R32, LORA_R64 = 0, 1                                                             # fk_lora_route
LORA_FWD_ROWS, LORA_WGRAD_ROWS = 32, 64                                               # rows per workgroup / per slice of fk_lora_fwd / fk_lora_wgrad
AUG_MAX_SPANS = 8                                                                     # the most time spans fk_augment_patchify draws
DAY_MAX_C = 512                                                                       # the envelope of fk_day_adapter_*
ADAMW_MAX_SLOTS, GRAD_SUMSQ_MAX_BLOCKS = 16, 1024
VQ_CHAIN, VQ_FUSED = 0, 1                                                             # fk_vq_route
VQ_EMA, VQ_KMEANS = 0, 1                                                              # fk_vq_codebook_update modes
CTC_WAVE, CTC_LDS = 0, 1                                                             # fk_ctc_route
CTC_NONE, CTC_SUM, CTC_MEAN = 0, 1, 2                                                 # fk_ctc_loss_* reductions
CTC_PREFIX_MAX_T, CTC_PREFIX_MAX_PROMPT, CTC_PREFIX_FLOOR = 1024, 64, -1e10               # the envelope of fk_ctc_prefix_* and its finite floor
NBEST_MAX_HYPS, NBEST_MAX_T, NBEST_MAX_NODES, NBEST_MAX_ROWS = 32, 1024, 32769, 4096         # the envelope of fk_nbest_* (csrc/rescore.hip)
EDIT_LANE, EDIT_ROWS4, EDIT_ROWS16 = 0, 1, 2                                          # fk_edit_distance_route
VQ_ROWS = 32                                                                          # data rows per workgroup of fk_vq_assign


class AdamwGroup(C.Structure):
    """fk_adamw_group: one slot's hyper-parameters as the host hands them to fk_adamw_step_groups"""
    _fields_ = [("lr", _f64), ("beta1", _f64), ("beta2", _f64), ("eps", _f64), ("weight_decay", _f64), ("step", _i64)]


class AugmentCfg(C.Structure):
    """fk_augment_cfg: the knobs of fk_augment_patchify, read on the host"""
    _fields_ = [("white_sd", _f32), ("offset_sd", _f32), ("chan_drop_p", _f32), ("time_shift", C.c_int32), ("n_time_masks", C.c_int32),
                ("time_mask_len", C.c_int32), ("keep_padding", C.c_int32), ("reserved", C.c_int32)]


_lib = None


class FrankenHipError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load (once) and return the C-ABI library; raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise FrankenHipError(
                f"{LIB_PATH} is missing: build it with `python -m frankenstein_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU / PyTorch fallback.")
        h = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)      # AttributeError if the header and the library disagree
            fn.restype, fn.argtypes = res, args
        _lib = h
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().fk_last_error().decode(errors="replace")
        raise FrankenHipError(f"{what or 'libfranken_hip'} failed (code {rc}): {msg}")


def call(name: str, *args):
    """Call an int-returning entry point and raise on a non-zero code."""
    check(getattr(lib(), name)(*args), name)
