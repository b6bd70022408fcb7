"""ctypes binding of libvlp_hip.so (include/vlp_hip.h).

The structures below mirror the header field for field.  Every wrapper takes torch tensors only to
extract raw device pointers (`data_ptr()`) and the current HIP stream; the library itself has no
torch dependency.  A failing call raises RuntimeError(vlp_last_error_string()).

The product path has NO fallback: if the shared library is missing or was not built, importing the
compute modules raises -- it never silently routes through torch ops or the CPU oracle.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VLP_HIP_LIB") or os.path.join(_HERE, "libvlp_hip.so")      # VLP_HIP_LIB: A/B runs against another build of the SAME ABI

ACT_NONE, ACT_GELU, ACT_RELU, ACT_TANH, ACT_GELU_SAVE_GRAD = 0, 1, 2, 3, 4
MUL_NONE, MUL_GELU_GRAD, MUL_RELU_MASK, MUL_PLAIN = 0, 1, 2, 3
ROWS_X, ROWS_MUL, ROWS_RES, ROWS_Y = 1, 2, 4, 8      # VLP_ROWS_*: operands of a listed-row launch addressed at row live[m]

vp, i64, i32, f32, u64, u32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_uint64, C.c_uint32


class GemmNtArgs(C.Structure):
    _fields_ = [("X", vp), ("ldx", i64), ("W", vp), ("ldw", i64), ("Y", vp), ("ldy", i64), ("bias", vp),
                ("residual", vp), ("ldr", i64), ("preact", vp), ("ldp", i64), ("mul_src", vp), ("ldm", i64),
                ("M", i32), ("N", i32), ("K", i32), ("act", i32), ("mul_mode", i32), ("alpha", f32),
                ("dropout_p", f32), ("seed", u64), ("rng_stream", u32), ("variant", i32), ("row_map", vp)]


class GemmTnArgs(C.Structure):
    _fields_ = [("A", vp), ("lda", i64), ("B", vp), ("ldb", i64), ("C", vp), ("ldc", i64),
                ("M", i32), ("N", i32), ("K", i32), ("beta", i32), ("workspace", vp), ("workspace_bytes", i64),
                ("variant", i32), ("splits", i32), ("bias_out", vp)]


class ColsumArgs(C.Structure):
    _fields_ = [("A", vp), ("lda", i64), ("M", i32), ("N", i32), ("out", vp), ("beta", i32),
                ("workspace", vp), ("workspace_bytes", i64)]


class AttnFwdArgs(C.Structure):
    _fields_ = [("qkv", vp), ("ld_qkv", i64), ("mask", vp), ("ctx", vp), ("ld_ctx", i64), ("lse", vp),
                ("B", i32), ("L", i32), ("heads", i32), ("scale", f32),
                ("dropout_p", f32), ("seed", u64), ("rng_stream", u32), ("row_off", vp)]


class AttnBwdArgs(C.Structure):
    _fields_ = [("qkv", vp), ("ld_qkv", i64), ("mask", vp), ("mask_t", vp), ("ctx", vp), ("ld_ctx", i64), ("dctx", vp), ("ld_dctx", i64),
                ("lse", vp), ("dqkv", vp), ("ld_dqkv", i64), ("delta", vp),
                ("B", i32), ("L", i32), ("heads", i32), ("scale", f32),
                ("dropout_p", f32), ("seed", u64), ("rng_stream", u32), ("row_off", vp)]


class LayerNormFwdArgs(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("gamma", vp), ("beta", vp), ("y", vp), ("ldy", i64), ("mean", vp), ("rstd", vp),
                ("M", i32), ("H", i32), ("eps", f32), ("dropout_p", f32), ("seed", u64), ("rng_stream", u32), ("row_map", vp)]


class LayerNormBwdArgs(C.Structure):
    _fields_ = [("dy", vp), ("lddy", i64), ("x", vp), ("ldx", i64), ("gamma", vp), ("mean", vp), ("rstd", vp),
                ("dx", vp), ("lddx", i64), ("dx_drop", vp), ("lddxd", i64), ("dgamma", vp), ("dbeta", vp),
                ("M", i32), ("H", i32), ("beta", i32),
                ("dy_drop_p", f32), ("dy_seed", u64), ("dy_stream", u32),
                ("out_drop_p", f32), ("out_seed", u64), ("out_stream", u32),
                ("workspace", vp), ("workspace_bytes", i64), ("defer_reduce", i32), ("row_map", vp)]


class EmbedFwdArgs(C.Structure):
    _fields_ = [("input_ids", vp), ("segment_ids", vp), ("word_emb", vp), ("pos_emb", vp), ("type_emb", vp),
                ("vis_h", vp), ("vispe_h", vp), ("pre", vp),
                ("B", i32), ("L", i32), ("Nv", i32), ("H", i32), ("vocab", i32), ("type_vocab", i32),
                ("position_ids", vp), ("max_pos", i32), ("region_mask", vp), ("row_map", vp), ("rows", i32)]


class AttnDecodeArgs(C.Structure):
    _fields_ = [("q", vp), ("ld_q", i64), ("q_rows_per_batch", i64), ("k", vp), ("v", vp), ("ld_kv", i64), ("kv_rows_per_batch", i64),
                ("mask", vp), ("ctx", vp), ("ld_ctx", i64), ("B", i32), ("Lq", i32), ("Lk", i32), ("heads", i32), ("scale", f32),
                ("k_prefix", vp), ("v_prefix", vp), ("prefix_rows_per_batch", i64), ("n_prefix", i32), ("beams", i32)]


class DecGemmArgs(C.Structure):
    _fields_ = [("X", vp), ("ldx", i64), ("W", vp), ("ldw", i64), ("bias", vp), ("Y", vp), ("ldy", i64), ("slab", vp), ("ldslab", i64),
                ("kv_cache", vp), ("kv_ld", i64), ("kv_col0", i32), ("kv_Lcap", i32), ("kv_T", i32), ("kv_start", i32),
                ("M", i32), ("N", i32), ("K", i32), ("splits", i32), ("act", i32),
                ("residual", vp), ("ldr", i64), ("ln_gamma", vp), ("ln_beta", vp), ("ln_eps", f32), ("ln_out", vp), ("ld_ln_out", i64)]


class DecReduceLnArgs(C.Structure):
    _fields_ = [("slab", vp), ("ldslab", i64), ("splits", i32), ("bias", vp), ("residual", vp), ("ldr", i64), ("gamma", vp), ("beta", vp),
                ("eps", f32), ("Y", vp), ("ldy", i64), ("M", i32), ("H", i32)]


class VisPePrepArgs(C.Structure):
    _fields_ = [("bbox", vp), ("cls", vp), ("ld_cls", i64), ("out", vp), ("ld_out", i64), ("B", i32), ("Nv", i32), ("n_cls", i32),
                ("pad_to", i32), ("cls_is_f32", i32), ("eps", f32)]


class BeamSelectArgs(C.Structure):
    _fields_ = [("kk_scores", vp), ("kk_ids", vp), ("last_total", vp), ("last_eos", vp), ("out_scores", vp), ("out_ids", vp),
                ("out_ptrs", vp), ("out_eos", vp), ("src_rows", vp), ("next_ids", vp), ("next_ids_stride", i64),
                ("B", i32), ("K", i32), ("first", i32), ("eos_id", i64)]


class EmbedBwdArgs(C.Structure):
    _fields_ = [("dpre", vp), ("input_ids", vp), ("segment_ids", vp), ("vis_h", vp), ("vispe_h", vp),
                ("d_word_emb", vp), ("d_pos_emb", vp), ("d_type_emb", vp), ("d_vis_h", vp), ("d_vispe_h", vp), ("acc32", vp),
                ("B", i32), ("L", i32), ("Nv", i32), ("H", i32), ("vocab", i32), ("type_vocab", i32),
                ("drop_p", f32), ("seed", u64), ("vis_stream", u32), ("vispe_stream", u32), ("region_mask", vp), ("parts", i32)]


class EmbedBwdPosArgs(C.Structure):
    _fields_ = [("base", EmbedBwdArgs), ("position_ids", vp), ("max_pos", i32)]


class ScstLayoutArgs(C.Structure):
    _fields_ = [("prefix_ids", vp), ("sample_ids", vp), ("segment_ids", vp), ("position_ids", vp), ("mask", vp),
                ("out_ids", vp), ("out_segment_ids", vp), ("out_position_ids", vp), ("out_mask", vp), ("masked_pos", vp),
                ("B", i32), ("L", i32), ("in_len", i32), ("T", i32), ("mask_word_id", i64)]


class TokenLogprobFwdArgs(C.Structure):
    _fields_ = [("logits", vp), ("ld_logits", i64), ("ids", vp), ("logp", vp), ("lse", vp), ("rows", i32), ("V", i32)]


class TokenLogprobBwdArgs(C.Structure):
    _fields_ = [("logits", vp), ("ld_logits", i64), ("ids", vp), ("lse", vp), ("g", vp), ("dlogits", vp), ("ld_dlogits", i64),
                ("rows", i32), ("V", i32)]


class TokenPolicyFwdArgs(C.Structure):
    _fields_ = [("logits", vp), ("ld_logits", i64), ("ids", vp), ("logp", vp), ("lse", vp), ("entropy", vp), ("rows", i32), ("V", i32),
                ("temperature", f32)]


class TokenScoreArgs(C.Structure):
    _fields_ = [("logits", vp), ("ld_logits", i64), ("ids", vp), ("logp", vp), ("lse", vp), ("entropy", vp), ("rank", vp), ("top_id", vp),
                ("top_logit", vp), ("rows", i32), ("V", i32)]


class TokenPolicyBwdArgs(C.Structure):
    _fields_ = [("logits", vp), ("ld_logits", i64), ("ids", vp), ("lse", vp), ("entropy", vp), ("g", vp), ("h", vp), ("dlogits", vp),
                ("ld_dlogits", i64), ("rows", i32), ("V", i32), ("temperature", f32)]


class PretextFwdArgs(C.Structure):
    _fields_ = [("vis_h", vp), ("vispe_h", vp), ("pooled", vp), ("vis_masked_pos", vp), ("probs", vp), ("sample_loss", vp), ("loss", vp),
                ("B", i32), ("Nv", i32), ("Pm", i32), ("H", i32)]


class PretextBwdArgs(C.Structure):
    _fields_ = [("vis_h", vp), ("vispe_h", vp), ("pooled", vp), ("vis_masked_pos", vp), ("probs", vp), ("gscale", vp),
                ("d_vis_h", vp), ("d_vispe_h", vp), ("d_pooled_pre", vp), ("B", i32), ("Nv", i32), ("Pm", i32), ("H", i32),
                ("drop_p", f32), ("seed", u64), ("vis_stream", u32), ("vispe_stream", u32)]


class TransposeDesc(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("lds", i64), ("ldd", i64), ("rows", i32), ("cols", i32), ("rows_pad", i32), ("reserved", i32)]


class CiderDArgs(C.Structure):
    _fields_ = [("hyp", vp), ("hyp_ld", i64), ("ref", vp), ("ref_group_stride", i64), ("ref_ld", i64), ("ref_count", vp),
                ("G", i32), ("R", i32), ("T", i32), ("mult", i32), ("sigma", f32), ("scores", vp), ("reward", vp),
                ("workspace", vp), ("workspace_bytes", i64)]


class CiderDDfArgs(C.Structure):
    _fields_ = [("s", CiderDArgs), ("df_keys", vp), ("df_vals", vp), ("df_n", i64), ("n_docs", i64)]


class CiderDConsensusArgs(C.Structure):
    _fields_ = [("hyp", vp), ("hyp_ld", i64), ("G", i32), ("K", i32), ("T", i32), ("sigma", f32), ("df_keys", vp), ("df_vals", vp), ("df_n", i64),
                ("n_docs", i64), ("utility", vp), ("pick", vp), ("pair", vp), ("workspace", vp), ("workspace_bytes", i64)]


class CaptionEvalArgs(C.Structure):
    _fields_ = [("d", CiderDDfArgs), ("bleu_stats", vp), ("lcs", vp)]


class Bleu4Args(C.Structure):
    _fields_ = [("hyp", vp), ("hyp_ld", i64), ("ref", vp), ("ref_group_stride", i64), ("ref_ld", i64), ("ref_count", vp),
                ("G", i32), ("R", i32), ("T", i32), ("mult", i32), ("bleu4", vp), ("stats", vp), ("base", vp), ("w_base", f32), ("w_bleu", f32),
                ("mixed", vp), ("reward", vp), ("reward_mode", i32)]


class MlmLossFwdArgs(C.Structure):
    _fields_ = [("logits", vp), ("ld_logits", i64), ("labels", vp), ("weights", vp), ("loss", vp), ("lse", vp), ("coef", vp),
                ("row_loss", vp), ("B", i32), ("P", i32), ("V", i32), ("drop_worst_ratio", f32)]


class MlmLossBwdArgs(C.Structure):
    _fields_ = [("logits", vp), ("ld_logits", i64), ("labels", vp), ("lse", vp), ("coef", vp), ("grad_scale", vp),
                ("dlogits", vp), ("ld_dlogits", i64), ("rows", i32), ("V", i32)]


class MlmLossLsFwdArgs(C.Structure):
    _fields_ = MlmLossFwdArgs._fields_ + [("smooth", f32), ("confidence", f32), ("q_sum", f32), ("q_log_q", f32), ("ignore_index", i32)]


class MlmLossLsBwdArgs(C.Structure):
    _fields_ = MlmLossBwdArgs._fields_ + [("smooth", f32), ("confidence", f32), ("q_sum", f32), ("ignore_index", i32)]


class FusedAdamArgs(C.Structure):
    _fields_ = [("p32", vp), ("m", vp), ("v", vp), ("g16", vp), ("p16", vp), ("n", i64),
                ("b1", f32), ("b2", f32), ("eps", f32), ("decay", f32), ("eps_inside_sqrt", i32), ("hyper", vp)]


class BertAdamArgs(C.Structure):
    _fields_ = [("p32", vp), ("m", vp), ("v", vp), ("g", vp), ("g_is_f32", i32), ("p16", vp),
                ("seg_off", vp), ("ntensors", i32), ("n", i64), ("norms", vp), ("norms_floats", i64),
                ("lr", f32), ("b1", f32), ("b2", f32), ("eps", f32), ("decay", f32), ("max_grad_norm", f32), ("grad_scale", f32),
                ("active", vp)]


# every symbol include/vlp_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "vlp_version": (C.c_int, []),
    "vlp_last_error_string": (C.c_char_p, []),
    "vlp_lab_build": (C.c_int, []),
    "vlp_debug_device_lookup_stats": (None, [vp, vp]),
    "vlp_gemm_nt": (C.c_int, [C.POINTER(GemmNtArgs), vp]),
    "vlp_gemm_nt_rows": (C.c_int, [C.POINTER(GemmNtArgs), vp, i32, vp]),
    "vlp_gemm_nt_resolved_variant": (C.c_int, []),
    "vlp_gemm_nt_splitk_workspace_bytes": (C.c_int64, [i32, i32, i32]),
    "vlp_gemm_nt_splitk": (C.c_int, [C.POINTER(GemmNtArgs), i32, vp, i64, vp]),
    "vlp_gemm_tn_workspace_bytes": (i64, [i32, i32, i32]),
    "vlp_gemm_tn": (C.c_int, [C.POINTER(GemmTnArgs), vp]),
    "vlp_gemm_tn_grouped": (C.c_int, [C.POINTER(GemmTnArgs), i32, vp]),
    "vlp_gemm_tn_grouped_rows": (C.c_int, [C.POINTER(GemmTnArgs), C.POINTER(vp), C.POINTER(i32), i32, vp]),
    "vlp_gemm_tn_grouped_workspace_bytes": (i64, [i32]),
    "vlp_gemm_tn_grouped_mapped": (C.c_int, [C.POINTER(GemmTnArgs), vp, vp, i32, vp]),
    "vlp_kept_rows_build": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
    "vlp_colsum_workspace_bytes": (i64, [i32, i32]),
    "vlp_colsum": (C.c_int, [C.POINTER(ColsumArgs), vp]),
    "vlp_attn_fwd": (C.c_int, [C.POINTER(AttnFwdArgs), vp]),
    "vlp_attn_bwd": (C.c_int, [C.POINTER(AttnBwdArgs), vp]),
    "vlp_attn_decode": (C.c_int, [C.POINTER(AttnDecodeArgs), vp]),
    "vlp_mask_pack_rect": (C.c_int, [vp, i64, i64, vp, i32, i32, i32, i32, vp]),
    "vlp_kv_append": (C.c_int, [vp, i64, vp, i32, i32, i32, i32, i32, vp]),
    "vlp_dec_gemm": (C.c_int, [C.POINTER(DecGemmArgs), vp]),
    "vlp_dec_reduce_ln": (C.c_int, [C.POINTER(DecReduceLnArgs), vp]),
    "vlp_argmax_rows2": (C.c_int, [vp, i64, i32, i32, vp, i64, vp, i64, vp, i64, vp]),
    "vlp_logsoftmax_topk": (C.c_int, [vp, i64, i32, i32, i32, vp, i32, i32, vp, vp, vp]),
    "vlp_beam_select": (C.c_int, [C.POINTER(BeamSelectArgs), vp]),
    "vlp_beam_select_groups": (C.c_int, [C.POINTER(BeamSelectArgs), i32, C.c_float, vp]),
    "vlp_beam_select_constrained": (C.c_int, [C.POINTER(BeamSelectArgs), vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "vlp_logsoftmax_topk_want": (C.c_int, [vp, i64, i32, i32, i32, vp, vp, i64, vp, i32, i32, vp, i32, vp, vp, vp, vp]),
    "vlp_ngram_candidates": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, i32, vp, i64, vp, vp]),
    "vlp_logsoftmax_topk_list": (C.c_int, [vp, i64, i32, i32, i32, vp, i64, vp, i32, i32, vp, vp, vp]),
    "vlp_kv_gather": (C.c_int, [vp, i64, vp, i64, vp, i32, i32, i32, i32, vp]),
    "vlp_beam_nbest": (C.c_int, [vp, vp, vp, i32, i32, i32, i64, C.c_double, i32, i32, vp, vp, vp, vp, vp, vp]),
    "vlp_embed_bwd_workspace_floats": (C.c_int64, [i32, i32, i32, i32]),
    "vlp_mask_build": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp]),
    "vlp_vis_pe_prep": (C.c_int, [C.POINTER(VisPePrepArgs), vp]),
    "vlp_sample_rows": (C.c_int, [vp, i64, i32, i32, C.c_uint64, C.c_uint32, vp, i64, vp, i64, vp]),
    "vlp_sample_rows_rep": (C.c_int, [vp, i64, i32, i32, i32, vp, C.c_uint64, C.c_uint32, vp, i64, vp, i64, vp, i64, vp]),
    "vlp_sample_rows_filtered": (C.c_int, [vp, i64, i32, i32, i32, vp, C.c_uint64, C.c_uint32, C.c_float, i32, C.c_float, vp, i64, vp, i64, vp, i64,
                                           vp, vp, vp]),
    "vlp_argmax_rows": (C.c_int, [vp, i64, i32, i32, vp, i64, vp, i64, vp]),
    "vlp_mask_pack": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
    "vlp_layernorm_fwd": (C.c_int, [C.POINTER(LayerNormFwdArgs), vp]),
    "vlp_layernorm_bwd_workspace_bytes": (i64, [i32]),
    "vlp_layernorm_bwd": (C.c_int, [C.POINTER(LayerNormBwdArgs), vp]),
    "vlp_layernorm_bwd_rows": (C.c_int, [C.POINTER(LayerNormBwdArgs), vp, i32, i32, vp]),
    "vlp_layernorm_bwd_reduce_batched": (C.c_int, [vp, vp, i32, i32, i32, i32, vp]),
    "vlp_embed_fwd": (C.c_int, [C.POINTER(EmbedFwdArgs), vp]),
    "vlp_embed_bwd": (C.c_int, [C.POINTER(EmbedBwdArgs), vp]),
    "vlp_embed_bwd_pos": (C.c_int, [C.POINTER(EmbedBwdPosArgs), vp]),
    "vlp_scst_layout": (C.c_int, [C.POINTER(ScstLayoutArgs), vp]),
    "vlp_token_logprob_fwd": (C.c_int, [C.POINTER(TokenLogprobFwdArgs), vp]),
    "vlp_token_logprob_bwd": (C.c_int, [C.POINTER(TokenLogprobBwdArgs), vp]),
    "vlp_token_policy_fwd": (C.c_int, [C.POINTER(TokenPolicyFwdArgs), vp]),
    "vlp_token_policy_bwd": (C.c_int, [C.POINTER(TokenPolicyBwdArgs), vp]),
    "vlp_token_score": (C.c_int, [C.POINTER(TokenScoreArgs), vp]),
    "vlp_region_mask_build": (C.c_int, [vp, i32, i32, i32, vp, vp]),
    "vlp_pretext_fwd": (C.c_int, [C.POINTER(PretextFwdArgs), vp]),
    "vlp_pretext_bwd": (C.c_int, [C.POINTER(PretextBwdArgs), vp]),
    "vlp_copy2d": (C.c_int, [vp, i64, i32, vp, i64, i32, i32, i32, i32, vp]),
    "vlp_transpose": (C.c_int, [vp, i64, vp, i64, i32, i32, i32, vp]),
    "vlp_transpose_batched": (C.c_int, [vp, vp, i32, i32, vp]),
    "vlp_gather_rows": (C.c_int, [vp, i64, vp, vp, i64, i32, i32, i32, i32, vp, vp]),
    "vlp_scatter_add_rows": (C.c_int, [vp, i64, vp, vp, i64, i32, i32, i32, i32, vp, vp]),
    "vlp_live_rows_build": (C.c_int, [vp, i32, i32, i32, vp, vp, vp, vp]),
    "vlp_rowmap_build": (C.c_int, [vp, i32, i32, vp, vp]),
    "vlp_rows_unpack": (C.c_int, [vp, i64, vp, i32, vp, i64, i32, vp]),
    "vlp_rows_pack": (C.c_int, [vp, i64, vp, i32, vp, i64, i32, vp]),
    "vlp_vqa_mul_fwd": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp]),
    "vlp_vqa_mul_bwd": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "vlp_relu_dropout_bwd": (C.c_int, [vp, vp, vp, i64, i64, f32, u64, u32, vp]),
    "vlp_gelu_bwd": (C.c_int, [vp, vp, vp, i64, vp]),
    "vlp_cider_d_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "vlp_cider_d": (C.c_int, [C.POINTER(CiderDArgs), vp]),
    "vlp_cider_d_df_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "vlp_cider_d_df": (C.c_int, [C.POINTER(CiderDDfArgs), vp]),
    "vlp_cider_d_multi_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "vlp_cider_d_multi": (C.c_int, [C.POINTER(CiderDArgs), vp]),
    "vlp_cider_d_multi_df_workspace_bytes": (i64, [i32, i32, i32, i32]),
    "vlp_cider_d_multi_df": (C.c_int, [C.POINTER(CiderDDfArgs), vp]),
    "vlp_cider_d_consensus_workspace_bytes": (i64, [i32, i32, i32]),
    "vlp_cider_d_consensus": (C.c_int, [C.POINTER(CiderDConsensusArgs), vp]),
    "vlp_bleu4": (C.c_int, [C.POINTER(Bleu4Args), vp]),
    "vlp_caption_eval_workspace_bytes": (i64, [i32, i32, i32]),
    "vlp_caption_eval": (C.c_int, [C.POINTER(CaptionEvalArgs), vp]),
    "vlp_mlm_loss_fwd": (C.c_int, [C.POINTER(MlmLossFwdArgs), vp]),
    "vlp_mlm_loss_bwd": (C.c_int, [C.POINTER(MlmLossBwdArgs), vp]),
    "vlp_mlm_loss_ls_fwd": (C.c_int, [C.POINTER(MlmLossLsFwdArgs), vp]),
    "vlp_mlm_loss_ls_bwd": (C.c_int, [C.POINTER(MlmLossLsBwdArgs), vp]),
    "vlp_bce_loss_fwd": (C.c_int, [vp, i64, vp, i64, i32, i32, vp, vp]),
    "vlp_bce_loss_bwd": (C.c_int, [vp, i64, vp, i64, i32, i32, vp, vp, i64, vp]),
    "vlp_bce_sparse_loss_fwd": (C.c_int, [vp, i64, vp, vp, i32, i32, i32, vp, vp]),
    "vlp_bce_sparse_loss_bwd": (C.c_int, [vp, i64, vp, vp, i32, i32, i32, vp, vp, i64, vp]),
    "vlp_vqa_answer_rows": (C.c_int, [vp, i64, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp]),
    "vlp_sumsq": (C.c_int, [vp, i64, vp, vp, vp]),
    "vlp_sumsq_acc": (C.c_int, [vp, i64, vp, vp, vp]),
    "vlp_fused_adam": (C.c_int, [C.POINTER(FusedAdamArgs), vp]),
    "vlp_adam_hyper": (C.c_int, [vp, vp, vp, f32, f32, vp, vp]),
    "vlp_loss_scale_update": (C.c_int, [vp, vp, vp]),
    "vlp_bert_adam": (C.c_int, [C.POINTER(BertAdamArgs), vp]),
    "vlp_bert_adam_norms_floats": (i64, [i64, i32]),
}

_lib = None


# ---- launch plans ----------------------------------------------------------------------------------------------------
# The incremental decoder issues ~160 tiny launches per token step whose arguments (workspace pointers, shapes) are identical from
# call to call; building the ctypes structs and looking up strides every time made it host-bound (7 us per launch).  record() collects
# the C calls a block of Python makes, replay() re-issues them: ~1 us per launch.  A plan holds its argument objects alive; it is only
# valid while every buffer it points to is (the engine keeps plans inside the workspace they were recorded against).
_recording = None


class _Recorder(object):
    """Stands in for the loaded library while recording: every C call is executed AND appended to the plan."""

    def __init__(self, lib, plan):
        self._lib, self._plan = lib, plan

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self._plan.append((fn, args))
            return fn(*args)
        return call


class record(object):
    """with _lib.record() as plan: ...   (plan = list of (cfunc, args))"""

    def __enter__(self):
        global _recording
        if _recording is not None:
            raise RuntimeError("vlp_amd._lib.record(): already recording")
        self.plan = []
        _recording = _Recorder(load(), self.plan)
        return self.plan

    def __exit__(self, *exc):
        global _recording
        _recording = None
        return False


def replay(plan):
    for fn, args in plan:
        rc = fn(*args)
        if rc:
            _check(rc)


def load():
    """Load libvlp_hip.so (built by vlp_amd/build.py).  Raises if it is absent: there is no fallback."""
    global _lib
    if _recording is not None:
        return _recording
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libvlp_hip.so not found at %s -- run `python -m vlp_amd.build` (or "
                           "__graft_entry__.build()).  vlp_amd has no CPU / torch fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.vlp_version() != 5:      # include/vlp_hip.h VLP_ABI_VERSION
        raise RuntimeError("libvlp_hip.so ABI version mismatch")
    _lib = lib
    return lib


def lab_build():
    """True when the loaded library carries the investigation variants (-DVLP_LAB_BUILD)."""
    return bool(load().vlp_lab_build())


def _check(rc):
    if rc != 0:
        lib = _lib if _lib is not None else load()
        raise RuntimeError("libvlp_hip: %s (status %d)" % (lib.vlp_last_error_string().decode(), rc))


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("vlp_amd kernels need device tensors (got a CPU tensor); there is no CPU fallback")


# --------------------------------------------------------------------------------------------------
# thin typed wrappers
# --------------------------------------------------------------------------------------------------
def _gemm_nt_args(x, w, y, M, N, K, ldx, ldw, ldy, bias, residual, ldr, preact, ldp, mul_src, ldm, act, mul_mode, alpha, dropout_p, seed, rng_stream,
                  variant=0, row_map=None):
    """GemmNtArgs of gemm_nt / gemm_nt_splitk: a pitch left None is the tensor's row stride (0 without the tensor)."""
    return GemmNtArgs(ptr(x), ldx if ldx is not None else x.stride(0), ptr(w), ldw if ldw is not None else w.stride(0),
                      ptr(y), ldy if ldy is not None else y.stride(0), ptr(bias),
                      ptr(residual), (ldr if ldr is not None else (residual.stride(0) if residual is not None else 0)),
                      ptr(preact), (ldp if ldp is not None else (preact.stride(0) if preact is not None else 0)),
                      ptr(mul_src), (ldm if ldm is not None else (mul_src.stride(0) if mul_src is not None else 0)),
                      M, N, K, act, mul_mode, alpha, dropout_p, seed, rng_stream, variant, ptr(row_map))


def gemm_nt(x, w, y, M, N, K, ldx=None, ldw=None, ldy=None, bias=None, residual=None, ldr=None, preact=None, ldp=None,
            mul_src=None, ldm=None, act=ACT_NONE, mul_mode=MUL_NONE, alpha=1.0, dropout_p=0.0, seed=0, rng_stream=0,
            variant=0, row_map=None):
    _req_cuda(x, w, y, row_map)
    a = _gemm_nt_args(x, w, y, M, N, K, ldx, ldw, ldy, bias, residual, ldr, preact, ldp, mul_src, ldm, act, mul_mode, alpha, dropout_p, seed,
                      rng_stream, variant, row_map)
    _check(load().vlp_gemm_nt(C.byref(a), stream_ptr()))


def gemm_nt_rows(x, w, y, live, flags, M, N, K, ldx=None, ldw=None, ldy=None, bias=None, residual=None, ldr=None, mul_src=None, ldm=None,
                 mul_mode=MUL_NONE, alpha=1.0, dropout_p=0.0, seed=0, rng_stream=0, variant=0, row_map=None):
    """gemm_nt over the M entries of the device row list `live` (int32, -1 = pad): the operands named by `flags` (ROWS_*) are addressed at
    row live[m], the others at row m."""
    _req_cuda(x, w, y, live, row_map)
    a = _gemm_nt_args(x, w, y, M, N, K, ldx, ldw, ldy, bias, residual, ldr, None, None, mul_src, ldm, ACT_NONE, mul_mode, alpha, dropout_p, seed,
                      rng_stream, variant, row_map)
    _check(load().vlp_gemm_nt_rows(C.byref(a), ptr(live), flags, stream_ptr()))


def gemm_nt_resolved_variant():
    """The variant this thread's last gemm_nt actually launched (after the launcher's fallbacks)."""
    return int(load().vlp_gemm_nt_resolved_variant())


def gemm_nt_splitk_workspace_bytes(M, N, splits):
    return int(load().vlp_gemm_nt_splitk_workspace_bytes(M, N, splits))


def gemm_nt_splitk(x, w, y, M, N, K, splits, workspace, ldx=None, ldw=None, ldy=None, bias=None, residual=None, ldr=None, preact=None, ldp=None,
                   mul_src=None, ldm=None, act=ACT_NONE, mul_mode=MUL_NONE, alpha=1.0, dropout_p=0.0, seed=0, rng_stream=0):
    _req_cuda(x, w, y, workspace)
    a = _gemm_nt_args(x, w, y, M, N, K, ldx, ldw, ldy, bias, residual, ldr, preact, ldp, mul_src, ldm, act, mul_mode, alpha, dropout_p, seed,
                      rng_stream)
    _check(load().vlp_gemm_nt_splitk(C.byref(a), splits, ptr(workspace), _nbytes(workspace), stream_ptr()))


def gemm_tn_workspace_bytes(M, N, K):
    return int(load().vlp_gemm_tn_workspace_bytes(M, N, K))


def gemm_tn(a_, b_, c_, M, N, K, lda=None, ldb=None, ldc=None, beta=0, workspace=None, variant=0, splits=0, bias_out=None):
    _req_cuda(a_, b_, c_)
    a = GemmTnArgs(ptr(a_), lda if lda is not None else a_.stride(0), ptr(b_), ldb if ldb is not None else b_.stride(0),
                   ptr(c_), ldc if ldc is not None else c_.stride(0), M, N, K, beta,
                   ptr(workspace), _nbytes(workspace), variant, splits,
                   ptr(bias_out))
    _check(load().vlp_gemm_tn(C.byref(a), stream_ptr()))


def gemm_tn_grouped_workspace_bytes(tiles):
    return int(load().vlp_gemm_tn_grouped_workspace_bytes(tiles))


def gemm_tn_grouped(problems, workspace=None):
    """problems: list of tuples (a, b, c, M, N, K, beta, bias_out) -- several wgrads in one launch (vlp_gemm_tn_grouped); `workspace`
    (gemm_tn_grouped_workspace_bytes) lets the launcher use its stream-K form."""
    arr = (GemmTnArgs * len(problems))()
    for i, (a_, b_, c_, M, N, K, beta, bias_out) in enumerate(problems):
        _req_cuda(a_, b_, c_, bias_out)
        w = workspace if i == 0 else None
        if w is not None:
            _req_cuda(w)
        arr[i] = GemmTnArgs(ptr(a_), a_.stride(0), ptr(b_), b_.stride(0), ptr(c_), c_.stride(0), M, N, K, beta, ptr(w),
                            _nbytes(w), 0, 0, ptr(bias_out))
    _check(load().vlp_gemm_tn_grouped(arr, len(problems), stream_ptr()))


def gemm_tn_grouped_mapped(problems, row_map, count):
    """gemm_tn_grouped contracting over the rows row_map[0 .. count[0]) of both operands (device int32 [M] and [1]; one M for all problems)."""
    _req_cuda(row_map, count)
    arr = (GemmTnArgs * len(problems))()
    for i, (a_, b_, c_, M, N, K, beta, bias_out) in enumerate(problems):
        _req_cuda(a_, b_, c_, bias_out)
        if row_map.numel() < M:
            raise RuntimeError("gemm_tn_grouped_mapped: the map has %d entries, the problem %d rows" % (row_map.numel(), M))
        arr[i] = GemmTnArgs(ptr(a_), a_.stride(0), ptr(b_), b_.stride(0), ptr(c_), c_.stride(0), M, N, K, beta, None, 0, 0, 0, ptr(bias_out))
    _check(load().vlp_gemm_tn_grouped_mapped(arr, ptr(row_map), ptr(count), len(problems), stream_ptr()))


def gemm_tn_grouped_rows(problems):
    """problems: list of tuples (a, b, c, M, N, K, beta, bias_out, live, flags): gemm_tn_grouped with a row list per problem (live = None:
    the problem as in gemm_tn_grouped); b is read at row live[m], a at live[m] with ROWS_X, else at row m."""
    n = len(problems)
    arr = (GemmTnArgs * n)()
    lives = (vp * n)()
    flags = (i32 * n)()
    for i, (a_, b_, c_, M, N, K, beta, bias_out, live, fl) in enumerate(problems):
        _req_cuda(a_, b_, c_, bias_out, live)
        arr[i] = GemmTnArgs(ptr(a_), a_.stride(0), ptr(b_), b_.stride(0), ptr(c_), c_.stride(0), M, N, K, beta, None, 0, 0, 0, ptr(bias_out))
        lives[i] = live.data_ptr() if live is not None else None
        flags[i] = fl
    _check(load().vlp_gemm_tn_grouped_rows(arr, lives, flags, n, stream_ptr()))


def colsum_workspace_bytes(M, N):
    return int(load().vlp_colsum_workspace_bytes(M, N))


def colsum(a_, out, M, N, lda=None, beta=0, workspace=None):
    _req_cuda(a_, out)
    a = ColsumArgs(ptr(a_), lda if lda is not None else a_.stride(0), M, N, ptr(out), beta, ptr(workspace),
                   _nbytes(workspace))
    _check(load().vlp_colsum(C.byref(a), stream_ptr()))


def attn_fwd(qkv, mask, ctx, lse, B, L, heads, scale, dropout_p=0.0, seed=0, rng_stream=0, row_off=None):
    """row_off (int32 [B+1], device): packed rows -- sample b owns rows [row_off[b], row_off[b+1]) of qkv / ctx (include/vlp_hip.h)."""
    _req_cuda(qkv, mask, ctx, lse, row_off)
    a = AttnFwdArgs(ptr(qkv), qkv.stride(0), ptr(mask), ptr(ctx), ctx.stride(0), ptr(lse), B, L, heads, scale, dropout_p, seed, rng_stream,
                    ptr(row_off))
    _check(load().vlp_attn_fwd(C.byref(a), stream_ptr()))


def attn_bwd(qkv, mask, mask_t, ctx, dctx, lse, dqkv, delta, B, L, heads, scale, dropout_p=0.0, seed=0, rng_stream=0, row_off=None):
    _req_cuda(qkv, mask, mask_t, ctx, dctx, lse, dqkv, delta, row_off)
    a = AttnBwdArgs(ptr(qkv), qkv.stride(0), ptr(mask), ptr(mask_t), ptr(ctx), ctx.stride(0), ptr(dctx), dctx.stride(0), ptr(lse),
                    ptr(dqkv), dqkv.stride(0), ptr(delta), B, L, heads, scale, dropout_p, seed, rng_stream, ptr(row_off))
    _check(load().vlp_attn_bwd(C.byref(a), stream_ptr()))


def attn_decode(q, ld_q, q_rows, k, v, ld_kv, kv_rows, mask, ctx, B, Lq, Lk, heads, scale, k_prefix=None, v_prefix=None, prefix_rows=0,
                n_prefix=0, beams=1):
    _req_cuda(q, k, v, mask, ctx, k_prefix, v_prefix)
    a = AttnDecodeArgs(ptr(q), ld_q, q_rows, ptr(k), ptr(v), ld_kv, kv_rows, ptr(mask), ptr(ctx), ctx.stride(0), B, Lq, Lk, heads, scale,
                       ptr(k_prefix), ptr(v_prefix), prefix_rows, n_prefix, beams)
    _check(load().vlp_attn_decode(C.byref(a), stream_ptr()))


def dec_gemm(x, w, M, N, Kd, y=None, bias=None, act=0, slab=None, splits=1, kv_cache=None, kv_col0=0, kv_Lcap=0, kv_T=1, kv_start=0,
             residual=None, ln_gamma=None, ln_beta=None, ln_eps=1e-5, ln_out=None):
    """Token-step Linear (csrc/decode.hip): y [M, N] fp16 (optionally K | V columns >= kv_col0 into kv_cache [seq, kv_Lcap, ld]) or, with
    `slab` (fp32 [splits, M, ldslab]), raw split-K partial sums for dec_reduce_ln."""
    _req_cuda(x, w, y, bias, slab, kv_cache, residual, ln_gamma, ln_beta, ln_out)
    a = DecGemmArgs(ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(y), y.stride(0) if y is not None else 0,
                    ptr(slab), slab.stride(1) if slab is not None else 0, ptr(kv_cache), kv_cache.stride(1) if kv_cache is not None else 0,
                    kv_col0, kv_Lcap, kv_T, kv_start, M, N, Kd, splits, act,
                    ptr(residual), residual.stride(0) if residual is not None else 0, ptr(ln_gamma), ptr(ln_beta), ln_eps,
                    ptr(ln_out), ln_out.stride(0) if ln_out is not None else 0)
    _check(load().vlp_dec_gemm(C.byref(a), stream_ptr()))


def dec_reduce_ln(slab, splits, bias, residual, gamma, beta, y, M, H, eps=1e-5):
    _req_cuda(slab, bias, residual, gamma, beta, y)
    a = DecReduceLnArgs(ptr(slab), slab.stride(1), splits, ptr(bias), ptr(residual), residual.stride(0) if residual is not None else 0,
                        ptr(gamma), ptr(beta), eps, ptr(y), y.stride(0), M, H)
    _check(load().vlp_dec_reduce_ln(C.byref(a), stream_ptr()))


def argmax_rows2(logits, ld, rows, V, ids_a, ids_b, vals):
    _req_cuda(logits, ids_a, ids_b, vals)
    _check(load().vlp_argmax_rows2(ptr(logits), ld, rows, V, ptr(ids_a), ids_a.stride(0), ptr(ids_b), ids_b.stride(0) if ids_b is not None else 0,
                                   ptr(vals), vals.stride(0), stream_ptr()))


def mask_pack_rect(mask_view, out_u8, B, Lq, Lk, Lkp):
    """mask_view: int64 tensor view [B, Lq, Lk] with unit column stride (any batch / row strides)."""
    _req_cuda(mask_view, out_u8)
    assert mask_view.stride(2) == 1 and mask_view.dtype == torch.int64
    _check(load().vlp_mask_pack_rect(ptr(mask_view), mask_view.stride(0), mask_view.stride(1), ptr(out_u8), B, Lq, Lk, Lkp, stream_ptr()))


def kv_append(qkv_new, ld, cache, Lcap, B, T, start, H):
    _req_cuda(qkv_new, cache)
    _check(load().vlp_kv_append(ptr(qkv_new), ld, ptr(cache), Lcap, B, T, start, H, stream_ptr()))


def argmax_rows(logits, ld, rows, V, ids, vals):
    """ids / vals: 1-D (possibly strided) views with `rows` elements."""
    _req_cuda(logits, ids, vals)
    _check(load().vlp_argmax_rows(ptr(logits), ld, rows, V, ptr(ids), ids.stride(0), ptr(vals), vals.stride(0), stream_ptr()))


def logsoftmax_topk(logits, ld, rows, V, K, out_scores, out_ids, forbid=None, eos_id=0, block_eos=False):
    _req_cuda(logits, out_scores, out_ids, forbid)
    _check(load().vlp_logsoftmax_topk(ptr(logits), ld, rows, V, K, ptr(forbid), eos_id, 1 if block_eos else 0, ptr(out_scores), ptr(out_ids),
                                      stream_ptr()))


def ngram_candidates(wids, ptrs, B, K, s, ngram_size, cand_ids, cand_cnt, ignore_ids=None):
    """wids / ptrs: contiguous int64 [frames, B, K]; cand_ids int32 [B*K, C] (row stride = stride(0) >= s + 1), cand_cnt int32 [B*K];
    ignore_ids: int64 device vector or None."""
    _req_cuda(wids, ptrs, cand_ids, cand_cnt, ignore_ids)
    assert wids.dtype == torch.int64 and ptrs.dtype == torch.int64 and wids.is_contiguous() and ptrs.is_contiguous()
    assert tuple(wids.shape[1:]) == (B, K) and tuple(ptrs.shape[1:]) == (B, K) and s < wids.shape[0] and s < ptrs.shape[0]
    assert cand_ids.dtype == torch.int32 and cand_cnt.dtype == torch.int32 and cand_ids.stride(1) == 1 and cand_cnt.is_contiguous()
    assert cand_ids.shape[0] >= B * K and cand_cnt.numel() >= B * K
    n_ignore = 0
    if ignore_ids is not None:
        assert ignore_ids.dtype == torch.int64 and ignore_ids.is_contiguous()
        n_ignore = ignore_ids.numel()
    _check(load().vlp_ngram_candidates(ptr(wids), ptr(ptrs), B, K, s, ngram_size, ptr(ignore_ids) if n_ignore else None, n_ignore, ptr(cand_ids),
                                       cand_ids.stride(0), ptr(cand_cnt), stream_ptr()))


def logsoftmax_topk_list(logits, ld, rows, V, K, out_scores, out_ids, cand_ids, cand_cnt, eos_id=0, block_eos=False):
    """logsoftmax_topk with row r's forbidden words = cand_ids[r, :cand_cnt[r]] (int32; what ngram_candidates writes)."""
    _req_cuda(logits, out_scores, out_ids, cand_ids, cand_cnt)
    assert cand_ids.dtype == torch.int32 and cand_cnt.dtype == torch.int32 and cand_ids.stride(1) == 1 and cand_cnt.is_contiguous()
    assert cand_ids.shape[0] >= rows and cand_cnt.numel() >= rows
    _check(load().vlp_logsoftmax_topk_list(ptr(logits), ld, rows, V, K, ptr(cand_ids), cand_ids.stride(0), ptr(cand_cnt), eos_id, 1 if block_eos else 0,
                                           ptr(out_scores), ptr(out_ids), stream_ptr()))


def beam_select(kk_scores, kk_ids, last_total, last_eos, out_scores, out_ids, out_ptrs, out_eos, src_rows, next_ids, B, K, first, eos_id):
    """next_ids: 1-D (possibly strided) int64 view with B*K elements."""
    _req_cuda(kk_scores, kk_ids, last_total, last_eos, out_scores, out_ids, out_ptrs, out_eos, src_rows, next_ids)
    a = BeamSelectArgs(ptr(kk_scores), ptr(kk_ids), ptr(last_total), ptr(last_eos), ptr(out_scores), ptr(out_ids), ptr(out_ptrs), ptr(out_eos),
                       ptr(src_rows), ptr(next_ids), next_ids.stride(0), B, K, 1 if first else 0, eos_id)
    _check(load().vlp_beam_select(C.byref(a), stream_ptr()))


def beam_select_groups(kk_scores, kk_ids, last_total, last_eos, out_scores, out_ids, out_ptrs, out_eos, src_rows, next_ids, B, K, first, eos_id,
                       groups, penalty):
    """beam_select with the K beams in `groups` groups and a penalty per earlier pick of the same word (vlp_amd.diverse is the rule)."""
    _req_cuda(kk_scores, kk_ids, last_total, last_eos, out_scores, out_ids, out_ptrs, out_eos, src_rows, next_ids)
    a = BeamSelectArgs(ptr(kk_scores), ptr(kk_ids), ptr(last_total), ptr(last_eos), ptr(out_scores), ptr(out_ids), ptr(out_ptrs), ptr(out_eos),
                       ptr(src_rows), ptr(next_ids), next_ids.stride(0) if next_ids is not None else 0, B, K, 1 if first else 0, eos_id)
    _check(load().vlp_beam_select_groups(C.byref(a), int(groups), float(penalty), stream_ptr()))


def logsoftmax_topk_want(logits, ld, rows, V, K, out_scores, out_ids, want_ids, want_val, forbid=None, cand_ids=None, cand_cnt=None, eos_id=0,
                         block_eos=False):
    """logsoftmax_topk (dense `forbid` or none) or logsoftmax_topk_list (`cand_ids` / `cand_cnt`) -- same kernels, same top-K bits -- that also
    writes want_val[r, c] f32 = row r's value of word want_ids[r, c] (int32 [rows, C], C <= 8; -1 gives -inf)."""
    _req_cuda(logits, out_scores, out_ids, want_ids, want_val, forbid, cand_ids, cand_cnt)
    assert want_ids.dtype == torch.int32 and want_val.dtype == torch.float32 and want_ids.is_contiguous() and want_val.is_contiguous()
    assert want_ids.dim() == 2 and want_ids.shape[0] >= rows and tuple(want_val.shape) == tuple(want_ids.shape)
    cand_ld = 0
    if cand_ids is not None:
        assert cand_ids.dtype == torch.int32 and cand_cnt.dtype == torch.int32 and cand_ids.stride(1) == 1 and cand_cnt.is_contiguous()
        assert cand_ids.shape[0] >= rows and cand_cnt.numel() >= rows
        cand_ld = cand_ids.stride(0)
    _check(load().vlp_logsoftmax_topk_want(ptr(logits), ld, rows, V, K, ptr(forbid), ptr(cand_ids), cand_ld, ptr(cand_cnt), eos_id,
                                           1 if block_eos else 0, ptr(want_ids), want_ids.shape[1], ptr(out_scores), ptr(out_ids), ptr(want_val),
                                           stream_ptr()))


def beam_select_constrained(kk_scores, kk_ids, last_total, last_eos, out_scores, out_ids, out_ptrs, out_eos, src_rows, next_ids, B, K, first, eos_id,
                            want_ids, want_val, prev_state, cons_ids, cons_len, C_, Lc, out_state, want_next, last=False):
    """beam_select under lexical constraints (vlp_amd.constrained is the rule): int32 want_ids / f32 want_val [rows, C], prev_state [B, K] (None
    on the first frame), cons_ids [B, C, Lc], cons_len [B, C], out_state [B, K], want_next [B*K, C]; all contiguous.  last: the search's last frame."""
    _req_cuda(kk_scores, kk_ids, last_total, last_eos, out_scores, out_ids, out_ptrs, out_eos, src_rows, next_ids, want_ids, want_val, prev_state,
              cons_ids, cons_len, out_state, want_next)
    for t in (want_ids, prev_state, cons_ids, cons_len, out_state, want_next):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous())
    assert want_val is None or (want_val.dtype == torch.float32 and want_val.is_contiguous())
    a = BeamSelectArgs(ptr(kk_scores), ptr(kk_ids), ptr(last_total), ptr(last_eos), ptr(out_scores), ptr(out_ids), ptr(out_ptrs), ptr(out_eos),
                       ptr(src_rows), ptr(next_ids), next_ids.stride(0) if next_ids is not None else 0, B, K, 1 if first else 0, eos_id)
    _check(load().vlp_beam_select_constrained(C.byref(a), ptr(want_ids), ptr(want_val), ptr(prev_state), ptr(cons_ids), ptr(cons_len), int(C_), int(Lc),
                                              1 if last else 0, ptr(out_state), ptr(want_next), stream_ptr()))


def kv_gather(src, src_rows, dst, dst_rows, idx, R, lo, hi, row_elems):
    _req_cuda(src, dst, idx)
    _check(load().vlp_kv_gather(ptr(src), src_rows, ptr(dst), dst_rows, ptr(idx), R, lo, hi, row_elems, stream_ptr()))


def beam_nbest(tot, wids, ptrs, n_best, eos_id, length_penalty, seq, score, value, length, ok):
    """tot f32 / wids / ptrs int64: contiguous frames [F, B, K] (Engine.decode_beam).  Outputs, sample-major (rank n of sample b = row n*B + b):
    seq int64 [n_best*B, T] (row stride = stride(0) = T >= F), score f32, value f64, length int32, ok uint8, each [n_best*B]."""
    _req_cuda(tot, wids, ptrs, seq, score, value, length, ok)
    shape = next((tuple(t.shape) for t in (tot, wids, ptrs) if t is not None), ())
    F, B, K = (int(v) for v in shape) if len(shape) == 3 else (0, 0, 0)
    for t, dt in ((tot, torch.float32), (wids, torch.int64), (ptrs, torch.int64)):
        assert t is None or (t.dtype == dt and t.is_contiguous() and tuple(t.shape) == (F, B, K))
    rows = int(n_best) * B
    T = 0
    if seq is not None:
        assert seq.dtype == torch.int64 and seq.dim() == 2 and seq.is_contiguous() and seq.shape[0] >= rows
        T = int(seq.shape[1])
    for t, dt in ((score, torch.float32), (value, torch.float64), (length, torch.int32), (ok, torch.uint8)):
        assert t is None or (t.dtype == dt and t.is_contiguous() and t.numel() >= rows)
    _check(load().vlp_beam_nbest(ptr(tot), ptr(wids), ptr(ptrs), F, B, K, int(eos_id), float(length_penalty), int(n_best), T, ptr(seq), ptr(score),
                                 ptr(value), ptr(length), ptr(ok), stream_ptr()))


def mask_build(second_st, second_end, is_s2s, out_u8, B, L, Lp, out_t=None, region_mask=None, Nv=0):
    """second_st / second_end / is_s2s: int32 [B] device tensors; region_mask: u8 [B*Nv] (region_mask_build) -> those key columns are blocked."""
    _req_cuda(second_st, second_end, is_s2s, out_u8, out_t, region_mask)
    for t in (second_st, second_end, is_s2s):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B
    _check(load().vlp_mask_build(ptr(second_st), ptr(second_end), ptr(is_s2s), ptr(out_u8), ptr(out_t), B, L, Lp, ptr(region_mask), Nv, stream_ptr()))


def vis_pe_prep(bbox, cls, out, B, Nv, n_cls, pad_to, eps=1e-5):
    """bbox f32 [B,Nv,6]; cls f16/f32 [B*Nv, >=n_cls] (row stride = stride(0)); out f16 [B*Nv, >=pad_to]."""
    _req_cuda(bbox, cls, out)
    assert bbox.dtype == torch.float32 and bbox.is_contiguous() and cls.dtype in (torch.float16, torch.float32) and cls.stride(-1) == 1
    a = VisPePrepArgs(ptr(bbox), ptr(cls), cls.stride(0), ptr(out), out.stride(0), B, Nv, n_cls, pad_to, 1 if cls.dtype == torch.float32 else 0, eps)
    _check(load().vlp_vis_pe_prep(C.byref(a), stream_ptr()))


def sample_rows(logits, ld, rows, V, seed, rng_stream, ids, logp):
    """ids / logp: 1-D (possibly strided) views with `rows` elements."""
    _req_cuda(logits, ids, logp)
    _check(load().vlp_sample_rows(ptr(logits), ld, rows, V, seed, rng_stream, ptr(ids), ids.stride(0), ptr(logp), logp.stride(0), stream_ptr()))


def sample_rows_rep(logits, ld, rows, V, rep, seed_cell, seed_add, rng_stream, ids, logp, ids2=None):
    """sample_rows with `rep` draws per logits row (draw r reads row r // rep, RNG row key r) and the seed *seed_cell + seed_add read on the
    device: seed_cell is an int64 device tensor of one element holding the uint64 seed's bits.  ids2 (optional) receives the same ids."""
    _req_cuda(logits, seed_cell, ids, logp, ids2)
    if seed_cell.dtype not in (torch.int64, torch.uint64) or seed_cell.numel() < 1:
        raise RuntimeError("vlp_amd.sample_rows_rep: seed_cell must be an int64 device tensor of one element")
    if logits.numel() < ((rows + rep - 1) // rep - 1) * ld + V:
        raise RuntimeError("vlp_amd.sample_rows_rep: logits are shorter than ceil(rows / rep) rows of pitch ld")
    _check(load().vlp_sample_rows_rep(ptr(logits), ld, rows, V, rep, ptr(seed_cell), int(seed_add) & 0xFFFFFFFFFFFFFFFF, rng_stream, ptr(ids),
                                      ids.stride(0), ptr(ids2), ids2.stride(0) if ids2 is not None else 0, ptr(logp), logp.stride(0), stream_ptr()))


def sample_rows_filtered(logits, ld, rows, V, rep, seed_cell, seed_add, rng_stream, temperature, top_k, top_p, ids, logp, ids2=None, cutoff=None,
                         kept=None):
    """sample_rows_rep's draw from softmax(logits / temperature) restricted to the top_k largest logits (0 = off; ties kept) and then to the
    smallest value threshold that holds a mass of top_p (1 = off); logp is the log-probability under that distribution.  cutoff (f32 [rows])
    / kept (int32 [rows]), optional and contiguous: the smallest kept logit and the size of the kept set of every draw."""
    _req_cuda(logits, seed_cell, ids, logp, ids2, cutoff, kept)
    if seed_cell.dtype not in (torch.int64, torch.uint64) or seed_cell.numel() < 1:
        raise RuntimeError("vlp_amd.sample_rows_filtered: seed_cell must be an int64 device tensor of one element")
    if rep >= 1 and logits.numel() < ((rows + rep - 1) // rep - 1) * ld + V:
        raise RuntimeError("vlp_amd.sample_rows_filtered: logits are shorter than ceil(rows / rep) rows of pitch ld")
    if cutoff is not None and (cutoff.dtype != torch.float32 or not cutoff.is_contiguous() or cutoff.numel() < rows):
        raise RuntimeError("vlp_amd.sample_rows_filtered: cutoff must be a contiguous float32 tensor of `rows` elements")
    if kept is not None and (kept.dtype != torch.int32 or not kept.is_contiguous() or kept.numel() < rows):
        raise RuntimeError("vlp_amd.sample_rows_filtered: kept must be a contiguous int32 tensor of `rows` elements")
    _check(load().vlp_sample_rows_filtered(ptr(logits), ld, rows, V, rep, ptr(seed_cell), int(seed_add) & 0xFFFFFFFFFFFFFFFF, rng_stream,
                                           float(temperature), int(top_k), float(top_p), ptr(ids), ids.stride(0), ptr(ids2),
                                           ids2.stride(0) if ids2 is not None else 0, ptr(logp), logp.stride(0), ptr(cutoff), ptr(kept), stream_ptr()))


def mask_pack(mask_i64, out_u8, B, L, Lp, out_t=None):
    _req_cuda(mask_i64, out_u8, out_t)
    _check(load().vlp_mask_pack(ptr(mask_i64), ptr(out_u8), ptr(out_t), B, L, Lp, stream_ptr()))


def layernorm_fwd(x, gamma, beta, y, M, H, mean=None, rstd=None, eps=1e-5, dropout_p=0.0, seed=0, rng_stream=0, ldx=None, ldy=None, row_map=None):
    _req_cuda(x, gamma, beta, y, row_map)
    a = LayerNormFwdArgs(ptr(x), ldx if ldx is not None else x.stride(0), ptr(gamma), ptr(beta), ptr(y),
                         ldy if ldy is not None else y.stride(0), ptr(mean), ptr(rstd), M, H, eps, dropout_p, seed, rng_stream, ptr(row_map))
    _check(load().vlp_layernorm_fwd(C.byref(a), stream_ptr()))


def layernorm_bwd_workspace_bytes(H):
    return int(load().vlp_layernorm_bwd_workspace_bytes(H))


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, M, H, workspace, beta=0, dx_drop=None,
                  dy_drop=(0.0, 0, 0), out_drop=(0.0, 0, 0), defer_reduce=False, row_map=None):
    """defer_reduce: leave the dgamma / dbeta partials in `workspace` (one private slot per LayerNorm) for layernorm_bwd_reduce_batched."""
    _req_cuda(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, workspace, row_map)
    a = LayerNormBwdArgs(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), dx.stride(0),
                         ptr(dx_drop), dx_drop.stride(0) if dx_drop is not None else 0, ptr(dgamma), ptr(dbeta), M, H, beta,
                         dy_drop[0], dy_drop[1], dy_drop[2], out_drop[0], out_drop[1], out_drop[2],
                         ptr(workspace), _nbytes(workspace), 1 if defer_reduce else 0, ptr(row_map))
    _check(load().vlp_layernorm_bwd(C.byref(a), stream_ptr()))


def layernorm_bwd_rows(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, live, flags, M, H, workspace, part_M, beta=0, dx_drop=None,
                       out_drop=(0.0, 0, 0), defer_reduce=False, row_map=None):
    """layernorm_bwd over the M entries of the device row list `live`: x / mean / rstd at row live[m], dy with ROWS_X, dx with ROWS_Y; the
    workspace gets the partial rows of an unlisted launch over part_M rows."""
    _req_cuda(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, workspace, row_map, live)
    a = LayerNormBwdArgs(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), dx.stride(0),
                         ptr(dx_drop), dx_drop.stride(0) if dx_drop is not None else 0, ptr(dgamma), ptr(dbeta), M, H, beta,
                         0.0, 0, 0, out_drop[0], out_drop[1], out_drop[2],
                         ptr(workspace), _nbytes(workspace), 1 if defer_reduce else 0, ptr(row_map))
    _check(load().vlp_layernorm_bwd_rows(C.byref(a), ptr(live), flags, part_M, stream_ptr()))


def layernorm_bwd_reduce_batched(parts, dst_table, count, M, H, beta=0):
    """parts: uint8/float32 buffer of `count` slots of layernorm_bwd_workspace_bytes(H); dst_table: int64 device tensor [count, 2] of
    dgamma / dbeta addresses."""
    _req_cuda(parts, dst_table)
    _check(load().vlp_layernorm_bwd_reduce_batched(ptr(parts), ptr(dst_table), count, M, H, beta, stream_ptr()))


def embed_fwd(input_ids, segment_ids, word_emb, pos_emb, type_emb, vis_h, vispe_h, pre, B, L, Nv, H, position_ids=None, region_mask=None,
              row_map=None, rows=0):
    """row_map (int32 [rows], device): packed output -- row p of `pre` is logical row row_map[p] = b*L + l."""
    _req_cuda(input_ids, segment_ids, word_emb, pos_emb, type_emb, pre, position_ids, region_mask, row_map)
    a = EmbedFwdArgs(ptr(input_ids), ptr(segment_ids), ptr(word_emb), ptr(pos_emb), ptr(type_emb), ptr(vis_h), ptr(vispe_h),
                     ptr(pre), B, L, Nv, H, word_emb.shape[0], type_emb.shape[0], ptr(position_ids), pos_emb.shape[0], ptr(region_mask),
                     ptr(row_map), rows)
    _check(load().vlp_embed_fwd(C.byref(a), stream_ptr()))


def embed_bwd_workspace_floats(B, L, Nv, H):
    return int(load().vlp_embed_bwd_workspace_floats(B, L, Nv, H))


def _embed_bwd_args(dpre, input_ids, segment_ids, vis_h, vispe_h, d_word, d_pos, d_type, d_vis_h, d_vispe_h, acc32,
                    B, L, Nv, H, vocab, type_vocab, drop_p, seed, vis_stream, vispe_stream, region_mask, parts):
    _req_cuda(dpre, input_ids, segment_ids, d_word, d_pos, d_type, acc32, region_mask)
    return EmbedBwdArgs(ptr(dpre), ptr(input_ids), ptr(segment_ids), ptr(vis_h), ptr(vispe_h), ptr(d_word), ptr(d_pos), ptr(d_type),
                        ptr(d_vis_h), ptr(d_vispe_h), ptr(acc32), B, L, Nv, H, vocab, type_vocab, drop_p, seed, vis_stream, vispe_stream,
                        ptr(region_mask), parts)


def embed_bwd(dpre, input_ids, segment_ids, vis_h, vispe_h, d_word, d_pos, d_type, d_vis_h, d_vispe_h, acc32,
              B, L, Nv, H, vocab, type_vocab, drop_p=0.0, seed=0, vis_stream=0, vispe_stream=0, region_mask=None, parts=0):
    """parts: 0 = everything, 1 = region rows only (d_vis_h / d_vispe_h), 2 = the embedding tables only."""
    a = _embed_bwd_args(dpre, input_ids, segment_ids, vis_h, vispe_h, d_word, d_pos, d_type, d_vis_h, d_vispe_h, acc32,
                        B, L, Nv, H, vocab, type_vocab, drop_p, seed, vis_stream, vispe_stream, region_mask, parts)
    _check(load().vlp_embed_bwd(C.byref(a), stream_ptr()))


def embed_bwd_pos(dpre, input_ids, segment_ids, position_ids, vis_h, vispe_h, d_word, d_pos, d_type, d_vis_h, d_vispe_h, acc32,
                  B, L, Nv, H, vocab, type_vocab, drop_p=0.0, seed=0, vis_stream=0, vispe_stream=0, region_mask=None, parts=0):
    """embed_bwd with position_ids (int64 [B, L], device): row (b, l) adds into d_pos[position_ids[b, l]]."""
    _req_cuda(position_ids)
    base = _embed_bwd_args(dpre, input_ids, segment_ids, vis_h, vispe_h, d_word, d_pos, d_type, d_vis_h, d_vispe_h, acc32,
                           B, L, Nv, H, vocab, type_vocab, drop_p, seed, vis_stream, vispe_stream, region_mask, parts)
    a = EmbedBwdPosArgs(base, ptr(position_ids), d_pos.shape[0])
    _check(load().vlp_embed_bwd_pos(C.byref(a), stream_ptr()))


def scst_layout(prefix_ids, sample_ids, segment_ids, position_ids, mask, out_ids, out_segment_ids, out_position_ids, out_mask, masked_pos,
                mask_word_id):
    """The SCST scoring sequence (include/vlp_hip.h vlp_scst_layout); every tensor contiguous int64 on the device."""
    _req_cuda(prefix_ids, sample_ids, segment_ids, position_ids, mask, out_ids, out_segment_ids, out_position_ids, out_mask, masked_pos)
    B, in_len = prefix_ids.shape
    T, L = sample_ids.shape[1], segment_ids.shape[1]
    for t in (prefix_ids, sample_ids, segment_ids, position_ids, mask, out_ids, out_segment_ids, out_position_ids, out_mask, masked_pos):
        if t.dtype != torch.long or not t.is_contiguous():
            raise RuntimeError("vlp_amd.scst_layout: operands must be contiguous int64")
    Lo = in_len + 2 * T - 1
    if (tuple(sample_ids.shape) != (B, T) or tuple(position_ids.shape) != (B, L) or tuple(mask.shape) != (B, L, L) or
            tuple(out_ids.shape) != (B, Lo) or tuple(out_segment_ids.shape) != (B, Lo) or tuple(out_position_ids.shape) != (B, Lo) or
            tuple(out_mask.shape) != (B, Lo, Lo) or tuple(masked_pos.shape) != (B, T)):
        raise RuntimeError("vlp_amd.scst_layout: shape mismatch")
    a = ScstLayoutArgs(ptr(prefix_ids), ptr(sample_ids), ptr(segment_ids), ptr(position_ids), ptr(mask), ptr(out_ids), ptr(out_segment_ids),
                       ptr(out_position_ids), ptr(out_mask), ptr(masked_pos), B, L, in_len, T, int(mask_word_id))
    _check(load().vlp_scst_layout(C.byref(a), stream_ptr()))


def token_logprob_fwd(logits, ld, ids, logp, lse, rows, V):
    _req_cuda(logits, ids, logp, lse)
    a = TokenLogprobFwdArgs(ptr(logits), ld, ptr(ids), ptr(logp), ptr(lse), rows, V)
    _check(load().vlp_token_logprob_fwd(C.byref(a), stream_ptr()))


def token_logprob_bwd(logits, ld, ids, lse, g, dlogits, ldd, rows, V):
    _req_cuda(logits, ids, lse, g, dlogits)
    a = TokenLogprobBwdArgs(ptr(logits), ld, ptr(ids), ptr(lse), ptr(g), ptr(dlogits), ldd, rows, V)
    _check(load().vlp_token_logprob_bwd(C.byref(a), stream_ptr()))


def token_policy_fwd(logits, ld, ids, logp, lse, rows, V, temperature=1.0, entropy=None):
    """logp / lse (and entropy [rows] f32, when given) of softmax(logits / temperature) at ids (include/vlp_hip.h vlp_token_policy_fwd)."""
    _req_cuda(logits, ids, logp, lse, entropy)
    a = TokenPolicyFwdArgs(ptr(logits), ld, ptr(ids), ptr(logp), ptr(lse), ptr(entropy), rows, V, float(temperature))
    _check(load().vlp_token_policy_fwd(C.byref(a), stream_ptr()))


def token_policy_bwd(logits, ld, ids, lse, g, dlogits, ldd, rows, V, temperature=1.0, h=None, entropy=None):
    """dlogits of g . logp + h . entropy under softmax(logits / temperature); h (with the forward's entropy) is optional."""
    _req_cuda(logits, ids, lse, g, dlogits, h, entropy)
    a = TokenPolicyBwdArgs(ptr(logits), ld, ptr(ids), ptr(lse), ptr(entropy), ptr(g), ptr(h), ptr(dlogits), ldd, rows, V, float(temperature))
    _check(load().vlp_token_policy_bwd(C.byref(a), stream_ptr()))


def token_score(logits, ld, ids, logp, lse, entropy, rank, top_id, top_logit, rows, V):
    """Per row of fp16 logits and its id (int64; < 0: not counted, the row is not read): logp / lse / entropy f32 (vlp_token_policy_fwd's bits at
    temperature 1), rank int32, top_id int64 and top_logit f32 (include/vlp_hip.h vlp_token_score)."""
    _req_cuda(logits, ids, logp, lse, entropy, rank, top_id, top_logit)
    a = TokenScoreArgs(ptr(logits), ld, ptr(ids), ptr(logp), ptr(lse), ptr(entropy), ptr(rank), ptr(top_id), ptr(top_logit), rows, V)
    _check(load().vlp_token_score(C.byref(a), stream_ptr()))


def cider_d_workspace_bytes(G, R, T, mult):
    """0 for a shape vlp_cider_d refuses."""
    return int(load().vlp_cider_d_workspace_bytes(G, R, T, mult))


def cider_d(hyp, ref, ref_count, mult, scores, reward=None, sigma=6.0, workspace=None):
    """CIDEr-D on the device (include/vlp_hip.h vlp_cider_d): hyp int64 [mult*G, T] (row i against group i % G), ref int64 [G, R, T],
    ref_count int32 [G] or None (all R valid), scores f32 [mult*G], reward f32 [G] or None (scores[:G] - scores[G:], mult == 2).  Rows may be
    strided, the ids of a row are contiguous.  workspace: the caller's uint8 device buffer of cider_d_workspace_bytes() (16-byte aligned);
    None = a fresh allocation of this call (torch's caching allocator: no synchronisation, ordered on the current stream, fine under graph
    capture).  Launches on the current stream."""
    a = _cider_d_args(hyp, ref, ref_count, mult, scores, reward, sigma, workspace, cider_d_workspace_bytes)
    _check(load().vlp_cider_d(C.byref(a), stream_ptr()))


def cider_d_multi_workspace_bytes(G, R, T, mult):
    """0 for a shape vlp_cider_d_multi refuses (2 <= mult <= 16)."""
    return int(load().vlp_cider_d_multi_workspace_bytes(G, R, T, mult))


def cider_d_multi(hyp, ref, ref_count, mult, scores, reward=None, sigma=6.0, workspace=None):
    """cider_d for 2 <= mult <= 16 hypotheses per group with the leave-one-out reward (include/vlp_hip.h vlp_cider_d_multi): reward f32
    [mult*G] or None, reward[k*G + g] = scores[k*G + g] - mean of the group's other scores.  workspace: cider_d_multi_workspace_bytes()."""
    a = _cider_d_args(hyp, ref, ref_count, mult, scores, reward, sigma, workspace, cider_d_multi_workspace_bytes, reward_rows=mult)
    _check(load().vlp_cider_d_multi(C.byref(a), stream_ptr()))


def _req_strings(who, hyp, ref, ref_count, mult):
    """The checks of hyp, ref and ref_count that the scoring entries share (`who` names the entry in the message); returns (G, R, T)."""
    if hyp.dtype != torch.int64 or ref.dtype != torch.int64 or hyp.dim() != 2 or ref.dim() != 3 or hyp.stride(1) != 1 or ref.stride(2) != 1:
        raise RuntimeError("vlp_amd.%s: hyp int64 [mult*G, T] and ref int64 [G, R, T] with contiguous rows" % who)
    G, R, T = ref.shape
    if hyp.shape[0] != mult * G or hyp.shape[1] != T:
        raise RuntimeError("vlp_amd.%s: hyp must be [%d, %d]" % (who, mult * G, T))
    if ref_count is not None and (ref_count.dtype != torch.int32 or not ref_count.is_contiguous() or ref_count.numel() != G):
        raise RuntimeError("vlp_amd.%s: ref_count must be contiguous int32 [%d]" % (who, G))
    return G, R, T


def _req_table(who, pre, keys, vals):
    """The checks of a document-frequency table that the entries with one share (`pre`: "df_" where the arguments are df_keys / df_vals);
    returns (keys pointer, vals pointer, N), the pointers None for an empty table."""
    _req_cuda(keys, vals)
    if (keys.dtype not in (torch.int64, torch.uint64) or vals.dtype != torch.int32 or keys.dim() != 1 or vals.dim() != 1
            or not keys.is_contiguous() or not vals.is_contiguous() or keys.numel() != vals.numel()):
        raise RuntimeError("vlp_amd.%s: %skeys int64 [N] (the uint64 keys' bits) and %svals int32 [N], contiguous" % (who, pre, pre))
    n = keys.numel()
    return (ptr(keys) if n else None), (ptr(vals) if n else None), n


def _cider_d_args(hyp, ref, ref_count, mult, scores, reward, sigma, workspace, workspace_bytes, reward_rows=1):
    """The operand checks and the argument struct the cider_d entries share (reward_rows: the reward holds reward_rows * G elements)."""
    _req_cuda(hyp, ref, ref_count, scores, reward, workspace)
    G, R, T = _req_strings("cider_d", hyp, ref, ref_count, mult)
    if scores.dtype != torch.float32 or not scores.is_contiguous() or scores.numel() < mult * G:
        raise RuntimeError("vlp_amd.cider_d: scores must be contiguous f32 [%d]" % (mult * G))
    if reward is not None and (reward.dtype != torch.float32 or not reward.is_contiguous() or reward.numel() < reward_rows * G):
        raise RuntimeError("vlp_amd.cider_d: reward must be contiguous f32 [%d]" % (reward_rows * G))
    if workspace is None:
        workspace = torch.empty(max(workspace_bytes(G, R, T, mult), 1), device=hyp.device, dtype=torch.uint8)
    a = CiderDArgs(ptr(hyp), hyp.stride(0), ptr(ref), ref.stride(0), ref.stride(1), ptr(ref_count), G, R, T, mult, sigma, ptr(scores), ptr(reward),
                   ptr(workspace), _nbytes(workspace))
    a._keep = workspace                      # a fresh allocation lives until the launch has been enqueued
    return a


def cider_d_df_workspace_bytes(G, R, T, mult):
    """0 for a shape vlp_cider_d_df refuses."""
    return int(load().vlp_cider_d_df_workspace_bytes(G, R, T, mult))


def cider_d_df(hyp, ref, ref_count, mult, scores, df_keys, df_vals, n_docs, reward=None, sigma=6.0, workspace=None):
    """cider_d with document frequencies from a resident table (include/vlp_hip.h vlp_cider_d_df; vlp_amd.scst.DocFreq.to(device) makes the
    two tensors): df_keys int64 [N] holding the table's uint64 keys bit for bit (ascending as unsigned), df_vals int32 [N], n_docs the
    number of documents.  N = 0 is an empty table.  workspace: cider_d_df_workspace_bytes() bytes.  Everything else as cider_d."""
    a = _cider_d_df_args(hyp, ref, ref_count, mult, scores, df_keys, df_vals, n_docs, reward, sigma, workspace, cider_d_df_workspace_bytes, 1)
    _check(load().vlp_cider_d_df(C.byref(a), stream_ptr()))


def _cider_d_df_args(hyp, ref, ref_count, mult, scores, df_keys, df_vals, n_docs, reward, sigma, workspace, workspace_bytes, reward_rows):
    """The table checks and the argument struct cider_d_df and cider_d_multi_df share."""
    table = _req_table("cider_d_df", "df_", df_keys, df_vals)
    s = _cider_d_args(hyp, ref, ref_count, mult, scores, reward, sigma, workspace, workspace_bytes, reward_rows=reward_rows)
    a = CiderDDfArgs(s, *table, int(n_docs))
    a._keep = s                              # (its workspace lives until the launch has been enqueued)
    return a


def cider_d_multi_df_workspace_bytes(G, R, T, mult):
    """0 for a shape vlp_cider_d_multi_df refuses (2 <= mult <= 16)."""
    return int(load().vlp_cider_d_multi_df_workspace_bytes(G, R, T, mult))


def cider_d_multi_df(hyp, ref, ref_count, mult, scores, df_keys, df_vals, n_docs, reward=None, sigma=6.0, workspace=None):
    """cider_d_multi with document frequencies from a resident table (cider_d_df's table arguments); workspace:
    cider_d_multi_df_workspace_bytes() bytes."""
    a = _cider_d_df_args(hyp, ref, ref_count, mult, scores, df_keys, df_vals, n_docs, reward, sigma, workspace, cider_d_multi_df_workspace_bytes, mult)
    _check(load().vlp_cider_d_multi_df(C.byref(a), stream_ptr()))


def cider_d_consensus_workspace_bytes(G, K, T):
    """0 for a shape vlp_cider_d_consensus refuses (2 <= K <= 16)."""
    return int(load().vlp_cider_d_consensus_workspace_bytes(G, K, T))


def cider_d_consensus(hyp, K, keys, vals, n_docs, utility, pick, pair=None, sigma=6.0, workspace=None):
    """The K samples of every image scored against each other (include/vlp_hip.h vlp_cider_d_consensus): hyp int64 [K*G, T], row k*G + g
    sample k of image g (rows may be strided); keys / vals / n_docs the table as for cider_d_df; utility f32 [K*G] (sample k against the
    image's other K - 1), pick int32 [G] (the first largest utility), pair f32 [G, K, K] or None (sample k against sample j alone, 0 on the
    diagonal).  workspace: cider_d_consensus_workspace_bytes() bytes or None (a fresh allocation).  Two launches on the current stream."""
    _req_cuda(hyp, utility, pick, pair, workspace)
    if hyp.dtype != torch.int64 or hyp.dim() != 2 or hyp.stride(1) != 1:
        raise RuntimeError("vlp_amd.cider_d_consensus: hyp int64 [K*G, T] with contiguous rows")
    KG, T = hyp.shape
    K = int(K)
    if K < 1 or KG % K:
        raise RuntimeError("vlp_amd.cider_d_consensus: %d rows are not %d samples of every image" % (KG, K))
    G = KG // K
    table = _req_table("cider_d_consensus", "", keys, vals)
    if utility.dtype != torch.float32 or not utility.is_contiguous() or utility.numel() < KG:
        raise RuntimeError("vlp_amd.cider_d_consensus: utility must be contiguous f32 [%d]" % KG)
    if pick.dtype != torch.int32 or not pick.is_contiguous() or pick.numel() < G:
        raise RuntimeError("vlp_amd.cider_d_consensus: pick must be contiguous int32 [%d]" % G)
    if pair is not None and (pair.dtype != torch.float32 or not pair.is_contiguous() or pair.numel() < G * K * K):
        raise RuntimeError("vlp_amd.cider_d_consensus: pair must be contiguous f32 [%d, %d, %d]" % (G, K, K))
    if workspace is None:
        workspace = torch.empty(max(cider_d_consensus_workspace_bytes(G, K, T), 1), device=hyp.device, dtype=torch.uint8)
    a = CiderDConsensusArgs(ptr(hyp), hyp.stride(0), G, K, T, sigma, *table, int(n_docs), ptr(utility), ptr(pick), ptr(pair), ptr(workspace),
                            _nbytes(workspace))
    _check(load().vlp_cider_d_consensus(C.byref(a), stream_ptr()))   # (a fresh workspace lives until the launches have been enqueued)


BLEU_REWARD_PAIR, BLEU_REWARD_LOO = 0, 1


def bleu4(hyp, ref, ref_count, mult, bleu4, stats=None, base=None, w_base=1.0, w_bleu=1.0, mixed=None, reward=None, loo=False):
    """Sentence BLEU-4 on the device with the mix and the baseline (include/vlp_hip.h vlp_bleu4): hyp, ref, ref_count as for cider_d (mult in
    1..16); bleu4 f32 [mult*G]; stats int32 [mult*G, 6] or None (correct_1..4, len_h, reflen); base f32 [mult*G] or None (the CIDEr-D scores);
    mixed f32 [mult*G] or None = w_base * base + w_bleu * bleu4 (w_bleu * bleu4 without base; may be the same tensor as base); reward f32 or
    None: [G] = mixed[:G] - mixed[G:] (mult == 2), or with loo=True [mult*G], every mixed score minus the mean of its group's others.  One
    launch on the current stream, no workspace."""
    _req_cuda(hyp, ref, ref_count, bleu4, stats, base, mixed, reward)
    G, R, T = _req_strings("bleu4", hyp, ref, ref_count, mult)
    n = mult * G
    for name, t, need in (("bleu4", bleu4, n), ("base", base, n), ("mixed", mixed, n), ("reward", reward, n if loo else G)):
        if t is None and name != "bleu4":
            continue
        if t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < need:
            raise RuntimeError("vlp_amd.bleu4: %s must be contiguous f32 [%d]" % (name, need))
    if stats is not None and (stats.dtype != torch.int32 or not stats.is_contiguous() or stats.numel() < 6 * n):
        raise RuntimeError("vlp_amd.bleu4: stats must be contiguous int32 [%d, 6]" % n)
    a = Bleu4Args(ptr(hyp), hyp.stride(0), ptr(ref), ref.stride(0), ref.stride(1), ptr(ref_count), G, R, T, mult, ptr(bleu4), ptr(stats), ptr(base),
                  w_base, w_bleu, ptr(mixed), ptr(reward), BLEU_REWARD_LOO if loo else BLEU_REWARD_PAIR)
    _check(load().vlp_bleu4(C.byref(a), stream_ptr()))


def caption_eval_workspace_bytes(G, R, T):
    """0 for a shape vlp_caption_eval refuses."""
    return int(load().vlp_caption_eval_workspace_bytes(G, R, T))


def caption_eval(hyp, ref, ref_count, cider, bleu_stats, lcs, df_keys, df_vals, n_docs, sigma=6.0, workspace=None):
    """Caption metrics of word strings on the device (include/vlp_hip.h vlp_caption_eval): hyp int64 [G, T] (one hypothesis per image), ref
    int64 [G, R, T], ref_count int32 [G] or None, the table as for cider_d_df.  A string is the ids of a row BEFORE its first 0.  Outputs:
    cider f32 [G], bleu_stats int32 [G, 6] (correct_1..4, len_h, reflen), lcs int32 [G, R, 2] (LCS length, len_r; (0, 0) for an invalid
    reference).  workspace: caption_eval_workspace_bytes() bytes or None (a fresh allocation).  Three launches on the current stream."""
    _req_cuda(bleu_stats, lcs)
    d = _cider_d_df_args(hyp, ref, ref_count, 1, cider, df_keys, df_vals, n_docs, None, sigma, workspace,
                         lambda G, R, T, mult: caption_eval_workspace_bytes(G, R, T), 1)
    G, R, T = ref.shape
    if bleu_stats.dtype != torch.int32 or not bleu_stats.is_contiguous() or bleu_stats.numel() < 6 * G:
        raise RuntimeError("vlp_amd.caption_eval: bleu_stats must be contiguous int32 [%d, 6]" % G)
    if lcs.dtype != torch.int32 or not lcs.is_contiguous() or lcs.numel() < 2 * G * R:
        raise RuntimeError("vlp_amd.caption_eval: lcs must be contiguous int32 [%d, %d, 2]" % (G, R))
    a = CaptionEvalArgs(d, ptr(bleu_stats), ptr(lcs))
    a._keep = d                              # (its workspace lives until the launches have been enqueued)
    _check(load().vlp_caption_eval(C.byref(a), stream_ptr()))


def region_mask_build(vis_masked_pos, out, B, Pm, Nv):
    """vis_masked_pos i64 [B, Pm] (1..Nv) -> out u8 [B*Nv], 1 on masked region rows (seq2seq_loader.py:267-269)."""
    _req_cuda(vis_masked_pos, out)
    _check(load().vlp_region_mask_build(ptr(vis_masked_pos), B, Pm, Nv, ptr(out), stream_ptr()))


def pretext_fwd(vis_h, vispe_h, pooled, vis_masked_pos, probs, sample_loss, loss, B, Nv, Pm, H):
    _req_cuda(vis_h, vispe_h, pooled, vis_masked_pos, probs, sample_loss, loss)
    a = PretextFwdArgs(ptr(vis_h), ptr(vispe_h), ptr(pooled), ptr(vis_masked_pos), ptr(probs), ptr(sample_loss), ptr(loss), B, Nv, Pm, H)
    _check(load().vlp_pretext_fwd(C.byref(a), stream_ptr()))


def pretext_bwd(vis_h, vispe_h, pooled, vis_masked_pos, probs, gscale, d_vis_h, d_vispe_h, d_pooled_pre, B, Nv, Pm, H,
                drop_p=0.0, seed=0, vis_stream=0, vispe_stream=0):
    _req_cuda(vis_h, vispe_h, pooled, vis_masked_pos, probs, gscale, d_vis_h, d_vispe_h, d_pooled_pre)
    a = PretextBwdArgs(ptr(vis_h), ptr(vispe_h), ptr(pooled), ptr(vis_masked_pos), ptr(probs), ptr(gscale), ptr(d_vis_h), ptr(d_vispe_h),
                       ptr(d_pooled_pre), B, Nv, Pm, H, drop_p, seed, vis_stream, vispe_stream)
    _check(load().vlp_pretext_bwd(C.byref(a), stream_ptr()))


def copy2d(src, lds, src_f32, dst, ldd, rows, cols_src, cols_dst, beta=0):
    _req_cuda(src, dst)
    _check(load().vlp_copy2d(ptr(src), lds, int(src_f32), ptr(dst), ldd, rows, cols_src, cols_dst, beta, stream_ptr()))


def transpose(src, lds, dst, ldd, rows, cols, rows_pad):
    _req_cuda(src, dst)
    _check(load().vlp_transpose(ptr(src), lds, ptr(dst), ldd, rows, cols, rows_pad, stream_ptr()))


def make_transpose_batch(items, device):
    """items: [(src, lds, dst, ldd, rows, cols, rows_pad)] -> (descs_dev, tile_start_dev, n, total_tiles).  The descriptor
    table is built once (pointers of the flat parameter buffers and shadows are stable) and reused every step."""
    import numpy as np
    arr = (TransposeDesc * len(items))()
    starts, tot = [], 0
    for i, (src, lds, dst, ldd, rows, cols, rows_pad) in enumerate(items):
        _req_cuda(src, dst)
        arr[i] = TransposeDesc(src.data_ptr(), dst.data_ptr(), lds, ldd, rows, cols, rows_pad, 0)
        starts.append(tot)
        tot += ((rows_pad + 63) // 64) * ((cols + 63) // 64)
    raw = np.frombuffer(bytes(arr), dtype=np.uint8).copy()
    descs = torch.from_numpy(raw).to(device)
    ts = torch.tensor(starts, dtype=torch.int32, device=device)
    return descs, ts, len(items), tot


def transpose_batched(batch):
    descs, ts, n, tot = batch
    _check(load().vlp_transpose_batched(ptr(descs), ptr(ts), n, tot, stream_ptr()))


def gather_rows(src, lds, pos, out, ldo, B, P, L, H, row_off=None):
    _req_cuda(src, pos, out, row_off)
    _check(load().vlp_gather_rows(ptr(src), lds, ptr(pos), ptr(out), ldo, B, P, L, H, ptr(row_off), stream_ptr()))


def scatter_add_rows(src, lds, pos, dst, ldd, B, P, L, H, row_off=None):
    _req_cuda(src, pos, dst, row_off)
    _check(load().vlp_scatter_add_rows(ptr(src), lds, ptr(pos), ptr(dst), ldd, B, P, L, H, ptr(row_off), stream_ptr()))


def kept_rows_build(B, L, Nv, lens, row_map, count, maskb=None, Lp=0, lens_in=None, pos=None):
    """Kept rows of the dense step (vlp_kept_rows_build): from the packed mask `maskb` [B, L, Lp] or the per-sample lengths `lens_in` (int32
    [B]), and the masked positions `pos` (int64 [B, P]); writes lens [B], row_map [B * L] and count [1] (int32, device)."""
    _req_cuda(lens, row_map, count, maskb, lens_in, pos)
    if lens.numel() < B or row_map.numel() < B * L or (pos is not None and (pos.dtype != torch.int64 or not pos.is_contiguous())):
        raise RuntimeError("kept_rows_build: lens [B], row_map [B * L], pos contiguous int64")
    P = pos.shape[1] if pos is not None else 0
    _check(load().vlp_kept_rows_build(ptr(maskb), ptr(lens_in), ptr(pos), B, P, L, Lp, Nv, ptr(lens), ptr(row_map), ptr(count), stream_ptr()))


def live_rows_build(pos, B, P, L, live, count, row_off=None):
    """live[0..n) = the distinct rows scatter_add_rows(pos) adds to, ascending; live[n..B*P) = -1; count[0] = n (device int32)."""
    _req_cuda(pos, live, count, row_off)
    _check(load().vlp_live_rows_build(ptr(pos), B, P, L, ptr(row_off), ptr(live), ptr(count), stream_ptr()))


def rowmap_build(row_off, B, L, row_map):
    """row_map[row_off[b] + l] = b*L + l for l < row_off[b+1] - row_off[b]  (packed rows -> logical rows)."""
    _req_cuda(row_off, row_map)
    _check(load().vlp_rowmap_build(ptr(row_off), B, L, ptr(row_map), stream_ptr()))


def rows_unpack(src, row_map, rows, dst, H):
    """dst[row_map[p]] = src[p]; untouched dst rows keep their contents (clear dst first)."""
    _req_cuda(src, row_map, dst)
    _check(load().vlp_rows_unpack(ptr(src), src.stride(0), ptr(row_map), rows, ptr(dst), dst.stride(0), H, stream_ptr()))


def rows_pack(src, row_map, rows, dst, H):
    """dst[p] = src[row_map[p]]"""
    _req_cuda(src, row_map, dst)
    _check(load().vlp_rows_pack(ptr(src), src.stride(0), ptr(row_map), rows, ptr(dst), dst.stride(0), H, stream_ptr()))


def vqa_mul_fwd(h, out, B, L, Nv, H, row_off=None):
    _req_cuda(h, out, row_off)
    _check(load().vlp_vqa_mul_fwd(ptr(h), ptr(out), B, L, Nv, H, ptr(row_off), stream_ptr()))


def vqa_mul_bwd(h, dout, dh, B, L, Nv, H, row_off=None):
    _req_cuda(h, dout, dh, row_off)
    _check(load().vlp_vqa_mul_bwd(ptr(h), ptr(dout), ptr(dh), B, L, Nv, H, ptr(row_off), stream_ptr()))


def relu_dropout_bwd(dy, y, dz, n, ncols, drop_p=0.0, seed=0, rng_stream=0):
    _req_cuda(dy, y, dz)
    _check(load().vlp_relu_dropout_bwd(ptr(dy), ptr(y), ptr(dz), n, ncols, drop_p, seed, rng_stream, stream_ptr()))


def gelu_bwd(dy, z, dz, n):
    _req_cuda(dy, z, dz)
    _check(load().vlp_gelu_bwd(ptr(dy), ptr(z), ptr(dz), n, stream_ptr()))


def mlm_loss_fwd(logits, ld, labels, weights, loss, lse, coef, row_loss, B, P, V, drop_worst_ratio=0.0):
    _req_cuda(logits, labels, weights, loss, lse, coef, row_loss)
    a = MlmLossFwdArgs(ptr(logits), ld, ptr(labels), ptr(weights), ptr(loss), ptr(lse), ptr(coef), ptr(row_loss), B, P, V, drop_worst_ratio)
    _check(load().vlp_mlm_loss_fwd(C.byref(a), stream_ptr()))


def mlm_loss_bwd(logits, ld, labels, lse, coef, grad_scale, dlogits, ldd, rows, V):
    _req_cuda(logits, labels, lse, coef, grad_scale, dlogits)
    a = MlmLossBwdArgs(ptr(logits), ld, ptr(labels), ptr(lse), ptr(coef), ptr(grad_scale), ptr(dlogits), ldd, rows, V)
    _check(load().vlp_mlm_loss_bwd(C.byref(a), stream_ptr()))


def mlm_loss_ls_fwd(logits, ld, labels, weights, loss, lse, coef, row_loss, B, P, V, smooth, confidence, q_sum, q_log_q, ignore_index=0,
                    drop_worst_ratio=0.0):
    """Label-smoothed masked-LM loss; smooth / confidence / q_sum / q_log_q are the smoothed one-hot's values in the model's dtype
    (vlp_amd.loss.LabelSmoothingLoss.kernel_scalars)."""
    _req_cuda(logits, labels, weights, loss, lse, coef, row_loss)
    a = MlmLossLsFwdArgs(ptr(logits), ld, ptr(labels), ptr(weights), ptr(loss), ptr(lse), ptr(coef), ptr(row_loss), B, P, V, drop_worst_ratio,
                         smooth, confidence, q_sum, q_log_q, ignore_index)
    _check(load().vlp_mlm_loss_ls_fwd(C.byref(a), stream_ptr()))


def mlm_loss_ls_bwd(logits, ld, labels, lse, coef, grad_scale, dlogits, ldd, rows, V, smooth, confidence, q_sum, ignore_index=0):
    _req_cuda(logits, labels, lse, coef, grad_scale, dlogits)
    a = MlmLossLsBwdArgs(ptr(logits), ld, ptr(labels), ptr(lse), ptr(coef), ptr(grad_scale), ptr(dlogits), ldd, rows, V,
                         smooth, confidence, q_sum, ignore_index)
    _check(load().vlp_mlm_loss_ls_bwd(C.byref(a), stream_ptr()))


def bce_loss_fwd(logits, ld, labels, ldl, B, N, loss257):
    _req_cuda(logits, labels, loss257)
    _check(load().vlp_bce_loss_fwd(ptr(logits), ld, ptr(labels), ldl, B, N, ptr(loss257), stream_ptr()))


def bce_loss_bwd(logits, ld, labels, ldl, B, N, grad_scale, dlogits, ldd):
    _req_cuda(logits, labels, grad_scale, dlogits)
    _check(load().vlp_bce_loss_bwd(ptr(logits), ld, ptr(labels), ldl, B, N, ptr(grad_scale), ptr(dlogits), ldd, stream_ptr()))


def _req_answers(ans_idx, ans_score, B):
    """The [B, S] (answer index, score) pairs of vlp_amd.input_prep.SparseAnswers as the kernels read them."""
    _req_cuda(ans_idx, ans_score)
    if ans_idx.dtype != torch.int32 or ans_score.dtype != torch.float32 or ans_idx.dim() != 2 or ans_idx.shape != ans_score.shape \
            or ans_idx.shape[0] != B or not (ans_idx.is_contiguous() and ans_score.is_contiguous()):
        raise RuntimeError("vlp_amd: sparse answers must be contiguous idx int32 / score f32 [%d, S]" % B)
    return ans_idx.shape[1]


def bce_sparse_loss_fwd(logits, ld, ans_idx, ans_score, B, N, loss257):
    """vlp_bce_loss_fwd with y given as [B, S] (answer index, score) pairs (idx -1 = empty slot) instead of the dense [B, N] target."""
    _req_cuda(logits, loss257)
    S = _req_answers(ans_idx, ans_score, B)
    _check(load().vlp_bce_sparse_loss_fwd(ptr(logits), ld, ptr(ans_idx), ptr(ans_score), S, B, N, ptr(loss257), stream_ptr()))


def bce_sparse_loss_bwd(logits, ld, ans_idx, ans_score, B, N, grad_scale, dlogits, ldd):
    _req_cuda(logits, grad_scale, dlogits)
    S = _req_answers(ans_idx, ans_score, B)
    _check(load().vlp_bce_sparse_loss_bwd(ptr(logits), ld, ptr(ans_idx), ptr(ans_score), S, B, N, ptr(grad_scale), ptr(dlogits), ldd, stream_ptr()))


def vqa_answer_rows(logits, ld, rows, N, first_col, out_ids, out_vals, ans_idx=None, ans_score=None, out_scores=None):
    """Per row: first maximum over columns [first_col, N) -> out_ids (absolute column, int64 [rows]) / out_vals (f32 [rows]); with the
    (ans_idx, ans_score) pairs given also out_scores[r] = the score the row lists for the chosen column, 0 if it lists none."""
    _req_cuda(logits, out_ids, out_vals)
    if out_ids.dtype != torch.int64 or out_vals.dtype != torch.float32 or out_ids.numel() < rows or out_vals.numel() < rows \
            or not (out_ids.is_contiguous() and out_vals.is_contiguous()):
        raise RuntimeError("vlp_amd: vqa_answer_rows needs contiguous out_ids int64 [rows] and out_vals f32 [rows]")
    S = 0
    if ans_idx is not None:
        S = _req_answers(ans_idx, ans_score, rows)
        _req_cuda(out_scores)
        if out_scores.dtype != torch.float32 or out_scores.numel() < rows or not out_scores.is_contiguous():
            raise RuntimeError("vlp_amd: vqa_answer_rows needs contiguous out_scores f32 [rows]")
    _check(load().vlp_vqa_answer_rows(ptr(logits), ld, rows, N, first_col, ptr(ans_idx), ptr(ans_score) if ans_idx is not None else None, S,
                                      ptr(out_ids), ptr(out_vals), ptr(out_scores) if ans_idx is not None else None, stream_ptr()))


def sumsq(g16, n, out2, partial, accumulate=False):
    _req_cuda(g16, out2, partial)
    fn = load().vlp_sumsq_acc if accumulate else load().vlp_sumsq
    _check(fn(ptr(g16), n, ptr(out2), ptr(partial), stream_ptr()))


def adam_hyper(sumsq2, any_overflow, scale_state, max_grad_norm, step_size, hyper3):
    _req_cuda(sumsq2, hyper3, scale_state)
    _check(load().vlp_adam_hyper(ptr(sumsq2), ptr(any_overflow), ptr(scale_state), max_grad_norm, step_size, ptr(hyper3), stream_ptr()))


def loss_scale_update(scale_state, overflow):
    _req_cuda(scale_state, overflow)
    _check(load().vlp_loss_scale_update(ptr(scale_state), ptr(overflow), stream_ptr()))


def fused_adam(p32, m, v, g16, p16, n, hyper, b1=0.9, b2=0.999, eps=1e-8, decay=0.0, eps_inside_sqrt=False):
    _req_cuda(p32, m, v, g16, p16, hyper)
    a = FusedAdamArgs(ptr(p32), ptr(m), ptr(v), ptr(g16), ptr(p16), n, b1, b2, eps, decay, int(eps_inside_sqrt), ptr(hyper))
    _check(load().vlp_fused_adam(C.byref(a), stream_ptr()))


def bert_adam_norms_floats(n, ntensors):
    return int(load().vlp_bert_adam_norms_floats(n, ntensors))


def bert_adam(p32, m, v, g, g_is_f32, p16, seg_off, ntensors, n, norms, lr, b1=0.9, b2=0.999, eps=1e-6, decay=0.01,
              max_grad_norm=1.0, grad_scale=1.0, active=None):
    _req_cuda(p32, m, v, g, seg_off, norms)
    a = BertAdamArgs(ptr(p32), ptr(m), ptr(v), ptr(g), int(g_is_f32), ptr(p16), ptr(seg_off), ntensors, n, ptr(norms), norms.numel(),   # the library checks the scratch size (ABI 3)
                     lr, b1, b2, eps, decay, max_grad_norm, grad_scale, ptr(active))
    _check(load().vlp_bert_adam(C.byref(a), stream_ptr()))
