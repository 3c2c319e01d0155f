"""ctypes binding of libzett_hip.so (C ABI: include/zett_hip.h).

The library is the product: if it cannot be loaded there is no fallback — the
import of anything that computes raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from .build import LIB_PATH

ZETT_OK = 0
E_INVALID, E_HIP, E_STATE, E_INDEX, E_NOT_IMPLEMENTED, E_KEY, E_RANGE = -1, -2, -3, -4, -5, -6, -7
RANGE_SOURCE, RANGE_ACTIVATION, RANGE_OUTPUT, RANGE_WEIGHT, RANGE_DEST = 1, 2, 4, 8, 16      # zett_range_bits
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2
PREC_BF16, PREC_F32, PREC_F16 = 0, 1, 2
RETOK_BPE, RETOK_UNIGRAM, RETOK_WORDPIECE = 0, 1, 2
OUT_IN, OUT_BIAS = 0, 1              # zett_output
LEXICAL_NO, LEXICAL_FVT, LEXICAL_BFVT = 0, 1, 2      # zett_lexical_mode
DIST_MSE, DIST_RMSE, DIST_HUBER = 0, 1, 2            # zett_distance
LOSS_MEAN, LOSS_LEXICAL = 0, 1                       # zett_loss_mode
ADAMW_DECAY, ADAMW_FROZEN = 1, 2                     # zett_adamw_flags
MT_CHUNK = 65536                                     # ZETT_MT_CHUNK
CE_AUTO, CE_ONCE, CE_TWICE = 0, 1, 2                 # zett_ce_path
CE_ONCE_MAX_COLS = 32768                             # ZETT_CE_ONCE_MAX_COLS
SPLICE_MAX_ROWS = 256                                # ZETT_SPLICE_MAX_ROWS
EMBED_BWD_CHUNK = 64                                 # ZETT_EMBED_BWD_CHUNK
BATCH_POSITIVES_ONLY, BATCH_RANDOM = 0, 1            # zett_batch_mode
BATCH_BAD_ID, BATCH_OVERFLOW, BATCH_BAD_ORDER, BATCH_REPEAT = 1, 2, 4, 8      # zett_batch_status
LABEL_CLM, LABEL_MLM = 0, 1                          # zett_label_mode
LABEL_BAD_ID = 1                                     # zett_label_status
LABEL_WORKSPACE_BYTES = 16384                        # ZETT_LABEL_WORKSPACE_BYTES
ENCODE_MAX_TEMPLATE = 8                              # ZETT_ENCODE_MAX_TEMPLATE
ENCODE_MARKS_ARE_LETTERS, ENCODE_RESPLIT = 1, 2      # zett_encode_flags
ENCODE_PREFIX_NONE, ENCODE_PREFIX_ALWAYS, ENCODE_PREFIX_UNLESS_SPACE = 0, 1, 2      # zett_encode_prefix
ENCODE_NO_UNK, ENCODE_BAD_OFFSETS, ENCODE_BAD_TABLE = 1, 2, 4      # zett_encode_status
ENCODE_MAX_ADDED, ENCODE_MAX_ADDED_BYTES = 512, 64   # zett_encode_texts_added: tokens of a table, bytes of a token
SAMPLE_BAD_OFFSETS, SAMPLE_TABLE_FULL, SAMPLE_LIST_FULL, SAMPLE_SUM_OVERFLOW, SAMPLE_OUT_FULL = 2, 4, 8, 16, 32      # zett_sample_status
VOCAB_NOT_A_SAMPLE, VOCAB_DUPLICATE, VOCAB_TABLE_FULL, VOCAB_OUT_FULL = 1, 2, 4, 8      # zett_vocab_status
VOCAB_SCORES_THROUGH_JSON = 1                        # zett_vocab_flags
SAMPLED_VOCAB_KEY_BYTES = 64                         # ZETT_SAMPLED_VOCAB_KEY_BYTES
COL_MOMENTS_CHUNK = 256                              # ZETT_COL_MOMENTS_CHUNK
ADAFACTOR_TILE_ROWS, ADAFACTOR_TILE_COLS, ADAFACTOR_GROUP = 64, 256, 40      # ZETT_ADAFACTOR_TILE_ROWS, ZETT_ADAFACTOR_TILE_COLS, ZETT_ADAFACTOR_GROUP

ABI_SYMBOLS = (
    "zett_last_error", "zett_abi_version", "zett_create", "zett_destroy", "zett_load_weight",
    "zett_finalize", "zett_forward", "zett_get_stats", "zett_workspace_bytes", "zett_set_option",
    "zett_retok_create", "zett_retok_destroy", "zett_retokenize", "zett_check_range", "zett_get_gemm_log",
    "zett_stream_wait_output", "zett_forward_prepare", "zett_retokenize_async", "zett_retok_result", "zett_retok_set_option",
    "zett_partition_rows", "zett_partition_workspace_bytes", "zett_scatter_rows",
    "zett_table_plan", "zett_table_rows", "zett_forward_table",
    "zett_forward_into", "zett_forward_table_into",
    "zett_lexical_create", "zett_lexical_destroy", "zett_lexical_plan", "zett_lexical_rows_into",
    # training primitives (zett_amd/autograd.py)
    "zett_op_gemm_f32", "zett_op_transpose_f32", "zett_op_colsum_f32", "zett_op_elementwise_f32", "zett_op_rowdot_f32",
    "zett_op_layernorm_fwd_f32", "zett_op_layernorm_bwd_f32", "zett_op_gelu_fwd_f32", "zett_op_gelu_bwd_f32",
    "zett_op_attention_fwd_f32", "zett_op_attention_bwd_f32", "zett_op_gather_fwd_f32", "zett_op_gather_bwd_f32",
    "zett_op_gather_rows_f32", "zett_op_scatter_add_rows_f32", "zett_op_gemm_lo", "zett_op_convert_lo", "zett_op_transpose_lo", "zett_op_grad_operands_lo", "zett_op_transpose_lo16", "zett_op_gelu_fwd_lo",
    # losses (zett_amd/training.py) and the parameter update (zett_amd/optim.py) of a training step
    "zett_op_single_token_mask", "zett_op_embed_dist_rows", "zett_op_embed_dist_finalize", "zett_op_embed_dist_grad", "zett_op_grad_norm", "zett_op_adamw",
    # the language-model loss over predicted output embeddings (zett_amd/training.py lm_head_loss)
    "zett_op_ce_addend", "zett_op_ce_rows", "zett_op_ce_finalize", "zett_op_ce_colsum", "zett_op_ce_scale", "zett_op_ce_cast",
    # the input side of a training step (zett_amd/training.py splice_special_rows, token_embeddings)
    "zett_op_splice_rows", "zett_op_embed_lookup", "zett_op_embed_lookup_workspace_bytes", "zett_op_embed_lookup_plan", "zett_op_embed_lookup_bwd",
    # the batch's sub-vocabulary (zett_amd/training.py subsample_batch_vocabulary)
    "zett_op_batch_vocab_workspace_bytes", "zett_op_batch_vocab",
    # the rest of the collator (zett_amd/collate.py label_batch, pad_vocabulary)
    "zett_op_label_batch", "zett_op_pad_vocabulary",
    # text encoding (zett_amd/text_encode.py DeviceTextEncoder)
    "zett_encode_workspace_bytes", "zett_encode_texts", "zett_encode_added_workspace_bytes", "zett_encode_texts_added",
    # tokenizer sampling (zett_amd/tokenizer_sampling.py DeviceTokenizerSampler)
    "zett_sampler_create", "zett_sampler_destroy", "zett_sampler_depth", "zett_sampler_workspace_bytes", "zett_sampler_sample", "zett_sampler_table",
    # the sampled tokenizer's vocabulary and encoder tables (zett_amd/sampled_vocab.py DeviceSampledVocabulary)
    "zett_retok_create_unigram_device", "zett_sampled_vocab_workspace_bytes", "zett_sampled_vocab_build", "zett_sampled_vocab_commit", "zett_sampled_vocab_table",
    "zett_sampled_vocab_patch_rows",
    # the order-stable sums of the hypernetwork's backward (zett_amd/autograd.py, deterministic=True)
    "zett_op_embed_lookup_plan_base", "zett_op_gather_bwd_rows_f32",
    # the forward's row kernels, one launch at a time (tests/test_rowops_direct_gpu.py)
    "zett_op_fwd_layernorm", "zett_op_fwd_embed_layernorm", "zett_op_fwd_attention", "zett_op_fwd_gather_src", "zett_op_fwd_ln_stats", "zett_op_fwd_fold_weight",
    # single rows whose query / key work the last forward skipped (HipEngine.single_rows)
    "zett_single_rows",
    # layer 0's Q/K/V once per source id: the row kernel on its own, and whether the last forward took the lever (HipEngine.id_qkv)
    "zett_op_fwd_pair_qkv", "zett_id_qkv",
    # one GEMM launch of the forward with any epilogue (tests/test_gemm_fwd_direct_gpu.py)
    "zett_op_fwd_gemm",
    # fitting a fresh hypernetwork's Rescalers (zett_amd/training.py column_moments, rescaler_fit)
    "zett_op_col_moments_workspace_bytes", "zett_op_col_moments", "zett_op_rescaler_fit",
    # the Adafactor branch of the optimizer (zett_amd/optim.py HypernetAdafactor)
    "zett_op_adafactor_workspace_floats", "zett_op_adafactor_step",
)


class ZettConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_embd", "n_in_embd", "hidden", "intermediate", "heads", "layers", "n_extra",
        "original_vocab_size", "pad_token_id", "separate_out", "single_head", "rescale",
        "predict_bias", "embed_lang", "n_langs", "max_positions")] + [
        ("ln_eps_encoder", C.c_float), ("ln_eps_projector", C.c_float)]


ABI_VERSION = 8      # ZETT_ABI_VERSION of include/zett_hip.h


class ZettStats(C.Structure):
    _fields_ = [("rows", C.c_int64), ("packed_tokens", C.c_int64), ("distinct_ids", C.c_int64),
                ("chunks", C.c_int64), ("executed_flops", C.c_double), ("gemm_ms", C.c_double),
                ("gemm_launches", C.c_int64), ("gemm_flops_timed", C.c_double), ("distinct_positions", C.c_int64)]


class ZettGemmRecord(C.Structure):
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("variant", C.c_int32), ("epilogue", C.c_int32),
                ("ms", C.c_float), ("flops", C.c_double), ("bytes", C.c_double)]


class ZettDest(C.Structure):
    """struct zett_dest (zett_forward_into / zett_forward_table_into): where the predicted rows go."""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("bias", C.c_void_p), ("dtype", C.c_int32), ("bias_dtype", C.c_int32),
                ("ld_in", C.c_int64), ("ld_out", C.c_int64), ("rows", C.c_void_p), ("n_dest_rows", C.c_int64)]


class ZettFwdGemmDesc(C.Structure):
    """struct zett_fwd_gemm_desc (zett_op_fwd_gemm): one GEMM launch of the forward, GemmArgs / GemmEpilogue field for field."""
    _fields_ = [("size", C.c_int64)] + [(n, C.c_void_p) for n in (
        "a", "w", "bias", "residual", "residual_lo", "res_stats", "res_gamma", "res_beta", "res_index", "stats_part", "fold_stats", "fold_c", "scale", "shift",
        "out_f32", "out_lo", "out_f32_b", "range_flag", "dst", "dst_rows")] + [("ld_dst", C.c_int64), ("a_rows_readable", C.c_int64)] + [(n, C.c_int32) for n in (
        "lda", "ldw", "m", "n", "k", "act", "ld_res", "ld_res_lo", "ld_part", "ld_f32", "ld_lo", "split_col", "range_final", "dst_dtype",
        "gemm_variant", "gemm4d_min_k", "gemm_tail_split", "gemm_tile_order", "gemm_group", "reserved")]


class ZettSampledVocabRecord(C.Structure):
    """struct zett_sampled_vocab_record: the 32 bytes zett_sampled_vocab_build leaves on the device."""
    _fields_ = [("n_vocab", C.c_int32), ("n_removed", C.c_int32), ("n_text", C.c_int32), ("status", C.c_int32), ("min_score", C.c_double), ("table_min_score", C.c_double)]


class ZettRetokModel(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("n_pieces", C.c_int32),
        ("piece_bytes", C.c_void_p), ("piece_offsets", C.c_void_p), ("piece_ids", C.c_void_p),
        ("piece_scores", C.c_void_p), ("unigram_min_score", C.c_double),
        ("n_merges", C.c_int32), ("merges", C.c_void_p),
        ("unk_id", C.c_int32), ("fuse_unk", C.c_int32), ("byte_fallback", C.c_int32),
        ("byte_fallback_ids", C.c_void_p), ("ignore_merges", C.c_int32),
        ("n_special", C.c_int32), ("special_bytes", C.c_void_p), ("special_offsets", C.c_void_p),
        ("special_ids", C.c_void_p),
        ("piece_continuing", C.c_void_p), ("max_input_chars_per_word", C.c_int32),
    ]


_lib = None
_lock = threading.Lock()


def lib_path() -> str:
    return os.environ.get("ZETT_HIP_LIB", LIB_PATH)


def load():
    """dlopen the library (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: the HIP extension has not been built. Run "
                "`python -m zett_amd.build` (needs hipcc); zett_amd has no CPU fallback.")
        lib = C.CDLL(path)
        lib.zett_last_error.restype = C.c_char_p
        lib.zett_abi_version.restype = C.c_int
        lib.zett_create.argtypes = [C.POINTER(ZettConfig), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        lib.zett_destroy.argtypes = [C.c_void_p]
        lib.zett_load_weight.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]
        lib.zett_finalize.argtypes = [C.c_void_p]
        lib.zett_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int, C.c_int64,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.zett_get_stats.argtypes = [C.c_void_p, C.POINTER(ZettStats)]
        lib.zett_single_rows.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        lib.zett_id_qkv.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        lib.zett_workspace_bytes.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        lib.zett_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        lib.zett_check_range.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        lib.zett_stream_wait_output.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.zett_get_gemm_log.argtypes = [C.c_void_p, C.POINTER(ZettGemmRecord), C.c_int64, C.POINTER(C.c_int64)]
        lib.zett_retok_create.argtypes = [C.POINTER(ZettRetokModel), C.c_int, C.POINTER(C.c_void_p)]
        lib.zett_retok_destroy.argtypes = [C.c_void_p]
        lib.zett_retok_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        lib.zett_retokenize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
        lib.zett_retokenize_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                              C.c_void_p, C.c_void_p]
        lib.zett_retok_result.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.zett_forward_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        lib.zett_table_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
        lib.zett_table_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.zett_forward_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.zett_forward_into.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int, C.c_int64, C.c_int32,
                                          C.POINTER(ZettDest), C.c_void_p]
        lib.zett_forward_table_into.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                C.POINTER(ZettDest), C.c_void_p]
        lib.zett_lexical_create.argtypes = [C.POINTER(ZettRetokModel), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        lib.zett_lexical_destroy.argtypes = [C.c_void_p]
        lib.zett_lexical_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
        lib.zett_lexical_rows_into.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                               C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.POINTER(ZettDest), C.c_void_p]
        lib.zett_partition_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        lib.zett_scatter_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
        lib.zett_partition_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                            C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        P, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
        lib.zett_op_gemm_f32.argtypes = [P, I32, P, I32, I64, I32, I32, P, I32, P, I32, P, I32, P]
        lib.zett_op_transpose_f32.argtypes = [P, I32, P, I32, I64, I32, I64, P]
        lib.zett_op_gemm_lo.argtypes = [I32, P, I32, P, I32, I64, I32, I32, P, I32, P, I32, P, I32, P]
        lib.zett_op_convert_lo.argtypes = [I32, P, I32, P, I32, I64, I32, I32, P]
        lib.zett_op_transpose_lo.argtypes = [I32, P, I32, P, I32, I64, I32, I64, P]
        lib.zett_op_grad_operands_lo.argtypes = [I32, P, I32, P, I32, I32, I64, I32, I64, P, I32, P, I32, P, P]
        lib.zett_op_transpose_lo16.argtypes = [I32, P, I32, P, I32, I64, I32, I64, P]
        lib.zett_op_gelu_fwd_lo.argtypes = [I32, P, P, I64, I32, P]
        lib.zett_op_colsum_f32.argtypes = [P, I32, I64, I32, P, I32, P]
        lib.zett_op_elementwise_f32.argtypes = [I32, P, P, P, P, P, P, I64, I32, P]
        lib.zett_op_rowdot_f32.argtypes = [P, I32, P, P, P, I64, I32, P]
        lib.zett_op_layernorm_fwd_f32.argtypes = [P, I32, P, P, F, P, P, I64, I32, P, I32, P]
        lib.zett_op_layernorm_bwd_f32.argtypes = [P, P, P, I32, P, P, P, P, I32, I64, I32, P]
        lib.zett_op_gelu_fwd_f32.argtypes = [P, P, I64, I32, P]
        lib.zett_op_gelu_bwd_f32.argtypes = [P, P, P, I64, I32, P]
        lib.zett_op_attention_fwd_f32.argtypes = [P, I32, P, P, I32, P, P, I64, I32, I32, I32, I32, P, I32, P, P, I32, P]
        lib.zett_op_attention_bwd_f32.argtypes = [P, I32, P, I32, P, P, I32, P, P, I64, I32, I32, I32, I32, P, I32, P, P, I32, P]
        lib.zett_op_gather_rows_f32.argtypes = [P, P, I32, P, P, I64, I32, P]
        lib.zett_op_scatter_add_rows_f32.argtypes = [P, I32, P, P, I64, I32, P]
        lib.zett_op_gather_fwd_f32.argtypes = [P, I64, P, I32, I32, I32, P, P, P, P, P]
        lib.zett_op_gather_bwd_f32.argtypes = [P, I64, P, I32, I32, I32, P, P, P, P, P]
        lib.zett_op_gather_bwd_rows_f32.argtypes = [P, I64, P, I32, I32, I32, P, P, P, P]
        D = C.c_double
        lib.zett_op_single_token_mask.argtypes = [P, I32, I64, I32, I64, I64, P, P]
        lib.zett_op_embed_dist_rows.argtypes = [P, I64, P, I32, I64, I64, I32, P, I32, I64, P, I64, I32, I32, P, P, P]
        lib.zett_op_embed_dist_finalize.argtypes = [P, P, P, I64, I32, P, P]
        lib.zett_op_embed_dist_grad.argtypes = [P, I64, P, I32, I64, I64, I32, P, I32, I64, P, P, I64, I32, I32, P, P, P, I64, I32, P]
        lib.zett_op_grad_norm.argtypes = [P, P, I32, D, D, D, P, I64, P, P]
        lib.zett_op_adamw.argtypes = [P, P, P, P, P, P, I32, D, D, D, D, D, I32, P, P]
        lib.zett_op_ce_addend.argtypes = [P, P, P, I32, I32, P, P]
        lib.zett_op_ce_rows.argtypes = [P, I64, P, P, I64, I32, I32, P, I32, I64, P, P, P, I32, P]
        lib.zett_op_ce_finalize.argtypes = [P, P, P, P, I64, P, P]
        lib.zett_op_ce_colsum.argtypes = [P, I32, I64, I64, I32, P, I32, P]
        lib.zett_op_ce_scale.argtypes = [P, I64, P, P, P, I32, P]
        lib.zett_op_ce_cast.argtypes = [P, I32, I64, P, I32, I64, I64, I32, I32, P]
        lib.zett_op_splice_rows.argtypes = [P, I64, P, I64, I64, I32, P, I32, I64, I64, I32, P, P, I32, P]
        lib.zett_op_embed_lookup.argtypes = [P, I32, I64, I64, I32, P, I32, I64, P, I32, P, P]
        lib.zett_op_embed_lookup_workspace_bytes.argtypes = [I64, I64, I32, C.POINTER(I64), C.POINTER(I64), C.POINTER(I64)]
        lib.zett_op_embed_lookup_plan.argtypes = [P, I32, I64, I64, P, I64, P, I64, P]
        lib.zett_op_embed_lookup_plan_base.argtypes = [P, I32, I64, I64, I64, P, I64, P, I64, P]
        lib.zett_op_embed_lookup_bwd.argtypes = [P, I32, I64, I64, I32, P, I64, P, I64, P, I64, P]
        lib.zett_op_batch_vocab_workspace_bytes.argtypes = [I64, I64, I64, C.POINTER(I64)]
        lib.zett_op_batch_vocab.argtypes = [P, I32, P, I32, I64, I64, I64, P, I32, I64, I32, P, P, I32, I32, P, P, P, I32, P, P, P, P, P, P, P, P, P, I64, P]
        U64 = C.c_uint64
        lib.zett_op_label_batch.argtypes = [P, I32, I64, I64, I32, P, I32, P, I32, I64, I64, I64, I64, I32, U64, U64, U64, U64, P, I64, P, P, P, P, P, I64, P]
        lib.zett_op_pad_vocabulary.argtypes = [P, I32, I64, I32, I64, I64, P, I32, P, P, P, P, P]
        lib.zett_encode_workspace_bytes.argtypes = [I64, I64, C.POINTER(I64)]
        lib.zett_encode_texts.argtypes = [P, P, P, I64, I64, P, I64, I32, I32, I32, P, I32, P, I32, P, P, I32, I32, P, P, I32, I64, P, I64, P, P]
        lib.zett_encode_added_workspace_bytes.argtypes = [I64, I64, I32, C.POINTER(I64)]
        lib.zett_encode_texts_added.argtypes = [P, P, P, I64, I64, P, I64, I32, I32, I32, P, I32, P, I32, P, P, I32, I32, P, P, I32, I64, P, P, P, I32, I32, P, I64, P, P]
        lib.zett_sampler_create.argtypes = [C.c_int, I32, I64, I64, I64, C.POINTER(P)]
        lib.zett_sampler_destroy.argtypes = [P]
        lib.zett_sampler_depth.argtypes = [P, C.POINTER(I32)]
        lib.zett_sampler_workspace_bytes.argtypes = [I64, I64, C.POINTER(I64)]
        lib.zett_sampler_sample.argtypes = [P, P, P, I64, I64, P, I64, I64, I32, I32, C.c_double, C.c_uint64, I32, I32, P, P, P, I64, P, P, I64, P, P]
        lib.zett_sampler_table.argtypes = [P, P, P, P, P, I64, P, P]
        lib.zett_retok_create_unigram_device.argtypes = [C.c_int, I64, C.POINTER(P)]
        lib.zett_sampled_vocab_workspace_bytes.argtypes = [I64, I32, C.POINTER(I64)]
        lib.zett_sampled_vocab_build.argtypes = [P, P, P, P, P, I64, I64, P, P, P, P, P, I32, I32, I32, P, P, P, I64, P, I64, P, I32, P, I64, P]
        lib.zett_sampled_vocab_commit.argtypes = [P, P]
        lib.zett_sampled_vocab_table.argtypes = [P, P, P, P, P, P, I64, P, P]
        lib.zett_sampled_vocab_patch_rows.argtypes = [P, P, P, P, I32, P, I64, I32, I32, P]
        lib.zett_op_fwd_layernorm.argtypes = [I32, P, P, I32, I32, I32, P, P, F, I32, P, P, P, P, P, P, P, I32, P, C.POINTER(I32), P]
        lib.zett_op_fwd_embed_layernorm.argtypes = [I32, P, P, P, P, P, P, P, P, P, P, I32, P, P, I64, I32, I32, I32, I32, P, P, F, I32, P, P, P, C.POINTER(I32), P]
        lib.zett_op_fwd_attention.argtypes = [I32, P, I64, P, P, I64, I32, I32, P, P, P, I64, I32, I32, F, I32, P, P, P]
        lib.zett_op_fwd_gather_src.argtypes = [I32, P, I32, I32, P, I32, I32, I32, P, P, P, P, P, P]
        lib.zett_op_fwd_ln_stats.argtypes = [I32, P, I32, I32, I32, F, P, P]
        lib.zett_op_fwd_fold_weight.argtypes = [I32, P, I32, I32, P, P, P, P, P, P, P, P]
        lib.zett_op_fwd_pair_qkv.argtypes = [I32, P, P, P, I32, I32, P, P, I64, I32, P, P, P, I32, P, P, I32, P, I64, P, P]
        lib.zett_op_fwd_gemm.argtypes = [I32, C.POINTER(ZettFwdGemmDesc), C.POINTER(I32), C.POINTER(I32), P]
        lib.zett_op_col_moments_workspace_bytes.argtypes = [I64, I32, C.POINTER(I64)]
        lib.zett_op_col_moments.argtypes = [P, I32, I64, I64, I32, I32, P, I32, P, I64, P]
        lib.zett_op_rescaler_fit.argtypes = [P, I32, P, D, D, P, P, P]
        lib.zett_op_adafactor_workspace_floats.argtypes = [P, P, P, I32, C.POINTER(I64)]
        lib.zett_op_adafactor_step.argtypes = [P, P, P, P, P, P, P, P, I32, D, D, D, I32, P, I64, P, P]
        for name in ABI_SYMBOLS:
            fn = getattr(lib, name)
            if name != "zett_last_error":
                fn.restype = C.c_int
        if lib.zett_abi_version() != ABI_VERSION:      # struct layouts below are those of this version
            raise RuntimeError(f"{path} has ABI version {lib.zett_abi_version()}, this package expects {ABI_VERSION}: "
                               "rebuild it (`python -m zett_amd.build`)")
        _lib = lib
    return _lib


class RangeError(OverflowError):
    """ZETT_E_RANGE: a value left the range of the 16-bit operand type, or an output is not finite."""


def check(rc: int, what: str = "") -> None:
    """Map a negative status to the exception the reference would raise."""
    if rc == ZETT_OK:
        return
    msg = load().zett_last_error().decode("utf-8", "replace")
    if what:
        msg = f"{what}: {msg}"
    if rc == E_INDEX:
        raise IndexError(msg)
    if rc == E_NOT_IMPLEMENTED:
        raise NotImplementedError(msg)
    if rc == E_KEY:
        raise KeyError(msg)
    if rc == E_INVALID:
        raise ValueError(msg)
    if rc == E_RANGE:
        raise RangeError(msg)
    raise RuntimeError(msg)
