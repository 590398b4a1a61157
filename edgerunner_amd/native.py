"""ctypes binding of ``libedgerunner_hip.so`` (C ABI: include/edgerunner_hip.h).

PyTorch is plumbing here: it owns the device tensors whose ``data_ptr()`` are
handed to the library and the HIP stream the work is enqueued on.  There is no
fallback: if the HIP extension is missing or fails to load this module raises,
it never routes around it.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

PKG = os.path.dirname(os.path.abspath(__file__))
# ER_LIB_PATH: A/B handle of the measurement scripts (another BUILD of the same library, e.g. build/ab/*.so); a path that
# does not exist fails as loudly as a missing default build
LIB_PATH = os.environ.get("ER_LIB_PATH") or os.path.join(PKG, "libedgerunner_hip.so")

ER_F32, ER_F16, ER_BF16, ER_F8E4M3, ER_F4E2M1 = 0, 1, 2, 3, 4
ER_COND_NONE, ER_COND_POINT, ER_COND_POINT_LATENT = 0, 1, 2
ER_GREEDY, ER_SAMPLE = 0, 1
ER_GRAMMAR_NONE, ER_GRAMMAR_NAIVE9, ER_GRAMMAR_LR_ABSCO = 0, 1, 2
ER_METO_LR_ABSCO, ER_METO_LR = 0, 1
ER_NUM_KERNEL_KINDS = 8
ER_PRED_V_PREDICTION, ER_PRED_EPSILON = 0, 1
ER_PE_EMBED, ER_PE_DOWNSAMPLE = 0, 1

# every symbol include/edgerunner_hip.h declares (tests/test_abi.py checks the .so exports them all)
EXPORTS = [
    "er_abi_version", "er_last_error", "er_create", "er_destroy", "er_load_tensor", "er_finalize_weights",
    "er_kv_reserve", "er_encode_cond", "er_embed_tokens", "er_prefill", "er_score", "er_point_latent", "er_set_point_encoder_mode", "er_logits", "er_feed", "er_decode",
    "er_meto_decode", "er_meto_encode", "er_dit_create", "er_dit_destroy", "er_dit_load_tensor",
    "er_dit_finalize_weights", "er_dit_project_cond", "er_dit_encode_image", "er_dit_forward", "er_dit_sample",
    "er_dit_set_prediction_type", "er_dit_attach_point_encoder", "er_dit_point_latent", "er_dit_set_point_encoder_mode", "er_dit_loss", "er_k_dit_loss",
    "er_set_row_streams", "er_set_prefix_groups", "er_plan_decode", "er_ctx_plan", "er_plan_gemm_tile", "er_kernel_kind_name", "er_profile_decode_kernels", "er_profile_decode_kernels_at", "er_last_decode_ms",
    "er_k_gemv", "er_k_gemv_form", "er_k_mlp_transpose", "er_k_mlp_sparse", "er_mlp_nnz", "er_k_attn_decode", "er_k_attn_stream_xt", "er_k_attn_shared", "er_k_attn_outproj3", "er_k_gemm", "er_k_gemm_f16", "er_k_gemm_hh", "er_k_gemm_hh_qkv", "er_k_gemm_hh_geglu", "er_k_gemm_f16s", "er_k_gemm_epi", "er_k_flash_attn_f16", "er_k_flash_attn_hh", "er_k_flash_attn_f32", "er_k_flash_attn_f16s", "er_k_layernorm", "er_k_softmax", "er_k_score_rows", "er_k_fps", "er_k_sample_head",
    "er_k_nn_dist2", "er_k_surface_sample", "er_k_fidelity_metrics",
    "er_queue_begin", "er_queue_admit", "er_queue_run", "er_queue_take", "er_queue_stats", "er_queue_end",
    "er_set_sampling", "er_get_logprobs", "er_queue_row_logprobs", "er_k_sample_head_ctl",
    "er_k_w8_quantize", "er_k_gemv_form_w8", "er_k_attn_outproj3_w8", "er_k_kv8_encode",
    "er_set_prefix_pass", "er_k_attn_shared_mfma", "er_ctx_w8_streams",
    "er_ctx_w4_streams", "er_ctx_w4_streams_batched", "er_k_w4_quantize", "er_k_gemv_form_w4", "er_k_w4_cvt_probe",
    "er_prefill_fork", "er_k_kv_fork", "er_queue_admit_copy",
    "er_k_softmax_batched", "er_k_kv_scatter", "er_k_split_rows_f16", "er_k_add_pos", "er_k_gather_rows", "er_k_point_embed", "er_k_geglu",
    "er_k_gelu", "er_k_silu", "er_k_ln_modulate", "er_k_adaln_gate", "er_k_adaln_gate_all", "er_k_timestep_embed", "er_k_ddim_cfg_step",
    "er_k_clip_preprocess", "er_k_clip_im2col", "er_k_clip_assemble",
    "er_prefill_extend", "er_embed_num_face", "er_k_attn_extend",
]


ER_ATTN_SPLIT1, ER_ATTN_SPLIT2, ER_ATTN_BALANCED, ER_ATTN_STREAM, ER_ATTN_SHARED, ER_ATTN_SHARED_MFMA = 1, 2, 3, 4, 5, 6
ER_PREFIX_PASS_VALU, ER_PREFIX_PASS_MFMA = 0, 1
PREFIX_PASSES = {"valu": ER_PREFIX_PASS_VALU, "mfma": ER_PREFIX_PASS_MFMA}


class ErDecodePlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batched", "decode_version", "attn_kernel", "attn_chunks", "merge_launch",
                                         "launches_per_layer")]


# er_k_gemv_form: prologue, epilogue and form of one decode projection (include/edgerunner_hip.h)
ER_PRO_NONE, ER_PRO_LN, ER_PRO_EMBED, ER_PRO_LN_SK = 0, 1, 2, 3
ER_EPI_STORE, ER_EPI_RELU, ER_EPI_RESID, ER_EPI_QKV = 0, 1, 2, 3
ER_FORM_ROW, ER_FORM_ROWS8, ER_FORM_VALU, ER_FORM_MFMA, ER_FORM_MFMA_XT, ER_FORM_NARROW, ER_FORM_NARROW_DEFER, ER_FORM_PREP = range(8)


class ErKGemvFormArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "w", "bias", "x", "ln_w", "ln_b", "xnorm_out", "embd", "posemb", "tok", "pos", "sk_part", "sk_bias", "sk_resid", "y", "resid",
        "q_out", "kcache", "vcache", "prep_xt_out", "xt_out", "part_out")] + [(n, C.c_int32) for n in (
        "w_half", "kv_half", "batch", "n", "k", "prologue", "epilogue", "form", "nw", "rw", "sk_slices", "heads", "head_dim",
        "l_cap")] + [("eps", C.c_float)]


class ErKMlpSparseArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "w2t", "zero_row", "b2", "x", "ln_w", "ln_b", "h1_out", "y", "part", "nnz")] + \
               [("w_half", C.c_int32), ("eps", C.c_float)]


# er_k_gemm_epi: one GEMM family with the whole plain epilogue (include/edgerunner_hip.h)
ER_GEMM_F32, ER_GEMM_F16, ER_GEMM_F16S, ER_GEMM_HH = range(4)


class ErKGemmEpiArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("a", "w", "bias", "resid", "gate", "c", "c16")] + [("gate_bstride", C.c_int64)] + \
               [(n, C.c_int32) for n in ("family", "m", "n", "k", "lda", "ldb", "ldc", "ldr", "resid_mod", "gate_rows", "relu", "force_tile")] + \
               [("div", C.c_float)]


class ErConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "hidden_dim", "num_heads", "num_layers", "intermediate_dim", "vocab_size", "max_positions",
        "num_cond_tokens", "point_hidden_dim", "point_num_heads", "point_latent_size", "point_latent_dim",
        "point_freq_dim", "num_face_buckets", "cond_mode", "pad_token_id", "bos_token_id", "eos_token_id",
        "weight_dtype", "kv_dtype")] + [("ln_eps", C.c_float)]


class ErDitConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hidden_dim", "num_heads", "num_layers", "latent_size", "latent_dim", "clip_dim",
                                         "clip_layers", "clip_heads", "clip_mlp_dim", "clip_image_size", "clip_patch", "weight_dtype")]


class ErDecodeParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("top_k", C.c_int32), ("grammar", C.c_int32),
                ("max_new_tokens", C.c_int32), ("min_new_tokens", C.c_int32), ("seed", C.c_uint64)]


class ErSampling(C.Structure):
    """er_sampling: the controls above TopK and the log-prob switch (top_k is read only when top_k_set != 0; 0 then means no filter)."""
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32), ("top_k_set", C.c_int32),
                ("logprobs", C.c_int32)]


class ErQueueCounters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("steps", "admissions", "occupied_row_steps", "wait_row_steps", "parked_row_steps")] + \
               [("prefill_ms", C.c_float), ("decode_ms", C.c_float)]


class NativeError(RuntimeError):
    pass


_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen the HIP extension (no GPU needed just to load it and list symbols)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise NativeError(
            f"HIP extension not built: {p} is missing. Run `python -m edgerunner_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU/eager fallback for this path.")
    lib = C.CDLL(p)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    lib.er_abi_version.restype = ci
    lib.er_last_error.restype = C.c_char_p
    lib.er_kernel_kind_name.restype = C.c_char_p
    lib.er_kernel_kind_name.argtypes = [ci]
    lib.er_create.argtypes = [C.POINTER(ErConfig), ci, C.POINTER(vp)]
    lib.er_destroy.argtypes = [vp]
    lib.er_load_tensor.argtypes = [vp, C.c_char_p, vp, ci, ci, C.POINTER(C.c_int64), ci]
    lib.er_finalize_weights.argtypes = [vp]
    lib.er_kv_reserve.argtypes = [vp, ci, ci]
    lib.er_encode_cond.argtypes = [vp, vp, ci, ci, C.POINTER(C.c_int32), vp, vp]
    lib.er_embed_tokens.argtypes = [vp, C.POINTER(C.c_int32), ci, ci, vp, vp]
    lib.er_prefill.argtypes = [vp, vp, ci, ci, vp]
    lib.er_prefill_fork.argtypes = [vp, vp, ci, ci, C.POINTER(C.c_int32), ci, vp]
    lib.er_prefill_extend.argtypes = [vp, vp, ci, ci, ci, vp]
    lib.er_embed_num_face.argtypes = [vp, C.POINTER(C.c_int32), ci, vp, vp]
    lib.er_k_kv_fork.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, C.POINTER(C.c_int32), C.POINTER(C.c_int32), ci, ci, vp]
    lib.er_logits.argtypes = [vp, vp, vp]
    lib.er_score.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]
    lib.er_point_latent.argtypes = [vp, vp, ci, ci, vp, vp, vp]
    lib.er_set_point_encoder_mode.argtypes = [vp, ci]
    lib.er_feed.argtypes = [vp, C.POINTER(C.c_int32), vp]
    lib.er_decode.argtypes = [vp, C.POINTER(ErDecodeParams), vp, C.POINTER(C.c_int32), vp]
    lib.er_profile_decode_kernels.argtypes = [vp, ci, C.POINTER(C.c_float), C.POINTER(C.c_double), vp]
    lib.er_profile_decode_kernels_at.argtypes = [vp, ci, ci, ci, C.POINTER(C.c_float), C.POINTER(C.c_double), vp]
    lib.er_last_decode_ms.argtypes = [vp, C.POINTER(C.c_float)]
    i32p = C.POINTER(C.c_int32)
    lib.er_meto_decode.argtypes = [i32p, ci, ci, ci, C.POINTER(C.c_float), i32p, i32p, i32p, i32p, i32p]
    lib.er_meto_encode.argtypes = [C.POINTER(C.c_float), ci, i32p, ci, ci, ci, i32p, i32p, i32p, i32p, i32p]
    lib.er_dit_create.argtypes = [C.POINTER(ErDitConfig), ci, C.POINTER(vp)]
    lib.er_dit_destroy.argtypes = [vp]
    lib.er_dit_load_tensor.argtypes = [vp, C.c_char_p, vp, ci, ci, C.POINTER(C.c_int64), ci]
    lib.er_dit_finalize_weights.argtypes = [vp]
    lib.er_dit_project_cond.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.er_dit_encode_image.argtypes = [vp, vp, ci, ci, ci, vp, vp]
    lib.er_dit_forward.argtypes = [vp, vp, vp, C.POINTER(C.c_float), ci, ci, vp, vp]
    lib.er_dit_sample.argtypes = [vp, vp, ci, ci, vp, ci, cf, ci, vp]
    lib.er_dit_set_prediction_type.argtypes = [vp, ci]
    lib.er_dit_attach_point_encoder.argtypes = [vp, ci, ci, ci]
    lib.er_dit_point_latent.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.er_dit_set_point_encoder_mode.argtypes = [vp, ci]
    lib.er_k_fps.argtypes = [vp, ci, ci, ci, vp, vp]
    lib.er_k_nn_dist2.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp]
    lib.er_k_surface_sample.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), ci, ci, C.c_uint64, C.POINTER(C.c_uint32),
                                        vp, vp, vp]
    lib.er_k_fidelity_metrics.argtypes = [vp, vp, ci, ci, ci, cf, vp, vp]
    lib.er_dit_loss.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int32), ci, ci, cf, vp, vp, vp, vp]
    lib.er_k_dit_loss.argtypes = [vp, vp, vp, C.POINTER(C.c_int32), ci, ci, ci, cf, vp, vp, vp]
    lib.er_plan_decode.argtypes = [ci, ci, ci, ci, ci, C.POINTER(ErDecodePlan)]
    lib.er_ctx_plan.argtypes = [vp, C.POINTER(ErDecodePlan)]
    lib.er_ctx_w8_streams.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.er_ctx_w4_streams.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.er_ctx_w4_streams_batched.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.er_set_row_streams.argtypes = [vp, C.POINTER(C.c_uint32), ci]
    lib.er_set_prefix_groups.argtypes = [vp, C.POINTER(C.c_int32), ci, ci]
    lib.er_set_prefix_pass.argtypes = [vp, ci]
    lib.er_plan_gemm_tile.argtypes = [ci, ci, ci]
    lib.er_queue_begin.argtypes = [vp, C.POINTER(ErDecodeParams), ci, vp]
    lib.er_queue_admit.argtypes = [vp, ci, ci, vp, ci, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), vp]
    lib.er_queue_admit_copy.argtypes = [vp, ci, C.POINTER(C.c_int32), ci, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), vp]
    lib.er_queue_run.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
    lib.er_queue_take.argtypes = [vp, ci, C.POINTER(C.c_int64), ci, C.POINTER(C.c_int32)]
    lib.er_queue_stats.argtypes = [vp, C.POINTER(ErQueueCounters)]
    lib.er_queue_end.argtypes = [vp]
    lib.er_k_gemv.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, vp]
    lib.er_k_gemv_form.argtypes = [C.POINTER(ErKGemvFormArgs), vp]
    lib.er_k_mlp_transpose.argtypes = [vp, vp, ci, vp]
    lib.er_k_mlp_sparse.argtypes = [C.POINTER(ErKMlpSparseArgs), vp]
    lib.er_mlp_nnz.argtypes = [vp, C.POINTER(C.c_int32), ci]
    lib.er_k_attn_stream_xt.argtypes = [vp, vp, vp, C.POINTER(C.c_int32), vp, vp, ci, ci, ci, ci, vp]
    lib.er_k_attn_shared.argtypes = [vp, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), ci, vp, vp, ci, ci, ci, ci, vp]
    lib.er_k_attn_shared_mfma.argtypes = lib.er_k_attn_shared.argtypes
    lib.er_k_attn_extend.argtypes = [vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, vp]
    lib.er_k_attn_decode.argtypes = [vp, vp, vp, C.POINTER(C.c_int32), vp, ci, ci, ci, ci, ci, ci, ci, vp]
    lib.er_k_attn_outproj3.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, vp]
    lib.er_k_w8_quantize.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
    lib.er_k_kv8_encode.argtypes = [vp, vp, C.c_longlong, vp]
    lib.er_k_w4_quantize.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp]
    lib.er_k_gemv_form_w4.argtypes = [C.POINTER(ErKGemvFormArgs), vp, vp]
    lib.er_k_w4_cvt_probe.argtypes = [vp, vp]
    lib.er_k_gemv_form_w8.argtypes = [C.POINTER(ErKGemvFormArgs), vp, vp, vp]
    lib.er_k_attn_outproj3_w8.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, vp]
    lib.er_k_gemm.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp]
    lib.er_k_gemm_f16.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
    lib.er_k_gemm_f16s.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
    lib.er_k_gemm_hh.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
    lib.er_k_gemm_epi.argtypes = [C.POINTER(ErKGemmEpiArgs), vp]
    lib.er_k_gemm_hh_qkv.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.er_k_gemm_hh_geglu.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.er_k_flash_attn_f16.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.er_k_flash_attn_hh.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.er_k_flash_attn_f32.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
    lib.er_k_flash_attn_f16s.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.er_k_layernorm.argtypes = [vp, vp, vp, vp, ci, ci, cf, vp]
    lib.er_k_softmax.argtypes = [vp, ci, ci, ci, ci, vp]
    ll = C.c_longlong
    lib.er_k_softmax_batched.argtypes = [vp, ci, ci, ll, ci, ci, ll, ci, ci, vp]
    lib.er_k_kv_scatter.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ll, vp]
    lib.er_k_split_rows_f16.argtypes = [vp, vp, vp, ll, ci, ci, vp]
    lib.er_k_add_pos.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp]
    lib.er_k_gather_rows.argtypes = [vp, ci, vp, vp, ci, ci, ll, vp]
    lib.er_k_point_embed.argtypes = [vp, vp, vp, ll, ci, ci, vp]
    lib.er_k_geglu.argtypes = [vp, vp, ll, ci, vp]
    lib.er_k_gelu.argtypes = [vp, vp, ll, vp]
    lib.er_k_silu.argtypes = [vp, vp, ll, vp]
    lib.er_k_ln_modulate.argtypes = [vp, vp, ci, ci, ci, vp, vp, ll, ll, ci, ci, vp, vp]
    lib.er_k_adaln_gate.argtypes = [vp, vp, vp, ci, ci, ci, vp]
    lib.er_k_adaln_gate_all.argtypes = [vp, vp, vp, ci, ci, ci, vp]
    lib.er_k_timestep_embed.argtypes = [vp, vp, ci, ci, vp]
    lib.er_k_ddim_cfg_step.argtypes = [vp, vp, ll, ci, cf, cf, cf, cf, cf, vp]
    lib.er_k_clip_preprocess.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    lib.er_k_clip_im2col.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    lib.er_k_clip_assemble.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp]
    lib.er_k_score_rows.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp]
    lib.er_k_sample_head.argtypes = [vp, C.POINTER(ErDecodeParams), ci, ci, ci, ci, ci, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
    f32p = C.POINTER(C.c_float)
    lib.er_set_sampling.argtypes = [vp, C.POINTER(ErSampling)]
    lib.er_get_logprobs.argtypes = [vp, vp, vp, ci, ci, vp]
    lib.er_queue_row_logprobs.argtypes = [vp, ci, f32p, f32p, ci]
    lib.er_k_sample_head_ctl.argtypes = [vp, C.POINTER(ErDecodeParams), C.POINTER(ErSampling), ci, ci, ci, ci, ci, i32p, i32p, i32p,
                                         i32p, i32p, i32p, f32p, f32p, i32p, vp]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("er_last_error", "er_kernel_kind_name"):
            fn.restype = ci
    if lib.er_abi_version() != 1:
        raise NativeError(f"ABI version mismatch: library {lib.er_abi_version()}, binding 1")
    if path is None:
        _lib = lib
    return lib


def check(rc: int, what: str = "") -> int:
    if rc < 0:
        msg = load_library().er_last_error().decode(errors="replace")
        raise NativeError(f"{what} failed ({rc}): {msg}")
    return rc


def i32_array(values: Sequence[int]):
    return (C.c_int32 * len(values))(*[int(v) for v in values])


def ptr(t) -> C.c_void_p:
    """Device (or host) pointer of a contiguous torch tensor; None -> NULL."""
    if t is None:
        return C.c_void_p(0)
    assert t.is_contiguous(), "tensor handed to the C ABI must be contiguous"
    return C.c_void_p(t.data_ptr())


def load_tensor(fn, ctx, key: str, t) -> int:
    """One checkpoint tensor through ``fn`` (er_load_tensor / er_dit_load_tensor): fp32 / fp16 / bf16 as they are, any other dtype
    as fp32, from host or device memory.  Returns 1 for a key the context does not hold."""
    import torch
    dtypes = {torch.float32: ER_F32, torch.float16: ER_F16, torch.bfloat16: ER_BF16}
    if t.dtype not in dtypes:
        t = t.float()
    t = t.detach().contiguous()
    shape = (C.c_int64 * max(1, t.dim()))(*(list(t.shape) or [1]))
    return check(fn(ctx, key.encode(), ptr(t), dtypes[t.dtype], max(1, t.dim()), shape, 1 if t.is_cuda else 0),
                 f"{fn.__name__}({key})")


def stream_ptr(stream) -> C.c_void_p:
    """hipStream_t of a torch.cuda.Stream (or the current stream when None)."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)
