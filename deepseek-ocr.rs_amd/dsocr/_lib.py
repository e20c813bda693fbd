"""ctypes binding of include/dsocr.h (the C ABI).  Loads the in-tree
deepseek-ocr.rs_amd/lib/libdsocr.so and fails loudly if it is missing: there is
no CPU fallback in the product path."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libdsocr.so")

OK, EINVAL, ENOENT, EDEVICE, ENOMEM, EINTERNAL = range(6)
STATUS_NAMES = {0: "OK", 1: "EINVAL", 2: "ENOENT", 3: "EDEVICE", 4: "ENOMEM", 5: "EINTERNAL"}
DTYPES = {"f32": 0, "f16": 1, "bf16": 2}


class DsocrError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status
        self.message = message


class LoadArgs(C.Structure):
    _fields_ = [("config_path", C.c_char_p), ("weights_path", C.c_char_p), ("snapshot_path", C.c_char_p),
                ("device_ordinal", C.c_int), ("dtype", C.c_int), ("synthetic_seed", C.c_uint64)]


class VisionSettingsC(C.Structure):
    _fields_ = [("base_size", C.c_uint32), ("image_size", C.c_uint32), ("crop_mode", C.c_int)]


class DecodeParamsC(C.Structure):
    _fields_ = [("max_new_tokens", C.c_size_t), ("do_sample", C.c_int), ("temperature", C.c_double),
                ("top_p", C.c_double), ("top_k", C.c_size_t), ("repetition_penalty", C.c_float),
                ("no_repeat_ngram_size", C.c_size_t), ("seed", C.c_uint64), ("use_cache", C.c_int),
                ("eos_token_id", C.c_int64), ("ignore_eos", C.c_int), ("has_seed", C.c_int)]


class RequestC(C.Structure):
    _fields_ = [("input_ids", C.POINTER(C.c_int64)), ("image_mask", C.POINTER(C.c_uint8)),
                ("prompt_len", C.c_size_t), ("page", C.c_void_p), ("image_rows", C.POINTER(C.c_float)),
                ("n_image_rows", C.c_size_t)]


class ResultC(C.Structure):
    _fields_ = [("out_ids", C.POINTER(C.c_int64)), ("cap", C.c_size_t), ("n_out", C.c_size_t),
                ("status", C.c_int)]


class TimingsC(C.Structure):
    _fields_ = [("vision_prepare_ms", C.c_double), ("vision_compute_ms", C.c_double),
                ("decode_prefill_ms", C.c_double), ("decode_iterative_ms", C.c_double),
                ("decode_generate_ms", C.c_double), ("decode_steps", C.c_size_t), ("pages", C.c_size_t),
                ("vision_flops", C.c_double), ("prefill_flops", C.c_double)]


class KernelProfileC(C.Structure):
    _fields_ = [("avg_us", C.c_double), ("bytes", C.c_double), ("flops", C.c_double), ("launches", C.c_int),
                ("replay_us", C.c_double), ("ctx_us", C.c_double)]


class DecodeProfileC(C.Structure):
    _fields_ = [("moe_gateup", KernelProfileC), ("moe_down", KernelProfileC), ("attention", KernelProfileC),
                ("lm_head", KernelProfileC), ("experts_touched", C.c_int), ("tokens", C.c_int), ("kv_len", C.c_int),
                ("qkv", KernelProfileC), ("o_proj", KernelProfileC), ("router", KernelProfileC),
                ("layers_step", KernelProfileC), ("lm_head_screened", KernelProfileC),
                ("moe_gateup_kernel", C.c_char_p), ("moe_down_kernel", C.c_char_p)]


class SlotStatusC(C.Structure):
    _fields_ = [("slot", C.c_int32), ("done", C.c_int32), ("out_len", C.c_int32), ("n_new", C.c_int32)]


class SessionDescC(C.Structure):
    _fields_ = [("slots", C.c_size_t), ("active", C.c_size_t), ("max_context", C.c_size_t), ("out_cap", C.c_size_t),
                ("kv_cap", C.c_size_t), ("burst_cap", C.c_size_t), ("steps", C.c_size_t), ("flags", C.c_size_t)]


class LogprobsC(C.Structure):
    """dsocr_logprobs: one page's caller buffers of dsocr_generate_logprobs."""
    _fields_ = [("token_lp", C.POINTER(C.c_float)), ("top_id", C.POINTER(C.c_int64)), ("top_lp", C.POINTER(C.c_float)),
                ("cap", C.c_size_t), ("n", C.c_size_t)]


class LogitBiasC(C.Structure):
    """dsocr_logit_bias: one request's constraint (host pointers)."""
    _fields_ = [("ids", C.POINTER(C.c_int64)), ("values", C.POINTER(C.c_float)), ("n", C.c_size_t),
                ("allow_only", C.c_int)]


class StopSetC(C.Structure):
    """dsocr_stop_set: one request's stop sequences, back to back (host pointers)."""
    _fields_ = [("ids", C.POINTER(C.c_int64)), ("lens", C.POINTER(C.c_size_t)), ("n", C.c_size_t)]


class StopHitC(C.Structure):
    """dsocr_stop_hit: the lowest matching sequence and its length (seq = -1: no stop fired)."""
    _fields_ = [("seq", C.c_int32), ("match_len", C.c_int32)]


class PenaltiesC(C.Structure):
    """dsocr_penalties: one request's frequency / presence penalties and min-p."""
    _fields_ = [("frequency", C.c_float), ("presence", C.c_float), ("min_p", C.c_double)]


class NgramWindowC(C.Structure):
    """dsocr_ngram_window: one request's windowed no-repeat n-gram ban."""
    _fields_ = [("ngram_size", C.c_int32), ("window", C.c_int32), ("whitelist", C.POINTER(C.c_int32)),
                ("n_whitelist", C.c_size_t)]


class GuidedC(C.Structure):
    """dsocr_guided: one request's token automaton."""
    _fields_ = [("n_states", C.c_int32), ("start", C.c_int32), ("accepting", C.POINTER(C.c_uint8)),
                ("row_ptr", C.POINTER(C.c_int32)), ("edge_tok", C.POINTER(C.c_int32)),
                ("edge_next", C.POINTER(C.c_int32))]


class GuidedResultC(C.Structure):
    """dsocr_guided_result: the automaton state and status (0 running, 1 complete, 2 violated) of a page."""
    _fields_ = [("state", C.c_int32), ("status", C.c_int32)]


class RowParamsC(C.Structure):
    """dsocr_row_params: one row of dsocr_k_select_rows."""
    _fields_ = [("do_sample", C.c_int), ("temperature", C.c_double), ("top_p", C.c_double), ("top_k", C.c_size_t),
                ("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_size_t), ("eos_token_id", C.c_int64)]


class ScreenStepsC(C.Structure):
    """dsocr_screen_steps: the arguments of dsocr_k_lmhead_screen_steps (host pointers)."""
    _fields_ = ([(n, C.c_int) for n in ("B", "V", "K", "wdtype", "steps", "probe")] +
                [("W", C.c_void_p), ("x", C.c_void_p), ("ldx", C.c_longlong), ("norm_w", C.c_void_p), ("eps", C.c_float),
                 ("ctx", C.c_void_p), ("ctx_cap", C.c_int), ("ctx_len", C.c_void_p), ("ngram", C.c_int), ("eos", C.c_int),
                 ("rows", C.POINTER(RowParamsC)), ("ban", C.c_void_p), ("ban_ld", C.c_int), ("out_cap", C.c_int),
                 ("table", C.c_void_p), ("table_dt", C.c_int), ("H", C.c_int)] +
                [(n, C.c_void_p) for n in ("out_tok", "ban_out", "ctx_out", "ctx_len_out", "out_ids", "out_len", "done",
                                           "kv_pos", "kv_len", "x_next", "blk_cnt", "blk_t", "cand", "cand_hi", "xn_out", "xn_gemv",
                                           "q", "scale", "bound", "qnorm", "qfrag")])


SESSION_PER_REQUEST = 1  # DSOCR_SESSION_PER_REQUEST
SESSION_LOGPROBS = 2     # DSOCR_SESSION_LOGPROBS
SESSION_LOGIT_BIAS = 4   # DSOCR_SESSION_LOGIT_BIAS
SESSION_STOP = 8         # DSOCR_SESSION_STOP
SESSION_PENALTIES = 16   # DSOCR_SESSION_PENALTIES
SESSION_NGRAM_WINDOW = 32  # DSOCR_SESSION_NGRAM_WINDOW
MAX_NGRAM_WHITELIST = 32   # DSOCR_MAX_NGRAM_WHITELIST
SESSION_GUIDED = 64        # DSOCR_SESSION_GUIDED
MAX_STOP_SEQS = 16       # DSOCR_MAX_STOP_SEQS
MAX_STOP_LEN = 32        # DSOCR_MAX_STOP_LEN
SESSION_ADMIT_PENDING = 0x100  # DSOCR_SESSION_ADMIT_PENDING (dsocr_session_info flags while an admission is pending)
MAX_TOP_LOGPROBS = 20    # DSOCR_MAX_TOP_LOGPROBS


class DotsTimingsC(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("patch_ms", C.c_double), ("blocks_ms", C.c_double),
                ("attention_ms", C.c_double), ("merger_ms", C.c_double), ("tokens", C.c_size_t), ("groups", C.c_size_t)]


LOAD_PACKED_EXPERTS = 1  # DSOCR_LOAD_PACKED_EXPERTS
STREAM_CB = C.CFUNCTYPE(None, C.c_size_t, C.POINTER(C.c_int64), C.c_void_p)

# every symbol include/dsocr.h declares (tests check the library exports all of them)
EXPORTS = [
    "dsocr_engine_load", "dsocr_engine_free", "dsocr_last_error", "dsocr_engine_info", "dsocr_prepare_page",
    "dsocr_page_free", "dsocr_page_to_device", "dsocr_page_info", "dsocr_page_pixels_view", "dsocr_image_embeddings", "dsocr_generate",
    "dsocr_generate_batch", "dsocr_last_timings", "dsocr_profile_decode", "dsocr_device_count", "dsocr_dev_alloc", "dsocr_dev_free",
    "dsocr_memcpy_h2d", "dsocr_memcpy_d2h", "dsocr_dev_sync", "dsocr_synth_bf16", "dsocr_resize_bicubic",
    "dsocr_k_gemm", "dsocr_k_gemm_f32a", "dsocr_k_gemm_grouped", "dsocr_k_gemv", "dsocr_k_layernorm", "dsocr_k_rmsnorm", "dsocr_k_attention", "dsocr_k_decode_attention", "dsocr_k_moe",
    "dsocr_k_sample_greedy", "dsocr_k_sample_stoch", "dsocr_k_dsq_dequant", "dsocr_prepare_page_device", "dsocr_page_read_device",
    "dsocr_generate_trace", "dsocr_k_moe_kernels", "dsocr_k_lmhead_screened",
    "dsocr_dots_load", "dsocr_dots_free", "dsocr_dots_info", "dsocr_dots_preprocess", "dsocr_dots_embed",
    "dsocr_dots_embed_device", "dsocr_dots_last_timings", "dsocr_k_attention_bf16", "dsocr_k_gemv_splitk",
    "dsocr_engine_set_spans", "dsocr_engine_spans", "dsocr_k_qkv_attention", "dsocr_k_poll_wait_fits",
    "dsocr_engine_set_persist_stamps", "dsocr_engine_persist_info",
    "dsocr_resize_catmull_rom",
    "dsocr_engine_load_flags", "dsocr_engine_packed_info", "dsocr_k_moe_packed", "dsocr_k_dsq_rows_dot",
    "dsocr_k_moe_ex", "dsocr_k_moe_route_kind", "dsocr_k_moe_prefill_route", "dsocr_k_moe_combine",
    "dsocr_k_gemm_bf16", "dsocr_k_dots_op",
    "dsocr_k_gemv_ex", "dsocr_k_gemv_kind", "dsocr_k_mm_swizzle", "dsocr_k_silu_mul",
    "dsocr_config_variant", "dsocr_engine_variant", "dsocr_prepare_page_variant", "dsocr_prepare_page_device_variant", "dsocr_k_attention_prefix",
    "dsocr_k_prefill_attention",
    "dsocr_session_open", "dsocr_session_admit", "dsocr_session_step", "dsocr_session_poll", "dsocr_session_retire",
    "dsocr_session_close", "dsocr_session_info", "dsocr_k_session_slot_move",
    "dsocr_session_open_ex", "dsocr_session_admit_params", "dsocr_session_head_steps", "dsocr_k_select_rows",
    "dsocr_generate_logprobs", "dsocr_session_logprobs", "dsocr_k_logprobs", "dsocr_k_logprobs_penalty",
    "dsocr_session_prefix_keep", "dsocr_session_admit_prefix", "dsocr_session_prefix_drop", "dsocr_session_prefix_stats",
    "dsocr_k_prefill_attention_past", "dsocr_k_session_prefix_copy",
    "dsocr_k_qkv_attention_layers",
    "dsocr_k_lmhead_screen_steps", "dsocr_k_lmhead_screen_grid",
    "dsocr_session_admit_begin", "dsocr_session_admit_advance", "dsocr_session_admit_cancel",
    "dsocr_session_admit_progress", "dsocr_k_attention_chunk",
    "dsocr_logit_bias_check", "dsocr_generate_logit_bias", "dsocr_session_stage_logit_bias", "dsocr_k_logit_bias",
    "dsocr_stop_set_check", "dsocr_generate_stop", "dsocr_session_stage_stop", "dsocr_session_stop_hit",
    "dsocr_stop_launches", "dsocr_k_stop_match", "dsocr_generate_stop_stream",
    "dsocr_penalties_check", "dsocr_generate_penalties", "dsocr_session_stage_penalties", "dsocr_k_out_penalty",
    "dsocr_k_sample_stoch_min_p",
    "dsocr_ngram_window_check", "dsocr_generate_ngram_window", "dsocr_session_stage_ngram_window",
    "dsocr_k_ngram_window",
    "dsocr_guided_check", "dsocr_generate_guided", "dsocr_session_stage_guided", "dsocr_session_guided_state",
    "dsocr_k_guided_mask", "dsocr_k_guided_advance",
    "dsocr_k_gemm_f32a_ex", "dsocr_k_layernorm_ex", "dsocr_k_rmsnorm_ex", "dsocr_k_sam_relbias", "dsocr_k_attention_fused",
    "dsocr_k_vision_op", "dsocr_window_maps",
]

# model variants behind the deepseek engine (dsocr_engine_variant)
VARIANT_OCR1, VARIANT_OCR2 = 0, 1

# dsocr_k_dots_op op codes (DSOCR_DOTS_*)
DOTS_RMSNORM, DOTS_LAYERNORM, DOTS_SWIGLU, DOTS_GELU, DOTS_ROPE_QK, DOTS_TO_BF16, DOTS_BF16_TO_F32 = range(7)

# dsocr_k_vision_op op codes (DSOCR_VIS_*)
(VIS_PATCH_IM2COL, VIS_CONV_IM2COL_NHWC, VIS_ADD_BROADCAST, VIS_CLIP_EMBED, VIS_CONCAT_CLIP_SAM, VIS_ASSEMBLE_ROWS,
 VIS_EMBED_TOKENS, VIS_TRACE_LOGITS, VIS_OCR2_BUILD_SEQ, VIS_OCR2_ROPE, VIS_OCR2_TAKE_QUERIES) = range(11)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DsocrError(EINTERNAL, f"libdsocr.so not built at {LIB_PATH}; run `python deepseek-ocr.rs_amd/build.py`")
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, u32, f32, i64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_float, C.c_int64
    L.dsocr_last_error.restype = C.c_char_p
    L.dsocr_engine_load.argtypes = [C.POINTER(LoadArgs), C.POINTER(vp)]
    L.dsocr_engine_load_flags.argtypes = [C.POINTER(LoadArgs), u32, C.POINTER(vp)]
    L.dsocr_engine_packed_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.dsocr_engine_free.argtypes = [vp]
    L.dsocr_engine_free.restype = None
    L.dsocr_engine_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(i64), C.POINTER(sz)]
    L.dsocr_prepare_page.argtypes = [vp, u32, u32, C.POINTER(VisionSettingsC), C.POINTER(vp)]
    L.dsocr_page_free.argtypes = [vp]
    L.dsocr_engine_variant.argtypes = [vp, C.POINTER(i32)]
    L.dsocr_config_variant.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(u32), C.POINTER(u32)]
    L.dsocr_prepare_page_variant.argtypes = [vp, u32, u32, C.POINTER(VisionSettingsC), i32, C.POINTER(vp)]
    L.dsocr_prepare_page_device_variant.argtypes = [vp, vp, u32, u32, C.POINTER(VisionSettingsC), C.POINTER(vp)]
    L.dsocr_k_attention_prefix.argtypes = [i32, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp]
    L.dsocr_prepare_page_device.argtypes = [vp, vp, u32, u32, C.POINTER(VisionSettingsC), C.POINTER(vp)]
    L.dsocr_page_read_device.argtypes = [vp, vp, vp]
    L.dsocr_page_free.restype = None
    L.dsocr_page_to_device.argtypes = [vp, vp]
    L.dsocr_page_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(sz)]
    L.dsocr_page_pixels_view.argtypes = [vp, C.POINTER(vp), C.POINTER(u32), C.POINTER(vp), C.POINTER(u32)]
    L.dsocr_image_embeddings.argtypes = [vp, C.POINTER(vp), sz, vp, sz, C.POINTER(sz)]
    L.dsocr_generate.argtypes = [vp, C.POINTER(RequestC), C.POINTER(DecodeParamsC), STREAM_CB, vp, vp, sz,
                                 C.POINTER(sz)]
    L.dsocr_generate_batch.argtypes = [vp, sz, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(ResultC)]
    L.dsocr_generate_trace.argtypes = [vp, sz, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(ResultC), vp,
                                       sz]
    L.dsocr_k_attention_bf16.argtypes = [i32, i32, i32, i32, f32, vp, C.c_long, vp, C.c_long, i32]
    L.dsocr_k_gemm_bf16.argtypes = [i32, i32, i32, vp, C.c_long, vp, C.c_long, vp, vp, C.c_long, i32, i32, i32, i32, i32,
                                    vp, vp, i32]
    L.dsocr_k_dots_op.argtypes = [i32, C.c_long, i32, i32, C.c_long, vp, vp, vp, f32, vp]
    L.dsocr_k_gemm_f32a_ex.argtypes = [i32, i32, i32, vp, C.c_long, vp, i32, vp, vp, C.c_long, vp, i32, i32, i32, i32, i32,
                                       C.POINTER(i32)]
    L.dsocr_k_layernorm_ex.argtypes = [i32, i32, vp, i32, vp, vp, f32, vp, i32, vp, i32]
    L.dsocr_k_rmsnorm_ex.argtypes = [i32, i32, vp, i32, vp, f32, vp, i32]
    L.dsocr_k_sam_relbias.argtypes = [i32, i32, i32, i32, i32, vp, C.c_long, vp, vp, vp]
    L.dsocr_k_attention_fused.argtypes = [i32, i32, i32, i32, f32, vp, C.c_long, vp, C.c_long, vp, vp, i32, i32]
    L.dsocr_k_vision_op.argtypes = [i32, C.POINTER(C.c_longlong), i32, C.POINTER(vp), i32]
    L.dsocr_window_maps.argtypes = [i32, i32, i32, vp, vp]
    L.dsocr_dots_load.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, i32, C.POINTER(vp)]
    L.dsocr_dots_free.argtypes = [vp]
    L.dsocr_dots_free.restype = None
    L.dsocr_dots_info.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.dsocr_dots_preprocess.argtypes = [C.c_char_p, vp, u32, u32, vp, sz, C.POINTER(sz), C.POINTER(u32)]
    L.dsocr_dots_embed.argtypes = [vp, vp, u32, u32, vp, sz, C.POINTER(sz), C.POINTER(u32)]
    L.dsocr_dots_embed_device.argtypes = [vp, vp, u32, u32, u32, vp, i32]
    L.dsocr_dots_last_timings.argtypes = [vp, C.POINTER(DotsTimingsC)]
    L.dsocr_k_lmhead_screened.argtypes = [i32, i32, i32, vp, vp, f32, vp, vp, i32, vp]
    L.dsocr_k_lmhead_screen_steps.argtypes = [C.POINTER(ScreenStepsC)]
    L.dsocr_k_lmhead_screen_grid.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(C.c_longlong), C.POINTER(i32)]
    L.dsocr_k_moe_kernels.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    L.dsocr_last_timings.argtypes = [vp, C.POINTER(TimingsC)]
    L.dsocr_profile_decode.argtypes = [vp, i32, C.POINTER(DecodeProfileC)]
    L.dsocr_engine_set_spans.argtypes = [vp, i32]
    L.dsocr_engine_spans.argtypes = [vp, vp, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.dsocr_engine_set_persist_stamps.argtypes = [vp, i32]
    L.dsocr_engine_persist_info.argtypes = [vp, C.POINTER(i32), vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]
    L.dsocr_device_count.argtypes = [C.POINTER(i32)]
    L.dsocr_dev_alloc.argtypes = [sz, C.POINTER(vp)]
    L.dsocr_dev_free.argtypes = [vp]
    L.dsocr_memcpy_h2d.argtypes = [vp, vp, sz]
    L.dsocr_memcpy_d2h.argtypes = [vp, vp, sz]
    L.dsocr_synth_bf16.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, vp]
    L.dsocr_resize_bicubic.argtypes = [vp, u32, u32, vp, u32, u32]
    L.dsocr_resize_catmull_rom.argtypes = [vp, u32, u32, vp, u32, u32]
    L.dsocr_k_gemm.argtypes = [i32, i32, i32, vp, vp, i32, vp, vp, i32, i32]
    L.dsocr_k_gemm_f32a.argtypes = [i32, i32, i32, vp, vp, i32, vp, vp, i32, i32, i32]
    L.dsocr_k_gemm_grouped.argtypes = [i32, i32, i32, vp, i32, vp, vp, i32, C.c_longlong, vp, C.c_longlong, vp, i32, vp, i32,
                                       i32, vp, i32, i32, i32]
    L.dsocr_k_gemv.argtypes = [i32, i32, i32, vp, vp, f32, vp, i32, vp, vp, i32, i32]
    L.dsocr_k_gemv_splitk.argtypes = [i32, i32, i32, vp, vp, i32, vp, vp, i32]
    L.dsocr_k_gemv_ex.argtypes = [i32, i32, i32, vp, i32, vp, f32, vp, i32, i32, vp, vp, i32, i32, i32, i32,
                                  C.POINTER(C.c_char_p)]
    L.dsocr_k_gemv_kind.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_char_p), C.POINTER(i32)]
    L.dsocr_k_mm_swizzle.argtypes = [i32, i32, vp, vp]
    L.dsocr_k_silu_mul.argtypes = [i32, i32, vp, i32, vp, i32]
    L.dsocr_k_layernorm.argtypes = [i32, i32, vp, vp, vp, f32, vp]
    L.dsocr_k_rmsnorm.argtypes = [i32, i32, vp, vp, f32, vp]
    L.dsocr_k_dsq_dequant.argtypes = [i32, vp, sz, sz, sz, vp]
    L.dsocr_k_attention.argtypes = [i32, i32, i32, i32, f32, i32, vp, vp, vp, vp, vp, vp, i32, i32]
    L.dsocr_k_decode_attention.argtypes = [i32, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp, i32]
    L.dsocr_k_prefill_attention.argtypes = [i32, i32, i32, i32, i32, i32, i32, f32, C.POINTER(i32), vp, vp, vp, vp, vp, vp,
                                            i32]
    L.dsocr_k_qkv_attention.argtypes = [i32, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp,
                                        vp, C.POINTER(i32)]
    L.dsocr_k_qkv_attention_layers.argtypes = [i32, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, i32, vp, vp, vp, vp,
                                               vp, vp, vp, vp, C.POINTER(i32)]
    L.dsocr_k_poll_wait_fits.argtypes = [C.c_long, i32, i32]
    L.dsocr_k_moe_packed.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, f32, vp, i32, vp, i32, vp, i32, vp, i32, vp,
                                     i32, f32, vp, vp, vp]
    L.dsocr_k_dsq_rows_dot.argtypes = [i32, sz, sz, vp, i32, vp, vp]
    L.dsocr_k_moe.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, vp]
    L.dsocr_k_moe_ex.argtypes = L.dsocr_k_moe.argtypes + [i32, vp, vp]
    L.dsocr_k_moe_route_kind.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_char_p)]
    L.dsocr_k_moe_prefill_route.argtypes = [i32, i32, i32, vp, i32, i32, f32, vp, vp, vp, vp, vp]
    L.dsocr_k_moe_combine.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, i32]
    L.dsocr_k_sample_greedy.argtypes =[i32, i32, vp, vp, i32, vp, i32, f32, vp]
    L.dsocr_k_sample_stoch.argtypes = [i32, i32, vp, vp, i32, vp, i32, f32, C.c_double, C.c_size_t, C.c_double,
                                       C.c_uint64, i32, vp]
    L.dsocr_session_open.argtypes = [vp, sz, sz, C.POINTER(DecodeParamsC)]
    L.dsocr_session_admit.argtypes = [vp, C.POINTER(RequestC), sz, i32, C.c_uint64, C.POINTER(i32)]
    L.dsocr_session_open_ex.argtypes = [vp, sz, sz, C.POINTER(DecodeParamsC), u32]
    L.dsocr_session_admit_params.argtypes = [vp, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(i32)]
    L.dsocr_session_head_steps.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.dsocr_k_select_rows.argtypes = [i32, i32, vp, vp, i32, vp, C.POINTER(RowParamsC), C.POINTER(C.c_uint64), i32, vp]
    L.dsocr_session_step.argtypes = [vp, sz, C.POINTER(SlotStatusC), sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]
    L.dsocr_session_poll.argtypes = [vp, C.POINTER(SlotStatusC), sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]
    L.dsocr_session_retire.argtypes = [vp, i32, vp, sz, C.POINTER(sz), C.POINTER(i32)]
    L.dsocr_session_close.argtypes = [vp]
    L.dsocr_session_info.argtypes = [vp, C.POINTER(SessionDescC)]
    L.dsocr_generate_logprobs.argtypes = [vp, sz, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(ResultC), sz,
                                          C.POINTER(LogprobsC)]
    L.dsocr_session_logprobs.argtypes = [vp, i32, sz, sz, sz, vp, vp, vp]
    L.dsocr_session_prefix_keep.argtypes = [vp, i32, sz, C.POINTER(i32)]
    L.dsocr_session_admit_prefix.argtypes = [vp, i32, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(i32)]
    L.dsocr_session_prefix_drop.argtypes = [vp, i32]
    L.dsocr_session_prefix_stats.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.dsocr_k_prefill_attention_past.argtypes = [i32, i32, i32, i32, i32, i32, i32, f32, C.POINTER(i32), C.POINTER(i32),
                                                 vp, vp, vp, vp, vp, vp]
    L.dsocr_session_admit_begin.argtypes = [vp, C.POINTER(RequestC), C.POINTER(DecodeParamsC), sz, C.POINTER(i32)]
    L.dsocr_session_admit_advance.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.dsocr_session_admit_cancel.argtypes = [vp]
    L.dsocr_session_admit_progress.argtypes = [vp, C.POINTER(i32), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz),
                                               C.POINTER(i32), C.POINTER(sz)]
    L.dsocr_k_attention_chunk.argtypes = [i32, i32, i32, i32, i32, i32, i32, f32, C.POINTER(i32), C.POINTER(i32),
                                          vp, vp, vp, vp, vp, vp, i32, i32]
    L.dsocr_k_session_prefix_copy.argtypes = [i32, i32, i32, i32, i32, vp, vp, i32, i32, vp, i32]
    L.dsocr_k_logprobs.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    L.dsocr_k_logprobs_penalty.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, i32, vp, f32, vp, vp, vp]
    L.dsocr_k_session_slot_move.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, C.c_longlong, vp, vp,
                                            C.c_longlong, vp, vp, vp, vp, i32, vp, C.c_longlong, vp, i32, i32, i32]
    L.dsocr_logit_bias_check.argtypes = [C.POINTER(LogitBiasC), sz]
    L.dsocr_generate_logit_bias.argtypes = [vp, sz, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(ResultC),
                                            C.POINTER(C.POINTER(LogitBiasC)), sz, C.POINTER(LogprobsC)]
    L.dsocr_session_stage_logit_bias.argtypes = [vp, C.POINTER(LogitBiasC)]
    L.dsocr_k_logit_bias.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.dsocr_stop_set_check.argtypes = [C.POINTER(StopSetC), sz]
    L.dsocr_generate_stop.argtypes = [vp, sz, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(ResultC),
                                      C.POINTER(C.POINTER(StopSetC)), C.POINTER(StopHitC),
                                      C.POINTER(C.POINTER(LogitBiasC)), sz, C.POINTER(LogprobsC)]
    L.dsocr_generate_stop_stream.argtypes = [vp, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(StopSetC),
                                             STREAM_CB, vp, vp, sz, C.POINTER(sz), C.POINTER(StopHitC)]
    L.dsocr_session_stage_stop.argtypes = [vp, C.POINTER(StopSetC)]
    L.dsocr_session_stop_hit.argtypes = [vp, i32, C.POINTER(StopHitC)]
    L.dsocr_stop_launches.argtypes = [vp, C.POINTER(sz)]
    L.dsocr_k_stop_match.argtypes = [i32, i32, i32] + [vp] * 14
    L.dsocr_penalties_check.argtypes = [C.POINTER(PenaltiesC)]
    L.dsocr_generate_penalties.argtypes = [vp, sz, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(ResultC),
                                           C.POINTER(C.POINTER(PenaltiesC)), C.POINTER(C.POINTER(StopSetC)),
                                           C.POINTER(StopHitC), C.POINTER(C.POINTER(LogitBiasC)), sz,
                                           C.POINTER(LogprobsC)]
    L.dsocr_session_stage_penalties.argtypes = [vp, C.POINTER(PenaltiesC)]
    L.dsocr_k_out_penalty.argtypes = [i32, i32, i32, vp, vp, i32, vp, C.POINTER(PenaltiesC)]
    L.dsocr_k_sample_stoch_min_p.argtypes = [i32, i32, vp, vp, i32, vp, i32, f32, C.c_double, C.c_size_t, C.c_double,
                                             vp, C.c_uint64, i32, vp]
    L.dsocr_ngram_window_check.argtypes = [C.POINTER(NgramWindowC), sz]
    L.dsocr_generate_ngram_window.argtypes = [vp, sz, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(ResultC),
                                              C.POINTER(C.POINTER(NgramWindowC)), C.POINTER(C.POINTER(PenaltiesC)),
                                              C.POINTER(C.POINTER(StopSetC)), C.POINTER(StopHitC),
                                              C.POINTER(C.POINTER(LogitBiasC)), sz, C.POINTER(LogprobsC)]
    L.dsocr_session_stage_ngram_window.argtypes = [vp, C.POINTER(NgramWindowC)]
    L.dsocr_k_ngram_window.argtypes = [i32, i32, i32, vp, vp, i32, vp, C.POINTER(C.POINTER(NgramWindowC)), i32]
    L.dsocr_guided_check.argtypes = [C.POINTER(GuidedC), i32, C.c_longlong]
    L.dsocr_generate_guided.argtypes = [vp, sz, C.POINTER(RequestC), C.POINTER(DecodeParamsC), C.POINTER(ResultC),
                                        C.POINTER(C.POINTER(GuidedC)), C.POINTER(GuidedResultC),
                                        C.POINTER(C.POINTER(NgramWindowC)), C.POINTER(C.POINTER(PenaltiesC)),
                                        C.POINTER(C.POINTER(StopSetC)), C.POINTER(StopHitC),
                                        C.POINTER(C.POINTER(LogitBiasC)), sz, C.POINTER(LogprobsC)]
    L.dsocr_session_stage_guided.argtypes = [vp, C.POINTER(GuidedC)]
    L.dsocr_session_guided_state.argtypes = [vp, i32, C.POINTER(GuidedResultC)]
    L.dsocr_k_guided_mask.argtypes = [i32, i32, i32, i32, vp, C.POINTER(GuidedC), C.c_longlong, vp, vp, vp, vp]
    L.dsocr_k_guided_advance.argtypes = [i32, i32, C.POINTER(GuidedC), vp, vp, vp, vp]
    _lib = L
    return L


def check(status: int):
    if status != OK:
        msg = lib().dsocr_last_error()
        raise DsocrError(status, msg.decode() if msg else "")
