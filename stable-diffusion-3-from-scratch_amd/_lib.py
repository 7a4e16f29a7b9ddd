"""ctypes binding of libmmdit_hip.so (C ABI: include/mmdit_hip.h).

There is no fallback: if the library is missing or a call fails, a RuntimeError is
raised.  The product path never routes through PyTorch math or the CPU oracle.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
def experiment(name: str, default: str) -> str:
    """A/B experiment switch (the fused-vs-unfused, schedule and layout switches listed in tools/README.md).  They are read ONLY when
    MMDIT_EXPERIMENTS=1 is set: the product has one path per operation, the switches exist for same-box A/B measurements."""
    return os.environ.get(name, default) if os.environ.get("MMDIT_EXPERIMENTS") == "1" else default


LIB_PATH = os.environ.get("MMDIT_LIB") or os.path.join(_HERE, "libmmdit_hip.so")   # MMDIT_LIB: A/B a scratch build
HEADER_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip.h")
HEADER_EXT_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip_ext.h")   # opt-in entry points outside the versioned core ABI
HEADER_HD128_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip_hd128.h")   # the head-width-128 entry points, outside it as well
HEADER_ROPE3_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip_rope3.h")   # the RoPE2dV2 entry points, outside it as well
HEADER_QKHALF_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip_qkhalf.h")   # the qk_half_dim entry points, outside it as well
HEADER_TEXTLOSS_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip_textloss.h")   # the text_loss entry point, outside it as well
HEADER_COS2_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip_cos2.h")   # the attn_type="cosine2" entry points, outside it as well
HEADER_FP8PAD_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip_fp8pad.h")   # the zero-padded e4m3 quantisers, outside it as well
HEADER_MXPAD_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip_mxpad.h")   # the MX producers on zero-padded rows, outside it as well
HEADER_OPTIM_PATH = os.path.join(_HERE, "..", "include", "mmdit_hip_optim.h")   # the AdamW update with per-tensor step counters, outside it as well

F32, BF16 = 0, 1
ACT_NONE, ACT_SILU, ACT_SWIGLU, ACT_SWIGLU_BWD = 0, 1, 2, 3
PREC_BF16, PREC_SPLIT = 0, 1
FP8 = 2   # dtype code of OCP e4m3 GEMM operands (stored in torch.uint8 / float8_e4m3fn tensors)

_vp, _i, _i64, _f, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double


class GemmArgs(ctypes.Structure):
    _fields_ = [
        ("A", _vp), ("a_dtype", _i), ("a_kmajor", _i), ("lda", _i64),
        ("B", _vp), ("b_dtype", _i), ("b_kmajor", _i), ("ldb", _i64),
        ("C", _vp), ("c_dtype", _i), ("ldc", _i64),
        ("M", _i), ("N", _i), ("K", _i),
        ("bias", _vp),
        ("act", _i),
        ("gate", _vp), ("ld_gate", _i64), ("rows_per_batch", _i),
        ("residual", _vp), ("ld_res", _i64),
        ("aux", _vp), ("aux_dtype", _i), ("ld_aux", _i64),
        ("accumulate", _i),
        ("precision", _i),
        ("split_k", _i),
        ("stream_k", _i),
        ("conv_mode", _i), ("conv_H", _i), ("conv_W", _i), ("conv_C", _i),
        ("scale_a", _vp), ("scale_b", _vp), ("scale_mode", _i), ("c_scales", _vp),
        ("dbias", _vp),
        ("cu_budget", _i),
    ]


# argument types of every entry point, in header order
class LnFwdProblem(ctypes.Structure):      # mirrors mmdit_ln_fwd_problem (include/mmdit_hip.h)
    _fields_ = [("x", ctypes.c_void_p), ("acc", ctypes.c_void_p), ("gate", ctypes.c_void_p), ("ld_gate", ctypes.c_int64), ("x_out", ctypes.c_void_p),
                ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("ld_mod", ctypes.c_int64), ("rows", ctypes.c_int), ("rows_per_batch", ctypes.c_int),
                ("out", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("rstd", ctypes.c_void_p)]


class LnBwdProblem(ctypes.Structure):      # mirrors mmdit_ln_bwd_problem
    _fields_ = [("dout", ctypes.c_void_p), ("x", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("rstd", ctypes.c_void_p), ("scale", ctypes.c_void_p),
                ("ld_mod", ctypes.c_int64), ("dres", ctypes.c_void_p), ("rows", ctypes.c_int), ("rows_per_batch", ctypes.c_int),
                ("dx", ctypes.c_void_p), ("dscale", ctypes.c_void_p), ("dshift", ctypes.c_void_p), ("ld_dmod", ctypes.c_int64),
                ("acc", ctypes.c_void_p), ("gate", ctypes.c_void_p), ("ld_gate", ctypes.c_int64), ("dacc", ctypes.c_void_p), ("dgate", ctypes.c_void_p),
                ("ld_dgate", ctypes.c_int64), ("dbias", ctypes.c_void_p), ("ld_dbias", ctypes.c_int64)]


class QkProblem(ctypes.Structure):        # mirrors mmdit_qk_problem
    _fields_ = [("qkv", ctypes.c_void_p), ("wq", ctypes.c_void_p), ("wk", ctypes.c_void_p), ("rope_cos", ctypes.c_void_p), ("rope_sin", ctypes.c_void_p),
                ("tokens", ctypes.c_int), ("tok0", ctypes.c_int), ("dqkv", ctypes.c_void_p), ("dwq", ctypes.c_void_p), ("dwk", ctypes.c_void_p)]


class MlpBwdProblem(ctypes.Structure):     # mirrors mmdit_mlp_bwd_problem
    _fields_ = [("dh", ctypes.c_void_p), ("gu", ctypes.c_void_p), ("dgu", ctypes.c_void_p), ("rows", ctypes.c_int), ("dbias", ctypes.c_void_p)]


class QkEpilogue(ctypes.Structure):
    """mmdit_qk_epilogue"""
    _fields_ = [("wq", _vp), ("wk", _vp), ("rope_cos", _vp), ("rope_sin", _vp), ("tokens", _i), ("tok0", _i)]


_SIGNATURES = {
    "mmdit_abi_version": ([], _i),
    "mmdit_struct_size": ([_i], _i),
    "mmdit_build_arch": ([], ctypes.c_char_p),
    "mmdit_gemm": ([ctypes.POINTER(GemmArgs), _vp], _i),
    "mmdit_gemm_grouped": ([ctypes.POINTER(GemmArgs), _i, _vp], _i),
    "mmdit_gemm_plan": ([ctypes.POINTER(GemmArgs), _i], _i),
    "mmdit_gemm_set_workspace": ([_vp, ctypes.c_longlong], _i),
    "mmdit_debug_occupy": ([_i, ctypes.c_longlong, _vp], _i),
    "mmdit_gemm_set_claiming": ([_i], _i),
    "mmdit_gemm_get_claiming": ([], _i),
    "mmdit_device_cus": ([], _i),
    "mmdit_gemm_qkv_norm_rope": ([ctypes.POINTER(GemmArgs), ctypes.POINTER(QkEpilogue), _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "mmdit_gemm_zero_mask": ([ctypes.POINTER(GemmArgs), _i, ctypes.POINTER(ctypes.c_uint)], _i),
    "mmdit_fp8_amax": ([_vp, _i, _i64, _vp, _vp], _i),
    "mmdit_fp8_quantize": ([_vp, _i, _i64, _vp, _vp, _vp, _vp], _i),
    "mmdit_fp8_quantize_delayed": ([_vp, _i, _i64, _vp, _i, ctypes.c_float, _vp, _vp], _i),
    "mmdit_mxfp8_quantize": ([_vp, _i, _i, _i, _i64, _vp, _vp, _vp], _i),
    "mmdit_ln_modulate_fwd_mx": ([_vp, _vp, _i, _vp, _i64, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "mmdit_swiglu_fwd_mx": ([_vp, _i, _i, _i, _vp, _vp, _vp], _i),
    "mmdit_attn_fwd_mx": ([_vp, _vp, _vp, _i, _i, _i, _i, ctypes.c_float, _vp, _vp, _vp, _vp, _vp], _i),
    "mmdit_cast": ([_vp, _i, _vp, _i, _i64, _vp], _i),
    # the row operations that take a list (array pointer, count = 1 or 2) of problem structs
    "mmdit_ln_modulate_fwd": ([ctypes.POINTER(LnFwdProblem), _i, _i, _i, _i, _vp], _i),
    "mmdit_ln_modulate_bwd": ([ctypes.POINTER(LnBwdProblem), _i, _i, _i, _vp], _i),
    "mmdit_qk_norm_rope_fwd": ([ctypes.POINTER(QkProblem), _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "mmdit_qk_norm_rope_bwd": ([ctypes.POINTER(QkProblem), _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mmdit_qk_norm_rope_fwd_merge": ([ctypes.POINTER(QkProblem), _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "mmdit_qk_norm_rope_bwd_merge": ([ctypes.POINTER(QkProblem), _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mmdit_mlp_act_bwd": ([ctypes.POINTER(MlpBwdProblem), _i, _i, _i, _i, _vp], _i),
    "mmdit_gate_residual_fwd": ([_vp, _vp, _i, _vp, _i64, _i, _i, _i, _vp, _vp], _i),
    "mmdit_text_rmsnorm_fwd": ([_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp], _i),
    "mmdit_text_rmsnorm_bwd": ([_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "mmdit_attn_fwd": ([_vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp], _i),
    "mmdit_attn_bwd_qk": ([_vp] * 9 + [_i, _i, _i, _i, _f] + [_vp] * 11 + [_vp], _i),
    "mmdit_attn_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp], _i),
    "mmdit_attn_fwd_kv": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp], _i),
    "mmdit_attn_bwd_kv": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp], _i),
    "mmdit_swiglu_fwd": ([_vp, _vp, _i, _i, _i, _vp], _i),
    "mmdit_gelu_fwd": ([_vp, _vp, _i, _i, _i, _vp], _i),
    "mmdit_silu_bwd": ([_vp, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp], _i),
    "mmdit_gate_residual_bwd": ([_vp, _vp, _i, _vp, _i64, _i, _i, _i, _vp, _i, _vp, _i64, _vp, _i64, _vp], _i),
    "mmdit_flow_loss": ([_vp, _vp, _vp, _i, _i64, _f, _vp, _vp, _vp, _vp], _i),
    "mmdit_colsum": ([_vp, _i, _i, _i, _i64, _vp, _vp], _i),
    "mmdit_vae_nchw_to_nhwc": ([_vp, _i, _i, _i, _i, _i, _i, ctypes.c_float, ctypes.c_float, _vp, _vp], _i),
    "mmdit_vae_nhwc_to_nchw": ([_vp, _i, _i, _i, _i, _i, ctypes.c_float, ctypes.c_float, _vp, _vp], _i),
    "mmdit_vae_im2col3x3": ([_vp, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "mmdit_vae_groupnorm": ([_vp, _i, _vp, _vp, _i, _i, _i, _i, _i, ctypes.c_float, _i, _vp, _vp, _i, _vp], _i),
    "mmdit_vae_pad_cast": ([_vp, _i, _i, _i, _i, _i, _i, _vp, _vp], _i),
    "mmdit_vae_softmax_rows": ([_vp, _i, _i, _i, ctypes.c_float, _vp, _vp], _i),
    "mmdit_vae_attn_fwd": ([_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp], _i),
    "mmdit_patchify": ([_vp, _i, _i, _i, _i, _i, _vp, _i, _vp], _i),
    "mmdit_unpatchify": ([_vp, _i, _i, _i, _i, _i, _vp, _i, _vp], _i),
    "mmdit_time_embed_fwd": ([_vp, _vp, _vp, _i, _i, _vp, _i, _vp], _i),
    "mmdit_time_embed_bwd": ([_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp], _i),
    "mmdit_grad_sumsq": ([_vp, _vp, _vp, _i, _vp, _vp], _i),
    "mmdit_clip_coef": ([_vp, _i, _vp, _f, _vp, _vp], _i),
    "mmdit_adamw_step": ([_vp, _vp, _vp, _i, _vp, _vp, _d, _d, _d, _d, _d, _vp], _i),
    "mmdit_adamw_step_dlr": ([_vp, _vp, _vp, _i, _vp, _vp, _vp, _d, _d, _d, _d, _vp], _i),
    "mmdit_cast_multi": ([_vp, _vp, _vp, _i, _vp], _i),
}
# entry points of include/mmdit_hip_ext.h: bound like the core table, not counted by MMDIT_ABI_VERSION
_EXT_SIGNATURES = {
    "mmdit_attn_fwd_e4m3": ([_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp], _i),
}
ATTN_E4M3_KEY_TILE, ATTN_E4M3_QUERY_TILE = 64, 128   # MMDIT_ATTN_E4M3_KEY_TILE / MMDIT_ATTN_E4M3_QUERY_TILE
# entry points of include/mmdit_hip_hd128.h: the argument lists of their 64-wide namesakes in the core table
_HD128_SIGNATURES = {
    "mmdit_attn_fwd_hd128": _SIGNATURES["mmdit_attn_fwd"],
    "mmdit_attn_bwd_hd128": _SIGNATURES["mmdit_attn_bwd"],
    "mmdit_qk_norm_rope_fwd_hd128": _SIGNATURES["mmdit_qk_norm_rope_fwd"],
    "mmdit_qk_norm_rope_bwd_hd128": _SIGNATURES["mmdit_qk_norm_rope_bwd"],
}
ATTN_HD128_KEY_TILE, ATTN_HD128_QUERY_TILE = 32, 128   # MMDIT_ATTN_HD128_KEY_TILE / MMDIT_ATTN_HD128_QUERY_TILE
QK_HD128_MAX_HEADS, QK_HD128_RL_MIN_ROWS = 21, 2048    # MMDIT_QK_HD128_MAX_HEADS / MMDIT_QK_HD128_RL_MIN_ROWS
# entry points of include/mmdit_hip_rope3.h (positional_encoding="RoPE2dV2"): the argument lists of the plain QK-norm / RoPE launches with
# head_dim after heads
_ROPE3_SIGNATURES = {
    "mmdit_qk_norm_rope3_fwd": ([ctypes.POINTER(QkProblem), _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "mmdit_qk_norm_rope3_bwd": ([ctypes.POINTER(QkProblem), _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
}
# entry points of include/mmdit_hip_qkhalf.h (qk_half_dim=True: 32-wide queries / keys, 64-wide values): the attention launches take the
# argument lists of their core namesakes, the QK-norm / RoPE launches those of the plain ones with (qk_dim, v_dim) after heads
_QKHALF_SIGNATURES = {
    "mmdit_attn_fwd_qkhalf": _SIGNATURES["mmdit_attn_fwd"],
    "mmdit_attn_bwd_qkhalf": _SIGNATURES["mmdit_attn_bwd"],
    "mmdit_qk_norm_rope_fwd_qkhalf": ([ctypes.POINTER(QkProblem), _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "mmdit_qk_norm_rope_bwd_qkhalf": ([ctypes.POINTER(QkProblem), _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
}
QKHALF_QK_DIM, QKHALF_V_DIM = 32, 64                   # MMDIT_QKHALF_QK_DIM / MMDIT_QKHALF_V_DIM
ATTN_QKHALF_KEY_TILE, ATTN_QKHALF_QUERY_TILE = 32, 128   # MMDIT_ATTN_QKHALF_KEY_TILE / MMDIT_ATTN_QKHALF_QUERY_TILE
# entry point of include/mmdit_hip_textloss.h (text_loss=True: the masked text-reconstruction loss of the training step)
_TEXTLOSS_SIGNATURES = {
    "mmdit_text_loss": ([_vp, _i, _vp, _i, _vp, _i64, _i, _f, _vp, _i, _vp, _vp, _vp], _i),
}
TEXT_LOSS_ROWS_PER_WG, TEXT_LOSS_MAX_PARTIALS = 4, 256   # MMDIT_TEXT_LOSS_ROWS_PER_WG / MMDIT_TEXT_LOSS_MAX_PARTIALS
TEXT_LOSS_LANE_COLS, TEXT_LOSS_WAVE_COLS = 8, 512        # MMDIT_TEXT_LOSS_LANE_COLS / MMDIT_TEXT_LOSS_WAVE_COLS
# entry points of include/mmdit_hip_cos2.h (attn_type="cosine2": L2-normalised queries / keys, linear-time attention through a 64 x 64 state)
_COS2_SIGNATURES = {
    "mmdit_qk_l2norm_rope_fwd": ([ctypes.POINTER(QkProblem), _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "mmdit_qk_l2norm_rope_bwd": ([ctypes.POINTER(QkProblem), _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mmdit_attn_cos2_ws_bytes": ([_i, _i, _i], ctypes.c_longlong),
    "mmdit_attn_cos2_fwd": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp], _i),
    "mmdit_attn_cos2_bwd": ([_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp], _i),
}
# entry points of include/mmdit_hip_fp8pad.h (fp8 / mxfp8 inference at K % 128 == 64: e4m3 codes in rows zero-padded to the 128-wide K tile)
_FP8PAD_SIGNATURES = {
    "mmdit_fp8_quantize_pad": ([_vp, _i, _i, _i, _i64, _vp, _vp, _vp, _vp], _i),
    "mmdit_fp8_quantize_delayed_pad": ([_vp, _i, _i, _i, _i64, _vp, _i, ctypes.c_float, _vp, _vp], _i),
    "mmdit_mxfp8_quantize_pad": ([_vp, _i, _i, _i, _i64, _vp, _vp, _vp], _i),
}
# entry points of include/mmdit_hip_mxpad.h ("mxfp8" inference at d % 128 == 64: the MX-emitting adaLN / attention kernels writing rows zero-padded
# to the 128-wide K tile); the attention forms take the argument lists of their unpadded namesakes
_MXPAD_SIGNATURES = {
    "mmdit_ln_modulate_fwd_mx_pad": ([ctypes.POINTER(LnFwdProblem), _i, _i, _i, _vp, _vp, _vp], _i),
    "mmdit_attn_fwd_mx_pad": _SIGNATURES["mmdit_attn_fwd_mx"],
    "mmdit_attn_fwd_e4m3_mx_pad": _EXT_SIGNATURES["mmdit_attn_fwd_e4m3"],
}
# entry points of include/mmdit_hip_optim.h (the AdamW update reading one step counter per tensor; otherwise the argument list of mmdit_adamw_step_dlr)
_OPTIM_SIGNATURES = {
    "mmdit_adamw_step_dlr_pt": _SIGNATURES["mmdit_adamw_step_dlr"],
}
COS2_HEAD_DIM = 64                                     # MMDIT_COS2_HEAD_DIM
ATTN_COS2_TOKEN_CHUNK, ATTN_COS2_ROW_TILE = 128, 64    # MMDIT_ATTN_COS2_TOKEN_CHUNK / MMDIT_ATTN_COS2_ROW_TILE
HEAD_DIMS = (64, 128)                                  # head widths the attention and QK-norm / RoPE kernels are built for
ADAMW_CHUNK = 65536   # MMDIT_ADAMW_CHUNK
ABI_VERSION = 10      # MMDIT_ABI_VERSION of include/mmdit_hip.h this binding mirrors
# struct ids of mmdit_struct_size() -> ctypes mirrors (None: laid out with numpy record dtypes in optim.py / ops.py: 48 / 24 bytes)
_STRUCTS = [("mmdit_gemm_args", GemmArgs), ("mmdit_ln_fwd_problem", LnFwdProblem), ("mmdit_ln_bwd_problem", LnBwdProblem),
            ("mmdit_qk_problem", QkProblem), ("mmdit_mlp_bwd_problem", MlpBwdProblem), ("mmdit_adamw_tensor", None), ("mmdit_cast_tensor", None), ("mmdit_qk_epilogue", QkEpilogue)]

_lib = None


def declared_symbols():
    """Entry points declared by include/mmdit_hip.h (parsed from the header text)."""
    with open(HEADER_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def declared_ext_symbols():
    """Entry points declared by include/mmdit_hip_ext.h (parsed the same way)."""
    with open(HEADER_EXT_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def declared_hd128_symbols():
    """Entry points declared by include/mmdit_hip_hd128.h (parsed the same way)."""
    with open(HEADER_HD128_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def declared_rope3_symbols():
    """Entry points declared by include/mmdit_hip_rope3.h (parsed the same way)."""
    with open(HEADER_ROPE3_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def declared_qkhalf_symbols():
    """Entry points declared by include/mmdit_hip_qkhalf.h (parsed the same way)."""
    with open(HEADER_QKHALF_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def declared_textloss_symbols():
    """Entry points declared by include/mmdit_hip_textloss.h (parsed the same way)."""
    with open(HEADER_TEXTLOSS_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def declared_cos2_symbols():
    """Entry points declared by include/mmdit_hip_cos2.h (parsed the same way)."""
    with open(HEADER_COS2_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def declared_fp8pad_symbols():
    """Entry points declared by include/mmdit_hip_fp8pad.h (parsed the same way)."""
    with open(HEADER_FP8PAD_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def declared_mxpad_symbols():
    """Entry points declared by include/mmdit_hip_mxpad.h (parsed the same way)."""
    with open(HEADER_MXPAD_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def declared_optim_symbols():
    """Entry points declared by include/mmdit_hip_optim.h (parsed the same way)."""
    with open(HEADER_OPTIM_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(mmdit_[a-z0-9_]+)\s*\(", txt)) - {"mmdit_stream_t"})


def lib():
    """Load the HIP library (once).  Raises RuntimeError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950).  There is no PyTorch/CPU fallback for the MMDiT hot path.")
        try:
            # The library must share PyTorch's HIP runtime instance and device context: initialise torch's first when a GPU
            # is present (loading this library before torch has touched the GPU left its launches with hipErrorNoDevice).
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in (list(_SIGNATURES.items()) + list(_EXT_SIGNATURES.items()) + list(_HD128_SIGNATURES.items()) + list(_ROPE3_SIGNATURES.items())
                                          + list(_QKHALF_SIGNATURES.items()) + list(_TEXTLOSS_SIGNATURES.items()) + list(_COS2_SIGNATURES.items()) + list(_FP8PAD_SIGNATURES.items()) + list(_MXPAD_SIGNATURES.items())
                                          + list(_OPTIM_SIGNATURES.items())):
            fn = getattr(L, name)  # AttributeError -> symbol missing: fail loudly
            fn.argtypes = argtypes
            fn.restype = restype
        # a library built for another ABI (a stale scratch build behind MMDIT_LIB, an old .so next to a new binding) must not be called
        if L.mmdit_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH}: ABI version {L.mmdit_abi_version()}, this binding is written for {ABI_VERSION}: rebuild (python __graft_entry__.py build)")
        for which, (name, struct) in enumerate(_STRUCTS):
            if struct is not None and L.mmdit_struct_size(which) != ctypes.sizeof(struct):
                raise RuntimeError(f"{LIB_PATH}: sizeof({name}) = {L.mmdit_struct_size(which)}, the binding's ctypes mirror has {ctypes.sizeof(struct)} bytes")
        _lib = L
    return _lib


ERR_ARG, ERR_DTYPE, ERR_SHAPE = -1, -2, -3      # MMDIT_ERR_* of include/mmdit_hip.h


def check(status: int, what: str):
    if status != 0:
        kind = {-1: "invalid argument", -2: "dtype combination not built", -3: "unsupported shape"}.get(status, f"hipError {status}")
        raise RuntimeError(f"{what} failed: {kind}")
