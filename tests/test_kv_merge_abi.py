"""kv_merge_attn (reference: Attention.py:243-251) at the ABI and construction level.  No GPU needed.

The four entry points of the feature -- mmdit_attn_fwd_kv / mmdit_attn_bwd_kv (attention whose keys have a length of their own) and
mmdit_qk_norm_rope_fwd_merge / mmdit_qk_norm_rope_bwd_merge (QK-norm + RoPE with adjacent keys / values averaged) -- are declared
in include/mmdit_hip.h, bound with the prototypes' types and exported by the built library; the modules that used to raise for
kv_merge_attn=True construct, with the state-dict keys and the params record of the reference; the options that stay out of scope keep
raising."""
import ctypes
import json
import os
import re

import pytest
import torch

NAMES = ["mmdit_attn_fwd_kv", "mmdit_attn_bwd_kv", "mmdit_qk_norm_rope_fwd_merge", "mmdit_qk_norm_rope_bwd_merge"]
MICRO = dict(dim=128, num_heads=2, num_blocks=3)


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _prototype(txt, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"no prototype of {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_in_header():
    L = _lib()
    with open(L.HEADER_PATH) as f:
        txt = f.read()
    for name in NAMES:
        assert name in L.declared_symbols()
    assert _prototype(txt, "mmdit_attn_fwd_kv") == ["const void* Q", "const void* K", "const void* V", "int batch", "int heads", "int S", "int s_kv", "int n_img",
                                                    "float scale", "int mode", "void* Ox", "void* Oc", "float* lse", "mmdit_stream_t stream"]
    assert _prototype(txt, "mmdit_attn_bwd_kv") == ["const void* Q", "const void* K", "const void* V", "const void* Ox", "const void* Oc", "const void* dOx",
                                                    "const void* dOc", "const float* lse", "float* delta", "int batch", "int heads", "int S", "int s_kv", "int n_img",
                                                    "float scale", "void* dQ", "void* dK", "void* dV", "int dq_dtype", "mmdit_stream_t stream"]
    assert _prototype(txt, "mmdit_qk_norm_rope_fwd_merge") == _prototype(txt, "mmdit_qk_norm_rope_fwd")
    assert _prototype(txt, "mmdit_qk_norm_rope_bwd_merge") == _prototype(txt, "mmdit_qk_norm_rope_bwd")
    # every prototype of the header cites its call site in the reference
    assert txt.count("Attention.py:243-251") >= 2
    # the version the row operations' list entry points came with (mmdit_qk_problem is pinned by mmdit_struct_size)
    assert "#define MMDIT_ABI_VERSION 10" in txt and L.ABI_VERSION == 10
    # the plain entry points keep their signatures
    assert _prototype(txt, "mmdit_attn_fwd") == ["const void* Q", "const void* K", "const void* V", "int batch", "int heads", "int S", "int n_img",
                                                 "float scale", "int mode", "void* Ox", "void* Oc", "float* lse", "mmdit_stream_t stream"]


def test_bound_with_the_prototype_types():
    L = _lib()
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert L._SIGNATURES["mmdit_attn_fwd_kv"] == ([vp, vp, vp, i, i, i, i, i, f, i, vp, vp, vp, vp], i)
    assert L._SIGNATURES["mmdit_attn_bwd_kv"] == ([vp] * 9 + [i, i, i, i, i, f, vp, vp, vp, i, vp], i)
    assert L._SIGNATURES["mmdit_qk_norm_rope_fwd_merge"] == L._SIGNATURES["mmdit_qk_norm_rope_fwd"]
    assert L._SIGNATURES["mmdit_qk_norm_rope_bwd_merge"] == L._SIGNATURES["mmdit_qk_norm_rope_bwd"]


def test_exported_by_the_built_library():
    L = _lib()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(L.lib(), name).argtypes == L._SIGNATURES[name][0]
    assert L.lib().mmdit_struct_size(3) == ctypes.sizeof(L.QkProblem)


def test_ops_expose_the_feature():
    import inspect
    import sd3_amd  # noqa: F401
    from sd3_amd import ops
    assert "s_kv" in inspect.signature(ops.attn_fwd).parameters and "s_kv" in inspect.signature(ops.attn_bwd).parameters
    assert callable(ops.qk_norm_rope_fwd_merge_pair) and callable(ops.qk_norm_rope_bwd_merge_pair)


def test_attention_module_constructs_with_kv_merge():
    import sd3_amd  # noqa: F401
    from sd3_amd.blocks.Attention import Attention
    a = Attention(dim=128, num_heads=2, attn_type="softmax", positional_encoding="RoPE2d", dual=True, kv_merge_attn=True)
    assert a.kv_merge_attn is True
    b = Attention(dim=128, num_heads=2, attn_type="softmax", positional_encoding="RoPE2d", dual=True)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())       # the option adds no parameter


def _micro(**kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    return diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=torch.device("cpu"),
                      positional_encoding="RoPE2d", checkpoint_MLP=False, checkpoint_attn=False, **MICRO, **kw)


def test_micro_model_constructs_with_kv_merge(golden_dir):
    net = _micro(kv_merge_attn=True)
    with open(os.path.join(golden_dir, "state_dict_spec_micro_swiglu.json")) as f:
        spec = json.load(f)
    assert list(net.state_dict().keys()) == [k for k, _, _ in spec["state_dict"]]
    assert [n for n, _ in net.named_parameters()] == spec["named_parameters"]
    assert net.defaults["kv_merge_attn"] is True
    assert all(b.attn.kv_merge_attn is True for b in net.blocks)
    assert _micro().defaults["kv_merge_attn"] is False
    # the params record is written as given: JSON-serialisable and round-trips
    assert json.loads(json.dumps(net.defaults))["kv_merge_attn"] is True


def test_fp8_precisions_refuse_kv_merge():
    net = _micro(kv_merge_attn=True)
    for prec in ("fp8", "mxfp8"):
        with pytest.raises(RuntimeError, match="kv_merge_attn"):
            net.set_precision(prec)
    assert net.set_precision("parity").precision == "parity" and net.set_precision("fast").precision == "fast"
    assert _micro().set_precision("mxfp8").precision == "mxfp8"            # without the option the e4m3 modes stay selectable


def test_out_of_scope_options_still_raise():
    import sd3_amd  # noqa: F401
    from sd3_amd.blocks.Attention import Attention
    from sd3_amd.blocks.Transformer_Block_Dual import Transformer_Block_Dual
    ok = dict(dim=128, num_heads=2, attn_type="softmax", positional_encoding="RoPE2d", dual=True, kv_merge_attn=True)
    for bad in (dict(qk_half_dim=True), dict(causal=True), dict(attn_type="cosine"), dict(positional_encoding="RoPE"), dict(dual=False), dict(emb_dim=64)):
        with pytest.raises(RuntimeError):
            Attention(**{**ok, **bad})
    with pytest.raises(RuntimeError):
        Transformer_Block_Dual(128, 128, num_heads=2, attn_type="softmax", MLP_type="swiglu", positional_encoding="RoPE2d", kv_merge_attn=True, qk_half_dim=True)
    for bad in (dict(qk_half_dim=True), dict(text_loss=True)):
        with pytest.raises(RuntimeError):
            _micro(kv_merge_attn=True, **bad)
