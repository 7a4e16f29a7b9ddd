"""Opt-in e4m3 attention (mmdit_attn_fwd_e4m3, reference call site Attention.py:266-293) at the ABI and construction level.  No GPU needed.

The entry point lives in the extension header include/mmdit_hip_ext.h and in the binding's _EXT_SIGNATURES table: the versioned core ABI
(include/mmdit_hip.h: 58 entry points, MMDIT_ABI_VERSION 10, _SIGNATURES) does not move.  set_precision(..., attention="e4m3") is accepted
with the two e4m3 inference modes only, and the kv_merge_attn refusal is unchanged."""
import ctypes
import inspect
import re

import pytest
import torch

NAME = "mmdit_attn_fwd_e4m3"
MICRO = dict(dim=128, num_heads=2, num_blocks=3)


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _micro(**kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    return diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=torch.device("cpu"),
                      positional_encoding="RoPE2d", checkpoint_MLP=False, checkpoint_attn=False, **MICRO, **kw)


def test_declared_in_the_extension_header_only():
    L = _lib()
    assert L.declared_ext_symbols() == [NAME]
    assert NAME not in L.declared_symbols()
    assert len(L.declared_symbols()) == 58 and L.ABI_VERSION == 10
    assert NAME not in L._SIGNATURES and set(L._SIGNATURES) == set(L.declared_symbols())
    with open(L.HEADER_EXT_PATH) as f:
        txt = f.read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, "no prototype"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "const void* Q", "const void* K", "const void* V", "int batch", "int heads", "int S", "int n_img", "float scale",
        "void* Ox", "void* Oc", "void* scales_x", "void* scales_c", "mmdit_stream_t stream"]
    assert '#include "mmdit_hip.h"' in txt
    assert "Attention.py:266-293" in txt                  # the prototype cites its call site in the reference
    # the tile edges the GPU tests are built around are the header's
    assert f"#define MMDIT_ATTN_E4M3_KEY_TILE {L.ATTN_E4M3_KEY_TILE}\n" in txt and f"#define MMDIT_ATTN_E4M3_QUERY_TILE {L.ATTN_E4M3_QUERY_TILE}\n" in txt


def test_bound_and_exported():
    L = _lib()
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert L._EXT_SIGNATURES[NAME] == ([vp, vp, vp, i, i, i, i, f, vp, vp, vp, vp, vp], i)
    assert hasattr(ctypes.CDLL(L.LIB_PATH), NAME)
    fn = getattr(L.lib(), NAME)
    assert fn.argtypes == L._EXT_SIGNATURES[NAME][0] and fn.restype is i
    assert L.lib().mmdit_abi_version() == 10


def test_ops_expose_the_feature():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops
    assert list(inspect.signature(ops.attn_fwd_e4m3).parameters) == ["Q", "K", "V", "n_img", "scale", "mx"]
    assert inspect.signature(ops.attn_fwd_e4m3).parameters["mx"].default is False


def test_set_precision_keyword():
    import sd3_amd  # noqa: F401
    from sd3_amd import engine
    net = _micro()
    assert engine.FP8.attn_e4m3 is False and engine.MXFP8.attn_e4m3 is False and engine.FAST.attn_e4m3 is False
    assert net.set_precision("mxfp8", attention="e4m3").precision == "mxfp8"
    assert engine.MXFP8.attn_e4m3 is True and engine.FP8.attn_e4m3 is False
    assert net.set_precision("fp8", attention="e4m3").precision == "fp8"
    assert engine.FP8.attn_e4m3 is True and engine.MXFP8.attn_e4m3 is False
    for prec in ("fast", "parity"):
        with pytest.raises(ValueError):
            net.set_precision(prec, attention="e4m3")
    with pytest.raises(ValueError):
        net.set_precision("fp8", attention="fp4")
    assert net.precision == "fp8"                              # a refused call changes nothing
    net.set_precision("mxfp8")
    assert engine.MXFP8.attn_e4m3 is False and engine.FP8.attn_e4m3 is False       # without the keyword the flag is off
    net.set_precision("mxfp8", attention="e4m3")
    net.set_precision("fast")
    assert engine.MXFP8.attn_e4m3 is False and engine.FP8.attn_e4m3 is False       # "fast" resets it
    assert inspect.signature(net.set_precision).parameters["attention"].default == "bf16"


def test_kv_merge_still_refused():
    net = _micro(kv_merge_attn=True)
    for prec in ("fp8", "mxfp8"):
        for kw in ({}, dict(attention="e4m3")):
            with pytest.raises(RuntimeError, match="kv_merge_attn"):
                net.set_precision(prec, **kw)
    assert net.set_precision("fast").precision == "fast"
