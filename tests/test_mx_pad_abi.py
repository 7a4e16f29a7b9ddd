"""MX-emitting producers on zero-padded rows ("mxfp8" at d % 128 == 64) at the ABI and rule level.  No GPU needed.

The three entry points (mmdit_ln_modulate_fwd_mx_pad, mmdit_attn_fwd_mx_pad, mmdit_attn_fwd_e4m3_mx_pad) live in a header of their own,
include/mmdit_hip_mxpad.h, and in the binding's _MXPAD_SIGNATURES table: the versioned core ABI (58 entry points, MMDIT_ABI_VERSION 10) and the
other headers do not move.  The device code is the unpadded kernels' own (a template flag), so no source is added.  The engine's width rule
(engine.mx_fuse_width / mx_fuse_padded) follows ops.fp8_k_pad."""
import ctypes
import os
import re

import torch

NAMES = ["mmdit_attn_fwd_e4m3_mx_pad", "mmdit_attn_fwd_mx_pad", "mmdit_ln_modulate_fwd_mx_pad"]
FP8PAD_NAMES = ["mmdit_fp8_quantize_delayed_pad", "mmdit_fp8_quantize_pad", "mmdit_mxfp8_quantize_pad"]


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _prototype(txt, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"no prototype of {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype(arg, L):
    ty = arg.rsplit(" ", 1)[0].replace("const ", "")      # drop the parameter name
    if ty == "mmdit_ln_fwd_problem*":
        return ctypes.POINTER(L.LnFwdProblem)
    if ty.endswith("*") or ty == "mmdit_stream_t":
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64}[ty]


def test_declared_in_the_mxpad_header_only():
    L = _lib()
    assert L.declared_mxpad_symbols() == NAMES and set(L._MXPAD_SIGNATURES) == set(NAMES)
    tables = (L._SIGNATURES, L._EXT_SIGNATURES, L._HD128_SIGNATURES, L._ROPE3_SIGNATURES, L._QKHALF_SIGNATURES, L._TEXTLOSS_SIGNATURES, L._COS2_SIGNATURES,
              L._FP8PAD_SIGNATURES)
    for n in NAMES:
        for table in tables:
            assert n not in table
    for path in (L.HEADER_PATH, L.HEADER_EXT_PATH, L.HEADER_HD128_PATH, L.HEADER_ROPE3_PATH, L.HEADER_QKHALF_PATH, L.HEADER_TEXTLOSS_PATH, L.HEADER_COS2_PATH,
                 L.HEADER_FP8PAD_PATH):
        with open(path) as f:
            assert not re.search(r"mx_pad|mxpad", f.read()), path
    with open(L.HEADER_MXPAD_PATH) as f:
        txt = f.read()
    assert '#include "mmdit_hip.h"' in txt and "K_pad = (d + 127) / 128 * 128" in txt


def test_the_other_headers_do_not_move():
    L = _lib()
    assert len(L.declared_symbols()) == 58 and L.ABI_VERSION == 10 and set(L._SIGNATURES) == set(L.declared_symbols())
    with open(L.HEADER_PATH) as f:
        assert re.search(r"#define\s+MMDIT_ABI_VERSION\s+10\b", f.read())
    assert L.declared_ext_symbols() == ["mmdit_attn_fwd_e4m3"] and set(L._EXT_SIGNATURES) == {"mmdit_attn_fwd_e4m3"}
    assert L.declared_fp8pad_symbols() == FP8PAD_NAMES and set(L._FP8PAD_SIGNATURES) == set(FP8PAD_NAMES)


def test_signatures_equal_the_prototypes():
    L = _lib()
    with open(L.HEADER_MXPAD_PATH) as f:
        txt = f.read()
    with open(L.HEADER_PATH) as f:
        core = f.read()
    with open(L.HEADER_EXT_PATH) as f:
        ext = f.read()
    for n in NAMES:
        argtypes, restype = L._MXPAD_SIGNATURES[n]
        assert restype is ctypes.c_int and argtypes == [_ctype(a, L) for a in _prototype(txt, n)], n
    # the attention forms take the argument lists of their unpadded namesakes
    assert _prototype(txt, "mmdit_attn_fwd_mx_pad") == _prototype(core, "mmdit_attn_fwd_mx")
    strip = lambda args: [a.replace("Ox_fp8", "Ox").replace("Oc_fp8", "Oc") for a in args]      # noqa: E731
    assert strip(_prototype(txt, "mmdit_attn_fwd_e4m3_mx_pad")) == _prototype(ext, "mmdit_attn_fwd_e4m3")


def test_bound_and_exported():
    L = _lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        fn = getattr(L.lib(), n)
        assert fn.argtypes == L._MXPAD_SIGNATURES[n][0] and fn.restype is L._MXPAD_SIGNATURES[n][1]
    assert L.lib().mmdit_abi_version() == 10


def test_build_lists_the_header_and_the_device_code_is_shared():
    import importlib.util
    L = _lib()
    spec = importlib.util.spec_from_file_location("_mmdit_build_mxpad", os.path.join(os.path.dirname(L.LIB_PATH), "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert os.path.samefile(B.HEADER_MXPAD, L.HEADER_MXPAD_PATH)
    # no copy of a kernel: each entry point sits in the source of the kernel it launches, and that source has ONE definition of the kernel
    for src, kernel, entry in (("rowops.hip", "ln_mod_fwd_kernel", "mmdit_ln_modulate_fwd_mx_pad"), ("attention.hip", "attn_fwd_dma_kernel", "mmdit_attn_fwd_mx_pad"),
                               ("attention_e4m3.hip", "attn_fwd_e4m3_kernel", "mmdit_attn_fwd_e4m3_mx_pad")):
        assert src in B.SOURCES
        with open(os.path.join(B.CSRC, src)) as f:
            txt = f.read()
        assert "mmdit_hip_mxpad.h" in txt and len(re.findall(r'extern "C" int ' + entry + r"\(", txt)) == 1
        assert len(re.findall(r"__global__[^;{]*\bvoid " + kernel + r"\(", txt)) == 1, kernel


def test_the_width_rule_follows_fp8_k_pad():
    import sd3_amd  # noqa: F401
    from sd3_amd import engine, ops
    for d in (192, 320, 1216):
        assert engine.mx_fuse_width(d) and engine.mx_fuse_padded(d) and ops.fp8_k_pad(d) == d + 64
    assert engine.mx_fuse_width(256) and not engine.mx_fuse_padded(256)
    assert not engine.mx_fuse_width(96) and not engine.mx_fuse_padded(96)
    for d in range(32, 2049, 32):
        assert engine.mx_fuse_width(d) == (ops.fp8_k_pad(d) is not None) and engine.mx_fuse_padded(d) == (ops.fp8_k_pad(d) not in (None, d))


def test_to_fp8_takes_a_padded_mxact_as_it_is(monkeypatch):
    """engine._to_fp8 on the CPU with the quantiser replaced by a recorder: an MxAct that is already fp8_k_pad(K) wide is paired with the cached
    padded weight copy and no activation reaches ops.quant_mxfp8."""
    import sd3_amd  # noqa: F401
    from sd3_amd import engine, ops
    calls = []

    def quant(x, pad=False):
        calls.append((tuple(x.shape), pad))
        Kp = ops.fp8_k_pad(x.shape[1]) if pad else x.shape[1]
        return torch.zeros((x.shape[0], Kp), dtype=torch.float8_e4m3fn), torch.zeros(1, dtype=torch.uint8)

    monkeypatch.setattr(ops, "quant_mxfp8", quant)
    m = engine.Mode(True, fp8=True, mx=True)
    A = ops.MxAct(torch.zeros((5, 256), dtype=torch.float8_e4m3fn), torch.zeros(ops.mx_scale_bytes(5, 256), dtype=torch.uint8))
    B = torch.zeros((7, 192), dtype=torch.bfloat16)
    q = engine._to_fp8(m, dict(A=A, B=B, aux=None))
    assert q["A"] is A.q and q["scale_a"] is A.sc and q["B"].shape == (7, 256) and q["scale_mode"] == 1 and "aux" not in q
    assert calls == [((7, 192), True)]
    engine._to_fp8(m, dict(A=A, B=B))
    assert calls == [((7, 192), True)]      # the weight copy is cached, the activation never quantised
