"""Zero-padded e4m3 quantisers (fp8 / mxfp8 inference at K % 128 == 64) at the ABI and rule level.  No GPU needed.

The three entry points (mmdit_fp8_quantize_pad, mmdit_fp8_quantize_delayed_pad, mmdit_mxfp8_quantize_pad) live in a header of their own,
include/mmdit_hip_fp8pad.h, and in the binding's _FP8PAD_SIGNATURES table: the versioned core ABI (58 entry points, MMDIT_ABI_VERSION 10) and
the six other headers do not move.  ops.fp8_k_pad is the one place the padding rule lives; engine._to_fp8 refuses by it."""
import ctypes
import os
import re

import torch

NAMES = ["mmdit_fp8_quantize_delayed_pad", "mmdit_fp8_quantize_pad", "mmdit_mxfp8_quantize_pad"]
COS2_NAMES = ["mmdit_attn_cos2_bwd", "mmdit_attn_cos2_fwd", "mmdit_attn_cos2_ws_bytes", "mmdit_qk_l2norm_rope_bwd", "mmdit_qk_l2norm_rope_fwd"]
HD128_NAMES = ["mmdit_attn_bwd_hd128", "mmdit_attn_fwd_hd128", "mmdit_qk_norm_rope_bwd_hd128", "mmdit_qk_norm_rope_fwd_hd128"]
ROPE3_NAMES = ["mmdit_qk_norm_rope3_bwd", "mmdit_qk_norm_rope3_fwd"]
QKHALF_NAMES = ["mmdit_attn_bwd_qkhalf", "mmdit_attn_fwd_qkhalf", "mmdit_qk_norm_rope_bwd_qkhalf", "mmdit_qk_norm_rope_fwd_qkhalf"]


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _prototype(txt, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"no prototype of {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype(arg):
    ty = arg.rsplit(" ", 1)[0].replace("const ", "")      # drop the parameter name
    if ty.endswith("*") or ty == "mmdit_stream_t":
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64}[ty]


def test_declared_in_the_fp8pad_header_only():
    L = _lib()
    assert L.declared_fp8pad_symbols() == NAMES and set(L._FP8PAD_SIGNATURES) == set(NAMES)
    for n in NAMES:
        for table in (L._SIGNATURES, L._EXT_SIGNATURES, L._HD128_SIGNATURES, L._ROPE3_SIGNATURES, L._QKHALF_SIGNATURES, L._TEXTLOSS_SIGNATURES, L._COS2_SIGNATURES):
            assert n not in table
    for path in (L.HEADER_PATH, L.HEADER_EXT_PATH, L.HEADER_HD128_PATH, L.HEADER_ROPE3_PATH, L.HEADER_QKHALF_PATH, L.HEADER_TEXTLOSS_PATH, L.HEADER_COS2_PATH):
        with open(path) as f:
            assert not re.search(r"quantize\w*_pad|fp8pad", f.read()), path
    with open(L.HEADER_FP8PAD_PATH) as f:
        txt = f.read()
    assert '#include "mmdit_hip.h"' in txt and "K_pad = (K + 127) / 128 * 128" in txt


def test_the_other_headers_do_not_move():
    L = _lib()
    assert len(L.declared_symbols()) == 58 and L.ABI_VERSION == 10 and set(L._SIGNATURES) == set(L.declared_symbols())
    with open(L.HEADER_PATH) as f:
        assert re.search(r"#define\s+MMDIT_ABI_VERSION\s+10\b", f.read())
    assert L.declared_ext_symbols() == ["mmdit_attn_fwd_e4m3"] and set(L._EXT_SIGNATURES) == {"mmdit_attn_fwd_e4m3"}
    assert L.declared_hd128_symbols() == HD128_NAMES and set(L._HD128_SIGNATURES) == set(HD128_NAMES)
    assert L.declared_rope3_symbols() == ROPE3_NAMES and set(L._ROPE3_SIGNATURES) == set(ROPE3_NAMES)
    assert L.declared_qkhalf_symbols() == QKHALF_NAMES and set(L._QKHALF_SIGNATURES) == set(QKHALF_NAMES)
    assert L.declared_textloss_symbols() == ["mmdit_text_loss"] and set(L._TEXTLOSS_SIGNATURES) == {"mmdit_text_loss"}
    assert L.declared_cos2_symbols() == COS2_NAMES and set(L._COS2_SIGNATURES) == set(COS2_NAMES)


def test_signatures_equal_the_prototypes():
    L = _lib()
    with open(L.HEADER_FP8PAD_PATH) as f:
        txt = f.read()
    with open(L.HEADER_PATH) as f:
        core = f.read()
    for n in NAMES:
        argtypes, restype = L._FP8PAD_SIGNATURES[n]
        assert restype is ctypes.c_int and argtypes == [_ctype(a) for a in _prototype(txt, n)], n
    # the argument lists: the plain quantisers' with (rows, K, ldx) in the place of the element count n (the MX form: the plain one's own)
    names = lambda args: [a.rsplit(" ", 1)[1].lstrip("*") for a in args]      # noqa: E731
    geometry = ["rows", "K", "ldx"]
    for padded, plain in (("mmdit_fp8_quantize_pad", "mmdit_fp8_quantize"), ("mmdit_fp8_quantize_delayed_pad", "mmdit_fp8_quantize_delayed")):
        want = names(_prototype(core, plain))
        at = want.index("n")
        assert names(_prototype(txt, padded)) == want[:at] + geometry + want[at + 1:], padded
    assert _prototype(txt, "mmdit_mxfp8_quantize_pad") == _prototype(core, "mmdit_mxfp8_quantize")


def test_bound_and_exported():
    L = _lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        fn = getattr(L.lib(), n)
        assert fn.argtypes == L._FP8PAD_SIGNATURES[n][0] and fn.restype is L._FP8PAD_SIGNATURES[n][1]
    assert L.lib().mmdit_abi_version() == 10


def test_build_lists_the_source_and_the_header_and_the_device_code_is_shared():
    import importlib.util
    L = _lib()
    spec = importlib.util.spec_from_file_location("_mmdit_build_fp8pad", os.path.join(os.path.dirname(L.LIB_PATH), "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert "fp8_pad.hip" in B.SOURCES and os.path.samefile(B.HEADER_FP8PAD, L.HEADER_FP8PAD_PATH)
    with open(os.path.join(B.CSRC, "fp8_pad.hip")) as f:
        padded = f.read()
    with open(os.path.join(B.CSRC, "rowops.hip")) as f:
        plain = f.read()
    # one spelling of the arithmetic: both sources include the device header, neither calls the e4m3 converter itself
    for txt in (padded, plain):
        assert '#include "fp8_quant.h"' in txt and "cvt_pk_fp8" not in txt
    assert "mmdit_hip_fp8pad.h" in padded


def test_fp8_k_pad_is_the_rule():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops
    assert (ops.fp8_k_pad(64), ops.fp8_k_pad(192), ops.fp8_k_pad(1216)) == (128, 256, 1280)
    for K in (128, 768, 4864):
        assert ops.fp8_k_pad(K) == K
    for K in (96, 72, 1, 0, 1217):
        assert ops.fp8_k_pad(K) is None
    for heads in range(1, 40):      # dim = 64 * heads with the default hidden_scale: every K of the four sites is eligible
        d = 64 * heads
        assert ops.fp8_k_pad(d) == (d + 127) // 128 * 128 and ops.fp8_k_pad(4 * d) == 4 * d
    assert ops.mx_scale_bytes(300, ops.fp8_k_pad(192)) == (256 // 64) * 384 * 2 + 512


def test_the_engine_refuses_by_the_rule_only(monkeypatch):
    """engine._to_fp8 on the CPU with the quantisers replaced by recorders: K = 192 is handed to the padding quantisers (pad=True) for the
    activation and the cached weight, K = 96 stays bf16, and the weight cache stays keyed on id(B) and the pack generation."""
    import sd3_amd  # noqa: F401
    from sd3_amd import engine, ops
    calls = []

    def quant(x, pad=False):
        calls.append((tuple(x.shape), pad))
        Kp = ops.fp8_k_pad(x.shape[1]) if pad else x.shape[1]
        return torch.zeros((x.shape[0], Kp), dtype=torch.float8_e4m3fn), torch.zeros(1)

    class Site:
        def quantise(self, x, pad=False):
            return quant(x, pad)

    monkeypatch.setattr(ops, "quant_fp8", quant)
    monkeypatch.setattr(ops, "quant_mxfp8", quant)
    monkeypatch.setattr(ops, "Fp8Site", Site)
    for m in (engine.Mode(True, fp8=True), engine.Mode(True, fp8=True, mx=True)):
        A, B = torch.zeros((5, 192), dtype=torch.bfloat16), torch.zeros((7, 192), dtype=torch.bfloat16)
        del calls[:]
        q = engine._to_fp8(m, dict(A=A, B=B, aux=None))
        assert q["A"].shape == (5, 256) and q["B"].shape == (7, 256) and "aux" not in q and q.get("scale_mode", 0) == int(m.mx)
        assert calls == [((7, 192), True), ((5, 192), True)]
        assert list(m._q) == [id(B)] and m._q[id(B)][0] is B and m._q[id(B)][4] == 0
        engine._to_fp8(m, dict(A=A, B=B))
        assert calls[2:] == [((5, 192), True)]      # the cached weight copy is reused ...
        B._mmdit_gen = 1
        engine._to_fp8(m, dict(A=A, B=B))
        assert calls[3:] == [((7, 192), True), ((5, 192), True)] and m._q[id(B)][4] == 1      # ... until the pack generation moves
        p = dict(A=torch.zeros((5, 96), dtype=torch.bfloat16), B=torch.zeros((7, 96), dtype=torch.bfloat16))
        assert engine._to_fp8(m, p) is p
