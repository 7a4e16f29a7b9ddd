"""attn_type="cosine2" at the ABI, construction, checkpoint and yardstick level.  No GPU needed.

The five entry points (mmdit_qk_l2norm_rope_fwd / _bwd, mmdit_attn_cos2_fwd / _bwd, mmdit_attn_cos2_ws_bytes) live in a header of their own,
include/mmdit_hip_cos2.h, and in the binding's _COS2_SIGNATURES table: the versioned core ABI (58 entry points, MMDIT_ABI_VERSION 10) and the five
other headers do not move.  diff_model accepts attn_type="cosine2" with dim = 64 * num_heads and "RoPE2d", with the reference's state dict (the
plain model's minus the twelve q_norm_* / k_norm_* weights); kv_merge_attn, qk_half_dim, text_loss, RoPE2dV2, another head width and the fp8 /
mxfp8 precisions are refused, and attn_type="cosine" raises as before.

Yardstick soundness: the float64 restatement of cosine2 attention that tests/test_cosine2_gpu.py holds the kernels to reproduces the REAL
reference's attention taps (forward_micro_cosine2.npz) from the reference's block-0 inputs (forward_micro_plain.npz), in its quadratic and in its
linear form, to the distance of an fp32 run from a float64 one (1e-5: the oracle's own bar in tests/test_rope2dv2_abi.py); its backward formulas
are autograd's; fp32 sums and a hi + lo bf16 state stay inside the 2^-14 cap of the GPU bounds and a state rounded to one bf16 does not.
"""
import copy
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cosine2_gpu as A  # noqa: E402

NAMES = ["mmdit_attn_cos2_bwd", "mmdit_attn_cos2_fwd", "mmdit_attn_cos2_ws_bytes", "mmdit_qk_l2norm_rope_bwd", "mmdit_qk_l2norm_rope_fwd"]
HD128_NAMES = ["mmdit_attn_bwd_hd128", "mmdit_attn_fwd_hd128", "mmdit_qk_norm_rope_bwd_hd128", "mmdit_qk_norm_rope_fwd_hd128"]
ROPE3_NAMES = ["mmdit_qk_norm_rope3_bwd", "mmdit_qk_norm_rope3_fwd"]
QKHALF_NAMES = ["mmdit_attn_bwd_qkhalf", "mmdit_attn_fwd_qkhalf", "mmdit_qk_norm_rope_bwd_qkhalf", "mmdit_qk_norm_rope_fwd_qkhalf"]
MICRO = dict(dim=128, num_heads=2, num_blocks=3)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NORM_KEY = re.compile(r"\.attn\.[qk]_norm_[xc]\.weight$")


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _model(attn_type="cosine2", positional_encoding="RoPE2d", **kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    return diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type=attn_type, MLP_type="swiglu", device=torch.device("cpu"),
                      positional_encoding=positional_encoding, checkpoint_MLP=False, checkpoint_attn=False, **kw)


def _prototype(txt, name):
    m = re.search(r"\b(int|long long)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"no prototype of {name}"
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def _ctype(L, arg):
    ty = arg.rsplit(" ", 1)[0] if not arg.endswith("*") else arg      # drop the parameter name
    ty = ty.replace("const ", "")
    if ty == "mmdit_qk_problem*":
        return ctypes.POINTER(L.QkProblem)
    if ty.endswith("*") or ty == "mmdit_stream_t":
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "float": ctypes.c_float}[ty]


# ---------------------------------------------------------------------------------------------- ABI
def test_declared_in_the_cos2_header_only():
    L = _lib()
    assert L.declared_cos2_symbols() == NAMES and set(L._COS2_SIGNATURES) == set(NAMES)
    for n in NAMES:
        for table in (L._SIGNATURES, L._EXT_SIGNATURES, L._HD128_SIGNATURES, L._ROPE3_SIGNATURES, L._QKHALF_SIGNATURES, L._TEXTLOSS_SIGNATURES):
            assert n not in table
    for path in (L.HEADER_PATH, L.HEADER_EXT_PATH, L.HEADER_HD128_PATH, L.HEADER_ROPE3_PATH, L.HEADER_QKHALF_PATH, L.HEADER_TEXTLOSS_PATH):
        with open(path) as f:
            txt = f.read().lower()
        assert "cos2" not in txt and "l2norm" not in txt and "cosine2" not in txt, path
    with open(L.HEADER_COS2_PATH) as f:
        txt = f.read()
    assert '#include "mmdit_hip.h"' in txt and "Attention.py:153-162, 330-339" in txt
    defs = dict(re.findall(r"#define (MMDIT_\w+) (\d+)", txt))
    assert int(defs["MMDIT_COS2_HEAD_DIM"]) == L.COS2_HEAD_DIM == A.HD == 64
    assert (int(defs["MMDIT_ATTN_COS2_TOKEN_CHUNK"]), int(defs["MMDIT_ATTN_COS2_ROW_TILE"])) == (L.ATTN_COS2_TOKEN_CHUNK, L.ATTN_COS2_ROW_TILE) == (A.T, A.RT)


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
    assert L.HEAD_DIMS == (64, 128)


def test_signatures_equal_the_prototypes():
    L = _lib()
    with open(L.HEADER_COS2_PATH) as f:
        txt = f.read()
    with open(L.HEADER_PATH) as f:
        core = f.read()
    strip = lambda args: [a.rsplit(" ", 1)[0] for a in args]      # noqa: E731  types without the parameter names
    for n in NAMES:
        ret, proto = _prototype(txt, n)
        argtypes, restype = L._COS2_SIGNATURES[n]
        assert restype is (ctypes.c_longlong if ret == "long long" else ctypes.c_int) and argtypes == [_ctype(L, a) for a in proto], n
    assert _prototype(txt, "mmdit_attn_cos2_ws_bytes") == ("long long", ["int batch", "int heads", "int S"])
    # the row launches: the argument lists of the plain ones, with out_dtype after qkv_dtype in the forward
    _, plain_f = _prototype(core, "mmdit_qk_norm_rope_fwd")
    _, plain_b = _prototype(core, "mmdit_qk_norm_rope_bwd")
    _, f = _prototype(txt, "mmdit_qk_l2norm_rope_fwd")
    _, b = _prototype(txt, "mmdit_qk_l2norm_rope_bwd")
    at = [a.rsplit(" ", 1)[1] for a in plain_f].index("qkv_dtype") + 1
    assert strip(f) == strip(plain_f[:at]) + ["int"] + strip(plain_f[at:]) and f[at] == "int out_dtype"
    assert strip(b) == strip(plain_b)


def test_bound_and_exported():
    L = _lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        fn = getattr(L.lib(), n)
        assert fn.argtypes == L._COS2_SIGNATURES[n][0] and fn.restype is L._COS2_SIGNATURES[n][1]
    assert L.lib().mmdit_abi_version() == 10
    # the host function: per (batch, head) two final states (M, M^T, two vectors) and two partial states per chunk of T tokens; no launch
    ws = L.lib().mmdit_attn_cos2_ws_bytes
    fstate, state = 2 * 64 * 64 + 128, 64 * 64 + 128
    for batch, heads, S in ((1, 1, 1), (2, 3, A.T), (2, 3, A.T + 1), (4, 19, 5 * A.T + 1)):
        assert ws(batch, heads, S) == 2 * batch * heads * (fstate + -(-S // A.T) * state) * 4
    assert ws(0, 1, 1) == ws(1, 0, 1) == ws(1, 1, 0) == 0


def test_build_lists_the_sources_and_the_header():
    import importlib.util
    L = _lib()
    spec = importlib.util.spec_from_file_location("_mmdit_build_cos2", os.path.join(os.path.dirname(L.LIB_PATH), "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert "attention_cos2.hip" in B.SOURCES and "rowops_cos2.hip" in B.SOURCES and os.path.samefile(B.HEADER_COS2, L.HEADER_COS2_PATH)
    for src in ("attention_cos2.hip", "rowops_cos2.hip"):
        with open(os.path.join(B.CSRC, src)) as f:
            txt = f.read()
        assert "mmdit_hip_cos2.h" in txt and "atomicAdd" not in txt, src


# ---------------------------------------------------------------------------------------------- construction, state dict, checkpoints
def test_model_constructs():
    """Fails on the parent commit: diff_model raised for attn_type="cosine2"."""
    from sd3_amd import engine
    from sd3_amd.blocks.rotary_embedding import RotaryEmbedding
    net = _model(**MICRO)
    assert net.defaults["attn_type"] == "cosine2" and net.cos2
    for blk in net.blocks:
        a = blk.attn
        assert a.cos2 and a.attn_type == "cosine2" and not a.rope3 and not a.kv_merge_attn and not a.qk_half_dim
        assert (a.head_dim_qk, a.head_dim) == (64, 64) and not hasattr(a, "scale")
        assert not any(hasattr(a, n) for n in ("q_norm_x", "k_norm_x", "q_norm_c", "k_norm_c"))
        for lin in (a.query_proj_x, a.key_proj_x, a.value_proj_x, a.query_proj_c, a.key_proj_c, a.value_proj_c, a.out_proj_x):
            assert lin.weight.shape == (128, 128)
        assert isinstance(a.rotary_emb, RotaryEmbedding) and a.rotary_emb.freqs.shape == (16,) and not a.rotary_emb.freqs.requires_grad
        cs, sn = a.rotary_emb.tables(4, 6, torch.device("cpu"))
        assert cs.shape == sn.shape == (24, 64) and cs.dtype == sn.dtype == torch.float32
        w = a.weights(engine.PARITY)      # (the fp32 views: the bf16 copies are made on the GPU)
        assert w.cos2 is True and w.hd == 64 and not w.kv_merge and not w.rope3 and not w.qk_half and not hasattr(w, "wq_x")
    plain = _model("softmax_flash", **MICRO).blocks[0].attn
    assert not plain.cos2 and plain.scale == 64 ** -0.5 and plain.q_norm_x.weight.shape == (64,)
    assert not getattr(plain.weights(engine.PARITY), "cos2", False)


def test_state_dict_equals_the_reference_spec_and_the_plain_spec_minus_the_norm_weights():
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu_cosine2.json")) as f:
        spec = json.load(f)
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu.json")) as f:
        spec_plain = json.load(f)
    net = _model(**MICRO)
    assert [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()] == spec["state_dict"]
    assert [n for n, _ in net.named_parameters()] == spec["named_parameters"]
    assert [n for n, p in net.named_parameters() if not p.requires_grad] == spec["no_grad"] and len(spec["no_grad"]) == 3
    assert sum(p.numel() for p in net.parameters()) == spec["num_params"] == spec_plain["num_params"] - 12 * 64
    dropped = [e for e in spec_plain["state_dict"] if NORM_KEY.search(e[0])]
    assert len(dropped) == 12 and spec["state_dict"] == [e for e in spec_plain["state_dict"] if not NORM_KEY.search(e[0])]
    assert spec["named_parameters"] == [n for n in spec_plain["named_parameters"] if not NORM_KEY.search(n)] and len(spec["named_parameters"]) == 100
    net.load_state_dict(A.own_state_dict(net), strict=True)
    full = A.make_state_dict(0, MLP_type="swiglu", **MICRO)
    assert all(torch.equal(v, full[k]) for k, v in net.state_dict().items())
    with pytest.raises(RuntimeError, match="q_norm_x"):      # the plain model's state dict has keys this model does not
        net.load_state_dict(full, strict=True)
    with open(os.path.join(GOLD, "generation_report_cosine2.json")) as f:
        rep = json.load(f)
    assert rep["state_dict_keys_dropped"] == [e[0] for e in dropped] and rep["gradients"]["parameters"] == 97
    assert 0 < rep["forward"]["bf16_autocast_vs_fp32"] < 2e-2 and 0 < rep["forward_nonsquare"]["bf16_autocast_vs_fp32"] < 2e-2
    limit = os.path.getsize(os.path.join(GOLD, "forward_micro_kvmerge.npz"))
    for name in ("forward_micro_cosine2.npz", "forward_micro_cosine2_nonsquare.npz"):
        assert os.path.getsize(os.path.join(GOLD, name)) <= limit


def test_defaults_round_trip_checkpoint_reload_and_deepcopy(tmp_path):
    net = _model(max_res_orig=128, max_res=256, **MICRO)
    assert net.blocks[0].attn.rotary_emb.interpolate_factor == 2.0
    assert json.loads(json.dumps(net.defaults)) == net.defaults and net.defaults["attn_type"] == "cosine2"
    rebuilt = type(net)(**{**json.loads(json.dumps(net.defaults)), "device": torch.device("cpu")})
    assert [(k, v.shape) for k, v in rebuilt.state_dict().items()] == [(k, v.shape) for k, v in net.state_dict().items()] and rebuilt.defaults == net.defaults
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())) * 0.01)
    net.saveModel(str(tmp_path))
    with open(os.path.join(str(tmp_path), "model_params.json")) as f:
        assert json.load(f)["attn_type"] == "cosine2"
    other = _model("softmax_flash", dim=256, num_heads=2, num_blocks=1).set_precision("parity")
    other.loadModel(str(tmp_path), "model.pkl", "model_params.json")
    assert other.defaults["attn_type"] == "cosine2" and other.cos2 and other.precision == "parity" and all(b.attn.cos2 and not hasattr(b.attn, "q_norm_x") for b in other.blocks)
    assert other.blocks[0].attn.rotary_emb.interpolate_factor == 2.0
    assert all(m.precision == "parity" for m in other.modules() if hasattr(m, "precision"))
    sd, sd2 = net.state_dict(), other.state_dict()
    assert list(sd.keys()) == list(sd2.keys()) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    twin = copy.deepcopy(net)
    assert twin.cos2 and all(b.attn.cos2 for b in twin.blocks) and twin.defaults == net.defaults
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(twin.state_dict().values(), sd.values()))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_option_and_leave_the_precision():
    from sd3_amd.blocks.Attention import Attention
    from sd3_amd.blocks.Transformer_Block_Dual import Transformer_Block_Dual
    for bad in (dict(kv_merge_attn=True, **MICRO), dict(qk_half_dim=True, **MICRO), dict(text_loss=True, **MICRO), dict(positional_encoding="RoPE2dV2", **MICRO),
                dict(dim=256, num_heads=2, num_blocks=1), dict(dim=96, num_heads=2, num_blocks=1)):
        with pytest.raises(RuntimeError, match="cosine2"):
            _model(**bad)
    ok = dict(dim=128, num_heads=2, attn_type="cosine2", positional_encoding="RoPE2d", dual=True)
    for bad in (dict(kv_merge_attn=True), dict(qk_half_dim=True), dict(positional_encoding="RoPE2dV2"), dict(dim=256)):
        with pytest.raises(RuntimeError, match="cosine2"):
            Attention(**{**ok, **bad})
    with pytest.raises(RuntimeError, match="cosine2"):
        Transformer_Block_Dual(128, 128, num_heads=2, attn_type="cosine2", MLP_type="swiglu", positional_encoding="RoPE2d", kv_merge_attn=True)
    assert Attention(**ok).cos2
    # "cosine" and every other attention type of the reference keep raising exactly as they did
    for other in ("cosine", "cosine3", "cosine4", "cosine_norm", "relu", "silu", "exp", "both"):
        with pytest.raises(RuntimeError, match="attn_type must be"):
            Attention(**{**ok, "attn_type": other})
        with pytest.raises(RuntimeError, match="attn_type must be"):
            _model(other, **MICRO)
    for bad in (dict(causal=True), dict(dual=False), dict(emb_dim=64), dict(positional_encoding="absolute"), dict(positional_encoding="RoPE")):
        with pytest.raises(RuntimeError):
            Attention(**{**ok, **bad})
    net = _model(**MICRO)
    assert net.set_precision("parity").precision == "parity"
    for args, kw in ((("fp8",), {}), (("mxfp8",), {}), (("fp8",), dict(attention="e4m3")), (("mxfp8",), dict(attention="e4m3"))):
        with pytest.raises(RuntimeError, match="cosine2"):
            net.set_precision(*args, **kw)
        assert net.precision == "parity" and all(m.precision == "parity" for m in net.modules() if hasattr(m, "precision"))
    assert net.set_precision("fast").precision == "fast"
    # the engine repeats the checks for direct use
    from sd3_amd import engine
    from types import SimpleNamespace as NS
    X, C = torch.zeros(2 * 4, 128), torch.zeros(2 * 2, 128)
    w = lambda **kw: NS(**{**dict(last=False, rope3=False, kv_merge=False, hd=64, qk_half=False, cos2=True), **kw})      # noqa: E731
    for m, ws in ((engine.FP8, w()), (engine.MXFP8, w()), (engine.FAST, w(kv_merge=True)), (engine.FAST, w(hd=128)), (engine.FAST, w(rope3=True)),
                  (engine.FAST, w(qk_half=True))):
        with pytest.raises(RuntimeError, match="cosine2"):
            engine.block_fwd(m, ws, X, C, torch.zeros(2, 128), (2, 4, 2, 2, 128), (None, None))


def test_a_plain_model_is_refused_nothing_new():
    net = _model("softmax_flash", **MICRO)
    for prec in ("parity", "fp8", "mxfp8", "fast"):
        assert net.set_precision(prec).precision == prec
    assert net.set_precision("fp8", attention="e4m3").precision == "fp8"
    assert not net.cos2 and net.defaults["attn_type"] == "softmax_flash"
    assert _model("softmax", kv_merge_attn=True, **MICRO).kv_merge_attn and _model("softmax", "RoPE2dV2", **MICRO).positional_encoding == "RoPE2dV2"
    assert _model("softmax", qk_half_dim=True, **MICRO).qk_half_dim and _model("softmax", text_loss=True, **MICRO).text_loss
    assert _model("softmax", dim=256, num_heads=2, num_blocks=1).blocks[0].attn.head_dim == 128


# ---------------------------------------------------------------------------------------------- yardstick soundness
def test_float64_restatement_reproduces_the_reference_taps():
    """Block 0's attention of the real reference (tap_attn_x / tap_attn_c of forward_micro_cosine2.npz) from its inputs (tap_norm1_x / tap_norm1_c of
    forward_micro_plain.npz: nothing in front of the first attention depends on the option), by the float64 functions of the GPU test file:
    projections, l2n, rotate2 with the module's own tables, cos2_quadratic (the reference's expression) or cos2_linear, head merge, out
    projections.  The reference ran in fp32: the bar is the distance of an fp32 run from a float64 one, 1e-5."""
    gold = np.load(os.path.join(GOLD, "forward_micro_cosine2.npz"))
    plain = np.load(os.path.join(GOLD, "forward_micro_plain.npz"))
    assert np.allclose(plain["inputs_checksum"], gold["inputs_checksum"], rtol=1e-12)
    net = _model(**MICRO)
    net.load_state_dict(A.own_state_dict(net), strict=True)
    a = net.blocks[0].attn
    n1x, n1c = torch.from_numpy(plain["tap_norm1_x"]).double(), torch.from_numpy(plain["tap_norm1_c"]).double()
    B, N, d = n1x.shape
    Mt, H = n1c.shape[1], a.num_heads
    assert (B, N, Mt, H) == (2, 64, 154, 2)
    cs, sn = (t.double() for t in a.rotary_emb.tables(8, 8, torch.device("cpu")))
    heads = lambda t, L: t.reshape(B, L, H, 64).permute(0, 2, 1, 3)      # noqa: E731
    proj = lambda lin, t, L: heads(t @ lin.weight.detach().double().T, L)      # noqa: E731
    q = torch.cat([A.rotate2(A.l2n(proj(a.query_proj_x, n1x, N)), cs, sn), A.l2n(proj(a.query_proj_c, n1c, Mt))], 2)
    k = torch.cat([A.rotate2(A.l2n(proj(a.key_proj_x, n1x, N)), cs, sn), A.l2n(proj(a.key_proj_c, n1c, Mt))], 2)
    v = torch.cat([proj(a.value_proj_x, n1x, N), proj(a.value_proj_c, n1c, Mt)], 2)
    assert float((q.norm(dim=-1) - 1).abs().max()) < 1e-7      # (the rotation by the module's fp32 tables: cos^2 + sin^2 = 1 to fp32)
    for form in (A.cos2_quadratic, A.cos2_linear):
        out, den = form(q, k, v)
        assert float((den / (N + Mt)).min()) > 0.5
        m = out.permute(0, 2, 1, 3).reshape(B, N + Mt, d)
        ax = m[:, :N] @ a.out_proj_x.weight.detach().double().T
        ac = m[:, N:] @ a.out_proj_c.weight.detach().double().T
        rx, rc = A.rel(ax, torch.from_numpy(gold["tap_attn_x"])), A.rel(ac, torch.from_numpy(gold["tap_attn_c"]))
        print(f"[cosine2 yardstick] {form.__name__} vs the reference's taps: attn_x {rx:.3e}, attn_c {rc:.3e} (bar 1e-5)")
        assert rx < 1e-5 and rc < 1e-5, (form.__name__, rx, rc)


def test_backward_formulas_are_autograd_of_the_quadratic_form():
    A.test_backward_formulas_are_autograd_of_the_quadratic_form()


def test_fp32_sums_and_a_hi_lo_state_stay_inside_the_cap_and_a_bf16_state_does_not():
    """The cap of the GPU bounds, |out - ref| <= 2^-14 (m_n + |ref| m_d) / den, is a condition on the arithmetic: an fp32 evaluation of the linear
    form satisfies it at the longest sequence of the sweep (and at S = 900), so does a state fed to a bf16 matrix product as a hi + lo pair, and a
    state rounded to ONE bf16 (2^-9 m) violates it."""
    bf = lambda t: t.to(torch.bfloat16).double()      # noqa: E731
    for S in (max(A._S), 900):
        g = torch.Generator().manual_seed(S)
        q, k, v = A.l2n(torch.randn(1, 3, S, 64, generator=g)), A.l2n(torch.randn(1, 3, S, 64, generator=g)), torch.randn(1, 3, S, 64, generator=g)
        qd, kd, vd = q.double(), k.double(), v.double()
        ref, den = A.cos2_quadratic(qd, kd, vd)
        m_n = qd.abs() @ (kd.abs().mT @ vd.abs()) + vd.abs().sum(-2, keepdim=True)
        m_d = (qd.abs() * kd.abs().sum(-2, keepdim=True)).sum(-1) + S
        cap = A.CAP * (m_n + ref.abs() * m_d.unsqueeze(-1)) / den.unsqueeze(-1)
        KV, ksum, vsum = kd.mT @ vd, kd.sum(-2, keepdim=True), vd.sum(-2, keepdim=True)

        def with_state(f):
            return (qd @ f(KV) + f(vsum)) / ((qd * f(ksum)).sum(-1, keepdim=True) + S)
        fp32 = A.cos2_linear(q, k, v)[0].double()
        hilo = with_state(lambda t: bf(t) + bf(t - bf(t)))
        one = with_state(bf)
        r32, rhl, r1 = (float(((o - ref).abs() / cap).max()) for o in (fp32, hilo, one))
        print(f"[cosine2 yardstick] S = {S}: worst |out - ref| / cap: fp32 sums {r32:.3f}, hi + lo state {rhl:.3f}, bf16 state {r1:.3f}")
        assert r32 <= 1.0 and rhl <= 1.0 and r1 > 1.0, (S, r32, rhl, r1)


def test_sweep_covers_the_chunk_and_tile_edges():
    T, RT = A.T, A.RT
    assert A._S == [1, T - 1, T, T + 1, 2 * T + 3, 5 * T + 1] and max(A._S) <= 900
    assert sorted(b * h for b, h in A._BH) == [1, 3, 8, 19] and len(A.ATTN_CASES) == 24
    assert {-(-S // T) for S in A._S} == {1, 2, 3, 6} and any(S % RT for S in A._S)
    for S in A._S:
        n = A.n_img_values(S)
        assert {0, 1, S - 1, S} & set(range(S + 1)) <= set(n) and (S == 1 or any(x % T and x % RT and 1 < x < S - 1 for x in n))
    heads = {s[1] for s in A._SHAPES}
    assert heads == {1, 2, 3, 19, 24}
    assert any(s[2][0] == 1 for s in A._SHAPES) and any(s[2][1] == 1 for s in A._SHAPES)
    chunks = [s[0] * s[2][0] * s[2][1] * 24 * s[1] for s in A._SHAPES]
    assert any(c < 256 for c in chunks) and any(c > 512 and c % 256 for c in chunks)
