"""positional_encoding="RoPE2dV2" at the ABI, construction, checkpoint and yardstick level.  No GPU needed.

The two entry points (mmdit_qk_norm_rope3_fwd, mmdit_qk_norm_rope3_bwd) live in a header of their own, include/mmdit_hip_rope3.h, and in the
binding's _ROPE3_SIGNATURES table: the versioned core ABI (58 entry points, MMDIT_ABI_VERSION 10), mmdit_hip_ext.h and mmdit_hip_hd128.h do
not move.  diff_model accepts the encoding at head widths 64 and 128, with the reference's state dict (`rotary_emb.inv_freq` buffers in place
of the `rotary_emb.freqs` parameters); kv_merge_attn and the fp8 / mxfp8 precisions are refused.

Yardstick: the float64 restatement of the rotation in tests/test_rope2dv2_gpu.py (rotate3) is what the GPU tests hold the kernels to; here it
is held to the reference module's recorded outputs (tests/golden/leaf_rope2dv2.npz), as are RoPE2D.forward and RoPE2D.tables.
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
import test_rope2dv2_gpu as R  # noqa: E402

NAMES = ["mmdit_qk_norm_rope3_bwd", "mmdit_qk_norm_rope3_fwd"]
HD128_NAMES = ["mmdit_attn_bwd_hd128", "mmdit_attn_fwd_hd128", "mmdit_qk_norm_rope_bwd_hd128", "mmdit_qk_norm_rope_fwd_hd128"]
MICRO = dict(dim=128, num_heads=2, num_blocks=3)
HD128 = dict(dim=256, num_heads=2, num_blocks=1)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _model(positional_encoding="RoPE2dV2", **kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    return diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=torch.device("cpu"),
                      positional_encoding=positional_encoding, checkpoint_MLP=False, checkpoint_attn=False, **kw)


def _rope(hd, f=1):
    import sd3_amd  # noqa: F401
    from sd3_amd.blocks.rotary_embedding_2d_v2 import RoPE2D
    return RoPE2D(hd, interpolate_factor=f)


def _prototype(txt, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"no prototype of {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype(L, arg):
    ty = arg.rsplit(" ", 1)[0] if not arg.endswith("*") else arg      # drop the parameter name
    ty = ty.replace("const ", "")
    if ty == "mmdit_qk_problem*":
        return ctypes.POINTER(L.QkProblem)
    if ty.endswith("*") or ty == "mmdit_stream_t":
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "float": ctypes.c_float}[ty]


# ---------------------------------------------------------------------------------------------- ABI
def test_declared_in_the_rope3_header_only():
    L = _lib()
    assert L.declared_rope3_symbols() == NAMES and set(L._ROPE3_SIGNATURES) == set(NAMES)
    assert len(L.declared_symbols()) == 58 and L.ABI_VERSION == 10 and set(L._SIGNATURES) == set(L.declared_symbols())
    assert L.declared_ext_symbols() == ["mmdit_attn_fwd_e4m3"] and set(L._EXT_SIGNATURES) == {"mmdit_attn_fwd_e4m3"}
    assert L.declared_hd128_symbols() == HD128_NAMES and set(L._HD128_SIGNATURES) == set(HD128_NAMES)
    for n in NAMES:
        for table in (L._SIGNATURES, L._EXT_SIGNATURES, L._HD128_SIGNATURES):
            assert n not in table
    for path in (L.HEADER_PATH, L.HEADER_EXT_PATH, L.HEADER_HD128_PATH):
        with open(path) as f:
            assert "rope3" not in f.read().lower(), path
    with open(L.HEADER_ROPE3_PATH) as f:
        txt = f.read()
    assert '#include "mmdit_hip.h"' in txt
    for cite in ("rotary_embedding_2d_v2.py", "Attention.py:105-107, 220-239"):
        assert cite in txt, cite


def test_signatures_equal_the_prototypes():
    L = _lib()
    with open(L.HEADER_ROPE3_PATH) as f:
        txt = f.read()
    with open(L.HEADER_PATH) as f:
        core = f.read()
    strip = lambda args: [a.rsplit(" ", 1)[0] for a in args]      # noqa: E731  types without the parameter names
    for n in NAMES:
        proto = _prototype(txt, n)
        argtypes, restype = L._ROPE3_SIGNATURES[n]
        assert restype is ctypes.c_int and argtypes == [_ctype(L, a) for a in proto], n
        # the argument list of the plain launch with head_dim after heads
        plain = _prototype(core, n.replace("rope3", "rope"))
        at = [a.rsplit(" ", 1)[1] for a in plain].index("heads") + 1
        assert strip(proto) == strip(plain[:at]) + ["int"] + strip(plain[at:]) and proto[at] == "int head_dim", n


def test_bound_and_exported():
    L = _lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        fn = getattr(L.lib(), n)
        assert fn.argtypes == L._ROPE3_SIGNATURES[n][0] and fn.restype is ctypes.c_int
    assert L.lib().mmdit_abi_version() == 10


def test_build_lists_the_source_and_the_header():
    import importlib.util
    L = _lib()
    spec = importlib.util.spec_from_file_location("_mmdit_build_rope3", os.path.join(os.path.dirname(L.LIB_PATH), "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert "rowops_rope3.hip" in B.SOURCES and os.path.samefile(B.HEADER_ROPE3, L.HEADER_ROPE3_PATH)


# ---------------------------------------------------------------------------------------------- construction, state dict, checkpoints
@pytest.mark.parametrize("cfg,hd", [(MICRO, 64), (HD128, 128)], ids=["hd64", "hd128"])
def test_model_constructs(cfg, hd):
    """Fails on the parent commit: diff_model raised for every positional_encoding but 'RoPE2d'."""
    from sd3_amd.blocks.rotary_embedding_2d_v2 import RoPE2D
    net = _model(**cfg)
    assert net.defaults["positional_encoding"] == "RoPE2dV2" and net.pos_enc.pos_embed is None
    for blk in net.blocks:
        a = blk.attn
        assert isinstance(a.rotary_emb, RoPE2D) and a.rope3 and a.head_dim == hd and a.scale == hd ** -0.5
        assert a.rotary_emb.inv_freq.shape == (hd // 3,) and a.rotary_emb.inv_freq.dtype == torch.float32
        assert "rotary_emb.inv_freq" in dict(a.named_buffers()) and not any("rotary" in n for n, _ in a.named_parameters())
        cs, sn = a.rotary_emb.tables(4, 6, torch.device("cpu"))
        assert cs.shape == sn.shape == (24, 2 * (hd // 3)) and cs.dtype == sn.dtype == torch.float32
    assert not _model("RoPE2d", **cfg).blocks[0].attn.rope3


def test_state_dict_equals_the_reference_spec():
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu_rope2dv2.json")) as f:
        spec = json.load(f)
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu.json")) as f:
        spec_v1 = json.load(f)
    net = _model(**MICRO)
    assert [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()] == spec["state_dict"]
    assert [n for n, _ in net.named_parameters()] == spec["named_parameters"]
    assert [n for n, p in net.named_parameters() if not p.requires_grad] == spec["no_grad"]
    assert sum(p.numel() for p in net.parameters()) == spec["num_params"]
    # the only difference from RoPE2d: the rotary module's entry
    assert [k[0].replace("rotary_emb.freqs", "rotary_emb.inv_freq") for k in spec_v1["state_dict"]] == [k[0] for k in spec["state_dict"]]
    assert [n for n in spec_v1["named_parameters"] if not n.endswith("rotary_emb.freqs")] == spec["named_parameters"]
    leaf = np.load(os.path.join(GOLD, "leaf_rope2dv2.npz"))
    assert np.array_equal(net.blocks[0].attn.rotary_emb.inv_freq.numpy(), leaf["inv_freq_64"])
    assert np.array_equal(_rope(128).inv_freq.numpy(), leaf["inv_freq_128"])


def test_defaults_round_trip_and_checkpoint_reload(tmp_path):
    net = _model(max_res_orig=256, max_res=128, **MICRO)
    assert net.blocks[0].attn.rotary_emb.interpolate_factor == 0.5 and json.loads(json.dumps(net.defaults)) == net.defaults
    rebuilt = type(net)(**{**json.loads(json.dumps(net.defaults)), "device": torch.device("cpu")})
    assert list(rebuilt.state_dict().keys()) == list(net.state_dict().keys()) and rebuilt.defaults == net.defaults
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())) * 0.01)
    net.saveModel(str(tmp_path))
    other = _model("RoPE2d", dim=256, num_heads=2, num_blocks=1).set_precision("parity")
    other.loadModel(str(tmp_path), "model.pkl", "model_params.json")
    assert other.defaults["positional_encoding"] == "RoPE2dV2" and other.precision == "parity" and all(b.attn.rope3 for b in other.blocks)
    assert other.blocks[0].attn.rotary_emb.interpolate_factor == 0.5
    sd, sd2 = net.state_dict(), other.state_dict()
    assert list(sd.keys()) == list(sd2.keys()) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_deepcopy_keeps_inv_freq():
    net = _model(**MICRO)
    net.blocks[0].attn.rotary_emb.tables(2, 2, torch.device("cpu"))      # (a filled table cache is not copied)
    dup = copy.deepcopy(net)
    assert list(dup.state_dict().keys()) == list(net.state_dict().keys())
    for a, b in zip(net.blocks, dup.blocks):
        ra, rb = a.attn.rotary_emb, b.attn.rotary_emb
        assert torch.equal(ra.inv_freq, rb.inv_freq) and ra.inv_freq.data_ptr() != rb.inv_freq.data_ptr()
        assert rb.interpolate_factor == ra.interpolate_factor and rb._tables == {} and "inv_freq" in dict(rb.named_buffers())


def test_refusals_name_the_encoding_and_leave_the_precision():
    with pytest.raises(RuntimeError, match="RoPE2dV2"):
        _model(kv_merge_attn=True, **MICRO)
    from sd3_amd.blocks.Attention import Attention
    with pytest.raises(RuntimeError, match="RoPE2dV2"):
        Attention(128, num_heads=2, attn_type="softmax", positional_encoding="RoPE2dV2", kv_merge_attn=True, dual=True)
    net = _model(**MICRO)
    assert net.set_precision("parity").precision == "parity"
    for prec in ("fp8", "mxfp8"):
        with pytest.raises(RuntimeError, match="RoPE2dV2"):
            net.set_precision(prec)
        assert net.precision == "parity" and all(m.precision == "parity" for m in net.modules() if hasattr(m, "precision"))
    assert net.set_precision("fast").precision == "fast"
    # the engine repeats both checks for direct use
    from sd3_amd import engine
    from types import SimpleNamespace as NS
    w = NS(last=False, rope3=True, kv_merge=False, hd=64)
    X, C = torch.zeros(2 * 4, 128), torch.zeros(2 * 2, 128)
    with pytest.raises(RuntimeError, match="RoPE2dV2"):
        engine.block_fwd(engine.FP8, w, X, C, torch.zeros(2, 128), (2, 4, 2, 2, 128), (None, None))
    w.kv_merge = True
    with pytest.raises(RuntimeError, match="RoPE2dV2"):
        engine.block_fwd(engine.FAST, w, X, C, torch.zeros(2, 128), (2, 4, 2, 2, 128), (None, None))
    # a RoPE2d model is refused nothing new
    assert _model("RoPE2d", **MICRO).set_precision("fp8").precision == "fp8"


# ---------------------------------------------------------------------------------------------- the mirror and the yardstick against the reference's outputs
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("f", [1, 2])
def test_forward_tables_and_yardstick_equal_the_reference_leaf(hd, f):
    leaf = np.load(os.path.join(GOLD, "leaf_rope2dv2.npz"))
    x, want = torch.from_numpy(leaf[f"in_{hd}"]), torch.from_numpy(leaf[f"out_{hd}_f{f}"])
    mod = _rope(hd, f)
    T = hd // 3
    # the host-side forward (rotates in place and returns its argument, as the reference does)
    arg = x.clone()
    got = mod(arg)
    assert got is arg and got.dtype == torch.float32
    assert (got - want).abs().max().item() <= 1e-6
    assert torch.equal(got[..., 3 * T:], x[..., 3 * T:])
    # the tables: cos / sin of (index / f) * inv_freq, theta by the row and alpha by the column; 2^-22 = two fp32 ulps at magnitude <= 1
    # (another libm build may round the last bit differently)
    H, W = x.shape[2], x.shape[3]
    cs, sn = mod.tables(H, W, torch.device("cpu"))
    assert cs.shape == sn.shape == (H * W, 2 * T) and cs.dtype == sn.dtype == torch.float32 and cs.is_contiguous() and sn.is_contiguous()
    fr = torch.from_numpy(leaf[f"inv_freq_{hd}"])
    row = (torch.arange(H * W) // W).float()[:, None] / f * fr
    col = (torch.arange(H * W) % W).float()[:, None] / f * fr
    ang = torch.cat([row, col], dim=-1).double()
    assert (cs.double() - ang.cos()).abs().max().item() <= 2.0 ** -22 and (sn.double() - ang.sin()).abs().max().item() <= 2.0 ** -22
    assert torch.equal(cs[:W, :T], torch.ones(W, T)) and torch.equal(sn[::W, T:], torch.zeros(H, T))      # row 0: theta = 0; column 0: alpha = 0
    assert mod.tables(H, W, torch.device("cpu"))[0] is cs      # cached
    # the GPU tests' float64 restatement, on the module's own tables
    B, Hh = x.shape[0], x.shape[1]
    z = x.double().reshape(B, Hh, H * W, hd)
    ref = R.rotate3(z, cs.double(), sn.double()).reshape(x.shape)
    assert (ref - want.double()).abs().max().item() <= 1e-6
    # ... it is orthogonal, and its transpose (the backward the kernels are held to) is the autograd of the forward
    # (with cos / sin of the angles in float64: the fp32 tables satisfy cos^2 + sin^2 = 1 to fp32 precision only)
    exact = R.rotate3(z, ang.cos(), ang.sin())
    assert (exact.norm(dim=-1) - z.norm(dim=-1)).abs().max().item() <= 1e-13
    zz = z.clone().requires_grad_(True)
    g = torch.randn(z.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    (R.rotate3(zz, cs.double(), sn.double()) * g).sum().backward()
    assert (R.rotate3_t(g, cs.double(), sn.double()) - zz.grad).abs().max().item() <= 1e-14


def test_restated_attention_reproduces_the_reference_golden(monkeypatch):
    """What licenses the GPU file's _attention_v2 as the 128-wide yardstick: at width 64, where a reference golden exists, the oracle with it in
    place of its RoPE2d attention reproduces the reference's output (fp32, on the CPU) to the oracle's own distance from the reference."""
    from oracle import mmdit_oracle as O
    from oracle.weights import make_inputs
    gold = np.load(os.path.join(GOLD, "forward_micro_rope2dv2.npz"))
    x, c, cp = make_inputs(0, 2, 16, 16, text_scale=1.0)
    sd = R._state_dict(_model(**MICRO), MICRO)
    monkeypatch.setattr(O, "attention", R._attention_v2)
    with torch.no_grad():
        v = O.forward(sd, O.OracleConfig(**MICRO), x.clone(), torch.tensor([0.3, 0.7]), c.clone(), cp.clone())
    r = float((v.double() - torch.from_numpy(gold["v"]).double()).norm() / torch.from_numpy(gold["v"]).double().norm())
    assert r < 1e-5, r
