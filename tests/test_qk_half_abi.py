"""qk_half_dim=True at the ABI, construction, checkpoint and yardstick level.  No GPU needed.

The four entry points (mmdit_attn_fwd_qkhalf, mmdit_attn_bwd_qkhalf, mmdit_qk_norm_rope_fwd_qkhalf, mmdit_qk_norm_rope_bwd_qkhalf) live in a
header of their own, include/mmdit_hip_qkhalf.h, and in the binding's _QKHALF_SIGNATURES table: the versioned core ABI (58 entry points,
MMDIT_ABI_VERSION 10), mmdit_hip_ext.h, mmdit_hip_hd128.h and mmdit_hip_rope3.h do not move.  diff_model accepts the option with
dim = 64 * num_heads and "RoPE2d", with the reference's state dict (the plain model's keys; query / key projections (dim / 2, dim), norm
weights (32,), rotary_emb.freqs (8,)); kv_merge_attn, RoPE2dV2, dim = 128 * num_heads and the fp8 / mxfp8 precisions are refused.

Yardstick soundness: a float64 model of the rounding points of csrc/attention_qkhalf.hip (P, dS, O and the outputs in bf16, delta from the
rounded O) is run over the cases of the GPU sweep (tests/test_qk_half_gpu.py) and held to the bars the kernels are held to there.
"""
import ctypes
import json
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_qk_half_gpu as A  # noqa: E402

NAMES = ["mmdit_attn_bwd_qkhalf", "mmdit_attn_fwd_qkhalf", "mmdit_qk_norm_rope_bwd_qkhalf", "mmdit_qk_norm_rope_fwd_qkhalf"]
HD128_NAMES = ["mmdit_attn_bwd_hd128", "mmdit_attn_fwd_hd128", "mmdit_qk_norm_rope_bwd_hd128", "mmdit_qk_norm_rope_fwd_hd128"]
ROPE3_NAMES = ["mmdit_qk_norm_rope3_bwd", "mmdit_qk_norm_rope3_fwd"]
MICRO = dict(dim=128, num_heads=2, num_blocks=3)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _model(qk_half_dim=True, positional_encoding="RoPE2d", **kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    return diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=torch.device("cpu"),
                      positional_encoding=positional_encoding, qk_half_dim=qk_half_dim, checkpoint_MLP=False, checkpoint_attn=False, **kw)


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
def test_declared_in_the_qkhalf_header_only():
    L = _lib()
    assert L.declared_qkhalf_symbols() == NAMES and set(L._QKHALF_SIGNATURES) == set(NAMES)
    for n in NAMES:
        for table in (L._SIGNATURES, L._EXT_SIGNATURES, L._HD128_SIGNATURES, L._ROPE3_SIGNATURES):
            assert n not in table
    for path in (L.HEADER_PATH, L.HEADER_EXT_PATH, L.HEADER_HD128_PATH, L.HEADER_ROPE3_PATH):
        with open(path) as f:
            assert "qkhalf" not in f.read().lower(), path
    with open(L.HEADER_QKHALF_PATH) as f:
        txt = f.read()
    assert '#include "mmdit_hip.h"' in txt and "Attention.py:33-67" in txt
    defs = dict(re.findall(r"#define (MMDIT_\w+) (\d+)", txt))
    assert (int(defs["MMDIT_QKHALF_QK_DIM"]), int(defs["MMDIT_QKHALF_V_DIM"])) == (L.QKHALF_QK_DIM, L.QKHALF_V_DIM) == (A.DQK, A.DV) == (32, 64)
    assert (int(defs["MMDIT_ATTN_QKHALF_KEY_TILE"]), int(defs["MMDIT_ATTN_QKHALF_QUERY_TILE"])) == (L.ATTN_QKHALF_KEY_TILE, L.ATTN_QKHALF_QUERY_TILE) == (A.KT, A.QT)


def test_the_other_headers_do_not_move():
    L = _lib()
    assert len(L.declared_symbols()) == 58 and L.ABI_VERSION == 10 and set(L._SIGNATURES) == set(L.declared_symbols())
    with open(L.HEADER_PATH) as f:
        assert re.search(r"#define\s+MMDIT_ABI_VERSION\s+10\b", f.read())
    assert L.declared_ext_symbols() == ["mmdit_attn_fwd_e4m3"] and set(L._EXT_SIGNATURES) == {"mmdit_attn_fwd_e4m3"}
    assert L.declared_hd128_symbols() == HD128_NAMES and set(L._HD128_SIGNATURES) == set(HD128_NAMES)
    assert L.declared_rope3_symbols() == ROPE3_NAMES and set(L._ROPE3_SIGNATURES) == set(ROPE3_NAMES)
    assert L.HEAD_DIMS == (64, 128)
    import sd3_amd  # noqa: F401
    from sd3_amd import ops
    with pytest.raises(RuntimeError, match="head_dim"):
        ops._head_dim(torch.empty(1, 1, 1, 32))


def test_signatures_equal_the_prototypes():
    L = _lib()
    with open(L.HEADER_QKHALF_PATH) as f:
        txt = f.read()
    with open(L.HEADER_PATH) as f:
        core = f.read()
    strip = lambda args: [a.rsplit(" ", 1)[0] for a in args]      # noqa: E731  types without the parameter names
    for n in NAMES:
        proto = _prototype(txt, n)
        argtypes, restype = L._QKHALF_SIGNATURES[n]
        assert restype is ctypes.c_int and argtypes == [_ctype(L, a) for a in proto], n
        plain = _prototype(core, n.replace("_qkhalf", ""))
        if "attn" in n:      # the argument list of the core launch
            assert proto == plain, n
        else:                # the argument list of the plain launch with (qk_dim, v_dim) after heads
            at = [a.rsplit(" ", 1)[1] for a in plain].index("heads") + 1
            assert strip(proto) == strip(plain[:at]) + ["int", "int"] + strip(plain[at:]) and proto[at:at + 2] == ["int qk_dim", "int v_dim"], n


def test_bound_and_exported():
    L = _lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        fn = getattr(L.lib(), n)
        assert fn.argtypes == L._QKHALF_SIGNATURES[n][0] and fn.restype is ctypes.c_int
    assert L.lib().mmdit_abi_version() == 10


def test_build_lists_the_sources_and_the_header():
    import importlib.util
    L = _lib()
    spec = importlib.util.spec_from_file_location("_mmdit_build_qkhalf", os.path.join(os.path.dirname(L.LIB_PATH), "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert "attention_qkhalf.hip" in B.SOURCES and "rowops_qkhalf.hip" in B.SOURCES and os.path.samefile(B.HEADER_QKHALF, L.HEADER_QKHALF_PATH)
    for src in ("attention_qkhalf.hip", "rowops_qkhalf.hip"):
        with open(os.path.join(B.CSRC, src)) as f:
            assert "mmdit_hip_qkhalf.h" in f.read(), src


# ---------------------------------------------------------------------------------------------- construction, state dict, checkpoints
def test_model_constructs():
    """Fails on the parent commit: diff_model raised for qk_half_dim=True."""
    from sd3_amd.blocks.rotary_embedding import RotaryEmbedding
    net = _model(**MICRO)
    assert net.defaults["qk_half_dim"] is True and net.qk_half_dim
    for blk in net.blocks:
        a = blk.attn
        assert a.qk_half_dim and not a.rope3 and not a.kv_merge_attn
        assert (a.head_dim_qk, a.head_dim, a.scale) == (32, 64, 64 ** -0.5)
        for lin in (a.query_proj_x, a.key_proj_x, a.query_proj_c, a.key_proj_c):
            assert lin.weight.shape == (64, 128)
        for lin in (a.value_proj_x, a.value_proj_c, a.out_proj_x):
            assert lin.weight.shape == (128, 128)
        for nm in (a.q_norm_x, a.k_norm_x, a.q_norm_c, a.k_norm_c):
            assert nm.weight.shape == (32,)
        assert isinstance(a.rotary_emb, RotaryEmbedding) and a.rotary_emb.freqs.shape == (8,) and not a.rotary_emb.freqs.requires_grad
        cs, sn = a.rotary_emb.tables(4, 6, torch.device("cpu"))
        assert cs.shape == sn.shape == (24, 32) and cs.dtype == sn.dtype == torch.float32
        assert a._pqkv_x.rows == [64, 64, 128] and a._pqkv_c.rows == [64, 64, 128]      # the N = 2 * dim projection: rows [q | k | v]
    plain = _model(False, **MICRO).blocks[0].attn
    assert not plain.qk_half_dim and plain.head_dim_qk == plain.head_dim == 64 and plain._pqkv_x.rows == [128, 128, 128]


def test_state_dict_equals_the_reference_spec_and_loads_the_sliced_weights():
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu_qkhalf.json")) as f:
        spec = json.load(f)
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu.json")) as f:
        spec_plain = json.load(f)
    net = _model(**MICRO)
    assert [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()] == spec["state_dict"]
    assert [n for n, _ in net.named_parameters()] == spec["named_parameters"]
    assert [n for n, p in net.named_parameters() if not p.requires_grad] == spec["no_grad"] and len(spec["no_grad"]) == 3
    assert sum(p.numel() for p in net.parameters()) == spec["num_params"]
    # the keys and the parameter order of the plain model; 27 tensors with other shapes
    assert [k[0] for k in spec["state_dict"]] == [k[0] for k in spec_plain["state_dict"]] and spec["named_parameters"] == spec_plain["named_parameters"]
    other = [a[0] for a, b in zip(spec["state_dict"], spec_plain["state_dict"]) if a[1] != b[1]]
    assert len(other) == 27 and all(re.search(r"(query_proj|key_proj|q_norm|k_norm)_[xc]\.weight$|rotary_emb\.freqs$", k) for k in other)
    sd = A.sliced_state_dict(net)
    net.load_state_dict(sd, strict=True)
    full = A.make_state_dict(0, MLP_type="swiglu", **MICRO)
    k = "blocks.1.attn.key_proj_c.weight"
    assert torch.equal(net.state_dict()[k], full[k][:64]) and torch.equal(net.state_dict()["blocks.2.attn.q_norm_x.weight"], full["blocks.2.attn.q_norm_x.weight"][:32])
    assert torch.equal(net.state_dict()["blocks.0.attn.rotary_emb.freqs"], full["blocks.0.attn.rotary_emb.freqs"][:8])


def test_defaults_round_trip_and_checkpoint_reload(tmp_path):
    net = _model(max_res_orig=128, max_res=256, **MICRO)
    assert net.blocks[0].attn.rotary_emb.interpolate_factor == 2.0
    assert json.loads(json.dumps(net.defaults)) == net.defaults and net.defaults["qk_half_dim"] is True
    rebuilt = type(net)(**{**json.loads(json.dumps(net.defaults)), "device": torch.device("cpu")})
    assert [(k, v.shape) for k, v in rebuilt.state_dict().items()] == [(k, v.shape) for k, v in net.state_dict().items()] and rebuilt.defaults == net.defaults
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())) * 0.01)
    net.saveModel(str(tmp_path))
    with open(os.path.join(str(tmp_path), "model_params.json")) as f:
        assert json.load(f)["qk_half_dim"] is True
    other = _model(False, dim=256, num_heads=2, num_blocks=1).set_precision("parity")
    other.loadModel(str(tmp_path), "model.pkl", "model_params.json")
    assert other.defaults["qk_half_dim"] is True and other.precision == "parity" and all(b.attn.qk_half_dim and b.attn.head_dim_qk == 32 for b in other.blocks)
    assert other.blocks[0].attn.rotary_emb.interpolate_factor == 2.0
    assert all(m.precision == "parity" for m in other.modules() if hasattr(m, "precision"))
    sd, sd2 = net.state_dict(), other.state_dict()
    assert list(sd.keys()) == list(sd2.keys()) and all(torch.equal(sd[k], sd2[k]) for k in sd)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_option_and_leave_the_precision():
    from sd3_amd.blocks.Attention import Attention
    from sd3_amd.blocks.Transformer_Block_Dual import Transformer_Block_Dual
    for bad in (dict(kv_merge_attn=True, **MICRO), dict(positional_encoding="RoPE2dV2", **MICRO), dict(dim=256, num_heads=2, num_blocks=1)):
        with pytest.raises(RuntimeError, match="qk_half_dim"):
            _model(**bad)
    ok = dict(dim=128, num_heads=2, attn_type="softmax", positional_encoding="RoPE2d", dual=True, qk_half_dim=True)
    for bad in (dict(kv_merge_attn=True), dict(positional_encoding="RoPE2dV2"), dict(dim=256)):
        with pytest.raises(RuntimeError, match="qk_half_dim"):
            Attention(**{**ok, **bad})
    with pytest.raises(RuntimeError, match="qk_half_dim"):
        Transformer_Block_Dual(128, 128, num_heads=2, attn_type="softmax", MLP_type="swiglu", positional_encoding="RoPE2d", kv_merge_attn=True, qk_half_dim=True)
    assert Attention(**ok).head_dim_qk == 32
    net = _model(**MICRO)
    assert net.set_precision("parity").precision == "parity"
    for args, kw in ((("fp8",), {}), (("mxfp8",), {}), (("fp8",), dict(attention="e4m3")), (("mxfp8",), dict(attention="e4m3"))):
        with pytest.raises(RuntimeError, match="qk_half_dim"):
            net.set_precision(*args, **kw)
        assert net.precision == "parity" and all(m.precision == "parity" for m in net.modules() if hasattr(m, "precision"))
    assert net.set_precision("fast").precision == "fast"
    # the engine repeats the checks for direct use
    from sd3_amd import engine
    from types import SimpleNamespace as NS
    X, C = torch.zeros(2 * 4, 128), torch.zeros(2 * 2, 128)
    for m, w in ((engine.FP8, NS(last=False, rope3=False, kv_merge=False, hd=64, qk_half=True)), (engine.MXFP8, NS(last=False, rope3=False, kv_merge=False, hd=64, qk_half=True)),
                 (engine.FAST, NS(last=False, rope3=False, kv_merge=True, hd=64, qk_half=True)), (engine.FAST, NS(last=False, rope3=False, kv_merge=False, hd=128, qk_half=True))):
        with pytest.raises(RuntimeError, match="qk_half_dim"):
            engine.block_fwd(m, w, X, C, torch.zeros(2, 128), (2, 4, 2, 2, 128), (None, None))


def test_a_plain_model_is_refused_nothing_new():
    net = _model(False, **MICRO)
    for prec in ("parity", "fp8", "mxfp8", "fast"):
        assert net.set_precision(prec).precision == prec
    assert net.set_precision("fp8", attention="e4m3").precision == "fp8"
    assert not net.qk_half_dim and net.defaults["qk_half_dim"] is False
    assert _model(False, kv_merge_attn=True, **MICRO).kv_merge_attn and _model(False, "RoPE2dV2", **MICRO).positional_encoding == "RoPE2dV2"
    assert _model(False, dim=256, num_heads=2, num_blocks=1).blocks[0].attn.head_dim == 128
    w = net.blocks[0].attn.weights
    assert callable(w) and not net.blocks[0].attn.qk_half_dim


# ---------------------------------------------------------------------------------------------- yardstick soundness
def _bf(x):
    return x.to(torch.bfloat16).double()


def rounding_model(Q, K, V, dO, n_img, last):
    """float64 arithmetic with the rounding points of csrc/attention_qkhalf.hip (mode 0 forward, bf16-output backward) and nothing else."""
    s = A.SCALE * Q @ K.mT
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    O = _bf((_bf(p) @ V) / l)
    lse = m + torch.log(l)
    if last:
        dO = dO.clone()
        dO[:, :, n_img:] = 0.0
    P = torch.exp(s - lse)
    dP = dO @ V.mT
    delta = (dO * O).sum(-1, keepdim=True)
    dS = _bf(P * (dP - delta))
    return dict(O=O, dQ=_bf(A.SCALE * dS @ K), dK=_bf(A.SCALE * dS.mT @ Q), dV=_bf(_bf(P).mT @ dO))


def test_rounding_model_stays_inside_the_bars():
    """See the module docstring.  One pass over all cases of the GPU sweep; prints the worst ratio per output."""
    worst = {k: [0.0, 0.0, ""] for k in ("O", "dQ", "dK", "dV")}
    fams = set()
    for shape, fam in A.CASES:
        S, n_img, Bt, H = shape
        Q, K, V, dO = (t.double() for t in A.make_inputs(shape, fam))
        assert Q.shape == K.shape == (Bt, H, S, 32) and V.shape == dO.shape == (Bt, H, S, 64)
        fams.add(fam)
        fwd = A._ref_fwd(Q, K, V)
        for last in (False, True):
            d = dO.clone()
            if last:
                d[:, :, n_img:] = 0.0
            ref = A._ref_bwd(Q, K, V, d, fwd)
            ref.update(O=fwd["O"], yO=fwd["yO"])
            out = rounding_model(Q, K, V, dO, n_img, last)
            for name in worst:
                row, el, _ = A._ratios(out[name], ref[name], ref["y" + name[-1]])
                if row > worst[name][0]:
                    worst[name][0], worst[name][2] = row, A._case_id((shape, fam))
                worst[name][1] = max(worst[name][1], el)
    assert fams == set(A.FAMILIES) and "lastkey" in fams
    print("\n[qk_half rounding model] worst ratio to the yardstick over %d cases x 2: " % len(A.CASES)
          + ", ".join(f"{k} per-row {v[0]:.3f} (@ {v[2]}) per-element {v[1]:.3f}" for k, v in worst.items()))
    for name, (row, el, cid) in worst.items():
        assert row <= A.ROW_BAR, (name, row, cid)
        assert el <= A.ELEM_BAR, (name, el)


def test_sweep_covers_the_tile_edges():
    """The shapes of the GPU sweep sit on, one before and one past every edge of the kernels' tiling, with both branches of the block map."""
    KT, QT = A.KT, A.QT
    shapes = A._PLAIN + A._SWIZZLED
    S_all = {s[0] for s in shapes}
    for edge in (32, KT, 2 * KT, 3 * KT, QT, 2 * QT):
        assert {edge - 1, edge, edge + 1} & S_all >= {edge + 1}, edge
    for edge in (32, KT, 2 * KT, 3 * KT, QT):
        assert {edge - 1, edge, edge + 1} <= S_all, edge
    assert max(S_all) == 2 * QT + 1
    nkv = {(s[0] + KT - 1) // KT for s in shapes}
    assert {1, 2, 3} <= nkv and max(nkv) > 3                            # the double buffer wraps at the third tile
    assert {(s[0] + QT - 1) // QT for s in A._SWIZZLED} >= {1, 2, 3} and all((s[2] * s[3]) % 8 == 0 for s in A._SWIZZLED)
    assert all((s[2] * s[3]) % 8 for s in A._PLAIN)
    assert any(s[0] == s[1] for s in A._PLAIN) and any(s[1] == 1 for s in A._PLAIN) and any(s[1] % 32 == 0 and s[1] < s[0] for s in A._PLAIN) and any(s[1] % 32 for s in A._PLAIN)
    assert all(s[0] % KT == 1 for s in A._EDGE) and len(A.CASES) == len(set(map(A._case_id, A.CASES)))
    ragged_lastkey = [s for s, fam in A.CASES if fam == "lastkey" and s[0] % KT]
    assert len(ragged_lastkey) >= 10                                    # all the shared attention mass on the last valid key of a ragged tile
    # row kernels: 16 * heads chunks per row, 256 per workgroup
    heads = {s[1] for s in A._SHAPES}
    assert heads == {1, 2, 3, 19, 24}
    assert any(s[2][0] == 1 for s in A._SHAPES) and any(s[2][1] == 1 for s in A._SHAPES)
    chunks = [s[0] * s[2][0] * s[2][1] * 16 * s[1] for s in A._SHAPES]
    assert any(c < 256 for c in chunks) and any(c > 512 and c % 256 for c in chunks)
