"""Head width 128 at the ABI, construction and yardstick level.  No GPU needed.

The four entry points (mmdit_attn_fwd_hd128, mmdit_attn_bwd_hd128, mmdit_qk_norm_rope_fwd_hd128, mmdit_qk_norm_rope_bwd_hd128) live in a
header of their own, include/mmdit_hip_hd128.h, and in the binding's _HD128_SIGNATURES table: the versioned core ABI (include/mmdit_hip.h:
58 entry points, MMDIT_ABI_VERSION 10, _SIGNATURES) and the extension header do not move.  diff_model accepts dim / num_heads in {64, 128};
every form that exists at width 64 only (kv_merge_attn, the fp8 / mxfp8 precisions, attention="e4m3") is refused at construction or in
set_precision.

Yardstick soundness (test_rounding_model_stays_inside_the_bars): a float64 model of the rounding points of the 128-wide attention kernels
-- forward: the unnormalised P rounded to bf16 for P V, O rounded to bf16; backward: P and dS rounded to bf16 for their products, delta from
the ROUNDED O, bf16 outputs -- with exact arithmetic everywhere else, run over every case of tests/test_attn_hd128_gpu.py (all seven input
families), must itself stay inside the bars that file holds the kernels to (per row 1.0, per element 2.0).  Measured at width 128 over the
85 cases x {text gradient, last block}: worst per row O 0.235, dQ 0.096, dK 0.258, dV 0.596; worst per element O 0.645, dQ 0.171, dK 0.448,
dV 0.969 (profiles/hd128_parity.txt; at width 64 the project measured 0.47 per row and 0.86 per element for the same model).
"""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_attn_hd128_gpu as A  # noqa: E402

NAMES = ["mmdit_attn_bwd_hd128", "mmdit_attn_fwd_hd128", "mmdit_qk_norm_rope_bwd_hd128", "mmdit_qk_norm_rope_fwd_hd128"]
HD128 = dict(dim=256, num_heads=2, num_blocks=3)
MICRO = dict(dim=128, num_heads=2, num_blocks=3)


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _model(**kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    return diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=torch.device("cpu"),
                      positional_encoding="RoPE2d", checkpoint_MLP=False, checkpoint_attn=False, **kw)


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


def test_declared_in_the_hd128_header_only():
    L = _lib()
    assert L.declared_hd128_symbols() == NAMES
    assert len(L.declared_symbols()) == 58 and L.ABI_VERSION == 10
    assert set(L._SIGNATURES) == set(L.declared_symbols())
    assert L.declared_ext_symbols() == ["mmdit_attn_fwd_e4m3"] and set(L._EXT_SIGNATURES) == {"mmdit_attn_fwd_e4m3"}
    assert set(L._HD128_SIGNATURES) == set(NAMES)
    for n in NAMES:
        assert n not in L.declared_symbols() and n not in L.declared_ext_symbols() and n not in L._SIGNATURES and n not in L._EXT_SIGNATURES
    for path in (L.HEADER_PATH, L.HEADER_EXT_PATH):
        with open(path) as f:
            assert "hd128" not in f.read().lower(), path
    with open(L.HEADER_HD128_PATH) as f:
        txt = f.read()
    assert '#include "mmdit_hip.h"' in txt
    # every prototype cites its call site in the reference
    for cite in ("Attention.py:293", "Attention.py:277-284", "Attention.py:266-293", "Attention.py:130-135", "rotary_embedding.py:36-76"):
        assert cite in txt, cite
    # the tile edges the GPU tests are built around are the header's
    assert f"#define MMDIT_ATTN_HD128_KEY_TILE {L.ATTN_HD128_KEY_TILE}\n" in txt and f"#define MMDIT_ATTN_HD128_QUERY_TILE {L.ATTN_HD128_QUERY_TILE}\n" in txt
    assert (A.KT, A.QT) == (L.ATTN_HD128_KEY_TILE, L.ATTN_HD128_QUERY_TILE)
    assert f"#define MMDIT_QK_HD128_MAX_HEADS {L.QK_HD128_MAX_HEADS}\n" in txt and f"#define MMDIT_QK_HD128_RL_MIN_ROWS {L.QK_HD128_RL_MIN_ROWS}\n" in txt
    assert (A.MAX_HEADS, A.RL_MIN_ROWS) == (L.QK_HD128_MAX_HEADS, L.QK_HD128_RL_MIN_ROWS) and 48 * L.QK_HD128_MAX_HEADS <= 1024 < 48 * (L.QK_HD128_MAX_HEADS + 1)


def test_signatures_equal_the_prototypes_and_their_64_wide_namesakes():
    L = _lib()
    with open(L.HEADER_HD128_PATH) as f:
        txt = f.read()
    with open(L.HEADER_PATH) as f:
        core = f.read()
    strip = lambda args: [a.rsplit(" ", 1)[0] for a in args]      # noqa: E731  types without the parameter names
    for n in NAMES:
        proto = _prototype(txt, n)
        assert strip(proto) == strip(_prototype(core, n[:-len("_hd128")])), n          # the argument list of the core entry point
        argtypes, restype = L._HD128_SIGNATURES[n]
        assert restype is ctypes.c_int and argtypes == [_ctype(L, a) for a in proto], n


def test_bound_and_exported():
    L = _lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        fn = getattr(L.lib(), n)
        assert fn.argtypes == L._HD128_SIGNATURES[n][0] and fn.restype is ctypes.c_int
    assert L.lib().mmdit_abi_version() == 10


def test_build_lists_the_sources_and_the_header():
    import importlib.util
    L = _lib()
    spec = importlib.util.spec_from_file_location("_mmdit_build_hd128", os.path.join(os.path.dirname(L.LIB_PATH), "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert "attention_hd128.hip" in B.SOURCES and "rowops.hip" in B.SOURCES      # (rowops.hip: the QK-norm / RoPE kernels are its HD = 128 instantiations)
    assert os.path.samefile(B.HEADER_HD128, L.HEADER_HD128_PATH)


def test_model_constructs_at_head_width_128():
    net = _model(**HD128)
    for blk in net.blocks:
        a = blk.attn
        assert a.head_dim == 128 and a.scale == 128 ** -0.5
        for nm in (a.q_norm_x, a.k_norm_x, a.q_norm_c, a.k_norm_c):
            assert nm.weight.shape == (128,)
        assert a.rotary_emb.tables(4, 6, torch.device("cpu"))[0].shape == (24, 128)
    assert list(net.state_dict().keys()) == list(_model(**MICRO).state_dict().keys())


@pytest.mark.parametrize("dim,heads", [(64, 2), (96, 2), (192, 2), (512, 2), (200, 3), (384, 2)], ids=lambda v: str(v))
def test_other_head_widths_still_raise(dim, heads):
    """32, 48, 96, 256, a dim that num_heads does not divide, 192."""
    with pytest.raises(RuntimeError):
        _model(dim=dim, num_heads=heads, num_blocks=1)


def test_forms_that_exist_at_width_64_only_are_refused_early():
    with pytest.raises(RuntimeError, match="kv_merge_attn"):
        _model(kv_merge_attn=True, **HD128)
    net = _model(**HD128)
    assert net.set_precision("parity").precision == "parity"
    for args, kw in ((("fp8",), {}), (("mxfp8",), {}), (("fp8",), dict(attention="e4m3")), (("mxfp8",), dict(attention="e4m3"))):
        with pytest.raises(RuntimeError, match="head width 128"):
            net.set_precision(*args, **kw)
        assert net.precision == "parity" and all(m.precision == "parity" for m in net.modules() if hasattr(m, "precision"))
    assert net.set_precision("fast").precision == "fast"
    # the 64-wide refusal is unchanged
    with pytest.raises(RuntimeError, match="kv_merge_attn"):
        _model(kv_merge_attn=True, **MICRO).set_precision("fp8")


def test_ops_dispatch_is_by_head_width():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops
    L = _lib()
    assert L.HEAD_DIMS == (64, 128)
    assert ops._head_dim(torch.empty(1, 1, 1, 64)) == 64 and ops._head_dim(torch.empty(1, 1, 1, 128)) == 128
    for hd in (32, 48, 96, 256):
        with pytest.raises(RuntimeError, match="head_dim"):
            ops._head_dim(torch.empty(1, 1, 1, hd))
    assert not ops.attn_bwd_qk_ok(torch.empty(1, 1, 64, 128), 32, torch.empty(1, 1, dtype=torch.bfloat16))      # (the fused backward stays 64 wide)
    with pytest.raises(RuntimeError, match="64 only"):
        ops._qk_hd128("mmdit_qk_norm_rope_fwd_merge", [], 2, False)
    with pytest.raises(RuntimeError, match="at most 21 heads"):
        ops._qk_hd128("mmdit_qk_norm_rope_fwd", [], 22, False)


# ---------------------------------------------------------------------------------------------- yardstick soundness
def _bf(x):
    return x.to(torch.bfloat16).double()


def rounding_model(Q, K, V, dO, n_img, last):
    """float64 arithmetic with the rounding points of csrc/attention_hd128.hip (mode 0 forward, bf16-output backward) and nothing else."""
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
    assert fams == set(A.FAMILIES)
    print("\n[hd128 rounding model] worst ratio to the yardstick over %d cases x 2: " % len(A.CASES)
          + ", ".join(f"{k} per-row {v[0]:.3f} (@ {v[2]}) per-element {v[1]:.3f}" for k, v in worst.items()))
    for name, (row, el, cid) in worst.items():
        assert row <= A.ROW_BAR, (name, row, cid)
        assert el <= A.ELEM_BAR, (name, el)


def test_sweep_covers_the_tile_edges():
    """The shapes of the GPU sweep sit on, one before and one past every edge of the kernels' tiling, with both branches of the block map."""
    KT, QT = A.KT, A.QT
    S_all = {s[0] for s in A._PLAIN + A._SWIZZLED}
    for edge in (32, KT, 2 * KT, 3 * KT, QT, 2 * QT):
        assert {edge - 1, edge, edge + 1} & S_all >= {edge + 1}, edge
    for edge in (32, KT, 2 * KT, 3 * KT, QT):
        assert {edge - 1, edge, edge + 1} <= S_all, edge
    nkv = {(s[0] + KT - 1) // KT for s in A._PLAIN + A._SWIZZLED}
    assert {1, 2, 3, 4, 5} <= nkv                                       # the double buffer wraps at the third tile
    assert {(s[0] + QT - 1) // QT for s in A._SWIZZLED} >= {1, 2, 3} and all((s[2] * s[3]) % 8 == 0 for s in A._SWIZZLED)
    assert all((s[2] * s[3]) % 8 for s in A._PLAIN)
    assert any(s[0] == s[1] for s in A._PLAIN) and any(s[1] == 1 for s in A._PLAIN) and any(s[1] % 32 == 0 and s[1] < s[0] for s in A._PLAIN) and any(s[1] % 32 for s in A._PLAIN)
    assert all(s[0] % KT == 1 for s in A._EDGE) and len(A.CASES) == len(set(map(A._case_id, A.CASES)))
    # QK-norm / RoPE: rows on and off the rows per workgroup, one and two streams, with and without RoPE, 1 / 2 / 3 / most heads, tok0 != 0
    heads = {c[1] for c in A.QK_CASES}
    assert {1, 2, 3, A.MAX_HEADS} <= heads
    assert {len(c[2]) for c in A.QK_CASES} == {1, 2} and any(c[4][0] for c in A.QK_CASES)
    assert any(r for c in A.QK_CASES for _, r in c[2]) and any(not r for c in A.QK_CASES for _, r in c[2])
    big = [c for c in A.QK_CASES if min(c[0] * t for t, _ in c[2]) >= A.RL_MIN_ROWS]
    assert len(big) >= 3 and any(1024 // (48 * c[1]) > 1 for c in big) and {c[3] for c in A.QK_CASES} == {0, 1, 2}
    # the launch policy is one rule for both widths with one 64-only line (one lane per token): both of its halves, several rows per workgroup
    # and one, are reached at 128, where the grid must stay the other one (restatement of tests/test_rowops_edges_gpu.py)
    import test_rowops_edges_gpu as R
    differ = {R.qk_bwd_rl(c[1], c[0] * t, hd=128) > 1 for c in A.QK_CASES for t, r in c[2] if len(c[2]) == 1
              and R.qk_bwd_grid(c[0] * t, t, r, R.qk_bwd_rl(c[1], c[0] * t, hd=128), hd=128) != R.qk_bwd_grid(c[0] * t, t, r, R.qk_bwd_rl(c[1], c[0] * t, hd=128), hd=64)}
    assert differ == {False, True}
    assert R.qk_bwd_path(3, 2, ((1000, True),), hd=128)[0] == 10 and R.qk_bwd_grid(3000, 1000, True, 10, hd=128) == 76 and R.qk_bwd_grid(600, 600, True, 1, hd=128) == 512
