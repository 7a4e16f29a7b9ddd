"""What tests/test_qkv_epilogue_edges_gpu.py relies on, checked without a GPU.

Fault model: a float model of the fused launch (fp32-accumulating matmul, bf16 rounding, fp32 norm and rotation on the rounded values, joint-layout
scatter with the kernels' row -> (sample, token) and column -> (part, head) rules restated) goes through the GPU file's references, yardsticks,
comparator and sentinel checks: it passes every bar with room in every input family, and each of ten single faults -- the table row of token n + 1,
wk used for q, the neighbouring head's destination, the sample index not advanced at a wrap inside a 32-row block, the row M - 1 written a second
time behind the end, one K tile dropped on the last row block, eps = 1e-6, a truncated bf16 Q, v copied from row + 1, a write into a gap position
-- fails at least one check on the family meant to catch it.
Coverage and plans: every combination the sweep's docstring names is in the case table, and the restated planner (pick_cfg / fused_path) agrees with
mmdit_gemm_plan on fake pointers for every case -- 387 for every wide-slot case, 386 where claiming is off and the 8-phase kernel runs, 0 for the
refusals -- and with the return code of the fused entry point itself for the refused launches (a refusal launches nothing, so it runs here).
Closed forms: stage 2 against torch.nn.functional.rms_norm plus an explicit rotation in float64."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gemm_edges_gpu as G  # noqa: E402
import test_qkv_epilogue_edges_gpu as Q  # noqa: E402

BF = torch.bfloat16


def _by_id(cid):
    return next(c for c in Q.ALL if c.id == cid)


# ---------------------------------------------------------------------------------------------- the float model of the fused launch
def _truncate_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def model(case, family, built, fault=None, eps=1.1920929e-07):
    """The fused launch on the CPU into fresh, guarded outputs.  Rows are handled as the kernels do: 32-row blocks, ONE division for the block's first
    row and at most one wrap when tokens >= 32, a division per row below; a wave's 64 columns are one head of one part."""
    got = Q.fresh_outputs(case, family == "poison", "cpu")
    H, D, S = case.H, case.H * 64, case.s_total
    last = len(case.streams) - 1
    for i, (s, t, c) in enumerate(zip(case.streams, built, got["C"])):
        A, B = t["A64"].float(), t["B64"].float()
        acc = A @ B.T
        T, M = s.tokens, s.M
        rows = torch.arange(M)
        rowb = rows // 32 * 32
        if fault == "ktile" and i == last:      # the last 32-row block lost its last K tile
            blk = rows >= (M - 1) // 32 * 32
            acc[blk] = A[blk, :case.K - 64] @ B[:, :case.K - 64].T if case.K > 64 else 0.0
        rawb = acc.to(BF)
        if T >= 32:
            b0 = rowb // T
            n = rowb - b0 * T + (rows - rowb)
            wrap = n >= T
            n, b = n - wrap * T, b0 + (0 if fault == "nowrap" else wrap.long())
        else:
            b = rows // T
            n = rows - b * T
        for colw in range(0, case.N, 64):
            part = colw // D
            head = (colw - part * D) >> 6
            chunk = rawb[:, colw:colw + 64]
            if part == 2:
                src = chunk[(rows + 1).clamp_max(M - 1)] if fault == "vrow" else chunk
                got["V"].win[b, head, s.tok0 + n] = src
                continue
            c.win[:, colw:colw + 64] = chunk
            x = chunk.float()
            w = (t["wk"] if part == 1 or fault == "wkq" else t["wq"]).float()
            rinv = torch.rsqrt((x * x).sum(-1, keepdim=True) * (1.0 / 64.0) + torch.tensor(eps, dtype=torch.float32))
            y = x * rinv * w
            if s.rope:
                tn = (n + 1) % T if fault == "table" else n
                cs, sn = t["cos"][tn], t["sin"][tn]
                a, bb = y[:, 0::2], y[:, 1::2]
                y = torch.stack([a * cs[:, 0::2] - bb * sn[:, 0::2], bb * cs[:, 1::2] + a * sn[:, 1::2]], -1).flatten(-2)
            out = _truncate_bf16(y) if fault == "trunc" and part == 0 else y.to(BF)
            dst = got["QK"[part]]
            dst.win[b, (head + 1) % H if fault == "head" and part == 0 else head, s.tok0 + n] = out
            if fault == "lastrow" and i == last and colw == 0:      # row M (clamped to M - 1) stored as if it were live: sample `batch`, token 0, and row M of C
                dst.big[Q.GUARD + s.batch * H * S + s.tok0] = out[M - 1]
                if c.r0:
                    c.big[c.r0 + M, :64] = chunk[M - 1]
        if fault == "gap" and i == 0:
            got["K"].win[0, 0, s.tok0 - 1] = 1.0
    return got


def _verdict(case, family, fault=None, **kw):
    built = Q.build(case, family, "cpu")
    return Q.judge(case, family, built, model(case, family, built, fault, **kw), record=False)


CLEAN = ["8p:H2-K128-b2-x100+t154-noraw", "8p:H3-K64-b8-x33", "8p:H3-K192-b8-x33-gap5.7-noraw", "8p:H3-K64-b9-x32-noraw", "8p:H5-K128-b26-t10-gap3.5",
         "mx:H3-K128-b11-x48-noraw"]


@pytest.mark.parametrize("cid", CLEAN)
@pytest.mark.parametrize("family", ["random", "integer", "smallrow", "poison"])
def test_float_model_passes_every_bar_in_every_family(cid, family):
    """(the ratios are printed by judge: run with -s)"""
    failures = _verdict(_by_id(cid), family)
    assert failures == [], "\n".join(failures)


# fault -> (case id, family meant to catch it, a word the failure must contain)
FAULTS = {"table": ("8p:H3-K64-b8-x33", "random", "over the bar"),
          "wkq": ("8p:H3-K64-b8-x33", "random", ".Q: "),
          "head": ("8p:H3-K64-b8-x33", "random", ".Q: "),
          "nowrap": ("8p:H3-K64-b8-x33", "random", ".Q: "),
          "lastrow": ("8p:H3-K64-b9-x32-noraw", "poison", "outside"),
          "ktile": ("8p:H2-K128-b2-x100+t154-noraw", "random", "p1.Cqk"),
          "eps": ("8p:H3-K64-b9-x32-noraw", "smallrow", "over the bar"),
          "trunc": ("8p:H3-K64-b8-x33", "random", "'bias'"),
          "vrow": ("8p:H3-K64-b8-x33", "random", ".V: "),
          "gap": ("8p:H3-K192-b8-x33-gap5.7-noraw", "random", "outside the written positions")}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_every_single_fault_fails_a_check_on_the_family_meant_to_catch_it(fault):
    cid, family, word = FAULTS[fault]
    kw = dict(eps=1e-6) if fault == "eps" else {}
    failures = _verdict(_by_id(cid), family, None if fault == "eps" else fault, **kw)
    print(f"[fault model] {fault} on {cid} / {family}:\n  " + "\n  ".join(f[:260] for f in failures))
    assert any(word in f for f in failures), (fault, failures)
    if fault == "nowrap":      # the rows behind a boundary went to the sample before: its tokens hold other values, the right positions keep their sentinel
        assert any("non-finite" in f for f in failures)
    if fault == "trunc":       # at most 2 U |ref| per element, so inside the per-element bar by construction: the rounding-bias bar is the one that sees it (19 times its bound)
        assert all("'bias'] over the bar" in f and "'el'," not in f.split(" over the bar")[0] for f in failures)
    if fault == "eps":         # ... and eps = 1e-5 fails as well, the kernels' 2^-23 passes (test_float_model_passes_...)
        assert any("over the bar" in f for f in _verdict(_by_id(cid), family, None, eps=1e-5))


def test_c_null_check_sees_a_changed_bit_and_a_written_c():
    case = _by_id("8p:H3-K64-b9-x32-noraw")
    built = Q.build(case, "random", "cpu")
    base = {n: model(case, "random", built)[n].win.clone() for n in "QKV"}
    got = Q.fresh_outputs(case, False, "cpu")
    for n in "QKV":
        got[n].win.copy_(base[n])
    assert Q.judge(case, "random", built, got, raw=False, base=base, record=False) == []
    got["K"].win.view(torch.int16)[1, 2, 3, 4] ^= 1
    got["C"][0].win[0, 0] = 1.0
    f = Q.judge(case, "random", built, got, raw=False, base=base, record=False)
    assert any("differs from the C != NULL launch" in x for x in f) and any("written although C == NULL" in x for x in f)


# ---------------------------------------------------------------------------------------------- coverage of the case table
def test_case_table_covers_every_combination_the_sweep_names():
    ids = [Q._case_id(c) for c in Q.CASES]
    assert len(ids) == len(set(ids))
    for kernel, ktiles, tile in (("wide", {1, 2, 3, 4, 5}, 64), ("8p", {1, 2, 3, 4, 5}, 64), ("mx", {1, 2, 3}, 128)):
        cs = [c for c in Q.ALL if c.kernel == kernel]
        assert {c.H for c in cs} >= {1, 2, 3, 4, 5, 7}, kernel
        assert {c.H for c in cs if len(c.streams) == 2} >= {1, 2, 3, 4, 5, 7}, kernel         # two streams at tok0 = (0, N) at every head count
        assert all(c.streams[1].tok0 == c.streams[0].tokens and c.gap == (0, 0) for c in cs if len(c.streams) == 2)
        rot = {s.tokens for c in cs for s in c.streams if s.rope}
        assert rot >= {1, 6, 31, 32, 33, 48, 63, 64, 65} and max(rot) > 256, (kernel, rot)
        assert {s.tokens for c in cs for s in c.streams if not s.rope} >= {1, 10, 31, 33, 154}, kernel
        assert {c.K // tile for c in cs} == ktiles, kernel
        edges = set().union(*(c.row_edge() for c in cs if c.edge))
        assert edges == {"on", "before", "past"}, (kernel, edges)
        assert {c.row_edge() == {"on"} for c in cs if c.edge and c.streams[0].tokens == 1} == {True, False}, kernel      # M = edge and edge +- 1 exactly
        assert any(c.gap[0] > 0 and c.gap[1] > 0 and c.streams[0].rope for c in cs) and any(c.gap[0] > 0 and c.gap[1] > 0 and not c.streams[0].rope for c in cs), kernel
        assert any(len(c.streams) == 2 and c.streams[0].M % c.tile_rows for c in cs), kernel       # the first problem ends mid-tile
        assert any(all(s.M % c.tile_rows == 0 for s in c.streams) for c in cs), kernel             # every tile full
        assert all(Q.fused_path(c, *c.modes[-1])[:2] == (kernel, c.walk) for c in cs), kernel
        if kernel != "wide":      # RAW on and off, each with a ragged last tile and with full tiles only
            nr = [c for c in cs if c.noraw]
            assert any(all(s.M % 256 == 0 for s in c.streams) for c in nr) and any(any(s.M % 256 for s in c.streams) for c in nr), kernel
            assert all(any(s.M % 256 for s in c.streams) or c.edge for c in nr)
        else:
            assert not any(c.noraw for c in cs)
    walks = {(c.kernel, c.walk) for c in Q.ALL}
    assert walks >= {("wide", "single"), ("wide", "multi"), ("8p", "single"), ("8p", "claimed"), ("mx", "single"), ("mx", "multi")}
    claimed = [c for c in Q.ALL if c.walk == "claimed"]
    assert all(c.modes == (Q.CLAIM_NO_WS, Q.CLAIM) and Q.fused_path(c, *Q.CLAIM_NO_WS)[1] == "multi" for c in claimed) and any(c.noraw for c in claimed)
    assert any(c.kernel == "8p" and c.modes == (Q.WS_ON,) for c in Q.ALL)      # claiming off, the planner's own 256 x 256 tile
    assert all(c.kernel == "mx" and c.noraw or c.kernel != "mx" for c in Q.ALL)
    # every C == NULL case and every edge case runs the poison family; edge cases run all four
    fams = {}
    for c, f in Q.CASES:
        fams.setdefault(c.id, set()).add(f)
    assert all(fams[c.id] == {"random", "integer", "smallrow", "poison"} for c in Q.ALL if c.edge)
    assert all("poison" in fams[c.id] for c in Q.ALL if c.noraw)
    assert max(s.M for c in Q.ALL for s in c.streams) <= 17000 and max(c.K for c in Q.ALL) <= 384


# ---------------------------------------------------------------------------------------------- the restated planner against the library
def _fake(case):
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    launch = G.L("qkv", None, [G.P(s.M, case.N, case.K, ab="mx" if case.kernel == "mx" else "bf16") for s in case.streams], budget=Q.BUDGET)
    return _lib, G.fake_args(_lib.GemmArgs, launch)


@pytest.mark.parametrize("case", [c for c in Q.ALL if c.kernel != "mx"] + [c for c, _ in Q.REFUSED], ids=lambda c: c.id)
def test_restated_planner_agrees_with_the_library(case):
    _lib, arr = _fake(case)
    lib = _lib.lib()
    assert lib.mmdit_gemm_set_claiming(0) == 0
    plan = lib.mmdit_gemm_plan(arr, len(case.streams))
    path = Q.fused_path(case, True, False)
    assert plan == (path[2] if path else 0), (case.id, plan, path)
    if case in Q.ALL:
        if case.kernel == "wide":
            assert plan == 387 and path[0] == "wide"
        elif case.modes == (Q.WS_ON,):
            assert plan == 386 and path[0] == "8p"
    elif path is None:
        assert plan != 387 and plan != 386


@pytest.mark.parametrize("cr", Q.REFUSED, ids=lambda cr: cr[0].id + ("" if cr[1] else "-C=NULL"))
def test_refused_launches_are_refused_by_the_entry_point_itself(cr):
    """A refusal returns before anything is launched, so the fused entry point runs on fake pointers: MMDIT_ERR_SHAPE exactly where fused_path says
    so (claiming off), and the C == NULL forms stop being refused by the planner's rules once claiming is on (not launched here)."""
    case, raw = cr
    _lib, arr = _fake(case)
    lib = _lib.lib()
    n = len(case.streams)
    qk = (_lib.QkEpilogue * n)()
    for i, s in enumerate(case.streams):
        qk[i].wq, qk[i].wk, qk[i].tokens, qk[i].tok0 = 1 << 36, (1 << 36) + 4096, s.tokens, s.tok0
        if s.rope:
            qk[i].rope_cos, qk[i].rope_sin = 1 << 37, (1 << 37) + (1 << 20)
    if not raw:
        for i in range(n):
            arr[i].C = None
    assert lib.mmdit_gemm_set_claiming(0) == 0
    assert Q.fused_path(case, True, False, raw) is None
    assert lib.mmdit_gemm_qkv_norm_rope(arr, qk, n, case.H, case.s_total, 1 << 38, 1 << 39, 1 << 40, None) == Q.ERR_SHAPE
    assert Q.fused_path(case, True, True, raw) is not None


def test_pick_cfg_thresholds_named_in_the_docstring():
    N = lambda H: 3 * H * 64      # noqa: E731
    assert Q.pick_cfg([(32 * 16, N(4)), (32 * 154, N(4))], 64) == 3 and Q.pick_cfg([(32 * 16, N(3)), (32 * 154, N(3))], 64) == 3
    assert Q.pick_cfg([(24 * 16, N(5)), (24 * 154, N(5))], 64) == 3 and Q.pick_cfg([(32 * 100, N(2)), (32 * 154, N(2))], 64) == 3
    assert Q.pick_cfg([(65 * 100, N(1)), (65 * 154, N(1))], 64) == 3 and Q.pick_cfg([(12900, N(4))], 64) == 3
    assert Q.pick_cfg([(5376, N(4))], 64) == 2 and Q.pick_cfg([(5377, N(4))], 64) == 3 and Q.pick_cfg([(6720, N(4))], 64) == 3 and Q.pick_cfg([(6721, N(4))], 64) != 3
    assert Q.pick_cfg([(16 * 16, N(4)), (16 * 154, N(4))], 64) == 2 and Q.pick_cfg([(72, N(4)), (30, N(4))], 64) == 0


# ---------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("rope", [True, False])
def test_stage2_closed_form_equals_rms_norm_plus_explicit_rotation_in_float64(rope):
    g = torch.Generator().manual_seed(5)
    B, T, H = 2, 7, 3
    x = torch.randn(B, T, H, 64, generator=g, dtype=torch.float64)
    w = 1 + 0.3 * torch.randn(64, generator=g, dtype=torch.float64)
    cos, sin = (2 * torch.rand(T, 64, generator=g, dtype=torch.float64) - 1 for _ in range(2))
    want = F.rms_norm(x, (64,), w, Q.RMS_EPS)
    assert Q.RMS_EPS == torch.finfo(torch.float32).eps
    if rope:
        rot = torch.empty_like(want)
        for b in range(B):
            for n in range(T):
                for h in range(H):
                    for j in range(32):
                        a, bb = want[b, n, h, 2 * j], want[b, n, h, 2 * j + 1]
                        rot[b, n, h, 2 * j] = a * cos[n, 2 * j] - bb * sin[n, 2 * j]
                        rot[b, n, h, 2 * j + 1] = bb * cos[n, 2 * j + 1] + a * sin[n, 2 * j + 1]
        want = rot
    ref, det, rnd = Q.stage2(x, w, cos if rope else None, sin if rope else None)
    assert ref.shape == (B * H * T, 64) and float((ref - want.permute(0, 2, 1, 3).reshape(-1, 64)).abs().max()) <= 1e-13
    assert bool((det > 0).all()) and torch.equal(rnd, Q.U * ref.abs())
    # the joint-layout order of to_heads: row (b, head, n)
    assert torch.equal(ref.view(B, H, T, 64)[1, 2, 3], Q.stage2(x[1:2, 3:4, 2:3], w, cos[3:4] if rope else None, sin[3:4] if rope else None)[0][0])


def test_mx_quant_is_a_valid_mx_operand():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(37, 128, generator=g) * torch.exp2(torch.randint(-6, 7, (37, 1), generator=g).float())
    x[3, 32:64] = 0
    q, by = Q.mx_quant(x.to(BF))
    back = G.mx_dequant(q, by)
    assert int(by[3, 1]) == 0 and float(back[3, 32:64].abs().max()) == 0.0
    assert bool(torch.isfinite(back).all()) and float((back - x.to(BF).double()).abs().max() / x.abs().max()) < 2.0 ** -3
    blocks = x.to(BF).double().view(37, 4, 32)
    # (3 mantissa bits at the block's top binade: 2^-4 amax; a block whose amax scales to (448, 512) saturates at 448: 2^-3 amax)
    assert bool(((back.view(37, 4, 32) - blocks).abs().amax(-1) <= 2.0 ** -3 * blocks.abs().amax(-1) + 1e-30).all())
