"""What tests/test_gemm_edges_gpu.py relies on, checked without a GPU: the planner's code (and zero mask) for every launch of the sweep, so that a
planner change that would move a GPU case to another kernel shows before anyone has a GPU; and the comparator itself -- a float32-accumulating CPU
model of a case's inputs passes the bars, a damaged output fails them on the row, column or element the damage touches, a changed byte outside an
output's window is reported."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # (the sweep's tables and comparator live in the GPU module next to this file)
import test_gemm_edges_gpu as G  # noqa: E402


@pytest.mark.parametrize("launch", G.LAUNCHES, ids=lambda l: l.id)
def test_sweep_plan_table(launch):
    """mmdit_gemm_plan / mmdit_gemm_zero_mask on fake pointers for every launch of the sweep, under each (workspace, claiming) mode it runs in."""
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    lib = _lib.lib()
    arr = G.fake_args(_lib.GemmArgs, launch)
    for i, (use_ws, claiming) in enumerate(launch.modes):
        if use_ws:      # (mmdit_gemm_set_workspace only stores the pointer)
            assert lib.mmdit_gemm_set_workspace(ctypes.c_void_p(1 << 40), G.WS_BYTES) == 0
        assert lib.mmdit_gemm_set_claiming(int(claiming)) == 0
        try:
            mask = ctypes.c_uint(0)
            rc = lib.mmdit_gemm_zero_mask(arr, len(launch.probs), ctypes.byref(mask))
            assert lib.mmdit_gemm_plan(arr, len(launch.probs)) == launch.plan, (launch.id, use_ws, claiming)
            assert rc == 0
            if launch.masks is not None:
                assert mask.value == launch.masks[i], (launch.id, use_ws, claiming)
        finally:
            assert lib.mmdit_gemm_set_claiming(0) == 0 and lib.mmdit_gemm_set_workspace(None, 0) == 0


def test_sweep_covers_every_family_and_edge_cases_run_all_input_families():
    plans = {l.plan for l in G.LAUNCHES}
    assert plans == {64, 0, 2, 386, 387, 418, 258}
    assert all(l.is_edge() for l in G.LAUNCHES if any(p.M % 256 == 1 or p.N % 256 == 8 for p in l.probs))
    ids = [G._case_id(c) for c in G.CASES]
    assert len(ids) == len(set(ids))


def test_mx_scale_layout_restatement_matches_the_binding():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops
    g = torch.Generator().manual_seed(3)
    for rows, K in ((257, 128), (1, 256), (128, 640)):
        by = torch.randint(0, 255, (rows, K // 32), generator=g, dtype=torch.uint8)
        packed = G.mx_pack(by, 0xFF, 0xFF)
        assert packed.numel() == ops.mx_scale_bytes(rows, K) and bool((packed[-512:] == 0xFF).all())
        assert torch.equal(ops.mx_scales_to_rows(packed, rows, K), by) and torch.equal(G.mx_unpack(packed, rows, K), by)
        assert int((packed != 0xFF).sum()) <= rows * (K // 32)


def _model(p, t):
    """float32-accumulating model of the kernel (operands as given, products and sums in fp32, epilogue in fp32), before the output rounding."""
    A, B = t["A64"].float(), t["B64"].float()
    v = A @ B.T
    if t["bias"] is not None:
        v = v + t["bias"].float()
    if p.act == G.ACT_SILU:
        v = v * torch.sigmoid(v)
    if t["gate_rows"] is not None:
        v = t["gate_rows"].float() * v
    if t["res"] is not None:
        v = v + t["res"].float()
    return v


def _truncate_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


_SELF = [G.P(129, 136, 200), G.P(129, 136, 200, out="f32"), G.P(129, 136, 200, ab="split", out="f32"), G.P(257, 264, 192, "dgrad"), G.P(264, 264, 320, "wgrad", out="f32"),
         G.P(129, 136, 192, out="f32", bias=True, gate=50), G.P(129, 136, 192, bias=True, act=G.ACT_SILU), G.P(129, 8, 512)]


@pytest.mark.parametrize("p", _SELF, ids=lambda p: p.tag())
def test_comparator_passes_the_fp32_model_and_fails_every_damage(p):
    t = G.build(p, "random", 0, "cpu")
    ref, det, rnd = G.reference(p, t)["out"]
    dt = torch.bfloat16 if p.out == "bf16" else torch.float32
    model = _model(p, t)
    r = G.ratios(model.to(dt), ref, det, rnd)
    print(f"[comparator] {p.tag()}: fp32 model elem {r['el']:.3f} row {r['row']:.3f} col {r['col']:.3f} bias {r['bias']}")
    assert G.verdict(r) == [], r
    row, k0 = p.M - 2, 64
    # one K tile dropped from one row
    lost = dict(t, A64=t["A64"].clone())
    lost["A64"][row, k0:k0 + 64] = 0
    out = model.clone()
    out[row] = _model(p, lost)[row]
    r = G.ratios(out.to(dt), ref, det, rnd)
    print(f"[comparator] {p.tag()}: lost K tile -> row {r['row']:.1f} elem {r['el']:.1f}")
    assert "row" in G.verdict(r) and "el" in G.verdict(r) and r["at"][2] == row and r["at"][0] == row, r
    # one row replaced by its neighbour
    out = model.clone()
    out[row] = model[row - 1]
    r = G.ratios(out.to(dt), ref, det, rnd)
    print(f"[comparator] {p.tag()}: duplicated row -> row {r['row']:.1f} elem {r['el']:.1f}")
    assert "row" in G.verdict(r) and "el" in G.verdict(r) and r["at"][2] == row and r["at"][0] == row, r
    # the last column accumulated twice
    out = model.clone()
    out[:, -1] = 2 * model[:, -1]
    r = G.ratios(out.to(dt), ref, det, rnd)
    print(f"[comparator] {p.tag()}: column added twice -> col {r['col']:.1f} elem {r['el']:.1f}")
    assert "col" in G.verdict(r) and "el" in G.verdict(r) and r["at"][3] == p.N - 1 and r["at"][1] == p.N - 1, r
    # a bf16 output truncated instead of rounded: below the three norm bars by construction, caught by the rounding-bias bar
    if dt == torch.bfloat16:
        r = G.ratios(_truncate_bf16(model), ref, det, rnd)
        print(f"[comparator] {p.tag()}: truncated -> bias {r['bias']:.1f} (elem {r['el']:.3f} row {r['row']:.3f})")
        assert "bias" in G.verdict(r), r


def test_integer_family_is_exact_in_fp32_and_the_exactness_check_sees_one_wrong_element():
    for p in (G.P(129, 136, 72, out="f32"), G.P(129, 136, 72), G.P(129, 136, 192, out="f32", bias=True, gate=50)):
        t = G.build(p, "integer", 0, "cpu")
        ref = G.reference(p, t)["out"][0]
        out = _model(p, t).to(torch.bfloat16 if p.out == "bf16" else torch.float32)
        wrong, of = G.exact_mismatches(out, ref)
        assert wrong == 0 and (of == ref.numel() or p.out == "bf16") and of > 0.9 * ref.numel()
        out[5, 7] += 1
        assert G.exact_mismatches(out, ref)[0] == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sentinel_check_reports_one_changed_byte_outside_the_window(dtype):
    o = G.Out(9, 16, dtype, True, "cpu")
    assert o.win.shape == (9, 16) and o.big.shape == (9 + 2 * G.GUARD, 24) and bool(torch.isnan(o.big.float()).all())
    o.snapshot()
    o.win.zero_()                                                   # writes inside the window are not reported
    assert o.touched() == ([], 0)
    es = o.big.element_size()
    for r, b in ((G.GUARD - 1, 0), (G.GUARD + 9, 3), (G.GUARD + 4, 16 * es), (0, 24 * es - 1)):      # row before, row behind, first byte right of the window, a corner
        o.big.view(torch.uint8)[r, b] ^= 1
        assert o.touched() == ([(r, b)], 1)
        o.big.view(torch.uint8)[r, b] ^= 1
    assert o.touched() == ([], 0)
