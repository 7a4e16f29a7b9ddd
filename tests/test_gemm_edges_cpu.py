"""What tests/test_gemm_edges_gpu.py relies on, checked without a GPU: the planner's code (and zero mask) for every launch of the sweep, so that a
planner change that would move a GPU case to another kernel shows before anyone has a GPU; and the comparator itself -- a float32-accumulating CPU
model of a case's inputs passes the bars, a damaged output fails them on the row, column or element the damage touches, a changed byte outside an
output's window is reported.  For the convolution launches also: the test's float64 gather against torch.nn.functional.conv2d, damages particular
to an implicit GEMM (a tap from the neighbouring pixel, a missed kernel-row jump, the wrong mode-2 origin, the previous image's rows), and the
planner's refusals (C not a multiple of 64, an operand of 4 GiB, a caller split-K)."""
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
    conv = [l for l in G.LAUNCHES if any(p.conv is not None for p in l.probs)]
    assert all(p.conv is not None for l in conv for p in l.probs) and {l.family for l in conv} == set(G.CONV_FAMILIES)
    assert {(l.family, l.plan, l.budget) for l in conv} == {("conv dma128", 0, 0), ("conv dma256", 2, 64), ("conv 8p", 258, 64)}
    p8 = [l for l in conv if l.family == "conv 8p"]
    # the 8-phase CONV instantiation: all three epilogues in both modes, cseg_len = 3 / 6 / 9, a second and third tile per workgroup, a grouped launch
    assert {(p.conv[0], p.out, p.bias, p.residual) for l in p8 for p in l.probs} == {(m, o, True, r) for m in (1, 2) for o, r in (("bf16", False), ("f32", False), ("f32", True))}
    assert {p.conv[4] for l in p8 for p in l.probs} == {64, 128, 192} and any(len(l.probs) == 2 and l.probs[0].conv[3:] != l.probs[1].conv[3:] for l in p8)
    assert any((p.M + 255) // 256 * ((p.N + 255) // 256) == 108 and l.budget == 64 for l in p8 for p in l.probs)      # 108 tiles on 64 workgroups
    assert {p.M for l in p8 for p in l.probs} >= {1537, 1536, 1535, 1567, 1569, 1663, 1665, 2817} and {p.N for l in p8 for p in l.probs} >= {1288, 1280, 1272}
    d256 = [p for l in conv if l.family == "conv dma256" for p in l.probs]
    assert any(p.act == G.ACT_SILU for p in d256) and any(p.out == "bf16" and p.residual for p in d256) and any(p.aux for p in d256)
    assert {p.conv[:4] for l in conv if l.family == "conv dma128" for p in l.probs} == {(1, 1, 1, 1), (1, 3, 5, 17), (1, 1, 1, 127), (1, 3, 1, 43), (1, 2, 8, 8),
                                                                                     (2, 2, 2, 2), (2, 3, 10, 34)}
    assert all(l.is_edge() for l in conv if l.probs[0].M % 256 in (1, 255) or l.probs[0].N % 256 == 8)
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


def _plan_of(p, budget=0):
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    launch = G.L("pin", None, p, budget=budget)
    return _lib.lib().mmdit_gemm_plan(G.fake_args(_lib.GemmArgs, launch), 1)


def test_planner_refuses_conv_channels_off_the_k_tile_a_4gib_operand_and_a_caller_split():
    """K = 9 C must be a multiple of the 64-wide K tile, so C = 32 and C = 96 are refused (mmdit_hip.h: conv_C % 64 == 0); the DMA kernels address
    the operand with a 32-bit byte offset, so B (H + 2) (W + 2) C 2 >= 2^32 is refused and one image column less is accepted (gemm.hip plan_gemm);
    a caller split_k > 1 is refused for every convolution -- the sweep therefore has no split-K convolution launch: one that plans must be added."""
    assert _plan_of(G.PC(8, 1, 1, 4, 4, 64)) == 0 and _plan_of(G.PC(8, 2, 1, 4, 4, 128)) == 0
    for C in (32, 96):
        for mode in (1, 2):
            assert _plan_of(G.PC(8, mode, 1, 4, 4, C)) == -1, (mode, C)
    assert 2 * 4096 * 4096 * 64 * 2 == 1 << 32
    assert _plan_of(G.PC(8, 1, 2, 4094, 4094, 64)) == -1
    assert _plan_of(G.PC(8, 1, 2, 4094, 4093, 64)) >= 0                       # 2^32 - 2^20 bytes
    assert _plan_of(G.PC(8, 2, 2, 4094, 4094, 64)) == -1 and _plan_of(G.PC(8, 2, 2, 4094, 4092, 64)) >= 0
    assert _plan_of(G.PC(1288, 1, 1, 29, 53, 64, out="f32"), 64) == 258 and _plan_of(G.PC(1288, 1, 1, 29, 53, 64, out="f32", split_k=2), 64) == -1
    assert _plan_of(G.PC(40, 1, 3, 5, 17, 64, out="f32", split_k=3)) == -1


@pytest.mark.parametrize("mode", [1, 2])
def test_conv_gather_equals_conv2d_in_float64(mode):
    """The test's own restatement of the implicit GEMM's addressing against torch.nn.functional.conv2d on the unpadded interior (non-square,
    three images), so that it cannot share an addressing mistake with the kernel."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(11 + mode)
    B, C, H, W, N = 3, 8, 6, 10, 5
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(N, C, 3, 3, generator=g, dtype=torch.float64)
    xp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    A = G.conv_gather(xp, mode)
    ref = F.conv2d(x, w, padding=1) if mode == 1 else F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    assert A.shape == (B * ref.shape[2] * ref.shape[3], 9 * C)
    got = A @ w.permute(0, 2, 3, 1).reshape(N, -1).T
    want = ref.permute(0, 2, 3, 1).reshape(-1, N)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # and the operand builder: dense, the border exactly zero, the poison family's spare rows NaN behind it
    p = G.PC(8, mode, 2, 4, 6, 64)
    xo = G.conv_operand(p, torch.ones(2, 4, 6, 64, dtype=torch.bfloat16), True)
    assert xo.is_contiguous() and float(xo.float().sum()) == 2 * 4 * 6 * 64 and float(xo[:, 1:-1, 1:-1].float().min()) == 1.0


def _row_ratios(out, ref, det, rnd):
    """ratios()' per-row figure for every row."""
    return (out.double() - ref).norm(dim=1) / (det + rnd).norm(dim=1).clamp_min(G.TINY)


_CONV_SELF = [G.PC(136, 1, 3, 5, 17, 64, out="f32", bias=True), G.PC(136, 2, 3, 10, 34, 64), G.PC(136, 1, 3, 5, 17, 128)]


@pytest.mark.parametrize("p", _CONV_SELF, ids=lambda p: p.tag())
def test_comparator_fails_every_convolution_damage_on_the_rows_it_touches(p):
    """Damages particular to an implicit GEMM, each applied to the float32 model of one case (255 output rows: two 128-row tiles, 85 pixels per
    image): exactly the rows the damage touches fail the per-row and the per-element bar, the undamaged model passes."""
    t = G.build(p, "random", 0, "cpu")
    ref, det, rnd = G.reference(p, t)["out"]
    dt = torch.bfloat16 if p.out == "bf16" else torch.float32
    mode, B, H, W, C = p.conv
    hw = p.M // B
    model = _model(p, t)
    r = G.ratios(model.to(dt), ref, det, rnd)
    assert G.verdict(r) == [] and float(_row_ratios(model.to(dt), ref, det, rnd).max()) == r["row"], r

    def check(A_damaged, rows, what):
        out = _model(p, dict(t, A64=A_damaged)).to(dt)
        rr = _row_ratios(out, ref, det, rnd)
        el = ((out.double() - ref).abs() / (det + rnd).clamp_min(G.TINY)).amax(1)
        hit = torch.zeros(p.M, dtype=torch.bool)
        hit[rows] = True
        print(f"[comparator] {p.tag()}: {what} -> damaged rows: row ratio >= {float(rr[hit].min()):.1f}, elem >= {float(el[hit].min()):.1f}; others row <= {float(rr[~hit].max()) if (~hit).any() else 0:.3f}")
        assert bool((rr[hit] > G.ROW_BAR).all()) and bool((el[hit] > G.ELEM_BAR).all()), what
        assert not (~hit).any() or (float(rr[~hit].max()) <= G.ROW_BAR and float(el[~hit].max()) <= G.ELEM_BAR), what
        v = G.verdict(G.ratios(out, ref, det, rnd))
        assert "row" in v and "el" in v, (what, v)

    A = t["A64"]
    # one tap (kh = 1, kw = 2) of one output row taken from the neighbouring pixel
    row, tap = hw + 7, 5
    d = A.clone()
    d[row, tap * C:(tap + 1) * C] = A[row + 1, tap * C:(tap + 1) * C]
    check(d, [row], "one tap from the neighbouring pixel")
    # the kernel-row jump missed in the second 128-row tile: kh = 1, 2 read from kh = 0's image row
    d = A.clone()
    d[128:, 3 * C:6 * C] = A[128:, :3 * C]
    d[128:, 6 * C:] = A[128:, :3 * C]
    check(d, list(range(128, p.M)), "kernel-row jump missed in one tile")
    # the last rows of image 1 computed from image 0
    d = A.clone()
    d[2 * hw - 5:2 * hw] = A[hw - 5:hw]
    check(d, list(range(2 * hw - 5, 2 * hw)), "last rows of image b from image b - 1")
    if mode == 2:      # origin o = 0 instead of 1: the gather of mode 1 at stride 2
        xp = t["kw"]["A"].double()
        yo, xo = 2 * torch.arange(H // 2), 2 * torch.arange(W // 2)
        d = torch.stack([xp[:, (yo + kh)[:, None], (xo + kw)[None, :], :] for kh in range(3) for kw in range(3)], 3).reshape(p.M, p.K)
        check(d, list(range(p.M)), "o = 0 instead of 1 for mode 2")


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
