"""What tests/test_rowops_edges_gpu.py relies on, checked without a GPU: the restated launch arithmetic reaches every path the sweep claims to reach;
the comparator and the yardsticks -- a float32 torch model of a case's inputs (summed in torch's order, not the kernels', rounded to the output dtype)
passes all bars for every kernel family and input family, each planted fault fails them on the element, row or column it touches, a changed byte
outside an output's window is reported; and the closed-form gradients of the reference equal float64 autograd."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # (the sweep's tables, references and comparator live in the GPU module next to this file)
import test_rowops_edges_gpu as R  # noqa: E402

G = R.G
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def _of(kind):
    return [c for c in R.ALL if c.kind == kind]


# ---------------------------------------------------------------------------------------------- coverage of the restated paths
def test_every_nit_bucket_runs_with_and_without_d_equal_256_n():
    for kind in ("ln_fwd", "ln_bwd"):
        seen = {(R.nit_bucket(c.d), c.d % 256 == 0) for c in _of(kind)}
        assert seen >= {(b, e) for b in R.NIT_BUCKETS for e in (True, False)}, (kind, sorted(seen))
    seen = {(R.nit_bucket(c.d), c.d % 256 == 0) for c in _of("rms")}
    assert seen >= {(1, True), (1, False), (2, False), (4, True), (9, True), (12, False), (16, True)}, sorted(seen)
    assert {R.ln_bwd_flush(c.d) for c in _of("ln_bwd")} == {"lds", "atomics"}
    assert all(R.nit_for(c.d) <= 16 and c.d % 4 == 0 for c in R.ALL if hasattr(c, "d"))


def test_adaln_rows_cover_every_remainder_and_both_list_lengths():
    assert {(b * rpb) % 4 for c in _of("ln_fwd") for b, rpb in c.probs[-1:]} == {0, 1, 2, 3}
    assert {rpb for c in _of("ln_fwd") for _, rpb in c.probs} >= {1, 3, 17, 33}
    for kind in ("ln_fwd", "ln_bwd"):
        assert {len(c.probs) for c in _of(kind)} == {1, 2}
        assert {(c.res if kind == "ln_fwd" else c.gated, c.dt) for c in _of(kind)} == {(a, b) for a in (True, False) for b in ("bf16", "f32")}
    for flush in ("lds", "atomics"):
        assert {c.probs[-1][1] for c in _of("ln_bwd") if R.ln_bwd_flush(c.d) == flush} >= set(R.LN_BWD_RPB), flush
    assert {(c.dbias, c.dres) for c in _of("ln_bwd") if c.gated} >= {(True, True), (False, False)}


def test_one_round_rule_moves_the_two_problem_case_off_16_rows():
    probs = ((300, 40), (300, 24))
    assert sum(b * ((rpb + 15) // 16) for b, rpb in probs) == 1500 and R.ln_bwd_rch(probs, 64) == 24
    assert any(c.probs == probs and c.d == 64 for c in _of("ln_bwd"))
    assert all(R.ln_bwd_rch(c.probs, c.d) == 16 for c in _of("ln_bwd") if c.probs != probs)


def test_qk_cases_reach_fast_and_general_paths_at_rl_1_and_above():
    seen_bwd, seen_fwd = set(), set()
    for c in _of("qk"):
        rl, fast = R.qk_bwd_path(c.batch, c.heads, c.streams)
        seen_bwd.add((fast, rl > 1))
        seen_fwd |= {R.qk_fwd_path(c.batch, t, r)[1] for t, r in c.streams if r}
        assert 24 * c.heads * rl <= 1024
    assert seen_bwd == {(True, False), (True, True), (False, False), (False, True)} and seen_fwd == {True, False}
    path = {(c.batch, c.heads, c.streams[0][0]): R.qk_bwd_path(c.batch, c.heads, c.streams) for c in _of("qk") if len(c.streams) == 1}
    assert path[(1, 1, 1)] == (1, True) and path[(3, 42, 6)] == (1, True) and path[(2, 3, 24)] == (1, True) and path[(1, 1, 1056)] == (1, False)
    assert path[(16, 5, 135)] == (8, False) and path[(2, 12, 1024)] == (3, False) and path[(2, 16, 1024)] == (2, True) and path[(9, 2, 256)] == (21, False)
    assert path[(700, 1, 3)] == (42, True)
    assert R.qk_bwd_grid(2048, 1024, True, 2) == 512 and R.qk_bwd_grid(2048, 1024, True, 3) == 256 and R.qk_bwd_grid(2160, 135, True, 8) == 96
    assert R.qk_fwd_path(1, 1056, True) == (1024, False) and R.qk_fwd_path(2, 24, True) == (48, True)
    assert {c.combo for c in _of("qk")} == {0, 1, 2} and {len(c.streams) for c in _of("qk")} == {1, 2}
    assert any(c.streams[0][1] and len(c.streams) == 2 for c in _of("qk")) and any(not c.streams[0][1] and len(c.streams) == 2 for c in _of("qk"))


def test_rms_colsum_and_the_other_tables_cover_their_edges():
    rms = _of("rms")
    assert any("unequal" in c.path for c in rms) and any("halves equal" in c.path for c in rms)
    halves = {r for c in rms for r in (c.batch * c.split, c.batch * (c.tokens - c.split))}
    assert halves >= {63, 64, 65, 129}
    assert any(min(a, b) <= 64 < max(a, b) for c in rms for a, b in [(c.batch * c.split, c.batch * (c.tokens - c.split))])
    assert {(c.ti, c.tg) for c in rms} == {(a, b) for a in ("bf16", "f32") for b in ("bf16", "f32")}
    assert {(c.tokens, c.split) for c in rms} >= {(2, 1), (10, 3), (10, 7), (131, 1), (154, 77)}
    assert {R.colsum_rch(c.rows) for c in _of("colsum")} == {8, 64} and {c.rows for c in _of("colsum")} == {1, 2, 7, 8, 9, 255, 256, 257, 321}
    assert {c.cols for c in _of("colsum")} == {8, 1016, 1024, 1032} and any(c.strided for c in _of("colsum"))
    assert {r for c in _of("mlp") for r in c.rows} >= {1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129}
    assert {(c.hidden, c.gelu) for c in _of("mlp")} >= {(h, g) for h in (8, 248, 256, 264, 520) for g in (True, False)}
    assert {len(c.rows) for c in _of("mlp")} == {1, 2} and {c.dt for c in _of("mlp")} == {"bf16", "f32"}
    assert any(c.batch * c.rpb * (c.d // 4) > 4096 * 256 for c in _of("gr_fwd")) and {c.d for c in _of("gr_fwd")} >= {4, 8, 260}
    assert {c.rpb for c in _of("gr_bwd")} == {1, 7, 8, 9, 63, 64, 65, 72, 73} and {c.d for c in _of("gr_bwd")} == {8, 248, 264}
    assert {c.dbias for c in _of("gr_bwd")} == {None, "vec", "per"}
    assert {(c.cols, c.rpg) for c in _of("silu_bwd")} == {(a, b) for a in (1, 63, 64, 65) for b in (1, 3, 4, 5)} and len({c.pair for c in _of("silu_bwd")}) == 3
    assert {c.n for c in _of("flow")} == {8, 2040, 2048, 2056, 524288 + 8, 3 * 524288 + 16}
    assert any((c.n // 8 + 255) // 256 > 256 for c in _of("flow"))
    assert {(c.rows, c.width) for c in _of("mx")} == {(1, 64), (129, 320), (131, 1536)}


def test_case_ids_are_unique_and_every_family_runs():
    ids = [R._case_id(cf) for cf in R.CASES]
    assert len(ids) == len(set(ids))
    for kind, fams in R.FAMILIES.items():
        assert {f for c, f in R.CASES if c.kind == kind} == set(fams) | set(R.EDGE_FAMILIES.get(kind, ())), kind
    assert all(any(c.edge for c in _of(kind)) for kind in R.EDGE_FAMILIES)


# ---------------------------------------------------------------------------------------------- honest models
def _small(c):
    if c.kind in ("ln_fwd", "ln_bwd"):
        return sum(b * r for b, r in c.probs) * c.d <= 160000
    if c.kind == "rms":
        return c.batch * c.tokens * c.d <= 300000
    if c.kind == "qk":
        return c.batch * sum(t for t, _ in c.streams) * c.heads <= 1200
    if c.kind == "mlp":
        return sum(c.rows) * c.hidden <= 40000
    if c.kind == "gr_fwd":
        return c.d <= 260
    if c.kind == "flow":
        return c.n <= 600000
    return c.kind != "mx"


def _model(c, t, fault=None):
    """The float32 torch model of one problem, rounded to the dtype the kernel stores."""
    return {k: v.to(R.out_dtype(c, k)) for k, v in R.KIND[c.kind][1](c, t, F32, fault)[0].items()}


def _reference(c, t):
    ref, aux = R.KIND[c.kind][1](c, t, F64)
    return ref, R.KIND[c.kind][2](c, t, ref, aux)


_HONEST = [(c, f) for c, f in R.CASES if f != "poison" and c.kind != "mx" and _small(c)]


@pytest.mark.parametrize("case", _HONEST, ids=R._case_id)
def test_fp32_model_passes_all_bars(case):
    c, fam = case
    failures = []
    for i, t in enumerate(R.KIND[c.kind][0](c, fam)):
        ref, yard = _reference(c, t)
        out = _model(c, t)
        for name, (det, rnd) in yard.items():
            R.compare(c, fam, i, name, out[name], ref[name], det, rnd, failures, record=False)
    assert not failures, "\n".join([c.id + " " + fam] + failures)


def test_honest_models_cover_every_kernel_family_and_input_family():
    seen = {(c.kind, f) for c, f in _HONEST}
    assert seen == {(k, f) for k, fams in R.FAMILIES.items() if k != "mx" for f in fams} | {(k, f) for k, fams in R.EDGE_FAMILIES.items() for f in fams if f != "poison"}


# ---------------------------------------------------------------------------------------------- planted faults
def _ln_case(dt, res=False, d=260, probs=((3, 17),)):
    return R.C("ln_fwd", "", d=d, probs=probs, res=res, dt=dt)


def _ratios(c, t, out, name):
    ref, yard = _reference(c, t)
    return G.ratios(out[name], ref[name], *yard[name])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("d", [4, 260, 1024, 4096])
def test_eps_and_one_pass_variance_fail_on_the_families_built_for_them(dt, d):
    c = _ln_case(dt, d=d)
    t = R.data_ln(c, "smallvar")[0]
    r, rs = _ratios(c, t, _model(c, t, "eps"), "out"), _ratios(c, t, _model(c, t, "eps"), "rstd")
    print(f"[planted] eps = 1e-6, d = {d} {dt}: out elem {r['el']:.1f} row {r['row']:.1f}, rstd elem {rs['el']:.1f}")
    assert {"el", "row"} <= set(G.verdict(r)) and "el" in G.verdict(rs) and r["el"] > 100
    t = R.data_ln(c, "offset")[0]
    r, rs = _ratios(c, t, _model(c, t, "onepass"), "out"), _ratios(c, t, _model(c, t, "onepass"), "rstd")
    print(f"[planted] one-pass variance, d = {d} {dt}: out elem {r['el']:.1f} row {r['row']:.1f}, rstd elem {rs['el']:.1f}")
    assert "el" in G.verdict(r) and "el" in G.verdict(rs) and rs["el"] > 100 and (dt == "bf16" or "row" in G.verdict(r))      # (a bf16 row's norm is its rounding)
    # ... and both are INVISIBLE on the random family at a Frobenius bar, which is why the families exist
    t = R.data_ln(c, "random")[0]
    ref = _reference(c, t)[0]["out"]
    assert float((_model(c, t, "eps")["out"].double() - ref).norm() / ref.norm()) < (1e-5 if dt == "f32" else 4e-3)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_neighbouring_samples_modulation_row_fails_on_the_last_row_of_the_sample(dt):
    c = _ln_case(dt)
    t = R.data_ln(c, "random")[0]
    r = _ratios(c, t, _model(c, t, "wrong_b"), "out")
    assert {"el", "row"} <= set(G.verdict(r)) and r["at"][0] == 16 and r["at"][2] == 16 and r["row"] > 100, r


@pytest.mark.parametrize("dt,rpb", [("f32", 16), ("bf16", 33), ("f32", 5)])
def test_last_row_of_a_chunk_missing_from_a_column_sum_fails_on_the_sample_it_touches(dt, rpb):
    c = R.C("ln_bwd", "", d=260, probs=((2, rpb),), gated=True, dbias=True, dres=True, dt=dt)
    t = R.data_ln(c, "random")[0]
    r = _ratios(c, t, _model(c, t, "lost_row"), "dscale")
    assert {"el", "row"} <= set(G.verdict(r)) and r["at"][2] == 0 and r["row"] > 100, r
    ok = _ratios(c, t, _model(c, t), "dscale")
    assert G.verdict(ok) == [], ok


@pytest.mark.parametrize("kind_dt", [("ln_fwd", "f32"), ("ln_fwd", "bf16"), ("mlp", "bf16"), ("rms", "bf16")])
def test_duplicated_row_and_truncation_fail(kind_dt):
    kind, dt = kind_dt
    c = {"ln_fwd": _ln_case(dt, res=True), "mlp": R.C("mlp", "", hidden=264, rows=(65,), gelu=False, dt=dt, dbias=True),
         "rms": R.C("rms", "", d=260, tokens=10, split=3, batch=9, ti="f32", tg=dt)}[kind]
    name = {"ln_fwd": "out", "mlp": "h", "rms": "out2"}[kind]
    t = R.KIND[kind][0](c, "random")[0]
    ref, yard = _reference(c, t)
    model = R.KIND[kind][1](c, t, F32)[0][name]
    out = model.clone()
    row = out.shape[0] - 2
    out[row] = model[row - 1]
    r = G.ratios(out.to(R.DT[dt]), ref[name], *yard[name])
    assert {"el", "row"} <= set(G.verdict(r)) and r["at"][0] == row and r["at"][2] == row, r
    if dt == "bf16":
        trunc = (model.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)
        r = G.ratios(trunc, ref[name], *yard[name])
        print(f"[planted] {kind} truncated: bias {r['bias']:.1f} elem {r['el']:.3f} row {r['row']:.3f}")
        assert "bias" in G.verdict(r), r
        assert G.verdict(G.ratios(model.to(BF), ref[name], *yard[name])) == []


def test_exact_family_is_exact_in_fp32_and_one_wrong_element_is_reported():
    for c in [c for c in R.ALL if c.kind in ("colsum", "gr_bwd") and c.edge][:6] + [c for c in _of("gr_fwd") if c.edge]:
        t = R.KIND[c.kind][0](c, "exact")[0]
        ref, yard = _reference(c, t)
        out = _model(c, t)
        for name in yard:
            assert torch.equal(out[name].double(), ref[name]), (c.id, name)
        name = R.EXACT_NAMES[c.kind][0]
        failures = []
        out[name][-1, -1] += 1
        R.compare(c, "exact", 0, name, out[name], ref[name], *yard[name], failures, record=False)
        assert any("differ from the exact" in f for f in failures), failures


# ---------------------------------------------------------------------------------------------- guard window
@pytest.mark.parametrize("dtype", [F32, BF])
def test_window_check_reports_one_changed_byte_outside_the_window(dtype):
    w = R.Win(9, 16, dtype, True, "cpu", ld=24)
    assert w.win.shape == (9, 16) and w.big.shape == (9 + 2 * R.GUARD, 24) and bool(torch.isnan(w.big.float()).all())
    w.snapshot()
    w.win.zero_()
    assert w.touched() == ([], 0)
    es = w.big.element_size()
    for r, b in ((R.GUARD - 1, 0), (R.GUARD + 9, 3), (R.GUARD + 4, 16 * es), (0, 24 * es - 1)):
        w.big.view(torch.uint8)[r, b] ^= 1
        assert w.touched() == ([(r, b)], 1)
        w.big.view(torch.uint8)[r, b] ^= 1
    allowed = torch.zeros(9, dtype=torch.bool)
    allowed[2:5] = True
    w.snapshot()
    w.win[1, 3] = 1.0      # a row inside the window that this launch may not write (another stream's token)
    assert w.touched(allowed)[1] > 0 and w.touched()[1] == 0
    v = R.place(torch.ones(3, 5), True, 8)
    base = v._base
    assert v.shape == (3, 5) and v.stride(0) == 8 and base.shape == (3 + R.GUARD, 8) and bool(torch.isnan(base[3:]).all()) and bool(torch.isnan(base[:3, 5:]).all())


# ---------------------------------------------------------------------------------------------- the closed-form gradients are the gradients
def _leaf(x):
    return x.double().clone().requires_grad_(True)


def test_closed_form_gradients_equal_float64_autograd():
    # adaLN backward: dx, dscale, dshift of L = sum(dout * out), out = LN(x) (1 + scale) + shift (dacc / dgate / dbias are products and sums of dx)
    c = R.C("ln_bwd", "", d=12, probs=((2, 5),), gated=False, dbias=False, dres=False, dt="f32")
    t = R.data_ln(c, "random")[0]
    x, sc, sh = _leaf(t["x"]), _leaf(t["scale"]), _leaf(t["shift"])
    b = R._bidx(10, 5, "cpu")
    m = x.mean(1, keepdim=True)
    out = (x - m) * (((x - m) ** 2).mean(1, keepdim=True) + R.LN_EPS).rsqrt() * (1 + sc[b]) + sh[b]
    (out * t["dout"].double()).sum().backward()
    t64 = dict(t, mean=t["mean"].double(), rstd=t["rstd"].double())
    t64["mean"], t64["rstd"] = m.detach(), (((x - m) ** 2).mean(1, keepdim=True) + R.LN_EPS).rsqrt().detach()
    ref = R.math_ln_bwd(c, t64, F64)[0]
    assert torch.allclose(ref["dx"], x.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(ref["dscale"] - t["dscale0"].double(), sc.grad, rtol=1e-9, atol=1e-12) and torch.allclose(ref["dshift"] - t["dshift0"].double(), sh.grad, rtol=1e-9, atol=1e-12)
    # text RMSNorm: dw, ds
    c = R.C("rms", "", d=8, tokens=5, split=2, batch=3, ti="f32", tg="f32")
    t = R.data_rms(c, "random")[0]
    leaves = {k: _leaf(t[k]) for k in ("w1", "w2", "s1", "s2")}
    ref = R.math_rms(c, dict(t, **{k: v.detach() for k, v in leaves.items()}), F64)[0]
    fwd = R.math_rms(c, dict(t, **leaves), F64)[0]
    (fwd["out1"] * t["dout1"].double()).sum().backward()
    (fwd["out2"] * t["dout2"].double()).sum().backward()
    for h in (1, 2):
        assert torch.allclose(ref[f"dw{h}"][0] - t[f"dw{h}0"].double(), leaves[f"w{h}"].grad, rtol=1e-9, atol=1e-12)
        assert torch.allclose(ref[f"ds{h}"][0] - t[f"ds{h}0"].double(), leaves[f"s{h}"].grad, rtol=1e-9, atol=1e-12)
    # QK-norm + RoPE: dqkv, dwq, dwk of L = sum(dQ Q + dK K + dV V)
    c = R.C("qk", "", batch=2, heads=2, streams=((3, True),), combo=1, pad=(1, 2))
    t = R.data_qk(c, "random")[0]
    leaves = {k: _leaf(t[k]) for k in ("qkv", "wq", "wk")}
    ref = R.math_qk(c, t, F64)[0]
    fwd = R.math_qk(c, dict(t, **leaves), F64)[0]
    pick = lambda z: z.double()[:, :, 1:4].reshape(-1, 64)      # noqa: E731
    (fwd["Q"] * pick(t["dQ"]) + fwd["K"] * pick(t["dK"]) + fwd["V"] * pick(t["dV"])).sum().backward()
    assert torch.allclose(ref["dqkv"], leaves["qkv"].grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(ref["dwq"][0] - t["dwq0"].double(), leaves["wq"].grad, rtol=1e-9, atol=1e-12) and torch.allclose(ref["dwk"][0] - t["dwk0"].double(), leaves["wk"].grad, rtol=1e-9, atol=1e-12)
    # SwiGLU / GELU / SiLU backward
    for gelu in (False, True):
        c = R.C("mlp", "", hidden=8, rows=(5,), gelu=gelu, dt="f32", dbias=True)
        t = R.data_mlp(c, "random")[0]
        gu = _leaf(t["gu"])
        ref = R.math_mlp(c, t, F64)[0]
        (R.math_mlp(c, dict(t, gu=gu), F64)[0]["h"] * t["dh"].double()).sum().backward()
        assert torch.allclose(ref["dgu"], gu.grad, rtol=1e-9, atol=1e-12)
    c = R.C("silu_bwd", "", cols=5, rpg=3, groups=2, pair=("f32", "f32"), dbias=True)
    t = R.data_silu(c, "random")[0]
    p = _leaf(t["pre"])
    (torch.nn.functional.silu(p) * t["dy"].double()).sum().backward()
    assert torch.allclose(R.math_silu(c, t, F64)[0]["dpre"], p.grad, rtol=1e-9, atol=1e-12)
