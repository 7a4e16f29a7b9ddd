"""What tests/test_optim_edges_gpu.py relies on, checked without a GPU: the restated chunk map and path rules reach every path the sweep claims to
reach; the float64 closed forms equal torch.optim.AdamW on float64 CPU parameters behind clip_grad_norm_ over several steps; a float32 torch model
of every case, in torch's own operation order, passes all bars for every family; and each planted fault fails the bars on the element or chunk it
touches (a fault that does not fail means the inputs are wrong, not the bar)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # (the sweep's tables, references and comparator live in the GPU module next to this file)
import test_optim_edges_gpu as O  # noqa: E402

G = O.G
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def _lay():
    return O.layout("small", "cpu")


def _model(lay, d, hp, fault=None):
    """The float32 torch model of one launch: p, m, v and the bf16 shadow of the tensors that have one."""
    out, _ = O.adamw_math(d, hp, F32, fault)
    out["s"] = out["p"].to(BF)[lay.has_s]
    return out


def _verdict(lay, d, hp, fam, out):
    failures = []
    lay.load(d)
    O.check_adamw(lay, d, hp, fam, out, failures, "cpu", record=False)
    O.check_shadow(lay, out, failures, "cpu")
    O.exact_family_checks(lay, d, hp, fam, out, failures, "cpu")
    O.check_guards(lay, failures, "cpu")
    return failures


# ---------------------------------------------------------------------------------------------- coverage of the restated paths
def test_chunk_map_is_the_optimizers_own():
    """chunk_map against the arithmetic of optim.py _build_table (np.arange(0, numel, ADAMW_CHUNK) per tensor) and the binding's chunk size."""
    import numpy as np
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    assert O.CHUNK == _lib.ADAMW_CHUNK
    ns = [t.n for t in O.GRID]
    ct, co = O.chunk_map(ns)
    want_ct = np.concatenate([np.full(len(np.arange(0, n, O.CHUNK)), i) for i, n in enumerate(ns)])
    want_co = np.concatenate([np.arange(0, n, O.CHUNK) for n in ns])
    assert ct == want_ct.tolist() and co == want_co.tolist()
    assert sum(O.chunk_len(ns[t], o) for t, o in zip(ct, co)) == sum(ns)


def test_the_grid_reaches_every_adamw_path():
    lay_ns = [(t, o, O.chunk_len(t.n, o)) for t in O.GRID for o in range(0, t.n, O.CHUNK)]
    paths = {(t.place,) + O.adamw_path(t.place, n) for t, _, n in lay_ns}
    vec = {p[2:] for p in paths if p[1] == "vector"}
    assert {loads for loads, _ in vec} == {0, 1, 2}                      # n4 = 0 (tail only), one load, two loads in flight
    assert {tail for _, tail in vec} == {0, 1, 2, 3}                     # the n % 4 tail
    n4 = {n >> 2 for t, _, n in lay_ns if O.adamw_path(t.place, n)[0] == "vector"}
    assert {256, 257, 511, 512, 513, 16384} <= n4                        # n4 = 256 / 257: the switch between one and two loads; the 2048-element edge
    scalar = {p[0] for p in paths if p[1] == "scalar"}
    assert scalar == {"param+1", "grad+1", "exp_avg+1", "exp_avg_sq+1", "shadow+1"}      # each of the five misalignments alone
    assert {p[0] for p in paths if p[1] == "vector"} == {"aligned", "all+4", "noshadow", "shadow8"}
    assert any(n < O.CHUNK and o > 0 for _, o, n in lay_ns)             # a last chunk shorter than 65536
    assert any(t.n == O.CHUNK for t in O.GRID)                           # a tensor of exactly one chunk
    assert {t.n for t in O.GRID} == set(O.SIZES) and {t.place for t in O.GRID} == set(O.PLACEMENTS) and len(O.GRID) == len(O.SIZES) * len(O.PLACEMENTS)
    assert {65535, 65536, 65537, 65536 + 1027, 2 * 65536, 3 * 65536 + 5} <= set(O.SIZES)
    # the small grid the models below run on reaches the same paths except the multi-chunk ones
    small = {(t.place,) + O.adamw_path(t.place, O.chunk_len(t.n, o)) for t in O.SMALL_GRID for o in range(0, t.n, O.CHUNK)}
    assert {p[1:3] for p in small} >= {("vector", 1), ("vector", 2), ("scalar", 0)} and {p[0] for p in small if p[1] == "scalar"} == scalar


def test_the_grid_reaches_both_sumsq_paths_and_the_cast_paths():
    seen = {O.sumsq_path(t.place, O.chunk_len(t.n, o))[0] for t in O.GRID for o in range(0, t.n, O.CHUNK)}
    assert seen == {"vector", "scalar"}
    assert O.sumsq_path("aligned", O.CHUNK) == ("vector", 33) and O.sumsq_path("grad+1", O.CHUNK) == ("scalar", 256) and O.sumsq_path("aligned", 5) == ("vector", 3)
    cast = {O.cast_path(so, do, O.chunk_len(n, o)) for so, do in O.CAST_PLACES for n in O.SIZES for o in range(0, n, O.CHUNK)}
    assert {p for p, _ in cast} == {"vector", "scalar"} and {t for p, t in cast if p == "vector"} >= {0, 1, 3, 4, 5, 6, 7}
    assert {(bool((4 * so) & 15), bool((2 * do) & 15)) for so, do in O.CAST_PLACES} == {(False, False), (True, False), (False, True), (True, True)}
    assert O.cast_trips(O.CAST_N[-1]) == 2 and all(O.cast_trips(n) <= 1 for n in O.CAST_N[:-1]) and set(O.CAST_N) == {1, 7, 8, 9, 15, 2055, 4096 * 256 * 8 + 13}
    assert O.patch_trips(*O.PATCH_SHAPES[-1]) == 2 and all(O.patch_trips(*s) == 1 for s in O.PATCH_SHAPES[:-1])
    assert len(O.PATCH_PAIRS) == 4 and set(O.TE_DIMS) == {2, 254, 256, 258, 768, 1024} and {len(t) for t in O.TE_BATCHES} == {1, 3}
    assert {v for t in O.TE_BATCHES for v in t} == set(O.TE_T) and {-(-d // 256) for d in O.TE_DIMS} == {1, 2, 3, 4}
    assert set(O.CLIP_N) == {1, 255, 256, 257, 1000}


def test_the_runs_cover_the_hyper_parameters():
    runs = [hp for _, _, hp in O.ADAMW_RUNS]
    steps = set()
    for hp in runs:
        steps |= set(hp["steps"]) if isinstance(hp["steps"], tuple) else {hp["steps"]}
    assert steps == {0.0, 1.0, 9.0, 999.0, 1e6}
    assert {(hp["b1"], hp["b2"]) for hp in runs} == {(0.9, 0.999), (0.5, 0.9)}
    assert {hp["wd"] for hp in runs} == {0.0, 0.01, 0.1} and {hp["lr"] for hp in runs} == {1e-3, 0.0}
    assert {hp["entry"] for hp in runs} == {"host", "dlr", "pt"}
    coefs = {None if hp["coef"] is None else hp["coef"][0] for hp in runs if hp["coef"] is None or hp["coef"][1] == 0.0}
    assert coefs == {None, 2.0 ** -10, 0.37}
    assert {f for f, _, _ in O.ADAMW_RUNS} == {"random", "first", "epsdom", "cancel", "tiny", "zerograd", "skip"}
    assert {hp["steps"] for f, _, hp in O.ADAMW_RUNS if f == "epsdom"} == {(0.0,), 999.0}
    assert {hp["wd"] for f, _, hp in O.ADAMW_RUNS if f == "zerograd"} == {0.0, 0.01, 0.1}
    assert any(isinstance(hp["steps"], tuple) and len(hp["steps"]) == 5 for hp in runs)      # counters that differ inside one launch
    ids = [f"{f}-{t}" for f, t, _ in O.ADAMW_RUNS]
    assert len(ids) == len(set(ids))


# ---------------------------------------------------------------------------------------------- the closed forms are torch's
def test_closed_forms_equal_torch_adamw_behind_clip_grad_norm():
    """Five steps of clip_grad_norm_(1.0) + torch.optim.AdamW on float64 CPU parameters against clip_math + adamw_math (float64), state carried."""
    g = torch.Generator().manual_seed(5)
    ns = [5, 1030, 70000]
    for b1, b2, wd in ((0.9, 0.999, 0.01), (0.5, 0.9, 0.1)):
        ps = [torch.nn.Parameter(torch.randn(n, generator=g, dtype=F64)) for n in ns]
        opt = torch.optim.AdamW(ps, lr=1e-3, betas=(b1, b2), eps=1e-8, weight_decay=wd)
        mine = dict(p=torch.cat([p.detach().clone() for p in ps]), m=torch.zeros(sum(ns), dtype=F64), v=torch.zeros(sum(ns), dtype=F64))
        for step in range(5):
            grads = [torch.randn(n, generator=g, dtype=F64) * (3.0 if step % 2 else 0.01) for n in ns]
            for p, gr in zip(ps, grads):
                p.grad = gr.clone()
            flat = torch.cat(grads)
            parts = torch.stack([(c * c).sum() for c in flat.split(O.CHUNK)])
            coef, found, norm = O.clip_math(parts, None, 1.0)
            total = torch.nn.utils.clip_grad_norm_(ps, 1.0)
            assert found == 0.0 and abs(norm - float(total)) <= 1e-12 * norm
            opt.step()
            hp = O.hp_of(betas=(b1, b2), wd=wd, coef=(coef, 0.0), steps=float(step), entry="host")
            d = dict(mine, g=flat, t=torch.full((sum(ns),), step + 1.0, dtype=F64))
            mine = O.adamw_math(d, hp, F64)[0]
            got = torch.cat([p.detach() for p in ps])
            # (1e-6 in clip_math is the kernel's fp32 constant: 2.5e-14 relative on the coefficient)
            assert float((mine["p"] - got).abs().max()) <= 1e-12 and float((mine["m"] - torch.cat([opt.state[p]["exp_avg"] for p in ps])).abs().max()) <= 1e-12
            assert float((mine["v"] - torch.cat([opt.state[p]["exp_avg_sq"] for p in ps])).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------- honest models
@pytest.mark.parametrize("run", [r for r in O.ADAMW_RUNS if r[0] != "skip"], ids=lambda r: f"{r[0]}-{r[1]}")
def test_float32_model_passes_every_bar(run):
    fam, tag, hp = run
    lay = _lay()
    d = O.make_data(lay, fam, hp)
    assert _verdict(lay, d, hp, fam, _model(lay, d, hp)) == []


def test_float32_models_of_the_sums_pass():
    lay = _lay()
    for fam in ("random", "exact", "tiny"):
        d = O.make_data(lay, fam, O.hp_of())
        ref = O.sumsq_math(d, lay)
        got = O.sumsq_math(d, lay, F32)
        assert float(((got.double() - ref).abs() / O.sumsq_yard(lay, ref).clamp_min(G.TINY)).max()) <= G.ELEM_BAR
        if fam == "exact":
            assert torch.equal(got.double(), ref)
    for n in O.CLIP_N:
        for scale in O.CLIP_SCALES:
            for max_norm in O.CLIP_MAX:
                for fam, side in (("random", "above"), ("random", "below"), ("exact", "")):
                    p = O.clip_partials(n, fam, scale, side)
                    ref = O.clip_math(p, scale, max_norm)
                    total = p.double().sum().sqrt().float()
                    inv = torch.tensor(1.0 if scale is None else 1.0 / scale, dtype=F32)
                    norm = total * inv
                    clip = torch.minimum(max_norm / (norm + 1e-6), torch.tensor(1.0)) if max_norm > 0 else torch.tensor(1.0)
                    failures = []
                    O.clip_check(torch.stack([inv * clip, torch.tensor(0.0), norm]), ref, failures, "model")
                    assert failures == [], (n, scale, max_norm, fam, side, failures)
                    if fam == "exact":
                        assert float(norm) == ref[2]


def test_float32_model_of_the_time_embedding_passes():
    for dim in O.TE_DIMS:
        for tvals in O.TE_BATCHES:
            t, ts, denom = O.te_inputs(dim, tvals, "cpu")
            ref, e = O.te_fwd_math(t, ts, denom)
            for bf in (False, True):
                got = O.te_fwd_math(t, ts, denom, F32)[0]
                got = got.to(BF) if bf else got
                y = O.te_fwd_yard(ref, e, bf)
                assert float(((got.double() - ref).abs() / y).max()) <= G.ELEM_BAR and float(((got.double() - ref).norm(dim=1) / y.norm(dim=1)).max()) <= G.ROW_BAR
                wrong = ref.clone()                                         # planted: the cosine half read with the sine half's denominators
                wrong[:, dim // 2:] = (t.double() * 1000.0)[:, None].div(denom.double()[None, 0::2]).cos()
                if dim > 2 and max(tvals) >= 0.5:
                    assert float(((wrong - ref).abs() / y).max()) > G.ELEM_BAR
            dout = torch.randn(len(tvals), dim, generator=O._gen("te", dim, *tvals))
            init = torch.tensor([0.37])
            want, w, terms, e2 = O.te_bwd_math(dout, t, ts, denom, init)
            got = O.te_bwd_math(dout, t, ts, denom, init, F32)[0]
            y = O.te_bwd_yard(w, terms, e2, init, dim, len(tvals))
            assert abs(float(got) - float(want)) <= G.ELEM_BAR * y
            if max(tvals) >= 0.5:
                assert abs(float(want) - 0.37) > G.ELEM_BAR * y             # started from zero instead of init: caught


# ---------------------------------------------------------------------------------------------- planted faults
def _chunk_of(lay, place, n, last=False):
    """Flat index of the first (or last) element of the chunk of tensor (n, place) -- in the small grid every tensor of these sizes is one chunk or two."""
    k = next(i for i, t in enumerate(lay.grid) if t.n == n and t.place == place)
    idx = (lay.tid == k).nonzero()[:, 0]
    return int(idx[-1] if last else idx[0])


@pytest.mark.parametrize("place,n", [("aligned", 2052), ("param+1", 1025), ("shadow+1", 65537), ("aligned", 1), ("all+4", 2049)])
def test_planted_element_faults_fail_where_they_sit(place, n):
    """One element not updated; one element given its neighbour's gradient; the last tail element of a chunk dropped (= not updated)."""
    lay = _lay()
    hp = O.hp_of()
    d = O.make_data(lay, "random", hp)
    ref = O.adamw_math(d, hp, F64)[0]
    for fault, last in (("stale", False), ("stale", True), ("neighbour", False)):
        j = _chunk_of(lay, place, n, last)
        if fault == "neighbour" and n == 1:
            continue
        out = _model(lay, d, hp, (fault, j))
        failures = []
        lay.load(d)
        O.check_adamw(lay, d, hp, "random", out, failures, "fault", record=False)
        assert failures, (fault, place, n)
        # ... on the element it touches and nowhere else: with that element repaired the model passes again
        for k in "pmv":
            out[k][j] = ref[k][j].float()
        failures = []
        O.check_adamw(lay, d, hp, "random", out, failures, "repaired", record=False)
        assert failures == [], (fault, place, n, failures)


def test_eps_inside_the_bias_correction_fails_on_the_eps_dominated_family_only():
    lay = _lay()
    for tag, hp in [(t, hp) for f, t, hp in O.ADAMW_RUNS if f == "epsdom"]:
        d = O.make_data(lay, "epsdom", hp)
        failures = _verdict(lay, d, hp, "epsdom", _model(lay, d, hp, "eps_inside"))
        if tag == "t1":
            assert any(" p:" in f for f in failures), failures      # a factor of 30 in the update at t = 1
    hp = O.hp_of()
    d = O.make_data(lay, "random", hp)
    out = _model(lay, d, hp, "eps_inside")
    ref = O.adamw_math(d, hp, F64)[0]
    assert float((out["p"].double() - ref["p"]).norm() / ref["p"].norm()) < 2e-6      # invisible to a Frobenius bar on the random family


@pytest.mark.parametrize("fam", ["random", "first", "epsdom"])
def test_step_counter_off_by_one_fails(fam):
    lay = _lay()
    hp = next(hp for f, _, hp in O.ADAMW_RUNS if f == fam)
    d = O.make_data(lay, fam, hp)
    assert any(" p:" in f for f in _verdict(lay, d, hp, fam, _model(lay, d, hp, "t_off")))


def test_truncated_shadow_and_changed_guard_word_are_reported():
    lay = _lay()
    hp = O.hp_of()
    d = O.make_data(lay, "random", hp)
    out = _model(lay, d, hp)
    out["s"] = O.bf16_trunc(out["p"])[lay.has_s]
    failures = _verdict(lay, d, hp, "random", out)
    assert failures and all("shadow" in f for f in failures)
    out = _model(lay, d, hp)
    for k in "pgmvs":
        lay.load(d)
        a = lay.ar[k]
        word = a.starts[3] + lay.grid[3].n      # the first guard word behind a window
        a.bits()[word] ^= 1
        failures = []
        O.check_guards(lay, failures, "guard")
        assert len(failures) == 1 and f"arena {k}" in failures[0]
        a.bits()[word] ^= 1
    lay.load(d)
    lay.ar["g"].buf[lay.ar["g"].idx[7]] += 1.0          # an INPUT changed
    failures = []
    O.check_guards(lay, failures, "input")
    assert failures == ["input arena g: an input changed"]


def test_dropped_tail_element_and_missing_partial_fail_the_norm_bars():
    lay = _lay()
    d = O.make_data(lay, "exact", O.hp_of())
    ref = O.sumsq_math(d, lay)
    bad = O.sumsq_math(d, lay, F32, drop_tail=True)
    differs = bad.double() != ref
    last = torch.tensor(lay.clen).cumsum(0) - 1
    assert torch.equal(differs, d["g"][last] != 0) and int(differs.sum()) > len(lay.ct) // 2      # every chunk whose last element is non-zero
    d = O.make_data(lay, "random", O.hp_of())
    ref = O.sumsq_math(d, lay)
    bad = O.sumsq_math(d, lay, F32, drop_tail=True)
    ratio = (bad.double() - ref).abs() / O.sumsq_yard(lay, ref).clamp_min(G.TINY)
    seen = (torch.tensor(lay.clen) <= 2052) & (d["g"][last].abs() >= 0.1)      # (a dropped element of 1e-3 in 2052 of order one is below any rounding bar: the exact family carries those)
    assert bool((ratio[seen] > G.ELEM_BAR).all()) and int(seen.sum()) > len(lay.ct) // 2
    for n in O.CLIP_N[1:]:
        for scale in O.CLIP_SCALES:
            p = O.clip_partials(n, "random", scale, "above")
            for skip in (0, n // 2, n - 1):
                failures = []
                O.clip_check(torch.tensor(O.clip_math(p, scale, 1.0, skip=skip), dtype=F64), O.clip_math(p, scale, 1.0), failures, "skip")
                assert len(failures) == 2, (n, scale, skip, failures)      # out[0] and out[2]
