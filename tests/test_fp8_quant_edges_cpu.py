"""What tests/test_fp8_quant_edges_gpu.py relies on, checked without a GPU: its integer e4m3 encoder equals torch.float8_e4m3fn's cast on every finite
bf16 value at several scales and inverts its decoder; its E8M0 rule is the sentence of mmdit_hip.h in exact arithmetic; its scale-byte layout is
ops.mx_scales_to_rows; every input family meets its precondition; the planner sends every SwiGLU launch of the sweep to the kernel the sweep names; and
each planted fault of the REFERENCE changes its answer on a case of the sweep (a fault that changes nothing means the inputs are wrong, not the bar)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # (the sweep's reference, families and comparator live in the GPU module next to this file)
import test_fp8_quant_edges_gpu as Q  # noqa: E402

G = Q.G
F32, F64 = np.float32, np.float64
DTYPES = ("bf16", "f32")


def _finite_bf16():
    x = (np.arange(65536, dtype=np.uint32) << 16).view(F32)
    return x[np.isfinite(x)]


# ---------------------------------------------------------------------------------------------- the reference against torch and against the header
def test_encoder_equals_torch_float8_cast():
    x = _finite_bf16()
    assert len(x) == 65536 - 2 * 128
    for scale in (1.0, 2.0 ** -7, 3.0, 1 / 3, 2.0 ** 100, 2.0 ** -100):
        with np.errstate(over="ignore", under="ignore"):
            t = Q.clamp448((x * F32(scale)).astype(F32))
        want = torch.from_numpy(t).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        got = Q.e4m3_encode(t.astype(F64))
        assert int((got != want).sum()) == 0, scale
    assert Q.e4m3_encode(np.array([0.0, -0.0])).tolist() == [0x00, 0x80]


def test_decode_then_encode_is_the_identity():
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)
    assert len(codes) == 254
    assert np.array_equal(Q.e4m3_encode(Q.e4m3_decode(codes)), codes)
    want = torch.from_numpy(np.arange(256, dtype=np.uint8)).view(torch.float8_e4m3fn).double().numpy()
    assert np.array_equal(np.isnan(want), np.isnan(Q.E4M3)) and np.array_equal(np.isnan(Q.E4M3), (np.arange(256) & 0x7F) == 0x7F)
    assert np.array_equal(want[~np.isnan(want)], Q.E4M3[~np.isnan(want)]) and np.array_equal(np.signbit(want), np.signbit(Q.E4M3))


def _all_amax():
    out = [from_fam for dt in DTYPES for from_fam in (Q.block_amax(Q.lay_out(Q.binade_blocks(dt, 0, 254)[0], 128)).ravel(),)]
    out += [Q.block_amax(Q.lay_out(b, 128)).ravel() for dt in DTYPES for b in Q.mx_families(dt).values()]
    return np.unique(np.concatenate(out))


def test_exponent_rule_is_the_headers_sentence():
    """mx_exponent_ref gives the smallest e in [-127, 127] with amax <= 448 * 2^e (float64 holds both sides exactly) on every amax of the sweep."""
    amax = _all_amax()
    assert len(amax) > 255 * 28
    e = Q.mx_exponent_ref(amax)
    a64 = amax.astype(F64)
    assert int(e.min()) == -127 and int(e.max()) == 120
    assert bool((a64 <= 448.0 * np.ldexp(1.0, e)).all())
    assert bool(((e == -127) | (a64 > 448.0 * np.ldexp(1.0, e - 1))).all())
    assert int(Q.mx_exponent_ref(np.array([0.0], dtype=F32))[0]) == -127 and int(Q.mx_exponent_ref(np.array([np.inf], dtype=F32))[0]) == 120


def _comparison_rule(amax):
    """The comparison mx_exponent used before this sweep: 448 * 2^ex with 2^ex built from exponent field max(ex + 127, 0)."""
    b = Q.bits32(amax).astype(np.int64)
    ex = ((b >> 23) & 0xFF) - 135
    two = (np.maximum(ex + 127, 0) << 23).astype(np.uint32).view(F32)
    with np.errstate(over="ignore"):
        ex = ex + (amax > F32(448) * two)
    return np.clip(ex, -127, 127)


def test_the_comparison_rule_deviated_at_field_8_only():
    """Emulated in numpy: the former comparison differs from the header's rule exactly on 0 < amax, exponent field 8, mantissa <= 1.75."""
    amax = np.concatenate([_all_amax(), np.array([np.inf], dtype=F32)])      # (+inf: 448 * 2^120 overflows, inf > inf is false -- field 255's exponent in both)
    b = Q.bits32(amax).astype(np.int64)
    differs = _comparison_rule(amax) != Q.mx_exponent_ref(amax)
    want = ((b >> 23) == 8) & ((b & 0x7FFFFF) <= 0x600000)
    assert np.array_equal(differs, want) and int(want.sum()) >= 2 + 6
    assert set((_comparison_rule(amax) - Q.mx_exponent_ref(amax))[differs].tolist()) == {1}


def test_layout_is_ops_mx_scales_to_rows():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops
    rng = np.random.default_rng(0)
    for rows in Q.MX_ROWS + (384, 385):
        for K in (64, 128, 192, 256):
            r, b = np.meshgrid(np.arange(rows), np.arange(K // 32), indexing="ij")
            idx = Q.mx_scale_index(r, b, rows)
            n = Q.mx_scale_bytes(rows, K)
            assert n == ops.mx_scale_bytes(rows, K)
            assert len(np.unique(idx)) == idx.size and int(idx.min()) >= 0 and int(idx.max()) < n - 512
            v = rng.integers(0, 256, (rows, K // 32)).astype(np.uint8)
            arena = np.full(n, 0xFF, dtype=np.uint8)
            arena[idx] = v
            assert np.array_equal(ops.mx_scales_to_rows(torch.from_numpy(arena), rows, K).numpy(), v), (rows, K)
            if rows > 32 and K == 128:
                assert not np.array_equal(Q.mx_scale_index(r, b, rows, "swap"), idx)


# ---------------------------------------------------------------------------------------------- the families
@pytest.mark.parametrize("dtype", DTYPES)
def test_binade_family(dtype):
    blocks, f, m = Q.binade_blocks(dtype, 0, 254)
    assert set(f.tolist()) == set(range(255))
    main, extra = Q.binade_mantissas(dtype)
    assert main[:2] == [0, 0x600000] and (len(extra) >= 24 or dtype == "bf16")
    above = Q.from_bits([(8 << 23) | main[2]])[0]
    step = 2.0 ** (-119 - (7 if dtype == "bf16" else 23))
    assert float(above) == 1.75 * 2.0 ** -119 + step and main[3] == (0x7F0000 if dtype == "bf16" else 0x7FFFFF)       # the next value above 1.75, the largest mantissa
    for field in (0, 8, 254):
        for mant in main:
            sel = (f == field) & (m == mant)
            where = {(int(np.argmax(np.abs(b) == np.abs(b).max())), bool(np.signbit(b[np.argmax(np.abs(b) == np.abs(b).max())]))) for b in blocks[sel]}
            assert where == {(p, s) for p in (0, 7, 8, 31) for s in (False, True)} or (field == 0 and mant == 0), (field, mant, where)
    amax = np.abs(blocks).max(-1)
    assert np.array_equal(Q.bits32(amax), ((f << 23) | m).astype(np.uint32))
    assert np.array_equal(Q.chop(blocks, dtype).view(np.uint32), blocks.view(np.uint32))
    # the other elements land in e4m3's subnormal range and on zero once the block is scaled (wherever the fp32 range leaves room below amax)
    codes, e = Q.mx_ref(Q.lay_out(blocks, 128))
    codes = codes.reshape(-1, 32)[:len(blocks)] & 0x7F
    room = f >= 40
    assert bool(((codes > 0) & (codes < 8)).any(-1)[room].all()) and bool(((codes == 0).sum(-1) >= 4)[room].all())
    assert bool(((codes >= 8).sum(-1) == 1)[room].all())                                     # amax alone is a normal e4m3 number


@pytest.mark.parametrize("dtype", DTYPES)
def test_other_mx_families(dtype):
    fam = Q.mx_families(dtype)
    mid, even = Q.midpoints()
    assert len(mid) == 126 and mid[0] == 2.0 ** -10 and mid[-1] == 432.0
    assert np.array_equal(mid, (Q.E4M3[:0x7E] + Q.E4M3[1:0x7F]) / 2) and bool((even % 2 == 0).all())
    assert np.array_equal(Q.e4m3_encode(mid), even) and np.array_equal(Q.e4m3_encode(-mid), even | 0x80)      # the even neighbour, either sign
    assert np.array_equal(np.abs(Q.e4m3_decode(even) - mid), np.abs(Q.e4m3_decode(np.where(even == np.arange(0x7E), even + 1, even - 1).astype(np.uint8)) - mid))
    ties = fam["ties"].astype(F64)
    per = len(ties) // len(Q.TIE_SCALES)
    for i, e in enumerate(Q.TIE_SCALES):
        blk = ties[i * per:(i + 1) * per]
        assert bool((blk[:, 0] == np.ldexp(448.0, e)).all())
        vals = np.ldexp(blk[:, 1:], -e).ravel()
        assert set(vals.tolist()) == set(mid.tolist()) | set((-mid).tolist())
        assert bool((Q.mx_exponent_ref(Q.block_amax(fam["ties"][i * per:(i + 1) * per].reshape(-1, 32)).ravel()) == e).all())
    z = fam["zero"]
    assert not z.any() and not np.signbit(z[0]).any() and np.signbit(z[1]).all() and np.signbit(z[2]).any() and not np.signbit(z[2]).all()
    codes, e = Q.mx_ref(Q.lay_out(z, 32 * 3))
    assert bool((e == -127).all()) and set(codes[0, :32].tolist()) == {0x00} and set(codes[0, 32:64].tolist()) == {0x80}
    den = fam["denormal"]
    fields = (Q.bits32(den) >> 23) & 0xFF
    amax_field = (Q.bits32(np.abs(den).max(-1)) >> 23) & 0xFF
    assert bool((amax_field == 0).any()) and bool(((amax_field > 0) & ((fields == 0).sum(-1) >= 20)).any()) and 8 not in amax_field.tolist()
    assert bool((np.abs(den).max(-1) > 0).all())
    top = 0x7F7FFFFF if dtype == "f32" else 0x7F7F0000
    assert bool((Q.bits32(np.abs(fam["top"]).max(-1)) == top).all())
    mag = np.log2(np.abs(fam["random"]).max(-1))
    assert mag.min() < -17 and mag.max() > 17 and bool(np.isfinite(fam["random"]).all())
    for name, b in fam.items():
        amax = Q.block_amax(b.reshape(-1, 32))
        assert 8 not in ((Q.bits32(amax) >> 23) & 0xFF).tolist() or name == "random", name      # (the field-8 interval belongs to the binade cases alone)
    b = Q.bits32(Q.block_amax(Q.shape_pool(dtype).reshape(-1, 32)))
    assert not bool((((b >> 23) & 0xFF) == 8).any())


def test_mx_shapes_sit_on_the_workgroup_edges():
    counts = {rows * (K // 32) for rows in Q.MX_ROWS for K in Q.MX_K}
    assert {254, 256, 258, 510, 512, 514} <= counts and {1, 127, 128, 129} <= set(Q.MX_ROWS)
    pool = Q.shape_pool("bf16")
    x = Q.shape_values(pool, 257, 192)
    e = Q.mx_ref(x)[1]
    assert len(np.unique(e)) > 30 and bool((e[:32] != e[32:64]).any())      # scales differ between 32-row groups: a layout mix-up shows


@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_families(dtype):
    assert Q.AMAX_CAP == 1024 * 256 * 8 and Q.QUANT_CAP == 4096 * 256 * 8 and {8, 16, 2040, 2048, 2056, 6136, 6152} == set(Q.TENSOR_N)
    for n in Q.TENSOR_N:
        fam = Q.tensor_families(n, dtype, seed=n)
        for name, (x, preset) in fam.items():
            assert x.shape == (n,) and np.array_equal(Q.chop(x, dtype).view(np.uint32), x.view(np.uint32)), (n, name)
        assert int(np.argmax(np.abs(fam["max first8"][0]))) < 8 and int(np.argmax(np.abs(fam["max last8"][0]))) >= n - 8
        assert fam["max first8"][0].min() == -64.0 == -Q.tensor_amax(fam["max last8"][0])
        assert not fam["zero"][0].any() and 0 < Q.tensor_amax(fam["tiny"][0]) < 1e-29
        assert fam["preset"][1] > Q.tensor_amax(fam["preset"][0]) and Q.tensor_amax(*fam["preset"]) == fam["preset"][1]
        codes, scale = Q.tensor_ref(*[fam["zero"][0], Q.tensor_amax(fam["zero"][0])])
        assert not codes.any() and scale == F32(1e-12) / F32(448)
        mid, even = Q.midpoints()
        for k in (0, -7):
            x = fam[f"ties 2^{k}"][0]
            a = Q.tensor_amax(x)
            assert float(a) == 448.0 * 2.0 ** k and float(F32(448) / a) == 2.0 ** -k
            if n >= 253:
                assert set(np.ldexp(x.astype(F64), -k).tolist()) == {448.0} | set(mid.tolist()) | set((-mid).tolist())
                assert not bool((Q.tensor_ref(x, a)[0][x != a] & 1).any())
    fam = Q.tensor_families(Q.AMAX_CAP + 8, "bf16", seed=1, only=["max last8", "max stride-end"])
    assert int(np.argmax(np.abs(fam["max last8"][0]))) >= Q.AMAX_CAP and Q.AMAX_CAP - 8 <= int(np.argmax(np.abs(fam["max stride-end"][0]))) < Q.AMAX_CAP


def test_delayed_sequence():
    assert len(Q.DELAYED_N) == len(Q.DELAYED_AMP) >= 7 and {Q.AMAX_CAP - 8, Q.AMAX_CAP + 8} <= set(Q.DELAYED_N) and all(n % 8 == 0 for n in Q.DELAYED_N)
    a = Q.DELAYED_AMP
    assert a[0] < a[1] < 1.1 * a[0] and 1.1 * a[1] < a[2] < 1.5 * a[1] and a[3] > 1.5 * a[2] and a[4] < a[3] and a[5] < a[4]
    state = np.array([1.0, 0.0, 7.0, 0.0], dtype=F32)
    x = np.array([0.5, -1.25, 2.0, 0.0] * 2, dtype=F32)
    codes, new = Q.delayed_ref(x, state, 0, 1.5)
    assert new.tolist() == [1.0, 2.0, 0.0, float(F32(1.5) / F32(448))] and codes[2] == 0x7E and codes[1] == Q.e4m3_encode([-1.25 * float(F32(448) / F32(1.5))])[0]


def test_nonfinite_values():
    for dtype in DTYPES:
        x = Q.nonfinite_block_values(dtype)
        assert np.isposinf(x[0, 5]) and np.isneginf(x[1, 40]) and np.isnan(x[2, 31]) and np.isnan(x[3, 32]) and np.signbit(x[3, 32]) and not np.signbit(x[2, 31])
        assert int(np.isnan(x).sum()) == 3 + 32 and int(np.isinf(x).sum()) == 4
        codes, e = Q.mx_ref(x)
        assert not bool(((codes & 0x7F) == 0x7F).any())


# ---------------------------------------------------------------------------------------------- the planner
def test_every_swiglu_mx_out_launch_goes_to_the_8_phase_kernel():
    """The SwiGLU epilogue that leaves as MX codes is spelled in gemm_tile.h and in gemm8p.hip; the product library's planner sends every such launch to
    the latter (plan 258), at the sweep's shapes and at a workload shape, whatever the CU budget: the sweep covers the kernel that runs."""
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    lib = _lib.lib()
    for M, h, K in Q.SWIGLU_SHAPES + [(16384, 3072, 768), (4096, 1536, 384)]:
        for budget in (0, 64, 128):
            arr = G.fake_args(_lib.GemmArgs, Q.swiglu_launch(M, h, K, budget))
            arr[0].c_dtype, arr[0].ldc, arr[0].c_scales = G._FP8, h, 1 << 40
            assert lib.mmdit_gemm_plan(arr, 1) == Q.SWIGLU_PLAN, (M, h, K, budget)
    assert {M for M, _, _ in Q.SWIGLU_SHAPES} == {1, 127, 129, 257} and {h for _, h, _ in Q.SWIGLU_SHAPES} == {128, 384} and {K for _, _, K in Q.SWIGLU_SHAPES} == {128, 256}


# ---------------------------------------------------------------------------------------------- planted faults of the reference
def test_each_planted_fault_changes_the_reference_on_the_sweep():
    """The GPU sweep asks for bit equality with the reference, so a single mutation of the reference that changes its answer on a case of the sweep is a
    kernel fault the sweep would catch.  The two faults that stay inside valid e4m3 / E8M0 output also fail the float64 bars."""
    # 1. truncate instead of round to nearest even
    for dtype in DTYPES:
        fam = Q.mx_families(dtype)
        for name in ("ties", "random"):
            x = Q.lay_out(fam[name], 128)
            assert not np.array_equal(Q.mx_ref(x, fault="truncate")[0], Q.mx_ref(x)[0]), name
        x = Q.lay_out(fam["random"], 128)
        codes, e = Q.mx_ref(x, fault="truncate")
        failures = []
        Q.mx_bars(x, 128, codes, (e + 127).astype(np.uint8), failures, "", "planted")
        assert len(failures) == 1 and "per element" in failures[0]
        ok = []
        Q.mx_bars(x, 128, *[Q.mx_ref(x)[0], (Q.mx_ref(x)[1] + 127).astype(np.uint8)], ok, "", "planted")
        assert not ok
        xs, _ = Q.tensor_families(2056, dtype, seed=2056)["random"]
        a = Q.tensor_amax(xs)
        codes, scale = Q.tensor_ref(xs, a, fault="truncate")
        assert not np.array_equal(codes, Q.tensor_ref(xs, a)[0])
        failures, ok = [], []
        Q.tensor_bar(xs, codes, scale, failures, "", "planted")
        Q.tensor_bar(xs, Q.tensor_ref(xs, a)[0], scale, ok, "", "planted")
        assert failures and not ok
    # 2. the exponent rule off by one at mantissa 1.75
    for dtype in DTYPES:
        blocks, f, m = Q.binade_blocks(dtype, 100, 101)
        x = Q.lay_out(blocks, 128)
        codes, e = Q.mx_ref(x, fault="exp175")
        assert int((e != Q.mx_ref(x)[1]).sum()) == int((m == 0x600000).sum()) > 0
        failures = []
        Q.mx_bars(x, 128, codes, (e + 127).astype(np.uint8), failures, "", "planted")
        assert len(failures) == 1 and "448 2^(e-1)" in failures[0]
    # 3. the last 8 elements of a capped launch dropped: the amax pass misses the largest element, the quantiser leaves 8 bytes of 0xFF
    n = Q.AMAX_CAP + 8
    x, _ = Q.tensor_families(n, "bf16", seed=n, only=["max last8"])["max last8"]
    assert Q.tensor_amax(x[:-8]) != Q.tensor_amax(x)
    assert bool(((Q.tensor_ref(x[-8:], Q.tensor_amax(x))[0] & 0x7F) != 0x7F).all())
    # 4. two 32-row groups of the scale layout swapped
    x = Q.shape_values(Q.shape_pool("bf16"), 33, 64)
    codes, e = Q.mx_ref(x)

    class Arena:
        def __init__(self, n):
            self.n = n

        def expected(self):
            return np.full(2 * Q.LEAD + self.n, Q.FILL, dtype=np.uint8)
    q, sc = Arena(x.size), Arena(Q.mx_scale_bytes(33, 64))
    assert not np.array_equal(Q.expected_mx_arenas(codes, e, q, sc, "swap")[1], Q.expected_mx_arenas(codes, e, q, sc)[1])
