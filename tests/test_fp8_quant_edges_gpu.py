"""Value- and size-edge sweep of the e4m3 quantisers through the C ABI, against an exact integer reference written here in numpy:

  mmdit_mxfp8_quantize, mmdit_mxfp8_quantize_pad                      MX: e4m3 codes + one E8M0 scale byte per 32 values (csrc/fp8_quant.h mx_quant_block,
                                                                      csrc/common.h mx_exponent / mx_pack4 / mx_scale_index)
  mmdit_fp8_amax, mmdit_fp8_quantize, mmdit_fp8_quantize_pad          per tensor, two passes (csrc/rowops.hip, csrc/fp8_pad.hip, csrc/fp8_quant.h fp8_range / fp8_pack8)
  mmdit_fp8_quantize_delayed                                          per tensor, one pass on a 4-float state
  mmdit_gemm with act = SwiGLU, c_dtype = MMDIT_FP8, c_scales         the activation leaving the GEMM epilogue as MX codes (csrc/gemm8p.hip)

Every other fp8 / mxfp8 test of the suite ends at these quantisers: the MX-emitting producers are held to byte equality with "bf16 output +
ops.quant_mxfp8", the e4m3 GEMM sweep takes the quantisers' outputs as inputs, and the quantisers themselves were compared with a torch restatement on
randn values only (test_kernels_gpu.py _mx_reference) or held to rel < 4e-2.

Reference (no ops.* call, no torch float8 cast; tests/test_fp8_quant_edges_cpu.py holds it to torch.float8_e4m3fn and to ops.mx_scales_to_rows):
  e4m3_encode     float64 -> OCP e4m3fn code, round to nearest even in integer arithmetic (the quantum of |x| is 2^(floor(log2 |x|) - 3), 2^-9 below 2^-6:
                  n = |x| / quantum is exact in float64, rounded on its fraction, and code = ((e + 7) << 3) + n - 8 carries into the next binade by itself);
                  the sign bit of the input, of a zero too.  e4m3_decode: all 256 codes.
  mx_exponent_ref the rule of mmdit_hip.h from the bit fields of amax: exponent field - 135, plus one when the mantissa bits exceed 0x600000 (1.75),
                  clamped to [-127, 127] = the smallest e in [-127, 127] with amax <= 448 * 2^e (the CPU partner checks that sentence in float64 on
                  every amax of the binade family); a zero block: -127.  +inf (no such e): field 255's 120, as the header says.
  mx_scale_index  the scale-byte layout of mmdit_hip.h (scale_mode 1), restated.
  mx_ref          t = fl32(x * 2^-e) (exact but for results below the fp32 normal range, which encode to zero either way), clamped, encoded.
  tensor_ref      the fp32 rounding points of fp8_quant.h: a = max(amax, 1e-12f), s = fl(448 / a), scale = fl(a / 448), t = fl(x s), clamp to +-448, encode;
                  delayed: a = max(fl(state[k % 3] margin), 1e-12f).  The build keeps correctly rounded fp32 division (test_optim_edges_gpu.py), numpy float32
                  reproduces these bits.  The clamp is fmaxf then fminf (np.fmax / np.fmin: a NaN operand is dropped).

Bars (derived, nothing tuned; no element is left out of any comparison):
  codes, scale bytes, amax[0], scale[0] and the delayed state[0 .. 3] are BIT-EQUAL to the reference: whole arenas are compared, so the same comparison
  holds every byte outside a window to its 0xFF fill -- code bytes before and behind, the scale bytes of the rows in [rows, rows_pad128) and the 512
  spare bytes.  Inputs come back bit-identical; the ldx - K gap between rows and the elements before and behind an input hold +-1e30 (not NaN: the
  kernels' fmaxf would ignore it), so a block that read into the gap changes its scale byte.
  MX, in float64 with e from the KERNEL's scale byte:   amax <= 448 * 2^e;   amax > 448 * 2^(e - 1) unless e = -127;
                                                        |q 2^e - x| <= max(2^-4 |x|, 2^-10 2^e) per element
  per tensor, in float64 with the KERNEL's scale:       |q scale - x| <= max(2^-4 |x|, 2^-10 scale) (1 + 2^-20) per element that does not saturate
  (one rounding to nearest at 3 mantissa bits or at half the smallest subnormal, plus three fp32 roundings; truncation reaches 2^-3 and fails.)

MX value families (each built exactly, once in bf16 and once in fp32, 32 values per block; mx_families):
  binade    amax at EVERY exponent field 0 .. 254 with mantissas 1.0, exactly 1.75, the next value above 1.75, the largest (fp32: 24 more per field), at
            element 0 / 7 / 8 / 31 with either sign; the other elements 2^-15 .. 2^-21 of it: e4m3 subnormals and zeros after scaling.
  ties      for block scales 2^-120 .. 2^118: every midpoint between adjacent e4m3 values (2^-10, half the smallest subnormal, and 432 below 448 among
            them), either sign, beside one element 448 * 2^e that fixes the scale.  5 significant bits: exact in bf16.  The result is the EVEN code.
  zero      all +0 (scale byte 0, codes 0x00), all -0 (codes 0x80), mixed.
  denormal  amax an fp32 / bf16 denormal; one normal element among denormals.
  top       amax the largest finite value of the input type.
  random    randn blocks with magnitudes 2^-20 .. 2^20.
MX shapes: rows 1, 3, 31, 32, 33, 127, 128, 129, 255, 256, 257 x K 64, 128, 192 (254 / 256 / 258 and 510 / 512 / 514 blocks around the 256-thread
workgroups) x ldx K, K + 8, K + 64, both types; mmdit_mxfp8_quantize_pad at K 64 and 192 against the same reference with zero blocks appended.

Three test ids (MX + the SwiGLU epilogue, per tensor, non-finite inputs) run the 84 cases in turn (run_cases: a failing case is reported under its own
label and does not stop the others), as test_optim_edges_gpu.py keeps one id per group of kernels.

Worst measured ratios per entry point and family, the parent commit's failing cases and the wall time of each case: profiles/fp8_quant_edge_sweep.txt.
"""
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # (the GEMM sweep's operand builder and planner arguments)
import test_gemm_edges_gpu as G  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DT = {"f32": G._F32, "bf16": G._BF16}
FILL = 0xFF                       # every output arena starts as 0xFF: the e4m3 NaN code, the E8M0 NaN scale, an fp32 NaN
LEAD = 256                        # guard bytes before and behind an output window; an input has 64 elements of +-1e30 on either side
BIG = 1e30
MX_ROWS = (1, 3, 31, 32, 33, 127, 128, 129, 255, 256, 257)
MX_K = (64, 128, 192)
TIE_SCALES = (-120, -20, -1, 0, 3, 40, 118)
AMAX_CAP, QUANT_CAP = 1024 * 256 * 8, 4096 * 256 * 8      # elements of one full grid: rowops.hip mmdit_fp8_amax / _delayed (1024 workgroups), grid_cap (4096)
TENSOR_N = (8, 16, 2040, 2048, 2056, 8 * 256 * 3 - 8, 8 * 256 * 3 + 8)
FIELD_GROUPS = ((0, 7), (8, 8), (9, 47), (48, 87), (88, 127), (128, 167), (168, 207), (208, 254))


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ---------------------------------------------------------------------------------------------- the reference
def _decode_table():
    v = np.empty(256, dtype=F64)
    for c in range(256):
        E, m = (c >> 3) & 15, c & 7
        a = np.nan if (E == 15 and m == 7) else m * 2.0 ** -9 if E == 0 else (1 + m / 8) * 2.0 ** (E - 7)
        v[c] = -a if c & 0x80 else a
    return v


E4M3 = _decode_table()


def e4m3_decode(codes):
    return E4M3[np.asarray(codes, dtype=np.uint8)]


def e4m3_encode(x, fault=None):
    """float64 (finite, |x| <= 448) -> e4m3fn codes, round to nearest even; fault "truncate": round towards zero."""
    x = np.asarray(x, dtype=F64)
    a = np.abs(x)
    assert bool(np.isfinite(a).all()) and (a.size == 0 or float(a.max()) <= 448.0)
    _, ex = np.frexp(a)                                        # a = m 2^ex, m in [0.5, 1): floor(log2 a) = ex - 1
    e = np.where(a < 2.0 ** -6, -6, ex - 1).astype(np.int64)   # subnormals share the quantum 2^-9 of the first binade
    q = np.ldexp(a, 3 - e)                                     # a / quantum, exact: [0, 8] below 2^-6, [8, 16) above
    fl = np.floor(q)
    r = q - fl
    n = fl.astype(np.int64)
    if fault != "truncate":
        n = n + ((r > 0.5) | ((r == 0.5) & ((n & 1) == 1)))
    code = ((e + 7) << 3) + n - 8                              # n = 16 carries into the next exponent; 448 = (15 << 3) + 14 - 8 = 0x7E
    assert code.size == 0 or (int(code.min()) >= 0 and int(code.max()) <= 0x7E)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def bits32(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def mx_exponent_ref(amax, fault=None):
    """E8M0 exponent e (scale 2^e, byte e + 127) of blocks with absolute maximum amax (float32, >= 0, never NaN), from the bit fields."""
    b = bits32(amax).astype(np.int64)
    f, m = (b >> 23) & 0xFF, b & 0x7FFFFF
    e = f - 135 + ((m >= 0x600000) if fault == "exp175" else (m > 0x600000))
    return np.clip(e, -127, 127)


def mx_scale_index(row, blk, rows, fault=None):
    """Byte offset of the scale of (row, 32-block blk) of a `rows`-row operand; fault "swap": the first two 32-row groups of a 128-row group change places."""
    rows_pad = (rows + 127) // 128 * 128
    g32 = (row >> 5) & 3
    if fault == "swap":
        g32 = np.where(g32 < 2, 1 - g32, g32)
    return ((blk >> 1) * rows_pad + (row & ~127)) * 2 + (row & 31) * 8 + (blk & 1) * 4 + g32


def mx_scale_bytes(rows, K):
    return (K // 64) * ((rows + 127) // 128 * 128) * 2 + 512


def block_amax(x):
    """fmaxf chain over |x| of every 32-block of x (rows, K) float32: a NaN is ignored."""
    rows, K = x.shape
    with np.errstate(invalid="ignore"):
        return np.fmax.reduce(np.abs(x.reshape(rows, K // 32, 32)), axis=-1, initial=F32(0)).astype(F32)


def clamp448(t):
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(t, F32(-448)), F32(448))        # fmaxf first: a NaN becomes -448


def mx_ref(x, Kq=None, fault=None):
    """x (rows, K) float32 -> (codes (rows, Kq) uint8, e (rows, Kq / 32) int64); columns [K, Kq) are zero blocks."""
    rows, K = x.shape
    Kq = K if Kq is None else Kq
    e = mx_exponent_ref(block_amax(x), fault)
    inv = np.ldexp(F32(1), (-e).astype(np.int32)).astype(F32)              # 2^-e: 2^127 .. 2^-127 (a denormal), all fp32 numbers
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        t = clamp448(x.reshape(rows, K // 32, 32) * inv[..., None])
    codes = np.zeros((rows, Kq), dtype=np.uint8)
    codes[:, :K] = e4m3_encode(t.astype(F64), fault).reshape(rows, K)
    eq = np.full((rows, Kq // 32), -127, dtype=np.int64)
    eq[:, :K // 32] = e
    return codes, eq


def tensor_amax(x, preset=0.0):
    with np.errstate(invalid="ignore"):
        return np.fmax(F32(preset), np.fmax.reduce(np.abs(x.ravel()), initial=F32(0))).astype(F32)


def tensor_ref(x, amax, fault=None):
    """Per-tensor quantiser: x float32 (any shape), amax float32 -> (codes, scale float32)."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        a = np.fmax(F32(amax), F32(1e-12))
        s, scale = F32(448) / a, a / F32(448)
        t = clamp448(x.astype(F32) * s)
    return e4m3_encode(t.astype(F64), fault), F32(scale)


def delayed_ref(x, state, phase, margin):
    """One call of the delayed quantiser: (codes, new state) from the 4-float state before the call."""
    with np.errstate(over="ignore", invalid="ignore"):
        rng = F32(state[phase % 3]) * F32(margin)
    codes, scale = tensor_ref(x, rng)
    new = np.array(state, dtype=F32)
    new[3] = scale
    new[(phase + 2) % 3] = 0
    new[(phase + 1) % 3] = tensor_amax(x, new[(phase + 1) % 3])
    return codes, new


# ---------------------------------------------------------------------------------------------- values
def to_bf16(x):
    """float32 -> the nearest bf16 number (ties to even), as float32."""
    b = bits32(x).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)).view(F32)


def chop(x, dtype):
    """x made representable in dtype by dropping low mantissa bits (never increases |x|)."""
    return x.astype(F32) if dtype == "f32" else (bits32(x) & np.uint32(0xFFFF0000)).view(F32)


def from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(F32)


def binade_mantissas(dtype):
    if dtype == "bf16":
        return [0, 0x600000, 0x610000, 0x7F0000], []
    extra = [0x5FFFFF, 0x600002, 0x400000, 1] + [int(m) for m in np.random.default_rng(175).integers(0, 1 << 23, 20)]
    return [0, 0x600000, 0x600001, 0x7FFFFF], extra


OTHERS = (-15, -16, -17, -18, -19, -21)      # the other elements: amax 2^k (and 3 amax 2^-18), cycled with alternating signs, every seventh one zero


def _binade_fill(amax, pos, sign, dtype):
    """Blocks (n, 32) with sign * amax at element pos (all (n,)) and the OTHERS pattern around it."""
    j = np.arange(32)
    k = np.array(OTHERS)[j % 6]
    with np.errstate(under="ignore"):
        blk = np.ldexp(amax.astype(F32)[:, None], k[None, :]).astype(F32) * np.where(k == -18, 3, 1).astype(F32) * np.where(j % 2, 1, -1).astype(F32)
    blk[:, j % 7 == 6] = 0
    blk = chop(blk, dtype)
    blk[np.arange(len(amax)), pos] = sign.astype(F32) * amax
    return blk


def binade_blocks(dtype, lo, hi):
    """(blocks (n, 32) float32, fields (n,), mantissas (n,)) for amax exponent fields lo .. hi."""
    main, extra = binade_mantissas(dtype)
    cases = []      # (field, mantissa bits, position, sign)
    for f in range(lo, hi + 1):
        cases += [(f, m, p, s) for m in main for p in (0, 7, 8, 31) for s in (1, -1)]
        cases += [(f, m, (0, 7, 8, 31)[i % 4], 1 if (i >> 2) % 2 else -1) for i, m in enumerate(extra)]
    fields, mants, pos, sign = (np.array(c) for c in zip(*cases))
    amax = from_bits(((fields << 23) | mants).astype(np.uint32))
    return _binade_fill(amax, pos, sign, dtype), fields, mants


def midpoints():
    """The 126 midpoints between adjacent non-negative finite e4m3 values, and the even code of each pair."""
    v = E4M3[:0x7F]
    mid = (v[:-1] + v[1:]) / 2
    even = np.array([c if c % 2 == 0 else c + 1 for c in range(0x7E)], dtype=np.uint8)
    return mid, even


def tie_blocks(e):
    """Blocks at scale 2^e: element 0 = 448 * 2^e, the other 31 midpoints * 2^e with alternating signs (all 126 midpoints, either sign)."""
    mid, _ = midpoints()
    vals = np.concatenate([mid, -mid])
    vals = np.concatenate([vals, vals[:(-len(vals)) % 31]])
    blocks = np.empty((len(vals) // 31, 32), dtype=F64)
    blocks[:, 0] = 448.0
    blocks[:, 1:] = vals.reshape(-1, 31)
    out = np.ldexp(blocks, e)
    assert np.array_equal(out.astype(F32).astype(F64), out)
    return out.astype(F32)


@functools.lru_cache(maxsize=None)
def mx_families(dtype, seed=0):
    """name -> blocks (n, 32) float32, every value a number of dtype (binade: see binade_blocks)."""
    rng = np.random.default_rng(1000 + seed)
    fam = {}
    fam["ties"] = np.concatenate([tie_blocks(e) for e in TIE_SCALES])
    z = np.zeros((3, 32), dtype=F32)
    z[1] = -0.0
    z[2, ::3] = -0.0
    fam["zero"] = z
    den_bits = [1, 0x7FFFFF, 0x400000, 0x2AAAAA, 0x000100] if dtype == "f32" else [0x10000, 0x7F0000, 0x400000, 0x2A0000]
    den = []
    for i, b in enumerate(den_bits):
        blk = from_bits(rng.integers(0, b + 1, 32).astype(np.uint32))
        blk = chop(blk, dtype) * np.where(rng.integers(0, 2, 32), 1, -1).astype(F32)
        blk[(5 * i) % 32] = from_bits([b])[0]
        den.append(blk)
        for f, m in ((1, 0), (5, 0x200000), (20, 0x700000)):      # one normal element among denormals (its field is never 8)
            b2 = blk.copy()
            b2[(7 * i + f) % 32] = -from_bits([(f << 23) | m])[0]
            den.append(b2)
    fam["denormal"] = np.stack(den)
    top = from_bits([0x7F7FFFFF if dtype == "f32" else 0x7F7F0000])[0]
    tops = []
    for pos in (0, 7, 8, 31):
        for sign in (1, -1):
            blk = chop((rng.standard_normal(32) * 2.0 ** rng.integers(60, 120, 32)).astype(F32), dtype)
            blk[pos] = sign * top
            tops.append(blk)
            tops.append(_binade_fill(np.array([top]), np.array([pos]), np.array([sign]), dtype)[0])
    fam["top"] = np.stack(tops)
    r = (rng.standard_normal((768, 32)) * 2.0 ** rng.integers(-20, 21, (768, 1))).astype(F32)
    fam["random"] = to_bf16(r) if dtype == "bf16" else r
    for name, b in fam.items():
        assert b.dtype == F32 and b.shape[1] == 32 and np.array_equal(chop(b, dtype).view(np.uint32), b.view(np.uint32)), name
    return fam


def lay_out(blocks, K):
    """blocks (n, 32) -> x (rows, K) with K / 32 blocks per row, zero blocks behind the last."""
    nb = K // 32
    rows = -(-len(blocks) // nb)
    x = np.zeros((rows * nb, 32), dtype=F32)
    x[:len(blocks)] = blocks
    return x.reshape(rows, K)


@functools.lru_cache(maxsize=None)
def shape_pool(dtype):
    f = mx_families(dtype, seed=1)
    return np.concatenate([f["random"], f["ties"][::3], f["zero"], f["top"], f["denormal"]])


def shape_values(pool, rows, K):
    idx = (np.arange(rows * (K // 32)) * 7 + 13 * rows + K) % len(pool)
    return pool[idx].reshape(rows, K)


def tensor_families(n, dtype, seed, only=None):
    """name -> (x (n,) float32 of dtype numbers, preset amax[0]); only: the names wanted (the large sizes build nothing else)."""
    rng = np.random.default_rng(seed)
    cast = to_bf16 if dtype == "bf16" else (lambda v: v.astype(F32))
    base = cast((rng.standard_normal(n) * 3).astype(F32))
    fam = {"random": (base, 0.0)}
    positions = {"first8": 3, "last8": n - 5}
    if n > AMAX_CAP:
        positions["stride-end"] = n - 13         # the last 8 elements of the full grid stride; last8 is then the grid-stride tail
    for name, at in positions.items():
        x = base.copy()
        x[at] = -64.0
        assert float(np.abs(np.delete(x, at)).max()) < 64.0
        fam["max " + name] = (x, 0.0)
    if only is not None:
        return {k: fam[k] for k in only}
    mid, _ = midpoints()
    for k in (0, -7):
        vals = np.ldexp(np.concatenate([[448.0], mid, -mid]), k)
        x = np.resize(vals, n).astype(F32) if n >= len(vals) else vals[:n].astype(F32)
        fam[f"ties 2^{k}"] = (x, 0.0)
    fam["zero"] = (np.zeros(n, dtype=F32), 0.0)
    fam["tiny"] = (cast((base * F32(1e-30 / 16)).astype(F32)), 0.0)
    fam["preset"] = (base, 100.0)
    return fam


# ---------------------------------------------------------------------------------------------- arenas and launches
def _stream():
    return torch.cuda.current_stream().cuda_stream


class In:
    """x (rows, K) float32 values as a dtype operand with leading dimension ldx inside an arena of +-1e30."""

    def __init__(self, x, dtype, ldx=None):
        rows, K = x.shape
        ldx = K if ldx is None else ldx
        self.lead, self.rows, self.K, self.ldx, self.dtype = 64, rows, K, ldx, dtype
        n = 2 * self.lead + rows * ldx
        big = bits32(np.array([BIG, -BIG]))
        if dtype == "bf16":
            assert not bool((bits32(x) & 0xFFFF).any()), "not bf16 numbers"
            arena = np.resize((big >> 16).astype(np.uint16), n)
            vals = (bits32(x) >> 16).astype(np.uint16)
        else:
            arena = np.resize(big, n)
            vals = bits32(x)
        arena[self.lead:self.lead + rows * ldx].reshape(rows, ldx)[:, :K] = vals
        self.host = arena
        self.dev = torch.from_numpy(arena.view(np.int16 if dtype == "bf16" else np.int32)).cuda()
        self.ptr = self.dev.data_ptr() + self.lead * arena.itemsize
        assert self.ptr % 16 == 0

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(self.host.dtype), self.host)


class OutBytes:
    """A window of `nbytes` bytes inside a 0xFF-filled arena."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.dev = torch.full((2 * LEAD + nbytes,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.dev.data_ptr() + LEAD
        assert self.ptr % 16 == 0

    def expected(self):
        return np.full(2 * LEAD + self.n, FILL, dtype=np.uint8)

    def host(self):
        return self.dev.cpu().numpy()


def diff_report(name, got, want, failures, tag):
    """Whole-arena comparison; returns the mismatch mask of the window."""
    bad = got != want
    if bad.any():
        inside = bad[LEAD:len(bad) - LEAD]
        at = np.flatnonzero(bad)[:6]
        failures.append(f"{tag} {name}: {int(bad.sum())} bytes differ from the reference ({int(bad.sum()) - int(inside.sum())} of them in the {LEAD}-byte guards); "
                        f"first (arena offset - {LEAD}, got, want): {[(int(i) - LEAD, hex(got[i]), hex(want[i])) for i in at]}")
    return bad[LEAD:len(bad) - LEAD]


WORST = {}


def record(key, **ratios):
    w = WORST.setdefault(key, {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), float(v))


def run_mx(lib, x, dtype, ldx, pad=False):
    """Launch the MX quantiser on x (rows, K); returns (input arena, code arena, scale arena, Kq)."""
    rows, K = x.shape
    Kq = (K + 127) // 128 * 128 if pad else K
    xin, q, sc = In(x, dtype, ldx), OutBytes(rows * Kq), OutBytes(mx_scale_bytes(rows, Kq))
    fn = lib.mmdit_mxfp8_quantize_pad if pad else lib.mmdit_mxfp8_quantize
    torch.cuda.synchronize()
    rc = fn(xin.ptr, DT[dtype], rows, K, ldx, q.ptr, sc.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return xin, q, sc, Kq


def expected_mx_arenas(codes, e, q, sc, fault=None):
    rows, Kq = codes.shape
    wq, ws = q.expected(), sc.expected()
    wq[LEAD:LEAD + rows * Kq] = codes.ravel()
    r, b = np.meshgrid(np.arange(rows), np.arange(Kq // 32), indexing="ij")
    ws[LEAD + mx_scale_index(r, b, rows, fault)] = (e + 127).astype(np.uint8)
    return wq, ws


def mx_bars(x, Kq, codes, scales, failures, tag, key):
    """The float64 bars on the kernel's own codes (rows, Kq) and scale bytes (rows, Kq / 32), x (rows, K) zero-extended to Kq."""
    rows, K = x.shape
    x64 = np.zeros((rows, Kq), dtype=F64)
    x64[:, :K] = x
    xb = x64.reshape(rows, Kq // 32, 32)
    amax = np.abs(xb).max(-1)
    e = scales.astype(np.int64) - 127
    s = np.ldexp(1.0, e)
    hi = amax / (448.0 * s)
    lo = np.where((e > -127), 448.0 * s / 2 / np.where(amax > 0, amax, 1.0), 0.0)
    lo = np.where((e > -127) & (amax == 0), np.inf, lo)
    err = np.abs(e4m3_decode(codes).reshape(rows, Kq // 32, 32) * s[..., None] - xb)
    el = err / np.maximum(2.0 ** -4 * np.abs(xb), 2.0 ** -10 * s[..., None])
    record(key, amax_hi=hi.max(), amax_lo=lo.max(), elem=np.nanmax(el) if not np.isnan(el).all() else np.inf)
    for name, r, ok in (("amax <= 448 2^e", hi, hi <= 1), ("amax > 448 2^(e-1)", lo, lo < 1), ("|q 2^e - x| per element", el, el <= 1)):
        if not bool(ok.all()):
            at = np.argwhere(~ok)[:4]
            failures.append(f"{tag} {name}: {int((~ok).sum())} over the bar, first (row, block[, element], ratio): {[tuple(int(i) for i in a) + (float(r[tuple(a)]),) for a in at]}")


def check_mx(lib, x, dtype, ldx, tag, key, pad=False, info=None):
    """One MX launch held to the reference bit for bit (whole arenas), to the float64 bars and to its guards.  Returns the failures."""
    failures = []
    rows, K = x.shape
    xin, q, sc, Kq = run_mx(lib, x, dtype, ldx, pad)
    codes, e = mx_ref(x, Kq)
    wq, ws = expected_mx_arenas(codes, e, q, sc)
    gq, gs = q.host(), sc.host()
    diff_report("codes", gq, wq, failures, tag)
    bad = diff_report("scale bytes", gs, ws, failures, tag)
    r, b = np.meshgrid(np.arange(rows), np.arange(Kq // 32), indexing="ij")
    idx = mx_scale_index(r, b, rows)
    if bad.any() and info is not None:
        wrong = bad[idx]
        failures.append(f"{tag}: amax exponent fields of the blocks with a wrong scale byte: {sorted(set(info[0].reshape(rows, -1)[wrong].tolist()))}, "
                        f"their mantissa bits from {hex(int(info[1].reshape(rows, -1)[wrong].min()))} to {hex(int(info[1].reshape(rows, -1)[wrong].max()))}, "
                        f"(got, want) bytes {sorted(set(zip(gs[LEAD + idx][wrong].tolist(), ws[LEAD + idx][wrong].tolist())))}")
    mx_bars(x, Kq, gq[LEAD:LEAD + rows * Kq].reshape(rows, Kq), gs[LEAD + idx], failures, tag, key)
    if not xin.unchanged():
        failures.append(f"{tag}: the input arena changed")
    return failures


# ---------------------------------------------------------------------------------------------- MX tests
def case_mx_binade(ops, fields, dtype):
    """Every exponent field of amax with mantissas at, beside and away from 1.75, at four positions with either sign (K = 128, ldx = K + 8)."""
    lib = ops._lib.lib()
    blocks, f, m = binade_blocks(dtype, *fields)
    x = lay_out(blocks, 128)
    pad = x.shape[0] * 4 - len(blocks)
    info = (np.concatenate([f, np.zeros(pad, dtype=f.dtype)]), np.concatenate([m, np.zeros(pad, dtype=m.dtype)]))
    assert np.array_equal(block_amax(x).ravel()[:len(blocks)].view(np.uint32), ((f << 23) | m).astype(np.uint32)), "a block's amax is not the intended one"
    key = f"mmdit_mxfp8_quantize binade {dtype}"
    failures = check_mx(lib, x, dtype, 136, f"binade {dtype} fields {fields}", key, info=info)
    print(f"[fp8 edges] {key} fields {fields[0]}-{fields[1]}: {x.shape[0] * 4} blocks, worst so far {WORST[key]}")
    assert not failures, "\n".join(failures)


def case_mx_family(ops, family, dtype):
    """The other value families at K = 128, ldx = K + 8, plain and zero-padding entry point (K = 192 -> 256 for the latter)."""
    lib = ops._lib.lib()
    blocks = mx_families(dtype)[family]
    failures = []
    for pad, K in ((False, 128), (True, 192)):
        x = lay_out(blocks, K)
        key = f"mmdit_mxfp8_quantize{'_pad' if pad else ''} {family} {dtype}"
        failures += check_mx(lib, x, dtype, K + 8, f"{family} {dtype} pad={pad}", key, pad=pad)
        print(f"[fp8 edges] {key}: {len(blocks)} blocks, worst {WORST[key]}")
    if family == "ties":       # (implied by the byte comparison; spelled out because it is the point of the family)
        x = lay_out(blocks, 128)
        _, q, _, _ = run_mx(lib, x, dtype, 128)
        got = q.host()[LEAD:LEAD + x.size].reshape(-1, 32)[:len(blocks)]
        assert not bool((got[:, 1:] & 1).any()), "a midpoint left as an odd code"
        assert bool((got[:, 0] == 0x7E).all())
    assert not failures, "\n".join(failures)


def case_mx_shapes(ops, K, gap, dtype):
    """rows around the 32-row and 128-row groups of the scale layout and around the 256-thread workgroups, ldx = K + gap; mixed values."""
    lib = ops._lib.lib()
    pool = shape_pool(dtype)
    failures = []
    for rows in MX_ROWS:
        x = shape_values(pool, rows, K)
        key = f"mmdit_mxfp8_quantize shapes {dtype}"
        failures += check_mx(lib, x, dtype, K + gap, f"rows {rows} K {K} ldx {K + gap} {dtype}", key)
        if K != 128:
            key = f"mmdit_mxfp8_quantize_pad shapes {dtype}"
            failures += check_mx(lib, x, dtype, K + gap, f"pad rows {rows} K {K} ldx {K + gap} {dtype}", key, pad=True)
    print(f"[fp8 edges] mx shapes K {K} ldx {K + gap} {dtype}: worst so far {WORST[key]}")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- per-tensor tests
class F32Arena:
    """16 floats of 0xFFFFFFFF; the test's scalars sit at [4] (amax or state[0 .. 3]) and [8] (scale)."""

    def __init__(self, values):
        self.want = np.full(16, 0xFFFFFFFF, dtype=np.uint32)
        for k, v in values.items():
            self.want[k] = bits32(np.array([v]))[0]
        self.dev = torch.from_numpy(self.want.view(np.int32).copy()).cuda()

    def ptr(self, k):
        return self.dev.data_ptr() + 4 * k

    def expect(self, k, v):
        self.want[k] = bits32(np.array([v]))[0]

    def check(self, failures, tag):
        got = self.dev.cpu().numpy().view(np.uint32)
        if not np.array_equal(got, self.want):
            failures.append(f"{tag}: scalars differ from the reference: got {[hex(v) for v in got[3:10]]} ({got[3:10].view(F32)}), want {[hex(v) for v in self.want[3:10]]} "
                            f"({self.want[3:10].view(F32)}) at words 3 .. 9")
        return got.view(F32)


def tensor_bar(x, codes, scale, failures, tag, key):
    """|q scale - x| <= max(2^-4 |x|, 2^-10 scale) (1 + 2^-20) on every element whose scaled value lies inside +-448."""
    x64, s = x.astype(F64).ravel(), float(scale)
    inside = np.abs(x64) <= 448.0 * s
    err = np.abs(e4m3_decode(codes).ravel() * s - x64)
    el = np.where(inside, err / (np.maximum(2.0 ** -4 * np.abs(x64), 2.0 ** -10 * s) * (1 + 2.0 ** -20)), 0.0)
    sat = np.where(inside, False, (codes.ravel() & 0x7F) != 0x7E)
    record(key, elem=np.nanmax(el) if el.size else 0.0)
    if not bool((el <= 1).all()):
        at = np.flatnonzero(~(el <= 1))[:4]
        failures.append(f"{tag} |q scale - x|: {int((~(el <= 1)).sum())} over the bar, first (index, ratio): {[(int(i), float(el[i])) for i in at]}")
    if sat.any():
        failures.append(f"{tag}: {int(sat.sum())} elements beyond the range did not saturate")


def check_two_pass(lib, x, preset, dtype, tag, key, quantize=True):
    """mmdit_fp8_amax (amax[0] preset by the caller) and mmdit_fp8_quantize on x (n,)."""
    failures = []
    n = x.size
    xin = In(x.reshape(1, n), dtype)
    scal = F32Arena({4: preset})
    torch.cuda.synchronize()
    assert lib.mmdit_fp8_amax(xin.ptr, DT[dtype], n, scal.ptr(4), _stream()) == 0
    amax = tensor_amax(x, preset)
    scal.expect(4, amax)
    if quantize:
        q = OutBytes(n)
        assert lib.mmdit_fp8_quantize(xin.ptr, DT[dtype], n, scal.ptr(4), q.ptr, scal.ptr(8), _stream()) == 0
        codes, scale = tensor_ref(x, amax)
        scal.expect(8, scale)
    torch.cuda.synchronize()
    got = scal.check(failures, tag)
    if quantize:
        want = q.expected()
        want[LEAD:LEAD + n] = codes
        gq = q.host()
        diff_report("codes", gq, want, failures, tag)
        tensor_bar(x, gq[LEAD:LEAD + n], got[8], failures, tag, key)
    if not xin.unchanged():
        failures.append(f"{tag}: the input arena changed")
    return failures


def case_tensor_two_pass(ops, n, dtype):
    """mmdit_fp8_amax + mmdit_fp8_quantize at the small sizes: one and two vectors, around one and three full workgroups, every family."""
    lib = ops._lib.lib()
    failures = []
    for name, (x, preset) in tensor_families(n, dtype, seed=n).items():
        key = f"mmdit_fp8_quantize {name.split(' 2^')[0]} {dtype}"
        failures += check_two_pass(lib, x, preset, dtype, f"n {n} {name} {dtype}", key)
    print(f"[fp8 edges] two-pass n {n} {dtype}: worst so far " + ", ".join(f"{k.split(' ', 1)[1]} {v['elem']:.4f}" for k, v in WORST.items() if k.startswith("mmdit_fp8_quantize ") and k.endswith(dtype)))
    assert not failures, "\n".join(failures)


def case_tensor_grid_cap(ops, n, quantize):
    """The grid caps: 1024 workgroups of mmdit_fp8_amax one vector short of and one vector past a full grid, 4096 workgroups of mmdit_fp8_quantize one vector
    past it (the vector of the second trip); the one largest element in the first 8, the last 8 (the grid-stride tail) and the last 8 of the full stride."""
    lib = ops._lib.lib()
    failures = []
    names = ["max last8"] if quantize else ["max first8", "max last8", "random"] + (["max stride-end"] if n > AMAX_CAP else [])
    fams = tensor_families(n, "bf16", seed=n, only=names)
    for name in names:
        x, preset = fams[name]
        failures += check_two_pass(lib, x, preset, "bf16", f"n {n} {name}", f"mmdit_fp8_quantize cap {name} bf16", quantize=quantize)
    assert not failures, "\n".join(failures)


def case_tensor_pad(ops, dtype):
    """mmdit_fp8_quantize_pad at a K % 128 == 64 shape (33 x 192 -> 33 x 256, ldx = 200): the plain quantiser's codes, zero codes behind column K."""
    lib = ops._lib.lib()
    rows, K, ldx, Kq = 33, 192, 200, 256
    failures = []
    for name, (x, preset) in tensor_families(rows * K, dtype, seed=33).items():
        tag = f"pad {name} {dtype}"
        x2 = x.reshape(rows, K)
        xin, q = In(x2, dtype, ldx), OutBytes(rows * Kq)
        amax = tensor_amax(x, preset)
        scal = F32Arena({4: amax})
        torch.cuda.synchronize()
        assert lib.mmdit_fp8_quantize_pad(xin.ptr, DT[dtype], rows, K, ldx, scal.ptr(4), q.ptr, scal.ptr(8), _stream()) == 0
        torch.cuda.synchronize()
        codes, scale = tensor_ref(x2, amax)
        scal.expect(8, scale)
        got = scal.check(failures, tag)
        want = q.expected()
        full = np.zeros((rows, Kq), dtype=np.uint8)
        full[:, :K] = codes
        want[LEAD:LEAD + rows * Kq] = full.ravel()
        gq = q.host()
        diff_report("codes", gq, want, failures, tag)
        tensor_bar(x2, gq[LEAD:LEAD + rows * Kq].reshape(rows, Kq)[:, :K], got[8], failures, tag, f"mmdit_fp8_quantize_pad {name.split(' 2^')[0]} {dtype}")
        if not xin.unchanged():
            failures.append(f"{tag}: the input arena changed")
    assert not failures, "\n".join(failures)


DELAYED_N = (2048, 8, 8 * 256 * 3 + 8, AMAX_CAP + 8, AMAX_CAP - 8, 2040, 16, 8 * 256 * 3 - 8)
DELAYED_AMP = (1.0, 1.04, 1.3, 2.5, 0.5, 0.01, 0.0109, 3.0)      # grows inside a margin of 1.1 / 1.5, outgrows it, shrinks, grows again


def case_tensor_delayed(ops, margin, dtype):
    """Eight consecutive mmdit_fp8_quantize_delayed calls on one state (phases 0 .. 7: every residue mod 3 at least twice), sizes from one vector to the
    1024-workgroup cap +- 8, the largest element of every call negative and in its last 8 elements (the grid-stride tail of the capped launch)."""
    lib = ops._lib.lib()
    rng = np.random.default_rng(7)
    failures, saturating = [], 0
    state = None
    scal = None
    for phase, (n, amp) in enumerate(zip(DELAYED_N, DELAYED_AMP)):
        x = (rng.uniform(-0.9, 0.9, n) * amp).astype(F32)
        x[n - 3] = -amp
        x = to_bf16(x) if dtype == "bf16" else x
        if phase == 0:      # the caller's initialisation: the ring slot of the first call holds the data's own amax, the next 0; the third is cleared by the call
            state = np.array([tensor_amax(x), 0.0, 7.0, 0.0], dtype=F32)
            scal = F32Arena({4: state[0], 5: state[1], 6: state[2]})
        tag = f"delayed margin {margin} {dtype} call {phase} n {n}"
        xin, q = In(x.reshape(1, n), dtype), OutBytes(n)
        torch.cuda.synchronize()
        assert lib.mmdit_fp8_quantize_delayed(xin.ptr, DT[dtype], n, scal.ptr(4), phase, margin, q.ptr, _stream()) == 0
        torch.cuda.synchronize()
        codes, state = delayed_ref(x, state, phase, margin)
        assert bits32(state[(phase + 1) % 3: (phase + 1) % 3 + 1])[0] == bits32(np.abs(x[n - 3:n - 2]))[0] and state[(phase + 2) % 3] == 0
        for k in range(4):
            scal.expect(4 + k, state[k])
        got = scal.check(failures, tag)
        want = q.expected()
        want[LEAD:LEAD + n] = codes
        gq = q.host()
        diff_report("codes", gq, want, failures, tag)
        sat_ref, sat_got = np.flatnonzero((codes & 0x7F) == 0x7E), np.flatnonzero((gq[LEAD:LEAD + n] & 0x7F) == 0x7E)
        if float(np.abs(x).max()) > 448.0 * float(state[3]):
            saturating += 1
            assert len(sat_ref) > 0
            if not np.array_equal(sat_ref, sat_got):
                failures.append(f"{tag}: the saturated positions differ: {len(sat_got)} against {len(sat_ref)} of the reference")
        tensor_bar(x, gq[LEAD:LEAD + n], got[7], failures, tag, f"mmdit_fp8_quantize_delayed margin {margin:.2f} {dtype}")
        if not xin.unchanged():
            failures.append(f"{tag}: the input arena changed")
    assert saturating >= 2 and saturating < len(DELAYED_N), "the sequence must hold saturating and non-saturating calls"
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- non-finite inputs
def nonfinite_block_values(dtype):
    """(rows 8, K 64): one +inf, one -inf, one NaN and one -NaN block, a block with inf and NaN, an all-NaN block, finite neighbours."""
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((8, 64)) * 2.0 ** rng.integers(-3, 4, (8, 1))).astype(F32)
    x[0, 5], x[1, 40], x[2, 31], x[3, 32] = np.inf, -np.inf, np.nan, -np.nan
    x[3, 33] = F32(3e38)
    x[4, 0], x[4, 1], x[4, 2] = np.nan, np.inf, -np.inf
    x[5, 32:] = np.nan
    return chop(x, dtype)


def case_nonfinite_inputs(ops, dtype):
    """The non-finite sentence of mmdit_hip.h, per entry point: +-inf leaves as the +-448 codes, a NaN as 0xFE and never as 0x7F / 0xFF, the amax ignores a NaN, an
    MX block with an inf gets scale byte 247; plain and _pad entry points agree.  (Whether a NaN should leave as 0x7F instead is an open decision.)"""
    lib = ops._lib.lib()
    failures = []
    x = nonfinite_block_values(dtype)
    rows, K = x.shape
    for pad in (False, True):
        xin, q, sc, Kq = run_mx(lib, x, dtype, K + 8, pad)
        codes, e = mx_ref(x, Kq)
        assert codes[0, 5] == 0x7E and codes[1, 40] == 0xFE and codes[2, 31] == 0xFE and codes[3, 32] == 0xFE and e[0, 0] == 120 and e[1, 1] == 120
        assert e[2, 0] < 10 and e[5, 1] == -127 and bool((codes[5, 32:64] == 0xFE).all()) and tuple(codes[4, :3]) == (0xFE, 0x7E, 0xFE)
        wq, ws = expected_mx_arenas(codes, e, q, sc)
        diff_report("codes", q.host(), wq, failures, f"nonfinite mx pad={pad} {dtype}")
        diff_report("scale bytes", sc.host(), ws, failures, f"nonfinite mx pad={pad} {dtype}")
    flat = x.ravel()
    n = flat.size
    for name, preset in (("finite range", 16.0), ("measured range", None)):
        xin = In(flat.reshape(1, n), dtype)
        scal = F32Arena({4: 0.0})
        q, qp = OutBytes(n), OutBytes(rows * 128)
        torch.cuda.synchronize()
        assert lib.mmdit_fp8_amax(xin.ptr, DT[dtype], n, scal.ptr(4), _stream()) == 0
        torch.cuda.synchronize()
        scal.expect(4, np.inf)
        scal.check(failures, f"nonfinite amax {dtype}")
        rng_ = F32(np.inf if preset is None else preset)
        scal = F32Arena({4: rng_})
        assert lib.mmdit_fp8_quantize(xin.ptr, DT[dtype], n, scal.ptr(4), q.ptr, scal.ptr(8), _stream()) == 0
        assert lib.mmdit_fp8_quantize_pad(xin.ptr, DT[dtype], rows, K, K, scal.ptr(4), qp.ptr, scal.ptr(8), _stream()) == 0
        torch.cuda.synchronize()
        codes, scale = tensor_ref(flat, rng_)
        if preset is None:
            assert np.isinf(scale) and codes[5] == 0xFE and codes[64 + 40] == 0xFE and set(np.delete(codes, np.flatnonzero(~np.isfinite(flat))).tolist()) <= {0x00, 0x80}
        else:
            assert codes[5] == 0x7E and codes[64 + 40] == 0xFE and codes[2 * 64 + 31] == 0xFE
        scal.expect(8, scale)
        scal.check(failures, f"nonfinite quantize {name} {dtype}")
        want = q.expected()
        want[LEAD:LEAD + n] = codes
        diff_report("codes", q.host(), want, failures, f"nonfinite quantize {name} {dtype}")
        full = np.zeros((rows, 128), dtype=np.uint8)
        full[:, :K] = codes.reshape(rows, K)
        want = qp.expected()
        want[LEAD:LEAD + rows * 128] = full.ravel()
        diff_report("codes", qp.host(), want, failures, f"nonfinite quantize_pad {name} {dtype}")
    state = np.array([16.0, 0.0, 7.0, 0.0], dtype=F32)
    scal = F32Arena({4: state[0], 5: state[1], 6: state[2]})
    xin, q = In(flat.reshape(1, n), dtype), OutBytes(n)
    assert lib.mmdit_fp8_quantize_delayed(xin.ptr, DT[dtype], n, scal.ptr(4), 0, 1.0, q.ptr, _stream()) == 0
    torch.cuda.synchronize()
    codes, state = delayed_ref(flat, state, 0, 1.0)
    assert np.isinf(state[1]) and state[2] == 0
    for k in range(4):
        scal.expect(4 + k, state[k])
    scal.check(failures, f"nonfinite delayed {dtype}")
    want = q.expected()
    want[LEAD:LEAD + n] = codes
    diff_report("codes", q.host(), want, failures, f"nonfinite delayed {dtype}")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- SwiGLU GEMM epilogue leaving as MX
SWIGLU_SHAPES = [(M, h, K) for M in (1, 127, 129, 257) for h in (128, 384) for K in (128, 256)]
SWIGLU_PLAN = 258      # the planner sends every SwiGLU launch on MX operands to the 8-phase e4m3 kernel (gemm.hip choose_kernel: mx8), whatever cu_budget
#                        says (test_fp8_quant_edges_cpu.py pins that without a GPU).  The second spelling of this epilogue, gemm_tile.h epilogue_swiglu on the
#                        LDS-DMA kernel, takes such a launch only when M * lda or N * ldb reaches 2^32 -- an e4m3 operand of 4 GiB: not reached here.


def swiglu_launch(M, h, K, budget=0):
    return G.L("8p mx swiglu mx-out", SWIGLU_PLAN, G.P(M, 2 * h, K, ab="mx", bias=True, act=G.ACT_SWIGLU), budget=budget)


def case_swiglu_epilogue_mx_out(ops, M, h, K):
    """act = SwiGLU with c_dtype = MMDIT_FP8 + c_scales: codes and scale bytes equal this file's reference quantiser applied to the bf16 output of the same
    plan (MX operands, a bias); the code window (ldc = h + 16) and the scale window sit in 0xFF arenas that come back unchanged outside them."""
    lib = ops._lib.lib()
    launch = swiglu_launch(M, h, K)
    p = launch.probs[0]
    t = G.build(p, "random", 0, "cuda", ops)
    arr = (ops.GemmArgs * 1)()
    y = torch.full((M, h), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops._fill_gemm(arr[0], **dict(t["kw"], out=y, cu_budget=launch.budget))
    assert lib.mmdit_gemm_plan(arr, 1) == launch.plan
    assert lib.mmdit_gemm_grouped(arr, 1, _stream()) == 0
    ldc, g = h + 16, 8
    qa = torch.full(((M + 2 * g) * ldc,), FILL, dtype=torch.uint8, device="cuda")
    sc = OutBytes(mx_scale_bytes(M, h))
    win = qa.view(M + 2 * g, ldc)[g:g + M, :h].view(torch.float8_e4m3fn)
    ops._fill_gemm(arr[0], **dict(t["kw"], out=win, out_scales=sc.dev[LEAD:], cu_budget=launch.budget))
    assert arr[0].ldc == ldc and arr[0].c_dtype == G._FP8
    assert lib.mmdit_gemm_plan(arr, 1) == launch.plan
    assert lib.mmdit_gemm_grouped(arr, 1, _stream()) == 0
    torch.cuda.synchronize()
    y32 = (y.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32) << 16).view(F32)
    assert bool(np.isfinite(y32).all())
    codes, e = mx_ref(y32)
    failures = []
    want = np.full((M + 2 * g, ldc), FILL, dtype=np.uint8)
    want[g:g + M, :h] = codes
    got = qa.cpu().numpy().reshape(M + 2 * g, ldc)
    if not np.array_equal(got, want):
        bad = got != want
        outside = bad.copy()
        outside[g:g + M, :h] = False
        failures.append(f"codes: {int(bad.sum())} bytes differ ({int(outside.sum())} outside the window), first (arena row, byte): {np.argwhere(bad)[:4].tolist()}")
    ws = sc.expected()
    r, b = np.meshgrid(np.arange(M), np.arange(h // 32), indexing="ij")
    idx = mx_scale_index(r, b, M)
    ws[LEAD + idx] = (e + 127).astype(np.uint8)
    gs = sc.host()
    diff_report("scale bytes", gs, ws, failures, "")
    mx_bars(y32, h, got[g:g + M, :h], gs[LEAD + idx], failures, "", "mmdit_gemm SwiGLU MX out")
    print(f"[fp8 edges] swiglu mx-out ({M}, {h}, {K}): worst so far {WORST['mmdit_gemm SwiGLU MX out']}")
    assert not failures, "\n".join([launch.id] + failures)


# ---------------------------------------------------------------------------------------------- the three tests
GRID_CAP_CASES = ((AMAX_CAP - 8, False), (AMAX_CAP + 8, False), (QUANT_CAP + 8, True))
DELAYED_CASES = ((1.0, "bf16"), (1.5, "f32"), (float(F32(1.1)), "bf16"))
DTYPES = ("bf16", "f32")


def run_cases(ops, cases, prefixes):
    """Runs every (case function, arguments) in turn -- a failing case does not hide the next ones -- prints each case's wall time and the worst ratios of
    the entry points named by `prefixes`, and fails with the cases' messages, each under its own label."""
    failed = []
    for fn, args in cases:
        label = f"{fn.__name__[5:]}[{'-'.join(str(a) for a in args)}]"
        t0 = time.perf_counter()
        try:
            fn(ops, *args)
        except AssertionError as e:
            failed.append(f"---- {label}\n{e}")
        print(f"[fp8 edges time] {label} {time.perf_counter() - t0:.3f} s")
    for key in sorted(WORST):
        if key.startswith(prefixes):
            print(f"[fp8 edges worst] {key}: " + " ".join(f"{k} {v:.6f}" for k, v in WORST[key].items()))
    assert not failed, f"{len(failed)} of {len(cases)} cases failed\n" + "\n".join(failed)


MX_CASES = ([(case_mx_binade, (g, dt)) for g in FIELD_GROUPS for dt in DTYPES]
            + [(case_mx_family, (fam, dt)) for fam in ("ties", "zero", "denormal", "top", "random") for dt in DTYPES]
            + [(case_mx_shapes, (K, gap, dt)) for K in MX_K for gap in (0, 8, 64) for dt in DTYPES]
            + [(case_swiglu_epilogue_mx_out, shape) for shape in SWIGLU_SHAPES])
TENSOR_CASES = ([(case_tensor_two_pass, (n, dt)) for n in TENSOR_N for dt in DTYPES] + [(case_tensor_grid_cap, c) for c in GRID_CAP_CASES]
                + [(case_tensor_pad, (dt,)) for dt in DTYPES] + [(case_tensor_delayed, c) for c in DELAYED_CASES])


def test_mx_quantiser_edges(ops):
    """mmdit_mxfp8_quantize / _pad over the binade groups, the other value families and the shape grid, and the SwiGLU GEMM epilogue that leaves as MX
    codes: 60 cases in turn (the suite keeps one id per group of kernels, as test_optim_edges_gpu.py does; a failure names its case)."""
    run_cases(ops, MX_CASES, ("mmdit_mxfp8", "mmdit_gemm"))


def test_per_tensor_quantiser_edges(ops):
    """mmdit_fp8_amax + mmdit_fp8_quantize at the small sizes and the grid caps, mmdit_fp8_quantize_pad, mmdit_fp8_quantize_delayed: 22 cases in turn."""
    run_cases(ops, TENSOR_CASES, ("mmdit_fp8",))


def test_nonfinite_inputs(ops):
    """+-inf and NaN through every entry point, both input types: the non-finite sentence of mmdit_hip.h (case_nonfinite_inputs)."""
    run_cases(ops, [(case_nonfinite_inputs, (dt,)) for dt in DTYPES], ("none",))
