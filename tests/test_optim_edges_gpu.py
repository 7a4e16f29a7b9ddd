"""Edge sweep of the optimizer, cast and embedding kernels (csrc/optim.hip; mmdit_cast, mmdit_patchify / _unpatchify, mmdit_time_embed_fwd / _bwd of
csrc/rowops.hip) with PER-ELEMENT and PER-CHUNK float64 parity through the C ABI.

test_kernels_gpu.py holds the optimizer to a whole-tensor Frobenius bar of 2e-6 after five steps: one element of 768 x 768 that misses an update,
an element updated with its neighbour's gradient, a dropped tail element of a chunk, eps on the wrong side of the bias correction and a step counter
off by one all pass there, and only one of its tensors reaches the float4 path.  This file puts MANY tensors into ONE device table per launch:

  SIZES       1, 3, 4, 5, 6, 1023, 1024, 1025, 1028, 2047, 2048, 2049, 2052, 65535, 65536, 65537, 65536 + 1027, 2 * 65536, 3 * 65536 + 5
              (n4 = 256 / 257: one and two 16-byte loads in flight; the 2048-element edge of the double-buffered loop; the n % 4 tail, 6 added for n % 4 = 2;
              MMDIT_ADAMW_CHUNK +- 1; a short last chunk; a tensor of exactly one chunk; several chunks)
  PLACEMENTS  aligned (shadow 16-byte aligned) | param / grad / exp_avg / exp_avg_sq alone offset by one element (scalar path) | all four offset by
              four elements | no shadow | shadow 8- but not 16-byte aligned | shadow offset by one bf16 element (scalar path although the fp32
              operands are aligned)

so the whole shape x alignment grid (171 tensors, 5.4 M elements) costs one launch.  Every operand is a window of a NaN-filled arena; every word
of every arena outside the windows is a guard whose bit pattern must come back identical (inputs: the whole arena).  The library has no query
for the path a chunk takes, so the chunk map and the path rules are RESTATED below (chunk_map: optim.py _build_table; adamw_path / sumsq_path /
cast_path: optim.hip adamw_kernel / grad_sumsq_kernel / cast_multi_kernel; grid_cap / cast_trips / patch_trips: rowops.hip grid_cap, mmdit_cast,
patch_dispatch).  The restatement can DRIFT from the sources and nothing detects that: optim.py _build_table and optim.hip (next to CHUNK / TPB) carry
a comment that points here.  tests/test_optim_edges_cpu.py asserts on the restatement that every path is present.

Reference: plain float64 torch of the operands exactly as stored, no ops.* call; hyper-parameters as the doubles the launch receives.

Yardstick (counted from the rounding points, not tuned).  u = 2^-24, U = 2^-8.  The build (hipcc -O3, no fast-math flag) keeps clang's HIP default
-fhip-fp32-correctly-rounded-divide-sqrt: sqrtf and the fp32 divisions are correctly rounded, ONE rounding each (in the kernel's ISA: v_div_scale /
v_div_fmas / v_div_fixup, and v_sqrt_f32 followed by the +-1 ulp correction from two fma residuals, with the scaling of subnormal arguments); products
feeding sums may be contracted to fma, which only removes roundings.

  AdamW   launch prologue, each computed in double and rounded ONCE to fp32: decay = 1 - lr wd, c1 = 1 - b1, b2, c2 = 1 - b2, eps,
          ss = lr / (1 - b1^t), bc = sqrt(1 - b2^t)  (t = step_count + 1; pow / sqrt in double: 1e-15, ignored)
          g' = g coef                    1 rounding (none for coef_found == NULL)           e_g  = u |g'|
          p1 = p decay                   decay, product                                     e_p1 = 2 u |p1|
          m' = m + c1 (g' - m)           difference, c1, product, sum                       e_m  = u (|m'| + (1 - b1) (|g'| + 3 |g' - m|))
                                         (relative to |m| + (1 - b1)(|g'| + |m|), NOT to |m'|: the cancelling family)
          v' = b2 v + (c2 g') g'         A = b2 v: b2, product; B: c2, g' twice, two products; sum of non-negative terms
                                                                                            e_v  = u (3 A + 6 B) + 2^-126
          s  = sqrtf(v')                 propagated exactly (v' may be 0), 1 rounding       e_s  = max(s - sqrt(v' - e_v), sqrt(v' + e_v) - s) + u s
          q  = s / bc                    bc, division                                       e_q  = e_s / bc + 2 u q
          den = q + eps                  eps, sum                                           e_den = e_q + u eps + u den
          num = ss m'                    ss, product                                        e_num = ss e_m + 2 u |num|
          r  = num / den                 division                                           e_r  = e_num / den + |r| e_den / den + u |r|
          p' = p1 - r                    difference (the store is exact)                    e_p  = e_p1 + e_r + u |p'|
          for p, m and v alike (test_gemm_edges_gpu ELEM_BAR / ROW_BAR):  |out - ref| <= 2 y per element,  ||out - ref||_2 <= 1 ||y||_2 per chunk
  shadow  EQUALS p_out.to(bfloat16) of the kernel's own fp32 output bit for bit (vector path, scalar path, every tail)
  sumsq   non-negative terms: relative (depth) u, depth = 1 (square) + 3 (the float4's four squares, vector path) + serial adds of one lane
          (ceil(n4 / 512) + 1 + 1 tail on the vector path, ceil(n / 256) on the scalar path) + 1 (a0 + a1) + 6 (wave) + 4 (block), + 2^-126 * n
  clip    S = sum of partials in double (1e-13 relative allowed for it).  out[2] = fl(fl(sqrt S) fl(1 / scale)): 3 roundings, y = 3 u |ref|.
          out[0] = fl(inv fl(max_norm / fl(norm + 1e-6f))) when clamped: total, norm, sum, quotient, product = 5 roundings (the rounding of inv
          cancels between norm and the final product except for the 1e-6 share, one more u); 1 rounding (inv) when not clamped, 0 without a scale.
          y = 6 u |ref|, |out - ref| <= 2 y.  out[1] exact.
  casts, patchify / unpatchify   bit-exact against torch (.to(dtype): round to nearest even; reshape / permute).
  time embedding   e = t ts / denom in float64 of the fp32 operands; y = 2 u |e| (tau and the quotient) + E + u |ref| (+ U |ref| for bf16 output).
          E, the absolute error of the device sinf / cosf, is not derivable: MEASURED alone against float64 by tools/probes/row_intrinsics_probe.hip
          over [0, 1100] (2^22 arguments): sinf worst 1.1684 * 2^-24 at 732.78, cosf worst 1.1783 * 2^-24 at 657.37; E = twice the worse.
          t = 0: exactly 0 in the sine half, exactly 1 in the cosine half.
          backward  dts = init + sum_b t_b sum_i +-dout cos|sin(e) / dn: per term |dout t / dn| (2 u |e| + E) + 3 u |term| (product, division, t_b),
          + (depth + batch + 2) u (sum |terms| + |init|), depth = ceil(dim / 256) + 6 (wave) + 3 (block).

Input families (seeded; each asserts its own precondition): random (p, g, m of order one, v >= 0) | first (m = v = 0, every counter 0) |
epsdom (sqrt(v') / bc <= 0.1 eps at t = 1 and t = 1000, asserted on the reference) | cancel (g within 1e-3 relative of m) | tiny (|g| from 1e-20:
g^2 leaves the fp32 normal range) | zerograd (g = m = v = 0: p' EQUALS fl32(p fl32(1 - lr wd)), both moments all-zero bits) | skip (flag != 0: every
bit of p, m, v and the shadow unchanged).  lr = 0: p comes back bit-identical while both moments move.

Worst measured ratios per kernel and family, the probe output and the wall time of each test: profiles/optim_edge_sweep.txt.
"""
import functools
import math
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # (the bars are the GEMM sweep's)
import test_gemm_edges_gpu as G  # noqa: E402

pytestmark = pytest.mark.gpu

u = 2.0 ** -24
U = 2.0 ** -8
FLUSH = 2.0 ** -126
SINCOS_ABS = 2 * 1.1783 * u      # twice the worst |sinf / cosf - float64| over [0, 1100] of tools/probes/row_intrinsics_probe.hip (profiles/optim_edge_sweep.txt)
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
CHUNK, TPB = 65536, 256          # optim.hip CHUNK = MMDIT_ADAMW_CHUNK, TPB
SIZES = (1, 3, 4, 5, 6, 1023, 1024, 1025, 1028, 2047, 2048, 2049, 2052, 65535, 65536, 65537, 65536 + 1027, 2 * 65536, 3 * 65536 + 5)
SMALL_SIZES = SIZES[:13]
# placement -> element offsets of (param, grad, exp_avg, exp_avg_sq) from a 16-byte boundary, and of the bf16 shadow (None: no shadow)
PLACEMENTS = {"aligned": (0, 0, 0, 0, 0), "param+1": (1, 0, 0, 0, 0), "grad+1": (0, 1, 0, 0, 0), "exp_avg+1": (0, 0, 1, 0, 0), "exp_avg_sq+1": (0, 0, 0, 1, 0),
              "all+4": (4, 4, 4, 4, 4), "noshadow": (0, 0, 0, 0, None), "shadow8": (0, 0, 0, 0, 4), "shadow+1": (0, 0, 0, 0, 1)}
STEPS = (0.0, 1.0, 9.0, 999.0, 1e6)
GUARD_F32, GUARD_BF = 0x7FC12345, 0x7FC5      # quiet NaNs with a payload


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ---------------------------------------------------------------------------------------------- the launch arithmetic, restated (see the docstring)
def chunk_map(numels):                            # optim.py _build_table: chunk c = elements [off, off + CHUNK) of tensor chunk_tensor[c]
    ct, co = [], []
    for i, n in enumerate(numels):
        for off in range(0, n, CHUNK):
            ct.append(i)
            co.append(off)
    return ct, co


def chunk_len(numel, off):                        # optim.hip: n = min(CHUNK, numel - off)
    return min(CHUNK, numel - off)


def adamw_path(place, n):                         # optim.hip adamw_kernel -> ("vector" | "scalar", loads in flight, tail elements)
    p, g, m, v, s = PLACEMENTS[place]
    if any((4 * o) & 15 for o in (p, g, m, v)) or (s is not None and (2 * s) & 7):
        return "scalar", 0, n
    n4 = n >> 2
    return "vector", (0 if n4 == 0 else 2 if n4 > TPB else 1), n - 4 * n4


def sumsq_path(place, n):                         # optim.hip grad_sumsq_kernel -> (path, serial adds of one lane)
    if (4 * PLACEMENTS[place][1]) & 15:
        return "scalar", -(-n // TPB)
    n4 = n >> 2
    return "vector", -(-n4 // (2 * TPB)) + 1 + (1 if n & 3 else 0)


def cast_path(src_off, dst_off, n):               # optim.hip cast_multi_kernel -> (path, tail elements)
    if (4 * src_off) & 15 or (2 * dst_off) & 15:
        return "scalar", n
    return "vector", n & 7


def grid_cap(n, bs=256):                          # rowops.hip grid_cap
    return max(1, min(4096, (n + bs - 1) // bs))


def cast_trips(n):                                # rowops.hip mmdit_cast / cast_kernel: trips of the grid-stride loop
    return -(-(n >> 3) // (grid_cap(n // 8 + 1) * 256))


def patch_trips(batch, ch, H, W):                 # rowops.hip patch_dispatch / patch_kernel
    items = batch * ch * H * (W // 2)
    return -(-items // (grid_cap(items) * 256))


class T:
    """One tensor of a grid: numel and placement."""

    def __init__(self, n, place):
        self.n, self.place = n, place


def make_grid(sizes=SIZES, places=tuple(PLACEMENTS)):
    return [T(n, pl) for pl in places for n in sizes]


GRID = make_grid()
SMALL_GRID = make_grid(SMALL_SIZES) + make_grid((65537,), ("aligned", "grad+1", "shadow+1"))      # (what the CPU twin models)
CAST_PLACES = ((0, 0), (1, 0), (0, 1), (1, 1), (4, 8))      # (source offset in fp32 elements, destination offset in bf16 elements)


# ---------------------------------------------------------------------------------------------- arenas
class Arena:
    """Windows (one per tensor; offs[k] None: absent) inside one NaN-filled buffer; everything outside the windows is guard."""

    def __init__(self, dtype, numels, offs, dev):
        al = 16 // torch.empty(0, dtype=dtype).element_size()
        cur, self.starts = 2 * al, []
        for n, o in zip(numels, offs):
            if o is None:
                self.starts.append(None)
                continue
            self.starts.append(cur + o)
            cur = (cur + o + n + al - 1) // al * al + 2 * al
        self.numels, self.dtype, self.al = list(numels), dtype, al
        ibits = torch.int32 if dtype == F32 else torch.int16
        self.buf = torch.full((cur,), GUARD_F32 if dtype == F32 else GUARD_BF, dtype=ibits, device=dev).view(dtype)
        assert self.buf.data_ptr() % 16 == 0
        self.idx = torch.cat([torch.arange(s, s + n) for s, n in zip(self.starts, numels) if s is not None] or [torch.zeros(0, dtype=torch.long)]).to(dev)
        self.snap = None

    def ptr(self, k):
        return 0 if self.starts[k] is None else self.buf.data_ptr() + self.starts[k] * self.buf.element_size()

    def put(self, flat):
        self.buf[self.idx] = flat.to(self.buf.device)

    def get(self):
        return self.buf[self.idx]

    def bits(self, t=None):
        return (self.buf if t is None else t).view(torch.int32 if self.dtype == F32 else torch.int16)

    def snapshot(self):
        self.snap = self.buf.clone()

    def guards_changed(self):
        """Number of words OUTSIDE the windows whose bits differ from the snapshot."""
        d = self.bits() != self.bits(self.snap)
        d[self.idx] = False
        return int(d.sum())

    def windows_changed(self, keep=None):
        """Number of words INSIDE the windows (restricted to the boolean mask `keep` over the flat order) whose bits changed."""
        d = (self.bits() != self.bits(self.snap))[self.idx]
        return int((d if keep is None else d & keep).sum())


class Layout:
    """A grid placed into five arenas (p, g, m, v fp32; s bf16), the device tensor table and the chunk map; flat order = tensor after tensor."""
    REC = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"), ("shadow", "<u8")])

    def __init__(self, grid, dev):
        self.grid, self.dev = grid, dev
        ns = [t.n for t in grid]
        self.numel = sum(ns)
        self.ct, self.co = chunk_map(ns)
        self.clen = [chunk_len(ns[t], o) for t, o in zip(self.ct, self.co)]
        self.tid = torch.repeat_interleave(torch.arange(len(ns)), torch.tensor(ns)).to(dev)               # element -> tensor
        self.cid = torch.repeat_interleave(torch.arange(len(self.ct)), torch.tensor(self.clen)).to(dev)      # element -> chunk
        self.ar = {k: Arena(F32, ns, [PLACEMENTS[t.place][i] for t in grid], dev) for i, k in enumerate("pgmv")}
        self.ar["s"] = Arena(BF, ns, [PLACEMENTS[t.place][4] for t in grid], dev)
        self.has_s = torch.tensor([PLACEMENTS[t.place][4] is not None for t in grid], device=dev)[self.tid]
        rec = np.zeros(len(grid), dtype=self.REC)
        for k, t in enumerate(grid):
            rec[k] = (self.ar["p"].ptr(k), self.ar["g"].ptr(k), self.ar["m"].ptr(k), self.ar["v"].ptr(k), t.n, self.ar["s"].ptr(k))
        if dev != "cpu":
            self.table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
            self.d_ct = torch.tensor(self.ct, dtype=torch.int32, device=dev)
            self.d_co = torch.tensor(self.co, dtype=torch.int64, device=dev)

    def load(self, d):
        for k in "pgmv":
            self.ar[k].put(d[k])
        self.ar["s"].buf[self.ar["s"].idx] = float("nan")      # (stale contents the kernel must overwrite; restored to a fixed NaN pattern)
        for a in self.ar.values():
            a.snapshot()

    def outputs(self):
        o = {k: self.ar[k].get() for k in "pmv"}
        o["s"] = self.ar["s"].get()
        return o


@functools.lru_cache(maxsize=None)
def layout(which, dev):
    return Layout(GRID if which == "full" else SMALL_GRID, dev)


# ---------------------------------------------------------------------------------------------- data
def _gen(*key):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(":".join(str(k) for k in key))) % (1 << 31))


@functools.lru_cache(maxsize=2)
def _base(n, fam):
    g = _gen("optim", fam, n)
    r = lambda: torch.randn(n, generator=g)      # noqa: E731
    if fam == "random":
        return dict(p=r(), g=r(), m=r(), v=r() ** 2)
    if fam == "first":
        return dict(p=r(), g=r(), m=torch.zeros(n), v=torch.zeros(n))
    if fam == "epsdom":
        return dict(p=r(), g=(5e-10 * r()).clamp(-6e-10, 6e-10), m=1e-9 * r(), v=3e-22 * torch.rand(n, generator=g))
    if fam == "cancel":
        m = r()
        m = torch.where(m.abs() < 1e-3, torch.ones(n), m)
        return dict(p=r(), g=m * (1 + 1e-3 * (2 * torch.rand(n, generator=g) - 1)), m=m, v=r() ** 2)
    if fam == "tiny":
        mag = torch.exp(math.log(10.0) * (-20 + 17 * torch.rand(n, generator=g)))
        v = torch.where(torch.rand(n, generator=g) < 0.5, torch.zeros(n), 1e-10 * torch.rand(n, generator=g))
        return dict(p=r(), g=mag * torch.sign(r()), m=1e-3 * r(), v=v)
    if fam in ("zerograd", "skip"):
        z = torch.zeros(n)
        return dict(p=r(), g=z, m=z, v=z) if fam == "zerograd" else dict(p=r(), g=r(), m=r(), v=r() ** 2)
    if fam == "exact":      # small integers: every chunk's sum of squares stays below 2^24
        return dict(p=r(), g=torch.randint(-3, 4, (n,), generator=g).float(), m=r(), v=r() ** 2)
    raise KeyError(fam)


def make_data(lay, fam, hp):
    """The flat operands of a family on lay.dev, the step t of every element (hp['steps']: one counter per launch or a per-tensor cycle) and the
    family's precondition."""
    d = {k: v.to(lay.dev) for k, v in _base(lay.numel, fam).items()}
    steps = hp["steps"]
    per_tensor = torch.tensor([steps[k % len(steps)] for k in range(len(lay.grid))] if isinstance(steps, tuple) else [steps] * len(lay.grid), dtype=F32, device=lay.dev)
    d["steps"] = per_tensor
    d["t"] = per_tensor.double()[lay.tid] + 1.0
    if fam == "cancel":
        assert hp["coef"] is None and float(((d["g"].double() - d["m"].double()).abs() / d["m"].double().abs()).max()) <= 1.01e-3
    if fam == "tiny":
        c = 1.0 if hp["coef"] is None else hp["coef"][0]
        assert bool(((1 - hp["b2"]) * (d["g"].double() * c) ** 2 < FLUSH).any()) and float(d["g"].abs().min()) < 1e-19
    if fam == "first":
        assert float(d["steps"].abs().max()) == 0.0
    return d


def hp_of(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.01, coef=None, steps=STEPS, entry="pt"):
    """coef: None (coef_found == NULL) or (coefficient, flag); steps: a tuple (per-tensor cycle: entry 'pt' only) or one float; entry: which launch."""
    assert entry == "pt" or not isinstance(steps, tuple)
    return dict(lr=lr, b1=betas[0], b2=betas[1], eps=eps, wd=wd, coef=coef, steps=steps, entry=entry)


# ---------------------------------------------------------------------------------------------- the operation in plain torch
def adamw_math(d, hp, dt, fault=None):
    """dt = float64: the reference (closed forms).  dt = float32: a model in torch's own operation order (torch/optim/adamw.py _single_tensor / fused:
    mul_, lerp_, mul_ + addcmul_, sqrt / bias_correction2_sqrt + eps, addcdiv_), with the constants rounded where a float32 tensor meets a python
    float.  fault: None | ('stale' | 'neighbour', j) | 'eps_inside' | 't_off'."""
    p, g, m, v = (d[k].to(dt) for k in "pgmv")
    lr, b1, b2, eps, wd = hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"]
    if hp["coef"] is not None:
        g = g * hp["coef"][0]
    if isinstance(fault, tuple) and fault[0] == "neighbour":
        g = g.clone()
        g[fault[1]] = g[fault[1] + 1]
    t = d["t"] + (1.0 if fault == "t_off" else 0.0)
    ss = (lr / (1.0 - b1 ** t)).to(dt)
    bc = (1.0 - b2 ** t).sqrt().to(dt)
    p1 = p * (1.0 - lr * wd)
    if dt == F64:
        m1 = m + (1.0 - b1) * (g - m)
        v1 = b2 * v + (1.0 - b2) * g * g
    else:
        m1 = torch.lerp(m, g, 1.0 - b1)
        v1 = (v * b2).addcmul(g, g, value=1.0 - b2)
    den = (v1.sqrt() + eps) / bc if fault == "eps_inside" else v1.sqrt() / bc + eps
    p2 = p1 - ss * (m1 / den) if dt == F32 else p1 - ss * m1 / den
    if isinstance(fault, tuple) and fault[0] == "stale":
        j = fault[1]
        p2, m1, v1 = p2.clone(), m1.clone(), v1.clone()
        p2[j], m1[j], v1[j] = p[j], m[j], v[j]
    return dict(p=p2, m=m1, v=v1), dict(g=g, p1=p1, ss=ss, bc=bc, den=den)


def adamw_yard(d, hp, ref, aux):
    """y for p, m, v (float64): the derivation of the docstring, line by line."""
    b1, b2, eps = hp["b1"], hp["b2"], hp["eps"]
    m, v = d["m"].double(), d["v"].double()
    g, p1, ss, bc, den = aux["g"], aux["p1"], aux["ss"], aux["bc"], aux["den"]
    ga = g.abs()
    e_g = u * ga if hp["coef"] is not None else torch.zeros_like(ga)
    e_p1 = 2 * u * p1.abs()
    e_m = e_g * (1 - b1) + u * (ref["m"].abs() + (1 - b1) * 3 * (g - m).abs())
    A, B = b2 * v, (1 - b2) * g * g
    e_v = u * (3 * A + 6 * B) + FLUSH
    s = ref["v"].sqrt()
    e_s = torch.maximum(s - (ref["v"] - e_v).clamp_min(0).sqrt(), (ref["v"] + e_v).sqrt() - s) + u * s
    q = s / bc
    e_q = e_s / bc + 2 * u * q
    e_den = e_q + u * eps + u * den
    num = ss * ref["m"]
    e_num = ss * e_m + 2 * u * num.abs()
    r = num / den
    e_r = e_num / den + r.abs() * e_den / den + u * r.abs()
    return dict(p=e_p1 + e_r + u * ref["p"].abs(), m=e_m, v=e_v)


def bf16_trunc(x):
    return (x.view(torch.int32) & -65536).view(F32).to(BF)


def sumsq_math(d, lay, dt=F64, drop_tail=False):
    """Per-chunk sum of squares (dt = float32: torch's own order per chunk).  drop_tail: the planted fault -- the last element of every chunk missing."""
    g = d["g"].to(dt)
    sq = g * g
    if drop_tail:
        last = torch.tensor(lay.clen, device=g.device).cumsum(0) - 1
        sq = sq.clone()
        sq[last] = 0
    if dt == F64:
        return torch.zeros(len(lay.ct), dtype=F64, device=g.device).index_add_(0, lay.cid, sq)
    return torch.stack([c.sum() for c in sq.split(lay.clen)])


def sumsq_yard(lay, ref):
    depth = torch.tensor([(4 if sumsq_path(lay.grid[t].place, n)[0] == "vector" else 1) + sumsq_path(lay.grid[t].place, n)[1] + 11 for t, n in zip(lay.ct, lay.clen)],
                         dtype=F64, device=ref.device)
    return depth * u * ref + FLUSH * torch.tensor(lay.clen, dtype=F64, device=ref.device)


def clip_math(partials, scale, max_norm, skip=None):
    """float64 (total norm, out0, out1, out2) of mmdit_clip_coef.  skip: the planted fault -- one partial left out of the norm."""
    ps = partials.double()
    if skip is not None:
        ps = torch.cat([ps[:skip], ps[skip + 1:]])
    S = float(ps.sum())
    inv = 1.0 if scale is None else 1.0 / scale
    norm = math.sqrt(S) * inv if S == S and S >= 0 else float("nan")
    clip = min(max_norm / (norm + float(np.float32(1e-6))), 1.0) if max_norm > 0 else 1.0
    return inv * clip, 0.0 if math.isfinite(S) else 1.0, norm


def clip_check(out, ref, failures, what):
    o0, o1, o2 = (float(x) for x in out)
    r0, r1, r2 = ref
    ratios = []
    for name, o, r, k in (("out0", o0, r0, 6), ("out2", o2, r2, 3)):
        y = k * u * abs(r) + 1e-13 * abs(r)
        ratio = abs(o - r) / max(y, G.TINY)
        ratios.append(ratio)
        if not ratio <= G.ELEM_BAR:
            failures.append(f"{what} {name}: {o!r} vs {r!r}, ratio {ratio:.3f}")
    if o1 != r1:
        failures.append(f"{what} found_inf: {o1} vs {r1}")
    return max(ratios)


# ---------------------------------------------------------------------------------------------- comparison and record
WORST = {}             # (kernel, family) -> {what: (ratio, where)}
WALL = {}              # test -> seconds


def _record(kernel, fam, what, ratio, where=""):
    w = WORST.setdefault((kernel, fam), {})
    if ratio > w.get(what, (-1.0, ""))[0]:
        w[what] = (ratio, where)


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\n[optim edge sweep] worst ratio to the yardstick per kernel and input family (bars: per element 2.0, per chunk 1.0)")
    for (k, fam), w in sorted(WORST.items()):
        print(f"  {k:<12} {fam:<9} " + "  ".join(f"{n} {v:.3f}{' @ ' + at if at else ''}" for n, (v, at) in sorted(w.items())))
    print("[optim edge sweep] wall time per test")
    for k, s in sorted(WALL.items()):
        print(f"  {k:<60} {s:.2f} s")


@pytest.fixture(autouse=True)
def _wall(request):
    t0 = time.time()
    yield
    WALL[request.node.name] = time.time() - t0


def chunk_ratios(lay, out, ref, y):
    """(worst per-element ratio, its flat index, worst per-chunk ratio, its chunk): the standing rule with a chunk in the place of a row."""
    diff = out.double() - ref
    el = diff.abs() / y.clamp_min(G.TINY)
    z = lambda: torch.zeros(len(lay.ct), dtype=F64, device=diff.device)      # noqa: E731
    row = (z().index_add_(0, lay.cid, diff * diff).sqrt() / z().index_add_(0, lay.cid, y * y).sqrt().clamp_min(G.TINY))
    return float(el.max()), int(el.argmax()), float(row.max()), int(row.argmax())


def check_adamw(lay, d, hp, fam, out, failures, tag, record=True):
    """p, m, v against the float64 reference under the two bars; returns (ref, worst ratios)."""
    ref, aux = adamw_math(d, hp, F64)
    yard = adamw_yard(d, hp, ref, aux)
    if fam == "epsdom":
        assert float((ref["v"].sqrt() / aux["bc"]).max()) <= 0.1 * hp["eps"], "eps-dominated family: sqrt(v') / bc above 0.1 eps"
    for k in "pmv":
        if not bool(torch.isfinite(out[k]).all()):
            failures.append(f"{tag} {k}: {int((~torch.isfinite(out[k])).sum())} non-finite elements")
            continue
        el, at, row, cat = chunk_ratios(lay, out[k], ref[k], yard[k])
        t = lay.grid[int(lay.tid[at])]
        where = f"n={t.n} {t.place}"
        print(f"[optim edges] adamw {fam} {tag} {k}: elem {el:.3f} @ {at} ({where}) chunk {row:.3f} @ chunk {cat} (n={lay.grid[lay.ct[cat]].n} {lay.grid[lay.ct[cat]].place})")
        if record:
            _record("adamw", fam, k + " elem", el, where)
            _record("adamw", fam, k + " chunk", row, "")
        if not el <= G.ELEM_BAR:
            failures.append(f"{tag} {k}: element ratio {el:.3f} @ {at} ({where})")
        if not row <= G.ROW_BAR:
            failures.append(f"{tag} {k}: chunk ratio {row:.3f} @ chunk {cat}")
    return ref


def check_shadow(lay, out, failures, tag):
    want = out["p"].to(BF).view(torch.int16)
    got = out["s"].view(torch.int16)
    # the flat shadow holds only the tensors that have one
    bad = int((got != want[lay.has_s]).sum())
    print(f"[optim edges] shadow {tag}: {bad} of {got.numel()} differ from bf16(p_out)")
    if bad:
        failures.append(f"{tag} shadow: {bad} elements differ from p_out.to(bfloat16)")


def check_guards(lay, failures, tag, written=("p", "m", "v", "s")):
    for k, a in lay.ar.items():
        n = a.guards_changed()
        if n:
            failures.append(f"{tag} arena {k}: {n} guard words changed")
        if k not in written and a.windows_changed():
            failures.append(f"{tag} arena {k}: an input changed")


# ---------------------------------------------------------------------------------------------- launches
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync_call(call):
    torch.cuda.synchronize()
    try:
        rc = call()
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device error is sticky: nothing more is launched in this session
        pytest.exit(f"device error after an optimizer-kernel launch: {e}", returncode=3)
    assert rc == 0, rc
    return rc


def launch_adamw(lay, d, hp, c0=0, c1=None, entry=None):
    from sd3_amd import _lib
    L = _lib.lib()
    c1 = len(lay.ct) if c1 is None else c1
    entry = entry or hp["entry"]
    cf = None if hp["coef"] is None else torch.tensor([hp["coef"][0], hp["coef"][1], 123.0], dtype=F32, device=lay.dev)
    steps = d["steps"] if entry == "pt" else d["steps"][:1].clone()
    lr_dev = torch.tensor([hp["lr"]], dtype=F64, device=lay.dev)
    head = (lay.table.data_ptr(), lay.d_ct.data_ptr() + 4 * c0, lay.d_co.data_ptr() + 8 * c0, c1 - c0, None if cf is None else cf.data_ptr(), steps.data_ptr())
    tail = (hp["b1"], hp["b2"], hp["eps"], hp["wd"], _stream())
    if entry == "host":
        return _sync_call(lambda: L.mmdit_adamw_step(*head, hp["lr"], *tail))
    fn = L.mmdit_adamw_step_dlr if entry == "dlr" else L.mmdit_adamw_step_dlr_pt
    return _sync_call(lambda: fn(*head, lr_dev.data_ptr(), *tail))


# ---------------------------------------------------------------------------------------------- AdamW
ADAMW_RUNS = [
    ("random", "A", hp_of()),
    ("random", "B", hp_of(betas=(0.5, 0.9), wd=0.1, coef=(2.0 ** -10, 0.0), steps=0.0, entry="dlr")),
    ("random", "C", hp_of(wd=0.0, coef=(0.37, 0.0), steps=9.0, entry="host")),
    ("random", "D", hp_of(lr=0.0, betas=(0.5, 0.9), wd=0.1, coef=(0.37, 0.0))),
    ("random", "E", hp_of(steps=999.0, entry="host")),
    ("random", "F", hp_of(coef=(2.0 ** -10, 0.0), steps=1e6, entry="dlr")),
    ("first", "A", hp_of(steps=(0.0,))),
    ("first", "B", hp_of(betas=(0.5, 0.9), wd=0.0, steps=0.0, entry="host")),
    ("epsdom", "t1", hp_of(steps=(0.0,))),
    ("epsdom", "t1000", hp_of(steps=999.0, entry="dlr")),
    ("cancel", "A", hp_of()),
    ("cancel", "B", hp_of(betas=(0.5, 0.9), wd=0.1, steps=1.0, entry="host")),
    ("tiny", "A", hp_of()),
    ("tiny", "B", hp_of(coef=(2.0 ** -10, 0.0), steps=1.0, entry="dlr")),
    ("zerograd", "wd0", hp_of(wd=0.0)),
    ("zerograd", "wd0.01", hp_of(wd=0.01, coef=(0.37, 0.0), steps=9.0, entry="dlr")),
    ("zerograd", "wd0.1", hp_of(wd=0.1, steps=0.0, entry="host")),
    ("skip", "flag1", hp_of(coef=(0.37, 1.0))),
    ("skip", "flagnan", hp_of(coef=(0.37, float("nan")), steps=1.0, entry="host")),
]


def exact_family_checks(lay, d, hp, fam, out, failures, tag):
    """The bit-level promises of the zerograd / skip families and of lr = 0."""
    i32 = lambda x: x.contiguous().view(torch.int32)      # noqa: E731
    if fam == "zerograd":
        want = d["p"] * torch.tensor(1.0 - hp["lr"] * hp["wd"], dtype=F32, device=d["p"].device)
        if not torch.equal(i32(out["p"]), i32(want)):
            failures.append(f"{tag}: p' differs from fl32(p fl32(1 - lr wd)) on {int((i32(out['p']) != i32(want)).sum())} elements")
        if hp["wd"] == 0.0 and not torch.equal(i32(out["p"]), i32(d["p"])):
            failures.append(f"{tag}: wd = 0 and a zero gradient moved p")
        for k in "mv":
            if int((i32(out[k]) != 0).sum()):
                failures.append(f"{tag}: {k} is not all-zero bits")
    if hp["lr"] == 0.0:
        if not torch.equal(i32(out["p"]), i32(d["p"])):
            failures.append(f"{tag}: lr = 0 changed {int((i32(out['p']) != i32(d['p'])).sum())} parameter elements")
        if fam == "random" and not (bool((out["m"] != d["m"]).any()) and bool((out["v"] != d["v"]).any())):
            failures.append(f"{tag}: lr = 0 and the moments did not move")


def _each(name, cases, fn, ident):
    """Every case of one test in turn (one test id per kernel, not per case: the cases share the arenas and cost a fraction of a second each);
    a case that fails does not hide the ones behind it, and every case's wall time is recorded."""
    failures = []
    for c in cases:
        t0 = time.time()
        try:
            fn(c)
        except AssertionError as e:
            failures.append(f"[{ident(c)}] {e}")
        WALL[f"{name}[{ident(c)}]"] = time.time() - t0
    assert not failures, "\n\n".join(failures)


def _adamw_case(run):
    fam, tag, hp = run
    lay = layout("full", "cuda")
    d = make_data(lay, fam, hp)
    lay.load(d)
    launch_adamw(lay, d, hp)
    out = lay.outputs()
    failures = []
    if fam == "skip":
        for k in "pmvs":
            if lay.ar[k].windows_changed():
                failures.append(f"{tag}: a skipped step changed {lay.ar[k].windows_changed()} words of {k}")
        check_guards(lay, failures, tag, written=())
    else:
        check_adamw(lay, d, hp, fam, out, failures, tag)
        check_shadow(lay, out, failures, tag)
        exact_family_checks(lay, d, hp, fam, out, failures, tag)
        check_guards(lay, failures, tag)
    assert not failures, "\n".join([f"adamw {fam} {tag} {hp}"] + failures)


def test_adamw_edges(ops):
    """Every run of ADAMW_RUNS (family x hyper-parameters x entry point), each ONE launch over the whole shape x placement grid: p, m, v of every
    element and every chunk within the bars against float64, the shadow equal to bf16(p_out), the family's bit-level promises, every guard word of
    every arena and every input bit-identical."""
    _each("adamw", ADAMW_RUNS, _adamw_case, lambda r: f"{r[0]}-{r[1]}")


def test_adamw_host_and_device_learning_rate_agree_bit_for_bit(ops):
    """mmdit_adamw_step (host lr), mmdit_adamw_step_dlr (the same lr from a device double) and mmdit_adamw_step_dlr_pt (every counter equal) give
    bit-identical p, m, v and shadow on the same inputs."""
    lay = layout("full", "cuda")
    hp = hp_of(lr=3e-4 * 0.9, wd=0.1, coef=(0.37, 0.0), steps=9.0, entry="host")
    d = make_data(lay, "random", hp)
    outs = []
    for entry in ("host", "dlr", "pt"):
        lay.load(d)
        launch_adamw(lay, d, hp, entry=entry)
        outs.append(lay.outputs())
    for o in outs[1:]:
        for k in "pmvs":
            assert torch.equal(o[k].view(torch.int16 if k == "s" else torch.int32), outs[0][k].view(torch.int16 if k == "s" else torch.int32)), k


def test_adamw_sub_range_of_the_chunk_map(ops):
    """chunk_tensor / chunk_off advanced past the first tensors, as step_clipped does per param group, with per-tensor counters: the tensors inside
    the range are updated with THEIR counters (the table index is absolute), every tensor outside is bit-untouched."""
    lay = layout("full", "cuda")
    hp = hp_of(coef=(0.37, 0.0))
    d = make_data(lay, "random", hp)
    lay.load(d)
    first, last = 20, 150                             # tensors [first, last) of the 171
    c0, c1 = lay.ct.index(first), lay.ct.index(last)
    assert 0 < c0 < c1 < len(lay.ct)
    launch_adamw(lay, d, hp, c0, c1)
    out = lay.outputs()
    inside = (lay.tid >= first) & (lay.tid < last)
    failures = []
    for k in "pmv":
        n = lay.ar[k].windows_changed(~inside)
        if n:
            failures.append(f"{k}: {n} words of tensors outside the range changed")
    ref, aux = adamw_math(d, hp, F64)
    yard = adamw_yard(d, hp, ref, aux)
    for k in "pmv":
        o = torch.where(inside, out[k].double(), ref[k])
        el, at, row, cat = chunk_ratios(lay, o, ref[k], yard[k])
        print(f"[optim edges] adamw sub-range {k}: elem {el:.3f} chunk {row:.3f}")
        _record("adamw", "subrange", k + " elem", el)
        if not (el <= G.ELEM_BAR and row <= G.ROW_BAR):
            failures.append(f"{k}: element {el:.3f} / chunk {row:.3f} inside the range")
        assert bool((out[k][inside] != d[k][inside]).any())
    sh_in = inside[lay.has_s]
    if not torch.equal(out["s"][sh_in].view(torch.int16), out["p"][lay.has_s][sh_in].to(BF).view(torch.int16)):
        failures.append("shadow inside the range differs from bf16(p_out)")
    if lay.ar["s"].windows_changed(~sh_in):
        failures.append("shadow outside the range changed")
    check_guards(lay, failures, "sub-range")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- grad_sumsq
def _sumsq_case(fam):
    from sd3_amd import _lib
    lay = layout("full", "cuda")
    d = make_data(lay, fam, hp_of())
    lay.load(d)
    nc = len(lay.ct)
    part = torch.full((nc + 16,), float("nan"), device="cuda")
    _sync_call(lambda: _lib.lib().mmdit_grad_sumsq(lay.table.data_ptr(), lay.d_ct.data_ptr(), lay.d_co.data_ptr(), nc, part.data_ptr() + 32, _stream()))
    got = part[8:8 + nc]
    ref = sumsq_math(d, lay)
    failures = []
    if not (bool(torch.isnan(part[:8]).all()) and bool(torch.isnan(part[8 + nc:]).all())):
        failures.append("words around the partials changed")
    ratio = (got.double() - ref).abs() / sumsq_yard(lay, ref).clamp_min(G.TINY)
    at = int(ratio.argmax())
    print(f"[optim edges] grad_sumsq {fam}: worst {float(ratio.max()):.3f} @ chunk {at} (n={lay.grid[lay.ct[at]].n} {lay.grid[lay.ct[at]].place} off {lay.co[at]})")
    _record("grad_sumsq", fam, "chunk", float(ratio.max()), f"n={lay.grid[lay.ct[at]].n} {lay.grid[lay.ct[at]].place}")
    if not float(ratio.max()) <= G.ELEM_BAR:
        failures.append(f"worst ratio {float(ratio.max()):.3f} @ chunk {at}")
    if fam == "exact":
        assert float(ref.max()) < 2 ** 24
        if not torch.equal(got.double(), ref):
            failures.append(f"exact family: {int((got.double() != ref).sum())} partials differ from the float64 sum")
    check_guards(lay, failures, "sumsq", written=())
    for k in "pmvs":
        if lay.ar[k].windows_changed():
            failures.append(f"grad_sumsq wrote into {k}")
    assert not failures, "\n".join(failures)


def test_grad_sumsq_edges(ops):
    """Families random, exact and tiny: per-chunk partials over the same grid (aligned gradients: vector path, grad+1: scalar path) against the
    float64 sum per chunk; the exact family (small integers) must EQUAL it; nothing but the partials is written."""
    _each("grad_sumsq", ("random", "exact", "tiny"), _sumsq_case, str)


# ---------------------------------------------------------------------------------------------- clip_coef
CLIP_N = (1, 255, 256, 257, 1000)
CLIP_SCALES = (None, 1024.0, 65536.0)
CLIP_MAX = (1.0, 0.0, -1.0)


def clip_partials(n, fam, scale, side):
    """Synthetic partials.  random: positive, total norm / scale on the given side of 1 ('above': the clamped branch).  exact: integers whose sum is a
    perfect square."""
    g = _gen("clip", n, fam, side)
    if fam == "exact":
        p = torch.randint(0, 1000, (n,), generator=g).float()
        k = int(math.isqrt(int(p.sum()))) + 1
        p[n // 2] += k * k - int(p.sum())
        assert int(p.double().sum()) == k * k and float(p.max()) < 2 ** 24
        return p
    p = torch.rand(n, generator=g) + 0.01
    target = (3.7 if side == "above" else 0.21) * (scale or 1.0)
    return (p * (target ** 2 / float(p.double().sum()))).float()


def test_clip_coef_edges(ops):
    """n_chunks around the 256-thread strided sum and its tree, three loss scales, max_norm 1 / 0 / < 0, norms on both sides of max_norm, the exact
    family, and non-finite partials in the first, a middle and the last slot."""
    from sd3_amd import _lib
    L = _lib.lib()
    failures = []
    out = torch.full((19,), float("nan"), device="cuda")

    def run(p, scale, max_norm):
        pd = p.cuda()
        sc = None if scale is None else torch.tensor([scale], device="cuda")
        out.fill_(float("nan"))
        _sync_call(lambda: L.mmdit_clip_coef(pd.data_ptr(), pd.numel(), None if sc is None else sc.data_ptr(), max_norm, out.data_ptr() + 32, _stream()))
        if not (bool(torch.isnan(out[:8]).all()) and bool(torch.isnan(out[11:]).all())):
            failures.append("words around out3 changed")
        return out[8:11].cpu()

    seen = set()
    for n in CLIP_N:
        for scale in CLIP_SCALES:
            for max_norm in CLIP_MAX:
                for fam, side in (("random", "above"), ("random", "below"), ("exact", "")):
                    p = clip_partials(n, fam, scale, side)
                    o = run(p, scale, max_norm)
                    ref = clip_math(p, scale, max_norm)
                    what = f"n={n} scale={scale} max_norm={max_norm} {fam} {side}"
                    r = clip_check(o, ref, failures, what)
                    _record("clip_coef", fam, "out", r, what)
                    if max_norm > 0 and fam == "random":
                        seen.add(ref[2] > max_norm)
                    if fam == "exact" and float(o[2]) != ref[2]:
                        failures.append(f"{what}: out[2] {float(o[2])!r} != {ref[2]!r}")
                    if fam == "exact" and max_norm <= 0 and float(o[0]) != ref[0]:
                        failures.append(f"{what}: out[0] {float(o[0])!r} != {ref[0]!r}")
        for bad in (float("inf"), float("-inf") ** 2, float("nan")):
            for slot in sorted({0, n // 2, n - 1}):
                p = clip_partials(n, "random", None, "below")
                p[slot] = bad
                o = run(p, 1024.0, 1.0)
                if float(o[1]) != 1.0:
                    failures.append(f"n={n} {bad} in slot {slot}: found_inf {float(o[1])}")
    assert seen == {True, False}, "both the clamped and the unclamped branch must run"
    print("[optim edges] clip_coef: worst", WORST.get(("clip_coef", "random")), WORST.get(("clip_coef", "exact")))
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- casts
def tie_values(n, g):
    """fp32 values around the bf16 rounding ties: low 16 bits 0x8000 (tie, both parities of the kept part), 0x7fff / 0x8001 (just below / above),
    mixed with N(0, 1)."""
    x = torch.randn(n, generator=g)
    bits = x.view(torch.int32).clone()
    kind = torch.randint(0, 6, (n,), generator=g)
    low = torch.tensor([0x8000, 0x7FFF, 0x8001, 0x0000, 0xFFFF], dtype=torch.int32)
    sel = kind < 5
    bits[sel] = (bits[sel] & -65536) | low[kind[sel]]
    out = bits.view(F32)
    assert bool(torch.isfinite(out).all())
    return out


class CastLayout:
    def __init__(self, dev):
        self.grid = [(n, so, do) for so, do in CAST_PLACES for n in SIZES]
        ns = [n for n, _, _ in self.grid]
        self.src = Arena(F32, ns, [so for _, so, _ in self.grid], dev)
        self.dst = Arena(BF, ns, [do for _, _, do in self.grid], dev)
        self.ct, self.co = chunk_map(ns)
        rec = np.zeros(len(ns), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("numel", "<i8")]))
        for k, n in enumerate(ns):
            rec[k] = (self.src.ptr(k), self.dst.ptr(k), n)
        self.table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        self.numel = sum(ns)


def _cast_multi_case(_):
    """mmdit_cast_multi over the size list x (source aligned or not) x (destination aligned or offset by one bf16 element): the output equals
    src.to(bfloat16) bit for bit at the rounding ties, guards and sources intact."""
    from sd3_amd import _lib
    lay = CastLayout("cuda")
    x = tie_values(lay.numel, _gen("cast_multi")).cuda()
    lay.src.put(x)
    lay.src.snapshot()
    lay.dst.snapshot()
    ct = torch.tensor(lay.ct, dtype=torch.int32, device="cuda")
    co = torch.tensor(lay.co, dtype=torch.int64, device="cuda")
    _sync_call(lambda: _lib.lib().mmdit_cast_multi(lay.table.data_ptr(), ct.data_ptr(), co.data_ptr(), len(lay.ct), _stream()))
    got = lay.dst.get()
    bad = int((got.view(torch.int16) != x.to(BF).view(torch.int16)).sum())
    print(f"[optim edges] cast_multi: {bad} of {got.numel()} elements differ")
    _record("cast_multi", "ties", "mismatches", float(bad))
    assert bad == 0
    assert lay.dst.guards_changed() == 0 and lay.src.guards_changed() == 0 and lay.src.windows_changed() == 0


CAST_N = (1, 7, 8, 9, 15, 2055, 4096 * 256 * 8 + 13)


def _cast_case(n):
    """mmdit_cast in both directions, bit-exact against torch, guards intact; the last length makes the capped grid's stride loop wrap."""
    from sd3_amd import _lib
    L = _lib.lib()
    x = tie_values(n, _gen("cast", n)).cuda()
    dst = Arena(BF, [n], [0], "cuda")
    dst.snapshot()
    _sync_call(lambda: L.mmdit_cast(x.data_ptr(), 0, dst.ptr(0), 1, n, _stream()))
    assert torch.equal(dst.get().view(torch.int16), x.to(BF).view(torch.int16)) and dst.guards_changed() == 0
    xb = x.to(BF)
    back = Arena(F32, [n], [0], "cuda")
    back.snapshot()
    _sync_call(lambda: L.mmdit_cast(xb.data_ptr(), 1, back.ptr(0), 0, n, _stream()))
    assert torch.equal(back.get().view(torch.int32), xb.float().view(torch.int32)) and back.guards_changed() == 0
    _record("cast", "ties", "mismatches", 0.0, f"n={n} trips {cast_trips(n)}")


# ---------------------------------------------------------------------------------------------- patchify / unpatchify
PATCH_SHAPES = ((1, 1, 2, 2), (2, 3, 2, 6), (3, 5, 4, 2), (1, 16, 6, 10), (2, 16, 256, 258))
PATCH_PAIRS = ((F32, F32), (F32, BF), (BF, BF), (BF, F32))


def patch_ref(x, b, c, H, W):
    return x.reshape(b, c, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(b * (H // 2) * (W // 2), c * 4)


def _patch_case(shape):
    """All four dtype pairs: tokens == the reshape / permute expression after the one output rounding, unpatchify the inverse, guards intact."""
    from sd3_amd import _lib
    L = _lib.lib()
    b, c, H, W = shape
    n = b * c * H * W
    code = {F32: 0, BF: 1}
    x32 = tie_values(n, _gen("patch", *shape)).cuda().view(b, c, H, W)
    for ti, to in PATCH_PAIRS:
        x = x32.to(ti)
        tok = Arena(to, [n], [0], "cuda")
        tok.snapshot()
        _sync_call(lambda: L.mmdit_patchify(x.data_ptr(), code[ti], b, c, H, W, tok.ptr(0), code[to], _stream()))
        want = patch_ref(x, b, c, H, W).to(to).reshape(-1)
        assert torch.equal(tok.get(), want) and tok.guards_changed() == 0, (ti, to)
        t_in = want.contiguous()
        img = Arena(ti, [n], [0], "cuda")
        img.snapshot()
        _sync_call(lambda: L.mmdit_unpatchify(t_in.data_ptr(), code[to], b, c, H, W, img.ptr(0), code[ti], _stream()))
        assert torch.equal(img.get().view(b, c, H, W), x.to(to).to(ti)) and img.guards_changed() == 0, (ti, to)      # (equal dtypes: the round trip is the identity)
    _record("patchify", "ties", "mismatches", 0.0, f"{shape} trips {patch_trips(*shape)}")


def test_cast_and_patchify_edges(ops):
    """The copy kernels, bit-exact against torch with guards intact: mmdit_cast_multi over the grid of sizes and placements, mmdit_cast at every
    length of CAST_N in both directions, mmdit_patchify / _unpatchify at every shape of PATCH_SHAPES under all four dtype pairs."""
    _each("cast_multi", (0,), _cast_multi_case, lambda _: "grid")
    _each("cast", CAST_N, _cast_case, str)
    _each("patchify", PATCH_SHAPES, _patch_case, lambda sh: "x".join(map(str, sh)))


# ---------------------------------------------------------------------------------------------- time embedding
TE_DIMS = (2, 254, 256, 258, 768, 1024)
TE_T = (0.0, 2.0 ** -20, 0.5, 1.0)


TE_BATCHES = ((0.0,), (2.0 ** -20,), (0.5,), (1.0,), (0.0, 2.0 ** -20, 0.5), (1.0, 0.5, 0.0))      # batch 1: every t alone; batch 3: all four between two launches


def te_inputs(dim, tvals, dev):
    denom = (torch.tensor(10000.0) ** ((2 * torch.arange(dim)) / dim)).float()
    return torch.tensor(tvals, dtype=F32, device=dev), torch.tensor([1000.0], device=dev), denom.to(dev)


def te_fwd_math(t, ts, denom, dt=F64):
    """(reference, |argument|): sin of t ts / denom[2 i] in the first half, cos of t ts / denom[2 i + 1] in the second."""
    tau = (t.to(dt) * ts.to(dt))[:, None]
    e = torch.cat([tau / denom.to(dt)[None, 0::2], tau / denom.to(dt)[None, 1::2]], 1)
    half = denom.numel() // 2
    return torch.cat([e[:, :half].sin(), e[:, half:].cos()], 1), e.abs()


def te_fwd_yard(ref, e, bf):
    return 2 * u * e + SINCOS_ABS + u * ref.abs() + (U * ref.abs() if bf else 0)


def te_bwd_math(dout, t, ts, denom, init, dt=F64):
    """(init + sum, per-term magnitudes |dout t / dn|, terms, |argument|)."""
    tau = (t.to(dt) * ts.to(dt))[:, None]
    dn = torch.cat([denom.to(dt)[0::2], denom.to(dt)[1::2]])[None]
    e = tau / dn
    half = denom.numel() // 2
    trig = torch.cat([e[:, :half].cos(), -e[:, half:].sin()], 1)
    w = dout.to(dt) * t.to(dt)[:, None] / dn
    terms = w * trig
    return init.to(dt) + terms.sum(), w.abs(), terms, e.abs()


def te_bwd_yard(w, terms, e, init, dim, batch):
    depth = -(-dim // 256) + 6 + 3
    return float((w * (2 * u * e + SINCOS_ABS) + 3 * u * terms.abs()).sum() + (depth + batch + 2) * u * (terms.abs().sum() + abs(float(init))))


def _time_embed_case(dim):
    from sd3_amd import _lib
    L = _lib.lib()
    failures = []
    for tvals in TE_BATCHES:
        batch = len(tvals)
        t, ts, denom = te_inputs(dim, tvals, "cuda")
        ref, e = te_fwd_math(t, ts, denom)
        for dt in (F32, BF):
            out = Arena(dt, [batch * dim], [0], "cuda")
            out.snapshot()
            _sync_call(lambda: L.mmdit_time_embed_fwd(t.data_ptr(), ts.data_ptr(), denom.data_ptr(), batch, dim, out.ptr(0), 0 if dt == F32 else 1, _stream()))
            got = out.get().view(batch, dim)
            ratio = (got.double() - ref).abs() / te_fwd_yard(ref, e, dt == BF)
            rowr = (got.double() - ref).norm(dim=1) / te_fwd_yard(ref, e, dt == BF).norm(dim=1)
            print(f"[optim edges] time_embed_fwd dim {dim} batch {batch} {dt}: elem {float(ratio.max()):.3f} row {float(rowr.max()):.3f}")
            _record("time_embed", "fwd " + ("bf16" if dt == BF else "f32"), "elem", float(ratio.max()), f"dim={dim}")
            _record("time_embed", "fwd " + ("bf16" if dt == BF else "f32"), "row", float(rowr.max()), f"dim={dim}")
            if not (float(ratio.max()) <= G.ELEM_BAR and float(rowr.max()) <= G.ROW_BAR):
                failures.append(f"fwd dim {dim} batch {batch} {dt}: elem {float(ratio.max()):.3f} row {float(rowr.max()):.3f}")
            zero = t == 0
            if bool(zero.any()):
                z = got[zero].float()
                if not (bool((z[:, :dim // 2] == 0).all()) and bool((z[:, dim // 2:] == 1).all())):
                    failures.append(f"fwd dim {dim} {dt}: t = 0 is not exactly (0, 1)")
            if out.guards_changed():
                failures.append(f"fwd dim {dim} {dt}: guard words changed")
        for dt in (F32, BF):
            dout = torch.randn(batch, dim, generator=_gen("te", dim, *tvals)).to(dt).cuda()
            init = torch.tensor([0.37], device="cuda")
            acc = Arena(F32, [1], [0], "cuda")
            acc.put(init)
            acc.snapshot()
            _sync_call(lambda: L.mmdit_time_embed_bwd(dout.data_ptr(), 0 if dt == F32 else 1, t.data_ptr(), ts.data_ptr(), denom.data_ptr(), batch, dim, acc.ptr(0), _stream()))
            want, w, terms, e2 = te_bwd_math(dout, t, ts, denom, init)
            y = te_bwd_yard(w, terms, e2, init, dim, batch)
            r = abs(float(acc.get()[0]) - float(want)) / max(y, G.TINY)
            print(f"[optim edges] time_embed_bwd dim {dim} batch {batch} {dt}: {r:.3f}")
            _record("time_embed", "bwd " + ("bf16" if dt == BF else "f32"), "dts", r, f"dim={dim}")
            if not r <= G.ELEM_BAR:
                failures.append(f"bwd dim {dim} batch {batch} {dt}: ratio {r:.3f}")
            if acc.guards_changed():
                failures.append(f"bwd dim {dim} {dt}: guard words changed")
    assert not failures, "\n".join(failures)


def test_time_embed_edges(ops):
    """Every width of TE_DIMS: forward (fp32 and bf16 output, batch 1 and 3, the four t values) and backward (fp32 and bf16 dout, dtime_scale from
    a non-zero value)."""
    _each("time_embed", TE_DIMS, _time_embed_case, str)
