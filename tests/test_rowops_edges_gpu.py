"""Edge sweep of the row kernels (csrc/rowops.hip) with PER-ELEMENT, PER-ROW and PER-COLUMN float64 parity through the C ABI.

test_kernels_gpu.py holds the row kernels to whole-tensor Frobenius bars against fp32 torch at a handful of workload shapes.  One wrong row of 616,
the last row of a 16-row chunk missing from a dscale sum, the neighbouring sample's modulation row on the last row of a sample, a truncated bf16
output, eps = 1e-6 instead of 1e-5 or a one-pass variance all pass there.  This file runs every row kernel family

  adaLN forward (plain / RES, fp32 / bf16, list of 1 and 2)      every NIT bucket, with and without d = 256 n, rows % 4 = 0 .. 3
  adaLN backward (plain / GATED, dbias, dres, list of 1 and 2)    both flush paths (LDS combine at NIT <= 6, per-lane atomics above), the one-round rch
  text RMSNorm forward / backward                                 range-checked and EXACT instantiations, unequal halves around TRB_ROWS = 64
  QK-norm + RoPE forward / backward                               FAST true / false at rl = 1 and rl > 1, forward with and without same_token
  SwiGLU / GELU forward / backward                                rows around the 8 row lanes, the two rows in flight, CO_RCH = 64, MB_RCH = 128
  gate-residual forward / backward, colsum, SiLU backward, flow loss (their grid-stride loops and chunk switches)
  the MX-emitting adaLN / SwiGLU forms                            bit-identical to "bf16 output + mmdit_mxfp8_quantize"

at the smallest shapes that reach each path.  The product library has no query for the shape of a row launch, so the launch arithmetic is RESTATED
below in pure Python (nit_for / nit_bucket, qk_rl / qk_grid / the fast rule, the forward grid and same_token, the colsum rch, the one-round
rch of a two-problem adaLN backward) and every case carries the path it is meant to reach; tests/test_rowops_edges_cpu.py asserts on that restatement
that every path is present.  The restatement can DRIFT from the C++ and nothing detects that: each restated launcher carries a comment that points
here (rowops.hip: nit_for and NIT_SWITCH, ln_bwd_one_round_rch, qk_rl, qk_bwd_lanes, qk_grid, qk_fwd_launch, qk_bwd_launch, mmdit_colsum).  The QK launch
policy is one rule for head width 64 and 128; it is restated with the width as an argument, and this file runs it at 64 (128: tests/test_attn_hd128_gpu.py).

Reference: plain float64 torch of the operands exactly as the kernel receives them (bf16 values widened, fp32 as is), no ops.* call inside; the
backward kernels read saved statistics (mean / rstd), which the test produces in float64 and rounds to fp32 -- the reference uses those fp32 numbers
as given.  Gradients are closed forms (the *_math functions; the CPU twin checks them against float64 autograd).

Yardstick (derived from the kernels' rounding points, not tuned).  u = 2^-24, U = 2^-8 (bf16), S = depth of the kernel's sum: 4 NIT + 7 for a row
reduction in one wave (4 NIT serial adds per lane, 6 butterfly steps, the division), (terms + 2) in any order for column sums that end in atomics.
|.| is elementwise, mean / sum run over the row (or, for column sums, over the rows of the sample).

  adaLN forward   x1 = x + gate acc (RES: ex = 2 u (|x| + |gate acc|), written as x_out; plain: ex = 0), m = mean x1, v = mean (x1 - m)^2, r = rstd
                  dm  = S u mean|x1| + mean ex                 dc = dm + u |x1 - m| + ex
                  dv  = (S + 4) u v + dm^2 + 2 mean(|x1 - m| ex)        dr = r (0.5 dv / (v + eps) + 2 u)
                  y   = |1 + a| (r dc + |x1 - m| dr) + 3 u |ref - shift| + u |ref|   (+ U |ref| for a bf16 output);  mean is held to dm, rstd to dr
  adaLN backward  xh = (x - mean) rstd, g = dy (1 + a), c1 = mean g, c2 = mean g xh, dx = dres + rstd (g - c1 - xh c2)
                  e_xh = 2 u |xh|, e_g = 2 u |g|, dc1 = S u mean|g| + mean e_g, dc2 = (S + 1) u mean|g xh| + mean(|g| e_xh + e_g |xh|)
                  y_dx = rstd (e_g + dc1 + e_xh |c2| + |xh| dc2) + 3 u rstd (|g| + |c1| + |xh c2|) + u |dres| + u |dx|
                  dacc = dx gate: |gate| y_dx + u |dacc| (+ U |dacc|);  per-sample column sums over T = rows_per_batch terms, summed BEFORE any rounding:
                  dscale: sum(|dy| e_xh + u |dy xh|) + (T + 2) u sum|dy xh|      dshift: (T + 2) u sum|dy|  
                  dgate:  sum(y_dx |acc| + u |dx acc|) + (T + 2) u sum|dx acc|   dbias:  sum(|gate| y_dx + u |dacc|) + (T + 2) u sum|dacc|
                  (every accumulated output, here and below: each atomic add rounds relative to the running sum, which contains the initial contents, so
                  init is one more summand of the chain: sum|.| includes |init|)
  RMSNorm         q = mean x^2, r = rsqrt(q + eps): dq = (S + 1) u q, dr = r (0.5 dq / (q + eps) + 2 u), xn = x r: e_xn = |x| dr + u |xn|
                  forward  y = |s w| e_xn + 2 u |ref| (+ U |ref|)
                  backward dw: sum(|dy s| e_xn + 2 u |dy s xn|) + (rows + 2) u sum|dy s xn|
                           ds: sum(|dy w| e_xn + 2 u |dy xn w|) + (32 NIT + 9 + workgroups) u sum|dy xn w|     (8 waves x 4 NIT terms per row and lane)
  QK-norm + RoPE  the RMSNorm forms over 64 elements with S = 12 (8 serial adds, 3 butterfly steps, the scaling); n = xn w: e_n = |w| e_xn + u |n|
                  RoPE (a, b) -> (a c0 - b s0, b c1 + a s1): y = |c| e_n,a + |s| e_n,b + 2 u (|a c| + |b s|) + U |ref|; V is a copy (U |ref| from fp32)
                  backward dz' = RoPE^T dz: e_dz = 2 u (|da c| + |db s|); dzw = dz' w: e_dzw = |w| e_dz + u |dzw|; dot = mean dzw xn:
                  ddot = 12 u mean|dzw xn| + mean(e_dzw |xn| + |dzw| e_xn)
                  y = r (e_dzw + e_xn |dot| + |xn| ddot + 2 u (|dzw| + |xn dot|)) + dr |dzw - xn dot| + u |ref| (+ U |ref|); the dV part is a copy
                  dwq / dwk: sum(e_dz |xn| + |dz'| e_xn + u |dz' xn|) + (rows heads + 2) u sum|dz' xn|
  SwiGLU          h = silu(g) u with the sigmoid evaluated in fp32 (v_exp_f32 on g log2 e, v_rcp_f32): the 8 * 2^-23 (1 + |g|) term of the GEMM file,
                  y = 8 * 2^-23 (1 + |g|) |h| + 2^-126 (1 + |u|) (results below the fp32 normal range are flushed) + U |h|
                  backward (common.h swiglu_bwd_f) as in the GEMM file: y = 8 * 2^-23 (1 + |g|) |dh| |u or 1| + 2^-126 + U |ref|
  GELU            h = 0.5 x (1 + erf(x / sqrt 2)): the error of 1.f + erff(x * 0.70710678f) is not derivable (erff is a library polynomial), so it is MEASURED
                  alone against float64 by tools/probes/row_intrinsics_probe.hip over x in [-12, 12] and +-20, +-100: worst 1.2726 * 2^-23 absolute;
                  E = twice that.  y = 0.5 |x| E + 2 u |h| + U |h|;  gradient 0.5 (1 + erf) + x phi(x), phi through v_exp_f32 on t = -x^2 / 2:
                  y = |dh| (0.5 E + |x| phi 8 * 2^-23 (1 + |t|)) + 2 u |ref| + U |ref|
                  (the same probe puts v_exp_f32 / v_rcp_f32 in the sigmoid at 1.10 of (1 + |g|) 2^-23, phi at 0.94 of (1 + |t|) 2^-23 and rsqrtf at 1.58 u:
                  inside the 8 * 2^-23 (1 + |.|) and 2 u terms above, which stay as derived)
                  dbias (both activations): summed before rounding: colsum(y_det) + (rows + 2) u colsum|ref|
  gate residual   out = x + gate acc: 2 u (|x| + |gate acc|); backward dacc = dy gate: u |ref| (+ U |ref|); dgate / dbias: sum(u |term|) + (T + 2) u (sum|terms| + |init|)   (each product dy acc, dy gate is rounded once before it is summed)
  colsum          (rows + 2) u (sum|x| + |init|)
  SiLU backward   dpre = dy s (1 + p (1 - s)): 8 * 2^-23 (1 + |p|) |dy| + 2^-126 + U |ref|; dbias: sum of the above + (rows per group + 2) u sum|ref|
  flow loss       label = eps - x0 (bf16 inputs: rounded to fp32, then to bf16, as torch's bf16 subtraction does -- the reference does the same),
                  d = v - label, dv = 2 coef d (coef arrives rounded to fp32): 2 coef (u |label| (fp32 inputs only) + u |d|) + 2 u |dv|, compared as (n / 8, 8)
                  loss = coef sum d^2: (8 ceil(n / 8 / threads) + 23) u |loss| + 2 coef sum(|d| e_d)

and every output of every case must satisfy, for every element, every row and every column, with nothing exempt (test_gemm_edges_gpu.ratios / verdict),

  |out - ref| <= 2.0 y          ||out_row - ref_row||_2 <= 1.0 ||y_row||_2          ||out_col - ref_col||_2 <= 1.0 ||y_col||_2
  bf16 outputs of >= 64 elements:  |sum_j sign(ref_j) (out_j - ref_j)| <= 6 ||y_rnd||_2 + ||y_det||_1                      (catches truncation)

Input families (seeded; each asserts its own precondition):
  random      x = 0.5 + 2 N(0, 1) and N(0, 1) elsewhere; every sample has its own scale / shift / gate row with its own magnitude.  Every case.
  offset      (norms) x = 100 + N(0, 1): a one-pass variance loses 7 digits.
  smallvar    (norms) row standard deviation <= 3e-3 (LayerNorm: x = 1.5 + 2e-3 N) or rms <= 1.2e-3 (RMS kernels), so eps carries more than 5 % of
              rstd; row 0 is constant (all-zero for the RMS kernels): out must equal shift rounded to the output dtype bit for bit, mean the value.
  saturating  (activations) g in {+-20, +-100} mixed into the random data: every output finite and within the bars.
  exact       (colsum, gate residual, edge shapes) small integers and power-of-two gates: every partial sum is exact, out must EQUAL the reference.
  poison      (list launches: edge shapes of adaLN and the MLP backward, EVERY QK case) operands are views into larger NaN-filled tensors (256 NaN rows behind, ld_mod / ld_gate / ld_dmod /
              ld_dgate / ld_dbias = d + 8), outputs sit between 256 guard rows whose bit pattern must come back identical.  Every byte a clamped
              re-read can touch (the QK kernels re-read row rows - 1) lies inside a tensor the test allocated: this family checks values, not faults.
Accumulated outputs (dscale, dshift, dgate, dbias, dwq, dwk, dw, ds, the colsum out) start from non-zero contents and are held to init + sum.

rows % 4 = 0 .. 3 cannot come from rpb in {1, 3, 17, 33} and batch in {1, 3} alone (products of odd numbers): batch 2 and 4 are added; d = 764 and 768
are added to the adaLN widths for NIT bucket 3.

Worst measured ratios per kernel family and input family: profiles/rowops_edge_sweep.txt.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # (the comparator is the GEMM sweep's)
import test_gemm_edges_gpu as G  # noqa: E402

pytestmark = pytest.mark.gpu

u = 2.0 ** -24
U = 2.0 ** -8
E23 = 2.0 ** -23
LN_EPS = 1e-5              # rowops.hip LN_EPS
RMS_EPS = 2.0 ** -23       # qk_rows.h RMS_EPS = FLT_EPSILON
FLUSH = 2.0 ** -126        # smallest normal fp32: the kernels' arithmetic flushes what lies below
ERF_ABS = 2 * 1.2726 * E23     # twice the worst |1.f + erff(x / sqrt 2) - (1 + erf)| of tools/probes/row_intrinsics_probe.hip (profiles/rowops_edge_sweep.txt)
GUARD = 256
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DT = {"bf16": BF, "f32": F32}


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ---------------------------------------------------------------------------------------------- the launch arithmetic, restated (see the docstring)
NIT_BUCKETS = (1, 2, 3, 4, 6, 9, 12, 16)


def nit_for(d):                                   # rowops.hip:1037 nit_for
    return (d // 4 + 63) // 64


def nit_bucket(d):                                # rowops.hip:1047-1057 NIT_SWITCH
    return next(b for b in NIT_BUCKETS if nit_for(d) <= b)


def ln_bwd_flush(d):                              # rowops.hip:217 ln_mod_bwd_body: `if constexpr (NIT <= 6)`
    return "lds" if nit_bucket(d) <= 6 else "atomics"


def ln_bwd_rch(probs, d, cus=256):                # rowops.hip:1136-1168 ln_bwd_one_round_rch (the occupancy query can only lower per_cu)
    if len(probs) != 2:
        return 16
    per_cu = 4 if nit_for(d) <= 3 else 3 if nit_for(d) == 4 else 2
    wgs = lambda r: sum(b * ((rpb + r - 1) // r) for b, rpb in probs)      # noqa: E731
    slots = cus * per_cu
    if slots < wgs(16) <= 2 * slots:
        for r in range(20, 65, 4):
            if wgs(r) <= slots:
                return r
    return 16


def qk_bwd_rl(heads, min_rows, hd=64):            # rowops.hip:1252-1258 qk_rl (row_threads = 3 * hd / 8 * heads)
    rl = 1024 // (3 * hd // 8 * heads)
    return 1 if rl < 1 or min_rows < 2048 else rl


def qk_grid(rows, tokens, rope, lanes_max, rl, hd=64):       # rowops.hip:1263-1273 qk_grid
    lanes = min(rows, lanes_max)
    if rope and tokens <= lanes:
        k = lanes // tokens
        while k > 1 and (k * tokens) % rl:
            k -= 1
        if (k * tokens) % rl == 0:
            return k * tokens // rl
    if hd == 64 and rope and tokens > lanes and tokens <= rows and tokens <= (2048 if rl > 1 else 1024) and tokens % rl == 0:
        return tokens // rl
    return max(lanes // rl, 1)


def qk_bwd_grid(rows, tokens, rope, rl, lanes_max=768, hd=64):      # rowops.hip:1259-1262 qk_bwd_lanes, then qk_grid
    return qk_grid(rows, tokens, rope, lanes_max if rl > 1 else 512, rl, hd)


def qk_bwd_path(batch, heads, streams, hd=64):    # rowops.hip:1300-1306 qk_bwd_launch; streams: ((tokens, rope), ...) -> (rl, fast = QK_ONCE; width 128 runs QK_PER_ROW whatever it is)
    rl = qk_bwd_rl(heads, min(batch * t for t, _ in streams), hd)
    fast = all((not rope) or (qk_bwd_grid(batch * t, t, rope, rl, hd=hd) * rl) % t == 0 for t, rope in streams)
    return rl, fast


def qk_fwd_path(batch, tokens, rope, hd=64):      # rowops.hip:1284 qk_fwd_launch and :402 qk_norm_rope_fwd_body -> (grid, same_token)
    g = qk_grid(batch * tokens, tokens, rope, 1024, 1, hd)
    return g, bool(rope and g % tokens == 0)


def colsum_rch(rows):                             # rowops.hip:1497 mmdit_colsum
    return 8 if rows <= 256 else 64


# ---------------------------------------------------------------------------------------------- cases
class C:
    """One case: kernel family (`kind`), the path it is meant to reach (`path`, from the restatement), whether its shape sits on an edge (the
    exact / poison families run there), and the shape parameters."""

    def __init__(self, kind, path, edge=False, **kw):
        self.kind, self.path, self.edge, self.kw = kind, path, edge, kw
        self.__dict__.update(kw)

    @property
    def id(self):
        def f(v):
            return "x".join(f(e) for e in v) if isinstance(v, (tuple, list)) else str(int(v)) if isinstance(v, bool) else str(v)
        return self.kind + ":" + ",".join(f"{k}={f(v)}" for k, v in self.kw.items())


LN_D = (4, 252, 256, 260, 512, 764, 768, 772, 1024, 1028, 1536, 1540, 2304, 2308, 3072, 3076, 4096)
LN_FWD_SHAPES = ((1, 1), (3, 3), (1, 17), (3, 33), (2, 17), (4, 3), (3, 1), (1, 33))      # (batch, rows per sample): rows % 4 = 1 1 1 3 2 0 3 1
LN_BWD_RPB = (1, 3, 4, 5, 15, 16, 17, 31, 33)


def _ln_path(d):
    return f"nit{nit_bucket(d)}" + ("" if d % 256 else " d=256n")


def _cases():
    out = []
    add = out.append
    # ---- adaLN forward: every d plain and RES, dtypes alternating, every third launch a list of two with the text problem first
    for i, d in enumerate(LN_D):
        for j in range(2):
            shape = LN_FWD_SHAPES[(2 * i + j) % 8]
            probs = (shape,) if (i + j) % 3 else ((2, 5), shape)
            add(C("ln_fwd", _ln_path(d), edge=d % 256 != 0, d=d, probs=probs, res=j == 1, dt=("f32", "bf16")[(i + j) % 2]))
    # ---- adaLN backward: every d plain and GATED; rpb walks around the 16-row chunk and the 4 waves; batch 2 (per-sample sums)
    k = 0
    for i, d in enumerate(LN_D):
        for j in range(2):
            rpb = LN_BWD_RPB[k % 9]
            k += 1
            probs = ((2, rpb),) if (i + j) % 4 else ((3, 7), (2, rpb))
            add(C("ln_bwd", _ln_path(d) + " flush " + ln_bwd_flush(d) + f" rch{ln_bwd_rch(probs, d)}", edge=d % 256 != 0, d=d, probs=probs,
                  gated=j == 1, dbias=j == 1 and i % 2 == 0, dres=(i // 2 + j) % 2 == 0, dt=("bf16", "f32")[(i + j) % 2]))
    for rpb in LN_BWD_RPB:      # ... every rpb at one width of each flush path
        add(C("ln_bwd", _ln_path(260) + " flush lds rch16", edge=True, d=260, probs=((2, rpb),), gated=True, dbias=rpb % 3 != 0, dres=rpb % 2 == 1, dt=("bf16", "f32")[(rpb // 2) % 2]))
        add(C("ln_bwd", _ln_path(1540) + " flush atomics rch16", edge=True, d=1540, probs=((2, rpb),), gated=rpb % 2 == 1, dbias=rpb % 4 == 1, dres=(rpb // 2) % 2 == 0, dt=("f32", "bf16")[(rpb // 4) % 2]))
    one_round = ((300, 40), (300, 24))      # 1500 workgroups of 16 rows on 1024 slots: rch = 24 on 256 CUs (values must hold whatever the device picks)
    add(C("ln_bwd", _ln_path(64) + f" flush lds rch{ln_bwd_rch(one_round, 64)}", d=64, probs=one_round, gated=True, dbias=True, dres=True, dt="bf16"))
    # ---- text RMSNorm forward + backward: (tokens, split, batch) puts the halves' rows at 63 / 64 / 65 / 129 and on both sides of TRB_ROWS = 64
    pairs = (("f32", "f32"), ("f32", "bf16"), ("bf16", "bf16"), ("bf16", "f32"))
    k = 0
    for d in (4, 256, 260, 1024, 2304, 2308, 4096):
        for tokens, split, batch in ((2, 1, 63), (2, 1, 64), (2, 1, 65), (2, 1, 129), (10, 3, 9), (10, 7, 9), (10, 3, 21), (131, 1, 1), (154, 77, 1)) \
                + (((131, 1, 64),) if d == 4 else ()):
            r1, r2 = batch * split, batch * (tokens - split)
            add(C("rms", _ln_path(d) + (" halves unequal" if (r1 + 63) // 64 != (r2 + 63) // 64 else " halves equal"), d=d, tokens=tokens, split=split,
                  batch=batch, ti=pairs[k % 4][0], tg=pairs[k % 4][1]))
            k += 1
    # ---- QK-norm + RoPE forward + backward: (batch, heads, tokens), streams = ((tokens, rope), ...) in launch order, dtype combo 0 / 1 / 2
    def qk(batch, heads, streams, combo, pad=(0, 0)):
        rl, fast = qk_bwd_path(batch, heads, streams)
        st = [qk_fwd_path(batch, t, r)[1] for t, r in streams if r]
        add(C("qk", f"rl{rl} {'fast' if fast else 'general'} fwd same_token {'/'.join(str(int(s)) for s in st) or 'n/a'}", edge=True,
              batch=batch, heads=heads, streams=streams, combo=combo, pad=pad))
    for combo in (0, 1, 2):
        qk(1, 1, ((1, True),), combo, (5, 2))
        qk(2, 3, ((24, True),), combo, (3, 0))
        qk(2, 3, ((24, True), (10, False)), combo)
        qk(2, 3, ((10, False), (24, True)), combo, (0, 4))
    qk(3, 42, ((6, True),), 0)
    qk(3, 42, ((6, True), (5, False)), 2)
    qk(1, 1, ((33 * 32, True),), 0, (7, 0))
    qk(1, 1, ((33 * 32, True),), 1)
    qk(1, 1, ((7, False), (33 * 32, True)), 2)
    qk(16, 5, ((135, True),), 0)
    qk(16, 5, ((135, True), (135, False)), 2)
    qk(2, 12, ((1024, True),), 0)
    qk(2, 12, ((1024, True),), 2)
    qk(2, 16, ((1024, True),), 0)
    qk(9, 2, ((256, True),), 1)
    qk(9, 2, ((256, False), (256, True)), 0)
    qk(700, 1, ((3, False),), 0)
    qk(700, 1, ((3, False),), 1, (2, 3))
    # ---- MLP activation forward + backward: rows around the 8 row lanes, two rows in flight (16), CO_RCH = 64, MB_RCH = 128
    mlp_rows = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129)
    k = 0
    for hidden in (8, 248, 256, 264, 520):
        for j in range(4):      # four row counts per width, walking the list; GELU / SwiGLU and the dtypes alternate
            rows = mlp_rows[k % 13]
            k += 1
            lst = (rows,) if j % 2 == 0 else (mlp_rows[(k + 5) % 13], rows)
            add(C("mlp", f"rows {lst}", edge=hidden % 256 != 0, hidden=hidden, rows=lst, gelu=j >= 2, dt=("bf16", "f32")[(k + j // 2) % 2], dbias=j != 2))
    for rows in mlp_rows:      # ... every row count at one ragged width
        add(C("mlp", f"rows {rows}", edge=True, hidden=264, rows=(rows,), gelu=rows % 2 == 0, dt="bf16", dbias=True))
    # ---- gate residual forward (2100 x 2048: 1 075 200 groups of 4 on 4096 x 256 threads, the grid stride iterates) and backward
    for d, batch, rpb, dt in ((4, 3, 5, "f32"), (8, 2, 7, "bf16"), (260, 3, 33, "bf16"), (260, 1, 1, "f32")):
        add(C("gr_fwd", "one pass", edge=True, d=d, batch=batch, rpb=rpb, dt=dt))
    add(C("gr_fwd", "grid stride", d=2048, batch=3, rpb=700, dt="bf16"))
    k = 0
    for rpb in (1, 7, 8, 9, 63, 64, 65, 72, 73):
        d = (8, 248, 264)[k % 3]
        add(C("gr_bwd", f"chunks {(rpb + 63) // 64}", edge=True, d=d, batch=2, rpb=rpb, dt=("bf16", "f32")[k % 2], dbias=(None, "vec", "per")[k % 3]))
        add(C("gr_bwd", f"chunks {(rpb + 63) // 64}", edge=True, d=(8, 248, 264)[(k + 1) % 3], batch=3, rpb=rpb, dt=("f32", "bf16")[k % 2], dbias=("per", None, "vec")[k % 3]))
        k += 1
    # ---- colsum: the switch from 8-row to 64-row chunks at 256 rows, cols around the 1024-column slab, a strided view
    k = 0
    for rows in (1, 2, 7, 8, 9, 255, 256, 257, 321):
        for cols in ((8, 1016), (1024, 1032), (1016, 1032))[k % 3]:
            add(C("colsum", f"rch{colsum_rch(rows)}", edge=True, rows=rows, cols=cols, dt=("f32", "bf16")[k % 2], strided=(k // 2 + (cols > 1020)) % 2 == 1))
        k += 1
    # ---- SiLU backward: cols around the 64-column block, rows per group around the 4 row lanes
    k = 0
    for cols in (1, 63, 64, 65):
        for rpg in (1, 3, 4, 5):
            add(C("silu_bwd", "rows per group " + str(rpg), cols=cols, rpg=rpg, groups=3, pair=(("bf16", "bf16"), ("f32", "f32"), ("f32", "bf16"))[k % 3], dbias=k % 4 != 3))
            k += 1
    # ---- flow loss: one workgroup, the 2048-element workgroup edge, a 256-workgroup grid that strides
    for n in (8, 2040, 2048, 2056, 524288 + 8, 3 * 524288 + 16):
        for dt in ("bf16", "f32"):
            add(C("flow", "grid stride" if n > 524288 else "one pass", n=n, dt=dt))
    # ---- MX-emitting forms: rows off the 4-row workgroup and the 128-row scale padding
    for rows, width in ((1, 64), (129, 320), (131, 1536)):
        add(C("mx", "bit-identical", rows=rows, width=width))
    return out


ALL = _cases()
FAMILIES = {"ln_fwd": ("random", "offset", "smallvar"), "ln_bwd": ("random", "offset", "smallvar"), "rms": ("random", "offset", "smallvar"),
            "qk": ("random", "smallvar"), "mlp": ("random", "saturating"), "gr_fwd": ("random",), "gr_bwd": ("random",), "colsum": ("random",),
            "silu_bwd": ("random", "saturating"), "flow": ("random",), "mx": ("random",)}
EDGE_FAMILIES = {"ln_fwd": ("poison",), "ln_bwd": ("poison",), "qk": ("poison",), "mlp": ("poison",), "gr_fwd": ("exact",), "gr_bwd": ("exact",), "colsum": ("exact",)}
CASES = [(c, f) for c in ALL for f in FAMILIES[c.kind]] + [(c, f) for c in ALL if c.edge for f in EDGE_FAMILIES.get(c.kind, ())]


def _case_id(case):
    return f"{case[0].id}-{case[1]}"


# ---------------------------------------------------------------------------------------------- data
def _gen(c, idx):
    return torch.Generator().manual_seed((sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) * 31 + idx) % (1 << 31))


def _rn(g, *s):
    return torch.randn(*s, generator=g)


def _ri(g, lo, hi, *s):
    return torch.randint(lo, hi + 1, s, generator=g).float()


def _pow2(g, *s):
    return torch.exp2(_ri(g, -2, 2, *s)) * (2 * _ri(g, 0, 1, *s) - 1)


def _bidx(rows, rpb, dev):
    return torch.arange(rows, device=dev) // rpb


def _cap_rows(z, cap, std):
    """Rows of z scaled down (never up) until their standard deviation (std) or rms is at most cap."""
    m = z.double().std(-1, unbiased=False, keepdim=True) if std else (z.double() ** 2).mean(-1, keepdim=True).sqrt()
    return z * (cap / m.clamp_min(1e-30)).clamp(max=1.0).float()


def _norm_x(g, fam, rows, d):
    if fam == "offset":
        x = 100.0 + _rn(g, rows, d)
        assert float(x.mean(1).abs().min()) > 90.0
    elif fam == "smallvar":
        x = 1.5 + _cap_rows(2e-3 * _rn(g, rows, d), 2.2e-3, True)
        x[0] = 1.5
    else:
        x = 0.5 + 2.0 * _rn(g, rows, d)
    return x


def data_ln(c, fam):
    """adaLN forward and backward problems: x fp32, per-sample scale / shift / gate rows of distinct magnitude, acc / dout in the case's dtype, the
    saved statistics in float64 rounded to fp32, non-zero initial contents of every accumulated output."""
    ts = []
    for i, (batch, rpb) in enumerate(c.probs):
        g = _gen(c, i)
        rows, d, dt = batch * rpb, c.d, DT[c.dt]
        t = dict(B=batch, rpb=rpb, x=_norm_x(g, fam, rows, d))
        mag = torch.arange(1, batch + 1).float()[:, None]
        t["scale"], t["shift"], t["gate"] = 0.3 * mag * _rn(g, batch, d), _rn(g, batch, d) + 3.0 * (mag - 1), mag * _rn(g, batch, d)
        t["acc"] = ((1e-4 if fam == "smallvar" else 1.0) * _rn(g, rows, d)).to(dt)
        if fam == "smallvar":
            t["acc"][0] = 0
        if c.kind == "ln_bwd":
            t["dout"] = _rn(g, rows, d).to(dt)
            t["dres"] = _rn(g, rows, d) if c.dres else None
            x64 = t["x"].double()
            m = x64.mean(1, keepdim=True)
            t["mean"], t["rstd"] = m.float(), (((x64 - m) ** 2).mean(1, keepdim=True) + LN_EPS).rsqrt().float()
            for k in ("dscale0", "dshift0", "dgate0", "dbias0"):
                t[k] = _rn(g, batch, d)
        if fam == "smallvar":
            x1 = t["x"].double() + (t["gate"].double()[_bidx(rows, rpb, "cpu")] * t["acc"].double() if c.kind == "ln_fwd" and c.res else 0)
            assert float(x1.std(1, unbiased=False).max()) <= 3e-3, "small-variance family: row standard deviation above 3e-3"
        ts.append(t)
    return ts


def data_rms(c, fam):
    g = _gen(c, 0)
    B, T, d, sp = c.batch, c.tokens, c.d, c.split
    x = 100.0 + _rn(g, B, T, d) if fam == "offset" else _cap_rows(1e-3 * _rn(g, B, T, d), 1.1e-3, False) if fam == "smallvar" else 0.5 + 2.0 * _rn(g, B, T, d)
    if fam == "smallvar":
        x[0, 0] = 0
        x[0, sp] = 0
    x = x.to(DT[c.ti])
    if fam == "smallvar":
        assert float((x.double() ** 2).mean(-1).sqrt().max()) <= 1.2e-3, "small-variance family: rms above 1.2e-3"
    t = dict(x=x, w1=1.0 + 0.3 * _rn(g, d), w2=1.0 + 0.3 * _rn(g, d), s1=torch.tensor([1.7]), s2=torch.tensor([-0.6]),
             dout1=_rn(g, B * sp, d).to(DT[c.tg]), dout2=_rn(g, B * (T - sp), d).to(DT[c.tg]))
    for k, n in (("dw10", d), ("dw20", d), ("ds10", 1), ("ds20", 1)):
        t[k] = _rn(g, n)
    return [t]


def qk_dtypes(combo):
    """(dQ / dK / dV, saved qkv, dqkv) of qk_rows.h qk_bwd_combo."""
    return ((BF, BF, BF), (F32, F32, F32), (BF, F32, F32))[combo]


def data_qk(c, fam):
    tg, ti, to = qk_dtypes(c.combo)
    B, H = c.batch, c.heads
    S = c.pad[0] + sum(t for t, _ in c.streams) + c.pad[1]
    g = _gen(c, 0)
    dQ, dK, dV = (_rn(g, B, H, S, 64).to(tg) for _ in range(3))
    ts, tok0 = [], c.pad[0]
    for i, (T, rope) in enumerate(c.streams):
        g = _gen(c, i + 1)
        qkv = _rn(g, B * T, 3 * H * 64)
        if fam == "smallvar":
            qkv = _cap_rows(1e-3 * qkv.view(-1, 64), 1.1e-3, False).view(B * T, 3 * H * 64)
        if fam == "smallvar":
            qkv[0, :64] = 0
        qkv = qkv.to(ti)
        if fam == "smallvar":
            assert float((qkv.double().view(-1, 64) ** 2).mean(-1).sqrt().max()) <= 1.3e-3
        t = dict(B=B, H=H, T=T, S=S, tok0=tok0, qkv=qkv, wq=1.0 + 0.3 * _rn(g, 64), wk=1.0 + 0.3 * _rn(g, 64), dQ=dQ, dK=dK, dV=dV,
                 cos=2 * torch.rand(T, 64, generator=g) - 1 if rope else None, sin=2 * torch.rand(T, 64, generator=g) - 1 if rope else None,
                 dwq0=_rn(g, 64), dwk0=_rn(g, 64))
        ts.append(t)
        tok0 += T
    return ts


def _saturate(g, x):
    pick = torch.rand(x.shape, generator=g) < 0.05
    vals = torch.tensor([20.0, -20.0, 100.0, -100.0])[torch.randint(0, 4, x.shape, generator=g)]
    out = torch.where(pick, vals, x)
    assert bool(pick.any()) or x.numel() < 64
    return out


def data_mlp(c, fam):
    ts = []
    for i, rows in enumerate(c.rows):
        g = _gen(c, i)
        h, dt = c.hidden, DT[c.dt]
        gu = 2.0 * _rn(g, rows, h if c.gelu else 2 * h)
        if fam == "saturating":
            gu[:, :h] = _saturate(g, gu[:, :h])
            gu[0, 0], gu[-1, h - 1] = -100.0, 20.0
        ts.append(dict(gu=gu.to(dt), dh=_rn(g, rows, h).to(dt), dbias0=_rn(g, h if c.gelu else 2 * h) if c.dbias else None))
    return ts


def data_gr(c, fam):
    g = _gen(c, 0)
    rows, d, dt, ex = c.batch * c.rpb, c.d, DT[c.dt], fam == "exact"
    t = dict(B=c.batch, rpb=c.rpb, x=_ri(g, -8, 8, rows, d) if ex else _rn(g, rows, d), acc=(_ri(g, -4, 4, rows, d) if ex else _rn(g, rows, d)).to(dt),
             gate=_pow2(g, c.batch, d) if ex else _rn(g, c.batch, d) * torch.arange(1, c.batch + 1).float()[:, None])
    if c.kind == "gr_bwd":
        t["dy"] = _ri(g, -3, 3, rows, d) if ex else _rn(g, rows, d)
        t["dgate0"] = _ri(g, -5, 5, c.batch, d) if ex else _rn(g, c.batch, d)
        t["dbias0"] = None if c.dbias is None else (_ri(g, -5, 5, *((d,) if c.dbias == "vec" else (c.batch, d))) if ex else _rn(g, *((d,) if c.dbias == "vec" else (c.batch, d))))
    return [t]


def data_colsum(c, fam):
    g = _gen(c, 0)
    ex = fam == "exact"
    return [dict(x=(_ri(g, -3, 3, c.rows, c.cols) if ex else _rn(g, c.rows, c.cols)).to(DT[c.dt]), out0=_ri(g, -9, 9, c.cols) if ex else _rn(g, c.cols))]


def data_silu(c, fam):
    g = _gen(c, 0)
    rows = c.groups * c.rpg
    pre = 2.0 * _rn(g, rows, c.cols)
    if fam == "saturating":
        pre = _saturate(g, pre)
        pre[0, 0] = -100.0
    return [dict(pre=pre, dy=_rn(g, rows, c.cols).to(DT[c.pair[0]]), dbias0=_rn(g, c.groups, c.cols) if c.dbias else None)]


def data_flow(c, fam):
    g = _gen(c, 0)
    return [dict(v=_rn(g, c.n), x0=_rn(g, c.n).to(DT[c.dt]), eps=_rn(g, c.n).to(DT[c.dt]))]


def to_dev(t, dev):
    return {k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in t.items()}


# ---------------------------------------------------------------------------------------------- the operations in plain torch (dt = float64: the reference)
# Each *_math(c, t, dt, fault=None) -> (outputs, intermediates): outputs name -> 2-D tensor in dt BEFORE the output rounding.  The CPU twin runs the
# same functions in float32 (torch's summation order, not the kernels') as the honest model, and with `fault` as the planted faults.
def math_ln_fwd(c, t, dt, fault=None):
    x = t["x"].to(dt)
    rows, rpb = x.shape[0], t["rpb"]
    b = _bidx(rows, rpb, x.device)
    o = {}
    if c.res:
        x = x + t["gate"].to(dt)[b] * t["acc"].to(dt)
        o["xo"] = x
    m = x.mean(1, keepdim=True)
    v = (x * x).mean(1, keepdim=True) - m * m if fault == "onepass" else ((x - m) ** 2).mean(1, keepdim=True)
    r = (v + (1e-6 if fault == "eps" else LN_EPS)).rsqrt()
    if fault == "wrong_b":      # the last row of sample 0 modulated with sample 1's rows
        b = b.clone()
        b[rpb - 1] += 1
    o.update(out=(x - m) * r * (1 + t["scale"].to(dt)[b]) + t["shift"].to(dt)[b], mean=m, rstd=r)
    return o, dict(x1=x, m=m, v=v, r=r, b=b)


def yard_ln_fwd(c, t, ref, aux):
    S = 4 * nit_bucket(c.d) + 7
    x1, m, v, r, b = aux["x1"], aux["m"], aux["v"], aux["r"], aux["b"]
    ex = 2 * u * (t["x"].double().abs() + (t["gate"].double()[b] * t["acc"].double()).abs()) if c.res else torch.zeros_like(x1)
    xc = (x1 - m).abs()
    dm = S * u * x1.abs().mean(1, keepdim=True) + ex.mean(1, keepdim=True)
    dc = dm + u * xc + ex
    dv = (S + 4) * u * v + dm * dm + 2 * (xc * ex).mean(1, keepdim=True)
    dr = r * (0.5 * dv / (v + LN_EPS) + 2 * u)
    out = ref["out"]
    shift = t["shift"].double()[b]
    det = (1 + t["scale"].double()[b]).abs() * (r * dc + xc * dr) + 3 * u * (out - shift).abs() + u * out.abs()
    y = dict(out=(det, U * out.abs() if c.dt == "bf16" else torch.zeros_like(out)), mean=(dm, torch.zeros_like(dm)), rstd=(dr, torch.zeros_like(dr)))
    if c.res:
        y["xo"] = (ex, torch.zeros_like(ex))
    return y


def _seg(z, B, rpb):
    return z.view(B, rpb, -1).sum(1)


def math_ln_bwd(c, t, dt, fault=None):
    dy, x, mean, rstd = t["dout"].to(dt), t["x"].to(dt), t["mean"].to(dt), t["rstd"].to(dt)
    B, rpb = t["B"], t["rpb"]
    b = _bidx(x.shape[0], rpb, x.device)
    xh = (x - mean) * rstd
    g = dy * (1 + t["scale"].to(dt)[b])
    c1, c2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    core = rstd * (g - c1 - xh * c2)
    dx = core + t["dres"].to(dt) if c.dres else core
    o = dict(dx=dx, dscale=t["dscale0"].to(dt) + _seg(dy * xh, B, rpb), dshift=t["dshift0"].to(dt) + _seg(dy, B, rpb))
    if fault == "lost_row":      # the last row of sample 0's first chunk missing from its dscale sum
        o["dscale"][0] -= (dy * xh)[min(rpb, 16) - 1]
    aux = dict(xh=xh, g=g, c1=c1, c2=c2, b=b)
    if c.gated:
        gate, acc = t["gate"].to(dt)[b], t["acc"].to(dt)
        o["dacc"] = dx * gate
        o["dgate"] = t["dgate0"].to(dt) + _seg(dx * acc, B, rpb)
        if c.dbias:
            o["dbias"] = t["dbias0"].to(dt) + _seg(o["dacc"], B, rpb)
    return o, aux


def yard_ln_bwd(c, t, ref, aux):
    S = 4 * nit_bucket(c.d) + 7
    B, T = t["B"], t["rpb"]
    xh, g, c1, c2, b = aux["xh"].abs(), aux["g"].abs(), aux["c1"].abs(), aux["c2"].abs(), aux["b"]
    dy, rstd = t["dout"].double().abs(), t["rstd"].double()
    mk = lambda z: z.mean(1, keepdim=True)      # noqa: E731
    e_xh, e_g = 2 * u * xh, 2 * u * g
    dc1 = S * u * mk(g) + mk(e_g)
    dc2 = (S + 1) * u * mk(g * xh) + mk(g * e_xh + e_g * xh)
    ydx = rstd * (e_g + dc1 + e_xh * c2 + xh * dc2) + 3 * u * rstd * (g + c1 + xh * c2) + u * ref["dx"].abs()
    if c.dres:
        ydx = ydx + u * t["dres"].double().abs()
    z = torch.zeros_like
    y = dict(dx=(ydx, z(ydx)))
    col = lambda per, terms, init: _seg(per, B, T) + (T + 2) * u * (_seg(terms, B, T) + init.double().abs())      # noqa: E731
    y["dscale"] = (col(dy * e_xh + u * dy * xh, dy * xh, t["dscale0"]), z(ref["dscale"]))
    y["dshift"] = (col(z(dy), dy, t["dshift0"]), z(ref["dshift"]))
    if c.gated:
        gate, acc, dacc = t["gate"].double()[b].abs(), t["acc"].double().abs(), ref["dacc"].abs()
        y["dacc"] = (gate * ydx + u * dacc, U * dacc if c.dt == "bf16" else z(dacc))
        y["dgate"] = (col(ydx * acc + u * ref["dx"].abs() * acc, ref["dx"].abs() * acc, t["dgate0"]), z(ref["dgate"]))
        if c.dbias:
            y["dbias"] = (col(gate * ydx + u * dacc, dacc, t["dbias0"]), z(ref["dbias"]))
    return y


def _rms_halves(c, t):
    sp, T = c.split, c.tokens
    return ((1, 0, sp), (2, sp, T - sp))


def math_rms(c, t, dt, fault=None):
    o, aux = {}, {}
    eps = 1e-6 if fault == "eps" else RMS_EPS
    for h, off, cnt in _rms_halves(c, t):
        x = t["x"].to(dt)[:, off:off + cnt].reshape(-1, c.d)
        w, s, dy = t[f"w{h}"].to(dt), t[f"s{h}"].to(dt), t[f"dout{h}"].to(dt)
        q = (x * x).mean(1, keepdim=True)
        r = (q + eps).rsqrt()
        xn = x * r
        o[f"out{h}"] = s * (xn * w)
        o[f"dw{h}"] = (t[f"dw{h}0"].to(dt) + (dy * s * xn).sum(0))[None]
        o[f"ds{h}"] = (t[f"ds{h}0"].to(dt) + (dy * xn * w).sum())[None]
        aux[h] = dict(x=x, q=q, r=r, xn=xn)
    return o, aux


def yard_rms(c, t, ref, aux):
    nit = nit_bucket(c.d)
    S = 4 * nit + 7
    y = {}
    z = torch.zeros_like
    for h, off, cnt in _rms_halves(c, t):
        a = aux[h]
        x, q, r, xn = a["x"].abs(), a["q"], a["r"], a["xn"].abs()
        w, s, dy = t[f"w{h}"].double().abs(), float(t[f"s{h}"].abs()), t[f"dout{h}"].double().abs()
        rows = x.shape[0]
        dr = r * (0.5 * (S + 1) * u * q / (q + RMS_EPS) + 2 * u)
        e_xn = x * dr + u * xn
        out = ref[f"out{h}"].abs()
        y[f"out{h}"] = (s * w * e_xn + 2 * u * out, U * out if c.tg == "bf16" else z(out))
        terms = dy * s * xn
        y[f"dw{h}"] = (((dy * s * e_xn + 2 * u * terms).sum(0) + (rows + 2) * u * (terms.sum(0) + t[f"dw{h}0"].double().abs()))[None], z(ref[f"dw{h}"]))
        terms = dy * xn * w
        depth = 32 * nit + 9 + (rows + 63) // 64
        y[f"ds{h}"] = (((dy * w * e_xn + 2 * u * terms).sum() + depth * u * (terms.sum() + t[f"ds{h}0"].double().abs()))[None], z(ref[f"ds{h}"]))
    return y


def _qk_split(z):
    return z[..., 0::2], z[..., 1::2]


def _qk_join(e, o):
    return torch.stack([e, o], -1).flatten(-2)


def _qk_tables(t, dt):
    if t["cos"] is None:
        return None
    c0, c1 = _qk_split(t["cos"].to(dt)[None, :, None, :])
    s0, s1 = _qk_split(t["sin"].to(dt)[None, :, None, :])
    return c0, c1, s0, s1


def math_qk(c, t, dt, fault=None):
    B, H, T, tok0 = t["B"], t["H"], t["T"], t["tok0"]
    x = t["qkv"].to(dt).view(B, T, 3, H, 64)
    tab = _qk_tables(t, dt)
    heads = lambda z: z.permute(0, 2, 1, 3).reshape(-1, 64)      # noqa: E731  (B, T, H, 64) -> rows of (B, H, T)
    o, aux, parts = {}, {}, []
    for part, name in ((0, "q"), (1, "k")):
        xp, w = x[:, :, part], t["w" + name].to(dt)
        q = (xp * xp).mean(-1, keepdim=True)
        r = (q + RMS_EPS).rsqrt()
        xn = xp * r
        n = xn * w
        if tab is not None:
            c0, c1, s0, s1 = tab
            a, b = _qk_split(n)
            fwd = _qk_join(a * c0 - b * s0, b * c1 + a * s1)
        else:
            fwd = n
        o[name.upper()] = heads(fwd)
        dz = t["d" + name.upper()].to(dt)[:, :, tok0:tok0 + T].permute(0, 2, 1, 3)
        if tab is not None:
            da, db = _qk_split(dz)
            dzr = _qk_join(da * c0 + db * s1, db * c1 - da * s0)
        else:
            dzr = dz
        dzw = dzr * w
        dot = (dzw * xn).mean(-1, keepdim=True)
        parts.append(r * (dzw - xn * dot))
        o["dw" + name] = (t[f"dw{name}0"].to(dt) + (dzr * xn).sum((0, 1, 2)))[None]
        aux[name] = dict(xp=xp, q=q, r=r, xn=xn, n=n, dz=dz, dzr=dzr, dzw=dzw, dot=dot)
    o["V"] = heads(x[:, :, 2])
    parts.append(t["dV"].to(dt)[:, :, tok0:tok0 + T].permute(0, 2, 1, 3))
    o["dqkv"] = torch.stack(parts, 2).reshape(B * T, 3 * H * 64)
    return o, aux


def yard_qk(c, t, ref, aux):
    tg, ti, to = qk_dtypes(c.combo)
    B, H, T = t["B"], t["H"], t["T"]
    tab = _qk_tables(t, F64)
    heads = lambda z: z.permute(0, 2, 1, 3).reshape(-1, 64)      # noqa: E731
    z = torch.zeros_like
    mk = lambda v: v.mean(-1, keepdim=True)      # noqa: E731
    y, parts = {}, []
    for name in ("q", "k"):
        a = aux[name]
        w = t["w" + name].double().abs()
        xp, q, r, xn, n = a["xp"].abs(), a["q"], a["r"], a["xn"].abs(), a["n"].abs()
        dr = r * (0.5 * 13 * u * q / (q + RMS_EPS) + 2 * u)
        e_xn = xp * dr + u * xn
        e_n = w * e_xn + u * n
        dz, dzr, dzw, dot = a["dz"].abs(), a["dzr"].abs(), a["dzw"].abs(), a["dot"].abs()
        if tab is not None:
            c0, c1, s0, s1 = (v.abs() for v in tab)
            na, nb = _qk_split(n)
            ea, eb = _qk_split(e_n)
            e_f = _qk_join(c0 * ea + s0 * eb + 2 * u * (na * c0 + nb * s0), c1 * eb + s1 * ea + 2 * u * (nb * c1 + na * s1))
            da, db = _qk_split(dz)
            e_dz = _qk_join(2 * u * (da * c0 + db * s1), 2 * u * (db * c1 + da * s0))
        else:
            e_f, e_dz = e_n, z(dz)
        f = ref[name.upper()].abs()
        y[name.upper()] = (heads(e_f), U * f)
        e_dzw = w * e_dz + u * dzw
        ddot = 12 * u * mk(dzw * xn) + mk(e_dzw * xn + dzw * e_xn)
        core = (a["dzw"] - a["xn"] * a["dot"]).abs()
        e_o = r * (e_dzw + e_xn * dot + xn * ddot + 2 * u * (dzw + xn * dot)) + dr * core + u * r * core
        parts.append(e_o)
        terms = dzr * xn
        y["dw" + name] = (((e_dz * xn + dzr * e_xn + u * terms).sum((0, 1, 2)) + (B * T * H + 2) * u * (terms.sum((0, 1, 2)) + t[f"dw{name}0"].double().abs()))[None],
                          z(ref["dw" + name]))
    v = ref["V"].abs()
    y["V"] = (z(v), U * v if ti == F32 else z(v))
    parts.append(z(parts[0]))
    det = torch.stack(parts, 2).reshape(B * T, 3 * H * 64)
    y["dqkv"] = (det, U * ref["dqkv"].abs() if to == BF else z(det))
    if to == BF:      # (the dV third of a bf16 dqkv is an exact copy)
        y["dqkv"][1].view(B, T, 3, H, 64)[:, :, 2] = 0
    return y


_SQ2, _PHI0 = 0.7071067811865476, 0.3989422804014327


def math_mlp(c, t, dt, fault=None):
    h = c.hidden
    gu, dh = t["gu"].to(dt), t["dh"].to(dt)
    if c.gelu:
        cdf = 0.5 * (1 + torch.erf(gu * _SQ2))
        o = dict(h=gu * cdf, dgu=dh * (cdf + gu * _PHI0 * torch.exp(-0.5 * gu * gu)))
    else:
        g, up = gu[:, :h], gu[:, h:]
        s = torch.sigmoid(g)
        o = dict(h=g * s * up, dgu=torch.cat([dh * up * s * (1 + g * (1 - s)), dh * g * s], 1))
    if c.dbias:
        o["dbias"] = (t["dbias0"].to(dt) + o["dgu"].sum(0))[None]
    return o, {}


def yard_mlp(c, t, ref, aux):
    h = c.hidden
    gu, dh = t["gu"].double(), t["dh"].double().abs()
    bf = c.dt == "bf16"
    z = torch.zeros_like
    rnd = lambda v: U * v.abs() if bf else z(v)      # noqa: E731
    if c.gelu:
        x = gu.abs()
        tt = 0.5 * gu * gu
        yh = 0.5 * x * ERF_ABS + 2 * u * ref["h"].abs() + FLUSH
        yg = dh * (0.5 * ERF_ABS + x * _PHI0 * torch.exp(-tt) * 8 * E23 * (1 + tt)) + 2 * u * ref["dgu"].abs() + FLUSH
    else:
        g, up = gu[:, :h].abs(), gu[:, h:].abs()
        yh = 8 * E23 * (1 + g) * ref["h"].abs() + FLUSH * (1 + up)
        yg = 8 * E23 * torch.cat([(1 + g) * dh * up, (1 + g) * dh], 1) + FLUSH
    y = dict(h=(yh, rnd(ref["h"])), dgu=(yg, rnd(ref["dgu"])))
    if c.dbias:
        y["dbias"] = ((yg.sum(0) + (gu.shape[0] + 2) * u * (ref["dgu"].abs().sum(0) + t["dbias0"].double().abs()))[None], z(ref["dbias"]))
    return y


def math_gr(c, t, dt, fault=None):
    B, rpb = t["B"], t["rpb"]
    b = _bidx(t["x"].shape[0], rpb, t["x"].device)
    gate, acc = t["gate"].to(dt)[b], t["acc"].to(dt)
    if c.kind == "gr_fwd":
        return dict(out=t["x"].to(dt) + gate * acc), dict(gate=gate)
    dy = t["dy"].to(dt)
    o = dict(dacc=dy * gate, dgate=t["dgate0"].to(dt) + _seg(dy * acc, B, rpb))
    if c.dbias == "per":
        o["dbias"] = t["dbias0"].to(dt) + _seg(o["dacc"], B, rpb)
    elif c.dbias == "vec":
        o["dbias"] = (t["dbias0"].to(dt) + o["dacc"].sum(0))[None]
    return o, dict(gate=gate)


def yard_gr(c, t, ref, aux):
    B, T = t["B"], t["rpb"]
    z = torch.zeros_like
    gate, acc = aux["gate"].abs(), t["acc"].double().abs()
    if c.kind == "gr_fwd":
        return dict(out=(2 * u * (t["x"].double().abs() + gate * acc), z(gate)))
    dy, dacc = t["dy"].double().abs(), ref["dacc"].abs()
    y = dict(dacc=(u * dacc, U * dacc if c.dt == "bf16" else z(dacc)))
    y["dgate"] = (u * _seg(dy * acc, B, T) + (T + 2) * u * (_seg(dy * acc, B, T) + t["dgate0"].double().abs()), z(ref["dgate"]))
    if c.dbias == "per":
        y["dbias"] = (u * _seg(dacc, B, T) + (T + 2) * u * (_seg(dacc, B, T) + t["dbias0"].double().abs()), z(ref["dbias"]))
    elif c.dbias == "vec":
        y["dbias"] = ((u * dacc.sum(0) + (B * T + 2) * u * (dacc.sum(0) + t["dbias0"].double().abs()))[None], z(ref["dbias"]))
    return y


def math_colsum(c, t, dt, fault=None):
    return dict(out=(t["out0"].to(dt) + t["x"].to(dt).sum(0))[None]), {}


def yard_colsum(c, t, ref, aux):
    det = ((c.rows + 2) * u * (t["x"].double().abs().sum(0) + t["out0"].double().abs()))[None]
    return dict(out=(det, torch.zeros_like(det)))


def math_silu(c, t, dt, fault=None):
    p, dy = t["pre"].to(dt), t["dy"].to(dt)
    s = torch.sigmoid(p)
    o = dict(dpre=dy * s * (1 + p * (1 - s)))
    if c.dbias:
        o["dbias"] = t["dbias0"].to(dt) + _seg(o["dpre"], c.groups, c.rpg)
    return o, {}


def yard_silu(c, t, ref, aux):
    z = torch.zeros_like
    det = 8 * E23 * (1 + t["pre"].double().abs()) * t["dy"].double().abs() + FLUSH
    y = dict(dpre=(det, U * ref["dpre"].abs() if c.pair[1] == "bf16" else z(det)))
    if c.dbias:
        y["dbias"] = (_seg(det, c.groups, c.rpg) + (c.rpg + 2) * u * _seg(ref["dpre"].abs(), c.groups, c.rpg) + u * t["dbias0"].double().abs(), z(ref["dbias"]))
    return y


def math_flow(c, t, dt, fault=None):
    lab = t["eps"].double() - t["x0"].double()
    lab = (lab.float().to(BF) if c.dt == "bf16" else lab.float()).to(dt)      # (the label as the kernel and torch round it: an input of the comparison)
    d = t["v"].to(dt) - lab
    coef = 1.0 / c.n
    return dict(loss=(coef * (d * d).sum())[None, None], dv=(2 * coef * d).view(-1, 8)), dict(lab=lab, d=d)


def yard_flow(c, t, ref, aux):
    coef = 1.0 / c.n
    n8 = c.n // 8
    grid = min((n8 + 255) // 256, 256)
    e_d = u * aux["d"].abs() + (u * aux["lab"].abs() if c.dt == "f32" else 0)
    det = (2 * coef * e_d).view(-1, 8) + 2 * u * ref["dv"].abs()
    S = 8 * math.ceil(n8 / (grid * 256)) + 23
    dl = (S * u * ref["loss"].abs()[0, 0] + 2 * coef * (aux["d"].abs() * e_d).sum())[None, None]
    return dict(loss=(dl, torch.zeros_like(dl)), dv=(det, torch.zeros_like(det)))


def out_dtype(c, name):
    """The dtype in which the kernel stores output `name` (the honest model rounds to it)."""
    if c.kind == "ln_fwd":
        return DT[c.dt] if name == "out" else F32
    if c.kind == "ln_bwd":
        return DT[c.dt] if name == "dacc" else F32
    if c.kind == "rms":
        return DT[c.tg] if name.startswith("out") else F32
    if c.kind == "qk":
        return BF if name in "QKV" else qk_dtypes(c.combo)[2] if name == "dqkv" else F32
    if c.kind == "mlp":
        return F32 if name == "dbias" else DT[c.dt]
    if c.kind == "gr_bwd":
        return DT[c.dt] if name == "dacc" else F32
    if c.kind == "silu_bwd":
        return DT[c.pair[1]] if name == "dpre" else F32
    return F32


KIND = {"ln_fwd": (data_ln, math_ln_fwd, yard_ln_fwd), "ln_bwd": (data_ln, math_ln_bwd, yard_ln_bwd), "rms": (data_rms, math_rms, yard_rms),
        "qk": (data_qk, math_qk, yard_qk), "mlp": (data_mlp, math_mlp, yard_mlp), "gr_fwd": (data_gr, math_gr, yard_gr), "gr_bwd": (data_gr, math_gr, yard_gr),
        "colsum": (data_colsum, math_colsum, yard_colsum), "silu_bwd": (data_silu, math_silu, yard_silu), "flow": (data_flow, math_flow, yard_flow)}


# ---------------------------------------------------------------------------------------------- placement: operands among NaN, outputs among sentinels
def place(x, poison, ld=None):
    """x (2-D or 1-D) as the kernel receives it: contiguous, or (poison) the leading part of a larger NaN-filled tensor the test owns -- GUARD rows
    behind the last row, and a leading dimension `ld` where the kernel takes one.  Without poison an `ld` still applies (the ld arguments always run)."""
    if x is None:
        return None
    x2 = x if x.dim() == 2 else x[None]
    r, cc = x2.shape
    big = torch.full((r + (GUARD if poison else 0), ld or cc), float("nan"), dtype=x.dtype, device=x.device)
    big[:r, :cc] = x2
    v = big[:r, :cc]
    return v if x.dim() == 2 else v[0]


class Win:
    """An output: the [rows, cols] window of a tensor the test owns, with leading dimension ld >= cols and (guarded) GUARD rows before and behind.
    Every byte starts as a NaN bit pattern (or, inside the window, as `init`); touched() counts the bytes that changed outside the window, or
    outside the rows `allowed` (bool per window row) inside it."""
    PATTERN = {F32: (torch.int32, 0x7FC0A5A5), BF: (torch.int16, 0x7FA5)}

    def __init__(self, rows, cols, dtype, guarded, device, ld=None, init=None):
        self.rows, self.cols, self.r0 = rows, cols, GUARD if guarded else 0
        self.big = torch.empty((rows + 2 * self.r0, ld or cols), dtype=dtype, device=device)
        it, pat = self.PATTERN[dtype]
        self.big.view(it).fill_(pat)
        self.win = self.big[self.r0:self.r0 + rows, :cols]
        if init is not None:
            self.win.copy_(init.view(rows, cols))
        self.snap = None

    def ptr(self):
        return self.win.data_ptr()

    def snapshot(self):
        self.snap = self.big.clone()

    def touched(self, allowed=None):
        d = self.big.view(torch.uint8) != self.snap.view(torch.uint8)
        w = d[self.r0:self.r0 + self.rows, :self.cols * self.big.element_size()]
        if allowed is None:
            w[:] = False
        else:
            w[allowed] = False
        return [tuple(i) for i in d.nonzero()[:8].tolist()], int(d.sum())


def _code(dt):
    return {F32: 0, BF: 1}[dt]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- launches: name -> (compared tensor, Win | None, allowed rows | None)
def run_ln_fwd(ops, c, ts, poison):
    from sd3_amd import _lib
    arr, keep, outs = (_lib.LnFwdProblem * len(ts))(), [], []
    dt, d, ld = DT[c.dt], c.d, c.d + 8
    for q, t in zip(arr, ts):
        rows = t["x"].shape[0]
        x, sc, sh = place(t["x"], poison), place(t["scale"], poison, ld), place(t["shift"], poison, ld)
        w = dict(out=Win(rows, d, dt, poison, "cuda"), mean=Win(rows, 1, F32, poison, "cuda"), rstd=Win(rows, 1, F32, poison, "cuda"))
        q.x, q.scale, q.shift, q.ld_mod, q.rows, q.rows_per_batch = x.data_ptr(), sc.data_ptr(), sh.data_ptr(), ld, rows, t["rpb"]
        keep += [x, sc, sh]
        if c.res:
            acc, gate = place(t["acc"], poison), place(t["gate"], poison, ld)
            w["xo"] = Win(rows, d, F32, poison, "cuda")
            q.acc, q.gate, q.ld_gate, q.x_out = acc.data_ptr(), gate.data_ptr(), ld, w["xo"].ptr()
            keep += [acc, gate]
        q.out, q.mean, q.rstd = w["out"].ptr(), w["mean"].ptr(), w["rstd"].ptr()
        outs.append(w)
    return _launch(outs, lambda: _lib.lib().mmdit_ln_modulate_fwd(arr, len(ts), d, _code(dt), _code(dt), _stream()), keep)


def _launch(outs, call, keep):
    for w in outs:
        for v in w.values():
            v.snapshot()
    torch.cuda.synchronize()
    try:
        rc = call()
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device error is sticky: nothing more is launched in this session
        pytest.exit(f"device error after a row-kernel launch: {e}", returncode=3)
    assert rc == 0, rc
    del keep
    return [{k: (v.win, v, None) for k, v in w.items()} for w in outs]


def run_ln_bwd(ops, c, ts, poison):
    from sd3_amd import _lib
    arr, keep, outs = (_lib.LnBwdProblem * len(ts))(), [], []
    dt, d, ld = DT[c.dt], c.d, c.d + 8
    for q, t in zip(arr, ts):
        rows, B = t["x"].shape[0], t["B"]
        ins = [place(t[k], poison) for k in ("dout", "x", "mean", "rstd")] + [place(t["scale"], poison, ld), place(t["dres"] if c.dres else None, poison)]
        w = dict(dx=Win(rows, d, F32, poison, "cuda"), dscale=Win(B, d, F32, poison, "cuda", ld, t["dscale0"]), dshift=Win(B, d, F32, poison, "cuda", ld, t["dshift0"]))
        q.dout, q.x, q.mean, q.rstd, q.scale, q.dres = (_ptr(v) for v in ins)
        q.ld_mod, q.rows, q.rows_per_batch, q.ld_dmod = ld, rows, t["rpb"], ld
        if c.gated:
            acc, gate = place(t["acc"], poison), place(t["gate"], poison, ld)
            ins += [acc, gate]
            w["dacc"] = Win(rows, d, dt, poison, "cuda")
            w["dgate"] = Win(B, d, F32, poison, "cuda", ld, t["dgate0"])
            q.acc, q.gate, q.ld_gate, q.dacc, q.dgate, q.ld_dgate = acc.data_ptr(), gate.data_ptr(), ld, w["dacc"].ptr(), w["dgate"].ptr(), ld
            if c.dbias:
                w["dbias"] = Win(B, d, F32, poison, "cuda", ld, t["dbias0"])
                q.dbias, q.ld_dbias = w["dbias"].ptr(), ld
        q.dx, q.dscale, q.dshift = w["dx"].ptr(), w["dscale"].ptr(), w["dshift"].ptr()
        keep += ins
        outs.append(w)
    return _launch(outs, lambda: _lib.lib().mmdit_ln_modulate_bwd(arr, len(ts), d, _code(dt), _stream()), keep)


def run_rms(ops, c, ts, poison):
    from sd3_amd import _lib
    t = ts[0]
    L, d, B, T, sp = _lib.lib(), c.d, c.batch, c.tokens, c.split
    r1, r2 = B * sp, B * (T - sp)
    w = dict(out1=Win(r1, d, DT[c.tg], True, "cuda"), out2=Win(r2, d, DT[c.tg], True, "cuda"))
    for h in (1, 2):
        w[f"dw{h}"] = Win(1, d, F32, True, "cuda", None, t[f"dw{h}0"])
        w[f"ds{h}"] = Win(1, 1, F32, True, "cuda", None, t[f"ds{h}0"])
    x = t["x"].contiguous()

    def call():
        rc = L.mmdit_text_rmsnorm_fwd(x.data_ptr(), _code(x.dtype), t["w1"].data_ptr(), t["w2"].data_ptr(), t["s1"].data_ptr(), t["s2"].data_ptr(), B, T, sp, d,
                                      w["out1"].ptr(), w["out2"].ptr(), _code(DT[c.tg]), _stream())
        return rc or L.mmdit_text_rmsnorm_bwd(t["dout1"].data_ptr(), t["dout2"].data_ptr(), _code(DT[c.tg]), x.data_ptr(), _code(x.dtype), t["w1"].data_ptr(), t["w2"].data_ptr(),
                                              t["s1"].data_ptr(), t["s2"].data_ptr(), B, T, sp, d, w["dw1"].ptr(), w["dw2"].ptr(), w["ds1"].ptr(), w["ds2"].ptr(), _stream())
    return _launch([w], call, [x])


def run_qk(ops, c, ts, poison):
    from sd3_amd import _lib
    L = _lib.lib()
    tg, ti, to = qk_dtypes(c.combo)
    B, H, S = ts[0]["B"], ts[0]["H"], ts[0]["S"]
    n = len(ts)
    arr, keep, outs = (_lib.QkProblem * n)(), [], []
    qkv_out = {k: Win(B * H * S, 64, BF, poison, "cuda") for k in "QKV"}
    dQ, dK, dV = (place(ts[0][k].view(-1, 64), poison) for k in ("dQ", "dK", "dV"))
    allowed = torch.zeros(B, H, S, dtype=torch.bool, device="cuda")
    for q, t in zip(arr, ts):
        T = t["T"]
        allowed[:, :, t["tok0"]:t["tok0"] + T] = True
        ins = [place(t[k], poison) for k in ("qkv", "wq", "wk", "cos", "sin")]
        w = dict(dqkv=Win(B * T, 3 * H * 64, to, poison, "cuda"), dwq=Win(1, 64, F32, poison, "cuda", None, t["dwq0"]), dwk=Win(1, 64, F32, poison, "cuda", None, t["dwk0"]))
        q.qkv, q.wq, q.wk, q.rope_cos, q.rope_sin = (_ptr(v) for v in ins)
        q.tokens, q.tok0, q.dqkv, q.dwq, q.dwk = T, t["tok0"], w["dqkv"].ptr(), w["dwq"].ptr(), w["dwk"].ptr()
        keep += ins
        outs.append(w)
    allowed = allowed.view(-1)

    def call():
        rc = L.mmdit_qk_norm_rope_fwd(arr, n, _code(ti), B, H, S, qkv_out["Q"].ptr(), qkv_out["K"].ptr(), qkv_out["V"].ptr(), _stream())
        return rc or L.mmdit_qk_norm_rope_bwd(arr, n, dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), _code(tg), _code(ti), _code(to), B, H, S, _stream())
    res = _launch(outs + [qkv_out], call, keep + [dQ, dK, dV])[:n]
    for r, t in zip(res, ts):
        for k in "QKV":
            r[k] = (qkv_out[k].win.view(B, H, S, 64)[:, :, t["tok0"]:t["tok0"] + t["T"]].reshape(-1, 64), qkv_out[k], allowed)
    return res


def run_mlp(ops, c, ts, poison):
    from sd3_amd import _lib
    L, dt, h = _lib.lib(), DT[c.dt], c.hidden
    arr, keep, outs = (_lib.MlpBwdProblem * len(ts))(), [], []
    for q, t in zip(arr, ts):
        rows = t["gu"].shape[0]
        dh, gu = place(t["dh"], poison), place(t["gu"], poison)
        w = dict(h=Win(rows, h, dt, True, "cuda"), dgu=Win(rows, gu.shape[1], dt, poison, "cuda"))
        if c.dbias:
            w["dbias"] = Win(1, gu.shape[1], F32, poison, "cuda", None, t["dbias0"])
        q.dh, q.gu, q.dgu, q.rows, q.dbias = dh.data_ptr(), gu.data_ptr(), w["dgu"].ptr(), rows, w["dbias"].ptr() if c.dbias else None
        keep += [dh, gu]
        outs.append(w)

    def call():
        for t, w in zip(keep[1::2], outs):
            rc = (L.mmdit_gelu_fwd if c.gelu else L.mmdit_swiglu_fwd)(t.data_ptr(), w["h"].ptr(), _code(dt), t.shape[0], h, _stream())
            if rc:
                return rc
        return L.mmdit_mlp_act_bwd(arr, len(ts), _code(dt), h, int(c.gelu), _stream())
    return _launch(outs, call, keep)


def run_gr(ops, c, ts, poison):
    from sd3_amd import _lib
    t = ts[0]
    L, d, B, rpb, dt = _lib.lib(), c.d, c.batch, c.rpb, DT[c.dt]
    rows, ld = B * rpb, d + 8
    gate, acc = place(t["gate"], False, ld), t["acc"].contiguous()
    if c.kind == "gr_fwd":
        w = dict(out=Win(rows, d, F32, True, "cuda"))
        return _launch([w], lambda: L.mmdit_gate_residual_fwd(t["x"].data_ptr(), acc.data_ptr(), _code(dt), gate.data_ptr(), ld, rows, d, rpb, w["out"].ptr(), _stream()), [gate, acc])
    w = dict(dacc=Win(rows, d, dt, True, "cuda"), dgate=Win(B, d, F32, True, "cuda", ld, t["dgate0"]))
    if c.dbias == "per":
        w["dbias"] = Win(B, d, F32, True, "cuda", ld, t["dbias0"])
    elif c.dbias == "vec":
        w["dbias"] = Win(1, d, F32, True, "cuda", None, t["dbias0"])
    return _launch([w], lambda: L.mmdit_gate_residual_bwd(t["dy"].data_ptr(), acc.data_ptr(), _code(dt), gate.data_ptr(), ld, rows, d, rpb, w["dacc"].ptr(), _code(dt),
                                                          w["dgate"].ptr(), ld, w["dbias"].ptr() if c.dbias else None, ld if c.dbias == "per" else 0, _stream()), [gate, acc])


def run_colsum(ops, c, ts, poison):
    from sd3_amd import _lib
    t = ts[0]
    x = place(t["x"], c.strided, c.cols + 16 if c.strided else None)
    w = dict(out=Win(1, c.cols, F32, True, "cuda", None, t["out0"]))
    return _launch([w], lambda: _lib.lib().mmdit_colsum(x.data_ptr(), _code(x.dtype), c.rows, c.cols, x.stride(0), w["out"].ptr(), _stream()), [x])


def run_silu(ops, c, ts, poison):
    from sd3_amd import _lib
    t = ts[0]
    rows = c.groups * c.rpg
    w = dict(dpre=Win(rows, c.cols, DT[c.pair[1]], True, "cuda"))
    if c.dbias:
        w["dbias"] = Win(c.groups, c.cols, F32, True, "cuda", None, t["dbias0"])
    return _launch([w], lambda: _lib.lib().mmdit_silu_bwd(t["dy"].data_ptr(), _code(DT[c.pair[0]]), t["pre"].data_ptr(), w["dpre"].ptr(), _code(DT[c.pair[1]]), rows, c.cols,
                                                          w["dbias"].ptr() if c.dbias else None, c.rpg, _stream()), [])


def run_flow(ops, c, ts, poison):
    from sd3_amd import _lib
    t = ts[0]
    w = dict(loss=Win(1, 1, F32, True, "cuda"), dv=Win(c.n // 8, 8, F32, True, "cuda"))
    part = torch.zeros(256, device="cuda")
    return _launch([w], lambda: _lib.lib().mmdit_flow_loss(t["v"].data_ptr(), t["x0"].data_ptr(), t["eps"].data_ptr(), _code(DT[c.dt]), c.n, 1.0 / c.n, w["dv"].ptr(),
                                                           part.data_ptr(), w["loss"].ptr(), _stream()), [part])


RUN = {"ln_fwd": run_ln_fwd, "ln_bwd": run_ln_bwd, "rms": run_rms, "qk": run_qk, "mlp": run_mlp, "gr_fwd": run_gr, "gr_bwd": run_gr, "colsum": run_colsum,
       "silu_bwd": run_silu, "flow": run_flow}


# ---------------------------------------------------------------------------------------------- comparison and record
WORST_OUT = {}         # (kernel family, output) -> worst [per-element, per-row, per-column] ratio over every case and input family
WORST = {}             # (kernel family, input family) -> [per-element, per-row, per-column, rounding bias] as (ratio, case id)


def _record(c, fam, r, what):
    w = WORST.setdefault((c.kind, fam), [(-1.0, "")] * 4)
    for i, k in enumerate(("el", "row", "col", "bias")):
        if r[k] is not None and r[k] > w[i][0]:
            w[i] = (r[k], f"{c.id} {what}")
    o = WORST_OUT.setdefault((c.kind, what.split(".")[1]), [0.0, 0.0, 0.0])
    for i, k in enumerate(("el", "row", "col")):
        o[i] = max(o[i], r[k])


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\n[rowops edge sweep] worst ratio to the yardstick per kernel family and input family (bars: per element 2.0, per row / column 1.0, rounding bias 1.0)")
    for (kf, fam), w in sorted(WORST.items()):
        print(f"  {kf:<9} {fam:<10} " + "  ".join(f"{n} {v:.3f} @ {cid}" for n, (v, cid) in zip(("elem", "row", "col", "bias"), w) if v >= 0))
    print("[rowops edge sweep] worst ratio per kernel family and output over every input family (fp32 outputs and sums show what the derived part leaves)")
    for (kf, name), o in sorted(WORST_OUT.items()):
        print(f"  {kf:<9} {name:<7} elem {o[0]:.3f}  row {o[1]:.3f}  col {o[2]:.3f}")


EXACT_NAMES = {"gr_fwd": ("out",), "gr_bwd": ("dacc", "dgate", "dbias"), "colsum": ("out",)}


def compare(c, fam, i, name, got, ref, det, rnd, failures, record=True):
    """One output against its reference: finite, the three bars and the rounding-bias bar; exact family: equality.  Appends to `failures`."""
    what = f"p{i}.{name}"
    if not bool(torch.isfinite(got).all()):
        failures.append(f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements")
        return None
    r = G.ratios(got, ref, det, rnd)
    if record:
        _record(c, fam, r, what)
    print(f"[rowops edges] {c.id} {fam} {what}: elem {r['el']:.3f} @ ({r['at'][0]}, {r['at'][1]}) row {r['row']:.3f} @ {r['at'][2]} col {r['col']:.3f} @ {r['at'][3]}"
          + (f" bias {r['bias']:.3f}" if r["bias"] is not None else ""))
    bad = G.verdict(r)
    if bad:
        failures.append(f"{what}: {bad} over the bar: {r}")
    if fam == "exact" and name in EXACT_NAMES.get(c.kind, ()):
        wrong = int((got.double() != ref).sum())
        if wrong:
            failures.append(f"{what}: {wrong} of {ref.numel()} elements differ from the exact float64 reference")
    return r


def constant_row_checks(c, t, got, failures):
    """smallvar family, row 0 (constant; all-zero for the RMS kernels): out == shift rounded to the output dtype bit for bit, mean == the value."""
    if c.kind == "ln_fwd":
        want = t["shift"][0].to(DT[c.dt])
        if not torch.equal(got["out"][0][0], want):
            failures.append("constant row: out differs from shift rounded to the output dtype")
        if float(got["mean"][0][0, 0]) != 1.5:
            failures.append(f"constant row: mean {float(got['mean'][0][0, 0])!r} != 1.5")
    elif c.kind == "rms":
        for h in (1, 2):
            if int((got[f"out{h}"][0][0] != 0).sum()):
                failures.append(f"all-zero row: out{h} is not zero")
    elif c.kind == "qk":
        if int((got["Q"][0][0] != 0).sum()):
            failures.append("all-zero head vector: Q is not zero")


@pytest.mark.parametrize("case", [cf for cf in CASES if cf[0].kind != "mx"], ids=_case_id)
def test_rowops_edge(ops, case):
    """One launch (forward and backward of the case where the family has both) under one input family: every output finite, within the three
    bars and the rounding-bias bar against float64, accumulated outputs equal to init + sum, exact for the exact family, the constant row of the
    small-variance family bit-exact, every byte outside an output's window (guard rows, ld padding, other streams' tokens) bit-identical."""
    c, fam = case
    data, fmath, fyard = KIND[c.kind]
    ts = [to_dev(t, "cuda") for t in data(c, "random" if fam == "poison" else fam)]
    outs = RUN[c.kind](ops, c, ts, fam == "poison")
    failures = []
    for i, (t, got) in enumerate(zip(ts, outs)):
        ref, aux = fmath(c, t, F64)
        yard = fyard(c, t, ref, aux)
        assert set(yard) == set(got) == set(ref), (sorted(yard), sorted(got), sorted(ref))
        for name, (det, rnd) in yard.items():
            tensor, win, allowed = got[name]
            where, count = win.touched(allowed)
            if count:
                failures.append(f"p{i}.{name}: {count} bytes outside the output window changed, first (row, byte) {where}")
            compare(c, fam, i, name, tensor, ref[name], det, rnd, failures)
        if fam == "smallvar" and i == 0:
            constant_row_checks(c, t, got, failures)
    assert not failures, "\n".join([c.id + " " + fam + " [" + c.path + "]"] + failures)


@pytest.mark.parametrize("c", [c for c in ALL if c.kind == "mx"], ids=lambda c: c.id)
def test_mx_producers_bit_identical_off_the_tile_edges(ops, c):
    """The MX-emitting adaLN (plain and with the pending gated residual) and SwiGLU at row counts off the 4-row workgroup and the 128-row scale
    padding: codes and scale bytes equal the bf16 output followed by mmdit_mxfp8_quantize, statistics and the residual row bit-identical."""
    g = _gen(c, 0)
    rows, d, rpb = c.rows, c.width, 50
    B = (rows + rpb - 1) // rpb
    x, acc = (3.0 * _rn(g, rows, d)).cuda(), _rn(g, rows, d).to(BF).cuda()
    sc, sh, gate = (0.3 * _rn(g, B, d)).cuda(), (0.3 * _rn(g, B, d)).cuda(), _rn(g, B, d).cuda()

    def same(mx, ref_bf16):
        q, s = ops.quant_mxfp8(ref_bf16)
        assert torch.equal(mx.q.view(torch.uint8), q.view(torch.uint8))
        assert torch.equal(ops.mx_scales_to_rows(mx.sc, *q.shape), ops.mx_scales_to_rows(s, *q.shape))

    out, mean, rstd = ops.ln_modulate_fwd(x, sc, sh, rpb, BF)
    _, mx, mean2, rstd2 = ops.ln_modulate_fwd_mx(x, sc, sh, rpb)
    same(mx, out)
    assert torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    xr, outr, meanr, rstdr = ops.ln_modulate_fwd_res(x, acc, gate, sc, sh, rpb, BF)
    xr2, mxr, meanr2, rstdr2 = ops.ln_modulate_fwd_mx(x, sc, sh, rpb, acc=acc, gate=gate)
    same(mxr, outr)
    assert torch.equal(xr, xr2) and torch.equal(meanr, meanr2) and torch.equal(rstdr, rstdr2)
    gu = (2.0 * _rn(g, rows, 2 * d)).to(BF).cuda()
    same(ops.swiglu_fwd_mx(gu, d), ops.mlp_act_fwd(gu, d, False))
