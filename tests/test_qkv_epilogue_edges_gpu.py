"""Edge sweep of the fused QKV launch mmdit_gemm_qkv_norm_rope (QKV projection + bf16 rounding + per-head QK RMSNorm + axial RoPE + joint-layout
scatter in ONE launch) through the C ABI, with PER-ELEMENT, PER-ROW and PER-COLUMN float64 parity for each of the three kernels that carry it.

test_kernels_gpu.py holds this launch to whole-tensor bars (6e-3 Frobenius against fp32 torch, "at most 1e-4 of the elements differ from the
two-launch path") at workload shapes only (H = 12 / 16: 3 H 64 a multiple of the 256-column tile, no q | k | v boundary inside a tile).  One token
rotated with its neighbour's table row, one head normalised with wk instead of wq, the first row behind a sample boundary written to the wrong
sample or a K tile dropped on the last row block passes there.  This file runs

  wide-slot kernel, 320 x 256 tile ("wide")       gemm_lean.hip -> gemm_tile.h epilogue_bf16_qk: bf16 operands, tile claiming off, planner code 387
  8-phase kernel, 256 x 256, EPI_QK ("8p")        gemm8p.hip epi8_qk: bf16 operands; tile claiming on (static and claimed walk), and claiming off
                                                  where the planner itself picks the 256 x 256 tile (code 386); C != NULL and C == NULL
  8-phase MX kernel, 256 x 256, EPI_QK ("mx")     gemm8p_inf.hip, the same epi8_qk: MX e4m3 operands, C != NULL and C == NULL

at the smallest shapes that reach each kernel, with heads 1 .. 5 and 7 (19 too on the MX kernel: q | k | v boundaries inside a tile, one to three
dead waves in the last tile), tokens per sample 1, 6, 31, 32, 33, 48, 63, 64, 65, 300 of a rotated stream and 1, 10, 31, 33, 154 of a stream
without tables (the per-row division of token_of, a 32-row block that wraps a sample boundary once, a block that starts on one, a sample that
spans two row tiles), M on, one sample before and one sample past a row-tile edge (256 k; 320 k for the wide kernel) and the wave tile inside
it (128 / 160 rows), 1 .. 5 K tiles (1 .. 3 for MX), one- and two-stream launches, gaps before and behind the written positions, FULL / ragged
tiles with and without the raw columns, and more tiles than workgroups.

Reaching a kernel (the library has no plan query for a launch WITH the epilogue; the rules of gemm.hip choose_kernel / pick_dma_cfg are restated
here as pick_cfg / fused_path, pinned against mmdit_gemm_plan without a GPU by test_qkv_epilogue_edges_cpu.py, and asserted before every launch):
  * MX operands, or bf16 operands with tile claiming on: the tile configuration is forced to 256 x 256 and the 8-phase EPI_QK kernel is the only
    kernel the launch can reach -- rc == 0 IS the path.  The walk is claimed when the workspace is registered, claiming is on, the operands are
    bf16 and there are more tiles than cu_budget; static otherwise.  C == NULL is accepted here only.
  * bf16 operands, claiming off: pick_dma_cfg decides as for the same problems without the epilogue.  320 x 256 (mmdit_gemm_plan == 387): the
    wide-slot kernel.  256 x 256 (386): the 8-phase EPI_QK kernel, static walk (MMDiT-B at batch 16 is such a launch).  128 x 128 (0):
    MMDIT_ERR_SHAPE, nothing written.  C == NULL: MMDIT_ERR_SHAPE whatever the tile.
  * every launch carries cu_budget = 64, so that the choice does not depend on the device's compute units.  With it the 320-row tile wins at
    roughly 4 000 .. 6 700 total rows (one round of at most 64 tiles of 320 x 256 against two rounds of 256 x 256), e.g. batch 32 x (16 + 154)
    tokens at H = 3 / 4, 24 x (16 + 154) at H = 5, 32 x (100 + 154) at H = 2, 65 x (100 + 154) at H = 1; at 12 900 rows and H = 4 it wins with
    two rounds (126 tiles: a workgroup walks two).

Reference and yardstick: two stages, each against plain float64 torch (no ops.* call; the MX quantiser mx_quant of this file is plain torch and
runs before the reference, its codes and scale bytes are the launch's inputs), nothing exempt.
  Stage 1, the projection.  raw = A B^T in float64 of the operands exactly as the kernel receives them (bf16 values; e4m3 codes x E8M0 scales
    through test_gemm_edges_gpu.mx_dequant).  The q and k columns of C are held to the GEMM sweep's bf16-output yardstick,
    y_det = c |A| |B|^T with c = (K + 8) 2^-23 (MX: max(c, 2 MX_KAPPA), as derived and probed there), y_rnd = U |raw|; the v columns of C must
    come back bit-identical to their sentinel (mmdit_hip.h: not written); V in the joint layout is the same rounded projection and is held to the
    same yardstick at row (b, head, tok0 + n).
  Stage 2, norm and rotation.  mmdit_hip.h: "the arithmetic of mmdit_qk_norm_rope_fwd on the ROUNDED raw values", so the q / k columns the launch
    itself wrote to C (exact bf16 inputs of this stage; stage 1 has held them to float64) go through the float64 closed form
      q = mean x^2 over the head's 64 features, r = rsqrt(q + eps), eps = 2^-23, n = x r w,  (a, b) -> (a c0 - b s0, b c1 + a s1)
    and Q / K are held to the row kernels' forward yardstick (test_rowops_edges_gpu.py, "QK-norm + RoPE", u = 2^-24, S = 12: 8 serial adds, 3
    butterfly steps, the scaling):  dq = (S + 1) u q, dr = r (0.5 dq / (q + eps) + 2 u), e_xn = |x| dr + u |xn|, e_n = |w| e_xn + u |n|,
      y_det = |c| e_n,a + |s| e_n,b + 2 u (|a c| + |b s|)   (without tables: e_n),   y_rnd = U |ref|
    compared as a 2-D tensor (batch heads tokens, 64) per stream and part: the "row" bar is per (sample, head, token), the "column" bar per feature.
    No term was added to either derivation.
  C == NULL launches have no raw output: Q, K and V must be bit-identical to the C != NULL launch of the same case in the same mode; both run.
  Every Q / K / V position outside [tok0, tok0 + tokens) of every (b, head), every guard row and every byte of C outside [M, 2 H 64] must come
  back bit-identical.
and every output must satisfy the bars of test_gemm_edges_gpu (ratios / verdict): per element 2.0, per row 1.0, per column 1.0, rounding bias 1.0.

Input families (seeded; each asserts its own precondition):
  random    every case.  randn operands, weight scale 0.05 sqrt(768 / K); wq, wk = 1 + 0.3 N(0, 1); cos and sin tables independent uniform values in
            [-1, 1] per (token, feature) -- no trigonometric pairs, so a swapped c0 / c1 or s0 / s1 or a neighbouring token's row shows.
  integer   cases on a tile edge.  Operands in [-3, 3] (MX: block scales 2^-2 .. 2^2): every partial sum is exact, the raw q / k columns and V
            must EQUAL the float64 reference wherever it is a bf16 number.
  smallrow  cases on a tile edge.  A rows scaled so that every head's rms is <= 1.2e-3: eps is then more than 5 % of the radicand q + eps
            (asserted on the launch's own raw columns), an eps of 1e-6 or 1e-5 fails (the CPU twin shows it).  One all-zero A row per stream:
            Q, K and V of that token must be exactly 0.
  poison    cases on a tile edge and every C == NULL case.  Operands (lda, ldb > K, 256 spare rows behind), wq / wk (64 floats) and the tables
            (exactly `tokens` rows) are views into larger NaN-filled tensors the test owns, MX scale buffers have padding bytes 0xFF, C has
            ldc > N and 256 guard rows before and behind.  Every byte a clamped or unconditional re-read can touch (the table's last row for rows
            past M, wq for a stream without rotation) lies inside a tensor the test allocated: this family checks values, never faults.
Q, K and V sit between 256 guard rows in every family.

Worst measured ratios per kernel, input family and output: profiles/qkv_epilogue_edge_sweep.txt.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # (comparator, poison helpers and MX layout are the GEMM sweep's, the closed-form helpers the row sweep's)
import test_gemm_edges_gpu as G  # noqa: E402
import test_rowops_edges_gpu as R  # noqa: E402

pytestmark = pytest.mark.gpu

U, E23, u = G.U, G.E23, R.u
RMS_EPS = R.RMS_EPS          # 2^-23 = finfo(float32).eps
GUARD = G.GUARD
BUDGET = 64                  # cu_budget of every launch
ERR_SHAPE = -3
BF = torch.bfloat16
PATTERN = G.Out.PATTERN[BF][1]
SMALL = 4e-4                 # smallrow family: scale of the A rows (head rms about 5.5e-4, at most 1e-3 over a case)


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ---------------------------------------------------------------------------------------------- the planner's rules, restated
def pick_cfg(shapes, cu, lean_ok=True, r256=1.58):      # gemm.hip pick_dma_cfg (no split, no stream-K); -> 0: 128 x 128, 2: 256 x 256, 3: 320 x 256
    cd = lambda a, b: (a + b - 1) // b      # noqa: E731
    t128 = sum(cd(M, 128) * cd(N, 128) for M, N in shapes)
    t256 = sum(cd(M, 256) * cd(N, 256) for M, N in shapes)
    c128, c256 = float(cd(t128, 2 * cu)), r256 * cd(t256, cu)
    if lean_ok:
        c320 = 1.25 * 1.58 * cd(sum(cd(M, 320) * cd(N, 256) for M, N in shapes), cu)
        if c320 < c256 and c320 < c128:
            return 3
    return 2 if c256 < c128 else 0


def fused_path(case, ws, claiming, raw=True, cu=BUDGET):      # gemm.hip choose_kernel, the branches of a launch with a QkRequest
    """(kernel, walk, plan code of the same problems without the epilogue | None) or None where the launch returns MMDIT_ERR_SHAPE."""
    mx = case.kernel == "mx"
    shapes = [(s.M, case.N) for s in case.streams]
    plain = None if mx else pick_cfg(shapes, cu)
    cfg = 2 if (mx or claiming) else plain
    code = None if mx else {0: 0, 2: 386, 3: 387}[plain]
    if cfg == 0 or (not raw and not (cfg == 2 and (mx or claiming))):
        return None
    tiles = sum(-(-M // (320 if cfg == 3 else 256)) * -(-N // 256) for M, N in shapes)
    if cfg == 3:
        return "wide", "multi" if tiles > cu else "single", code
    return ("mx" if mx else "8p"), ("claimed" if not mx and ws and claiming and tiles > cu else "multi" if tiles > cu else "single"), code


# ---------------------------------------------------------------------------------------------- the case table
class St:
    """One stream (problem) of a launch: `batch` samples of `tokens` rows, rotated (tables given) or not, written at joint position tok0."""

    def __init__(self, batch, tokens, rope, tok0):
        self.batch, self.tokens, self.rope, self.tok0, self.M = batch, tokens, rope, tok0, batch * tokens


WS_ON, CLAIM, CLAIM_NO_WS = (True, False), (True, True), (False, True)      # (workspace registered, tile claiming on)


class Case:
    """kernel: wide | 8p | mx; streams: (("x" rotated | "t" without tables, tokens per sample), ...) of one batch; gap: untouched joint positions
    before the first and behind the last stream; modes: the (workspace, claiming) settings it runs under (outputs bit-identical across them);
    walk: what fused_path must answer for the LAST mode; noraw: the C == NULL launch runs too; edge: runs the integer, smallrow and poison families."""

    def __init__(self, kernel, walk, H, K, batch, streams, gap=(0, 0), modes=None, noraw=False, edge=False, path=""):
        self.kernel, self.walk, self.H, self.K, self.batch, self.gap, self.noraw, self.edge, self.path = kernel, walk, H, K, batch, gap, noraw, edge, path
        self.N = 3 * H * 64
        self.modes = modes or ((CLAIM,) if kernel == "8p" else (WS_ON,))
        self.streams, pos = [], gap[0]
        for kind, tokens in streams:
            self.streams.append(St(batch, tokens, kind == "x", pos))
            pos += tokens
        self.s_total = pos + gap[1]
        self.id = (f"{kernel}:H{H}-K{K}-b{batch}-" + "+".join(f"{k}{t}" for k, t in streams) + (f"-gap{gap[0]}.{gap[1]}" if gap != (0, 0) else "")
                   + ("-noraw" if noraw else "") + ("-claimoff" if kernel == "8p" and self.modes[-1] == WS_ON else "") + (f"-{walk}" if walk != "single" else ""))

    @property
    def tile_rows(self):
        return 320 if self.kernel == "wide" else 256

    def row_edge(self):
        """on | before | past: some stream's M on, one sample before, one sample past a row-tile edge (None otherwise)."""
        out = set()
        for s in self.streams:
            r = s.M % self.tile_rows
            out |= {"on"} if r == 0 else {"before"} if r == self.tile_rows - s.tokens else {"past"} if r == s.tokens and s.M > self.tile_rows else set()
        return out


K8 = (64, 128, 192, 256, 320)


def _cases():
    out = []
    add = lambda *a, **kw: out.append(Case(*a, **kw))      # noqa: E731
    # ---- wide-slot kernel (claiming off, plan 387 at cu_budget 64).  Heads 1 .. 5, two streams; the first problem ends inside a 320-row tile
    add("wide", "single", 1, 64, 65, (("x", 100), ("t", 154)), edge=True, path="q, k, v and a dead wave in one tile")
    add("wide", "single", 2, 128, 32, (("x", 100), ("t", 154)), edge=True, path="tile 0 = q0 q1 k0 k1, tile 1 = v0 v1 + two dead waves")
    for K in K8:
        add("wide", "single", 3, K, 32, (("x", 16), ("t", 154)), edge=K == 64, path="part boundaries inside tiles 0 and 1; 1 .. 5 K tiles")
    add("wide", "single", 4, 64, 32, (("x", 16), ("t", 154)), path="aligned parts")
    add("wide", "single", 5, 192, 24, (("x", 16), ("t", 154)), edge=True, path="a last tile of 192 live columns")
    add("wide", "single", 7, 64, 16, (("x", 16), ("t", 154)), edge=True, path="a last tile of 64 live columns: three dead waves")
    # ... tokens per sample of a rotated stream; M = 17 x 320 on, one sample before, one sample past the edge
    for T, b, e in ((1, 5439, 1), (1, 5440, 1), (1, 5441, 1), (6, 907, 0), (31, 176, 0), (32, 169, 1), (32, 170, 1), (32, 171, 1), (33, 165, 0), (48, 114, 0),
                    (63, 87, 0), (64, 85, 1), (65, 84, 0), (300, 19, 0)):
        add("wide", "single", 4, 64, b, (("x", T),), edge=bool(e), path="token_of: per-row division (tokens < 32) / one wrap per 32-row block")
    for b in (5599, 5600, 5601):
        add("wide", "single", 4, 64, b, (("x", 1),), edge=True, path="M one row before, on and past the 160-row wave tile inside the last row tile")
    add("wide", "single", 3, 128, 165, (("x", 33),), gap=(5, 7), path="gaps on both sides of a rotated stream")
    # ... tokens of a stream without tables, gaps on both sides
    for T, b in ((1, 5441), (10, 544), (31, 176), (33, 165), (154, 36)):
        add("wide", "single", 3, 128, b, (("t", T),), gap=(3, 5), path="no tables: wq stands in for the factors and is ignored")
    add("wide", "multi", 4, 64, 43, (("x", 300),), path="126 tiles of 320 x 256 on 64 workgroups: a workgroup walks two")
    # ---- 8-phase kernel, bf16 operands, claiming on.  Heads 1 .. 5 x K tiles 1 .. 5, ragged tiles, raw columns on and off
    for H, K in zip((1, 2, 3, 4, 5), K8):
        add("8p", "single", H, K, 2, (("x", 100), ("t", 154)), noraw=True, edge=True, path="ragged tiles (FULL = false), RAW on and off; the first problem ends mid-tile")
    add("8p", "single", 7, 64, 2, (("x", 100), ("t", 154)), noraw=True, edge=True, path="a last tile of 64 live columns: three dead waves")
    add("8p", "single", 4, 64, 8, (("x", 32), ("t", 32)), noraw=True, edge=True, path="every tile full (FULL = true), RAW on and off")
    for T, b, e, nr in ((1, 255, 1, 0), (1, 256, 1, 1), (1, 257, 1, 1), (6, 43, 0, 0), (31, 9, 0, 0), (32, 7, 1, 0), (32, 8, 1, 0), (32, 9, 1, 1), (33, 8, 0, 0),
                        (48, 11, 0, 0), (63, 5, 0, 0), (64, 5, 0, 0), (65, 4, 0, 0), (300, 2, 0, 1)):
        add("8p", "single", 3, 64, b, (("x", T),), noraw=bool(nr), edge=bool(e), path="token_of; M on / one sample before / past 256; a sample across two row tiles (48, 300)")
    for b in (511, 512, 513):
        add("8p", "single", 2, 128, b, (("x", 1),), edge=True, path="the second row-tile edge")
    for b in (127, 128, 129):
        add("8p", "single", 5, 64, b, (("x", 1),), edge=True, noraw=b == 129, path="M one row before, on and past the 128-row wave tile inside the row tile")
    add("8p", "single", 3, 192, 8, (("x", 33),), gap=(5, 7), noraw=True, path="gaps on both sides of a rotated stream")
    for T, b in ((1, 257), (10, 26), (31, 9), (33, 8), (154, 2)):
        add("8p", "single", 5, 128, b, (("t", T),), gap=(3, 5), noraw=T in (1, 154), path="no tables: wq stands in for the factors and is ignored")
    # ... more tiles than the budget: the static walk (claiming on, no workspace), then the claimed walk -- bit-identical
    for K in (64, 192):
        add("8p", "claimed", 5, K, 18, (("x", 300),), modes=(CLAIM_NO_WS, CLAIM), path="88 tiles on 64 workgroups: static, then claimed")
    add("8p", "claimed", 4, 128, 36, (("x", 16), ("t", 154)), modes=(CLAIM_NO_WS, CLAIM), noraw=True, path="75 tiles, two streams: static, then claimed; RAW on and off")
    # ... claiming off, the planner's own 256 x 256 tile (plan 386): the same kernel, static walk; C == NULL is refused there (test_refusals)
    add("8p", "single", 4, 64, 16, (("x", 16), ("t", 154)), modes=(WS_ON,), path="claiming off, plan 386 (MMDiT-B at batch 16)")
    add("8p", "single", 5, 320, 16, (("x", 16), ("t", 154)), modes=(WS_ON,), path="claiming off, plan 386")
    # ---- 8-phase MX kernel (K % 128 == 0: heads and K independently), every case with C != NULL and C == NULL
    for H, K in ((1, 128), (2, 256), (3, 384), (4, 128), (5, 256), (3, 128), (3, 256)):
        add("mx", "single", H, K, 2, (("x", 100), ("t", 154)), noraw=True, edge=H != 3 or K == 384, path="ragged tiles, RAW on and off; 1 .. 3 K tiles")
    for H in (7, 19):      # (the head counts of the odd-width fp8 / mxfp8 models)
        add("mx", "single", H, 128, 2, (("x", 100), ("t", 154)), noraw=True, edge=True, path="a last tile of 64 live columns: three dead waves")
    add("mx", "single", 4, 128, 8, (("x", 32), ("t", 32)), noraw=True, edge=True, path="every tile full, RAW on and off")
    for T, b, e in ((1, 255, 1), (1, 256, 1), (1, 257, 1), (6, 43, 0), (31, 9, 0), (32, 7, 1), (32, 8, 1), (32, 9, 1), (33, 8, 0), (48, 11, 0), (63, 5, 0),
                    (64, 5, 0), (65, 4, 0), (300, 2, 0)):
        add("mx", "single", 3, 128, b, (("x", T),), noraw=True, edge=bool(e), path="token_of; M on / one sample before / past 256")
    for b in (127, 128, 129):
        add("mx", "single", 5, 128, b, (("x", 1),), edge=True, noraw=True, path="M one row before, on and past the 128-row wave tile inside the row tile")
    for T, b in ((1, 257), (10, 26), (31, 9), (33, 8), (154, 2)):
        add("mx", "single", 2, 256, b, (("t", T),), gap=(3, 5), noraw=True, path="no tables")
    add("mx", "single", 3, 256, 8, (("x", 33),), gap=(5, 7), noraw=True, path="gaps on both sides of a rotated stream")
    add("mx", "multi", 5, 128, 18, (("x", 300),), noraw=True, path="88 tiles on 64 workgroups (static walk)")
    return out


ALL = _cases()
# launches the library must refuse with MMDIT_ERR_SHAPE, writing nothing: (case, raw)
REFUSED = [(Case("8p", "single", 4, 256, 3, (("x", 24), ("t", 10)), modes=(WS_ON,), path="claiming off, 128 x 128 (plan 0)"), True),
           (Case("8p", "single", 3, 64, 8, (("x", 33),), modes=(WS_ON,), path="claiming off, 128 x 128 (plan 0)"), True),
           (Case("wide", "single", 4, 64, 32, (("x", 16), ("t", 154)), path="bf16, C == NULL, claiming off (plan 387)"), False),
           (Case("8p", "single", 4, 64, 16, (("x", 16), ("t", 154)), modes=(WS_ON,), path="bf16, C == NULL, claiming off (plan 386)"), False)]
CASES = ([(c, "random") for c in ALL] + [(c, f) for f in ("integer", "smallrow") for c in ALL if c.edge]
         + [(c, "poison") for c in ALL if c.edge or c.noraw])


def _case_id(case):
    return f"{case[0].id}-{case[1]}"


# ---------------------------------------------------------------------------------------------- operands
def mx_quant(x):
    """(rows, K) -> e4m3 codes (rows, K) and E8M0 bytes (rows, K / 32): the block's scale is 2^(floor(log2 amax) - 8) (e4m3's largest binade is
    2^8), an all-zero block gets byte 0 and codes 0.  Plain torch: what it returns are the launch's INPUTS."""
    rows, K = x.shape
    xb = x.float().view(rows, K // 32, 32)
    amax = xb.abs().amax(-1)
    e = torch.where(amax > 0, torch.floor(torch.log2(amax.clamp_min(1e-38))) - 8, torch.full_like(amax, -127.0)).clamp(-127, 127)
    q = (xb * torch.exp2(-e).unsqueeze(-1)).clamp(-448, 448).reshape(rows, K).to(torch.float8_e4m3fn)
    return q, (e + 127).to(torch.uint8)


def _view_in_nan(x, rows_before, poison):
    """x (fp32, 1-D or 2-D, contiguous rows) as the kernel receives it: itself, or (poison) a view into a larger NaN-filled tensor."""
    if not poison:
        return x.contiguous()
    lead = 16 if x.dim() == 1 else rows_before
    big = torch.full((x.shape[0] + 2 * lead,) + tuple(x.shape[1:]), float("nan"), dtype=x.dtype, device=x.device)
    big[lead:lead + x.shape[0]] = x
    return big[lead:lead + x.shape[0]]


def build(case, family, device):
    """Operands and epilogue inputs of every stream of a case.  Per stream a dict: kw (A, B and the scale arguments of ops._fill_gemm), A64 (M, K)
    and B64 (N, K) in float64, wq, wk (64,), cos, sin (tokens, 64) or None, zero_row (smallrow: the all-zero A row), unit (integer: the spacing
    of every partial sum)."""
    poison, fam = family == "poison", "random" if family == "poison" else family
    mx = case.kernel == "mx"
    out = []
    for i, s in enumerate(case.streams):
        g = torch.Generator().manual_seed(1000003 * s.M + 1009 * case.N + 17 * case.K + 7 * i + {"random": 1, "integer": 2, "smallrow": 3}[fam])
        rn = lambda *sh: torch.randn(*sh, generator=g)      # noqa: E731
        ri = lambda lo, hi, *sh: torch.randint(lo, hi + 1, sh, generator=g).float()      # noqa: E731
        t = dict(unit=1.0, zero_row=None)
        if fam == "integer":
            A, W = ri(-3, 3, s.M, case.K), ri(-3, 3, case.N, case.K)
        else:
            A, W = rn(s.M, case.K), rn(case.N, case.K) * (0.05 * math.sqrt(768.0 / case.K))
        if fam == "smallrow":
            A = A * SMALL
            t["zero_row"] = s.M // 2
            A[t["zero_row"]] = 0.0
        wq, wk = (1 + 0.3 * rn(64)).to(device), (1 + 0.3 * rn(64)).to(device)
        cos = sin = None
        if s.rope:
            cos, sin = (2 * torch.rand(s.tokens, 64, generator=g) - 1).to(device), (2 * torch.rand(s.tokens, 64, generator=g) - 1).to(device)
        A, W = A.to(BF).to(device), W.to(BF).to(device)
        kw = {}
        if not mx:
            t["A64"], t["B64"] = A.double(), W.double()
        else:
            sc = []
            for name, x, rows in (("A64", A, s.M), ("B64", W, case.N)):
                if fam == "integer":
                    qx, by = x.to(torch.float8_e4m3fn), (127 + ri(-2, 2, rows, case.K // 32)).to(torch.uint8).to(device)
                else:
                    qx, by = mx_quant(x)
                t[name] = G.mx_dequant(qx, by)
                sc.append(G.mx_pack(by, 0xFF if poison else 127, 0xFF if poison else 127))
                A, W = (qx, W) if name == "A64" else (A, qx)
            kw.update(scale_a=sc[0], scale_b=sc[1], scale_mode=1)
            t["unit"] = 2.0 ** -4
        kw.update(A=G._place(A, poison), B=G._place(W, poison))
        t.update(kw=kw, wq=_view_in_nan(wq, 0, poison), wk=_view_in_nan(wk, 0, poison),
                 cos=None if cos is None else _view_in_nan(cos, 1, poison), sin=None if sin is None else _view_in_nan(sin, 1, poison))
        if fam == "integer":
            worst = float((t["A64"].abs() @ t["B64"].abs().T).max())
            assert worst / t["unit"] < 2.0 ** 24, f"integer family: max |A||B|^T = {worst} units of {t['unit']}"
        if fam == "smallrow":
            assert float(t["A64"][t["zero_row"]].abs().max()) == 0.0
        out.append(t)
    return out


# ---------------------------------------------------------------------------------------------- float64 references + yardsticks
def stage1(case, t):
    """raw = A B^T, its deterministic and its rounding yardstick, (M, N) each."""
    raw, absP = t["A64"] @ t["B64"].T, t["A64"].abs() @ t["B64"].abs().T
    c = (case.K + 8) * E23
    return raw, (max(c, 2 * G.MX_KAPPA) if case.kernel == "mx" else c) * absP, U * raw.abs()


def to_heads(z):
    """(batch, tokens, heads, 64) -> rows (batch heads tokens, 64): the joint layout's order."""
    return z.permute(0, 2, 1, 3).reshape(-1, 64)


def stage2(x, w, cos, sin, eps=RMS_EPS):
    """QK RMSNorm + RoPE of the exact inputs x (batch, tokens, heads, 64) in float64 with the row kernels' forward yardstick: ref, y_det, y_rnd as
    rows (batch heads tokens, 64)."""
    w = w.double()
    q = (x * x).mean(-1, keepdim=True)
    r = (q + eps).rsqrt()
    xn = x * r
    n = xn * w
    dr = r * (0.5 * 13 * u * q / (q + eps) + 2 * u)
    e_xn = x.abs() * dr + u * xn.abs()
    e_n = w.abs() * e_xn + u * n.abs()
    if cos is None:
        ref, det = n, e_n
    else:
        c0, c1 = R._qk_split(cos.double()[None, :, None, :])
        s0, s1 = R._qk_split(sin.double()[None, :, None, :])
        a, b = R._qk_split(n)
        ea, eb = R._qk_split(e_n)
        ref = R._qk_join(a * c0 - b * s0, b * c1 + a * s1)
        det = R._qk_join(c0.abs() * ea + s0.abs() * eb + 2 * u * ((a * c0).abs() + (b * s0).abs()),
                         c1.abs() * eb + s1.abs() * ea + 2 * u * ((b * c1).abs() + (a * s1).abs()))
    ref = to_heads(ref)
    return ref, to_heads(det), U * ref.abs()


# ---------------------------------------------------------------------------------------------- outputs
class Joint:
    """Q, K or V (batch, heads, s_total, 64) bf16, contiguous, between GUARD guard rows of 64; every element starts as a NaN bit pattern.
    touched(spans): the elements outside the (tok0, tokens) spans of every (b, head) -- guard rows included -- that differ from the snapshot."""

    def __init__(self, batch, heads, s_total, device):
        self.shape, self.rows = (batch, heads, s_total, 64), batch * heads * s_total
        self.big = torch.empty((self.rows + 2 * GUARD, 64), dtype=BF, device=device)
        self.big.view(torch.int16).fill_(PATTERN)
        self.win = self.big[GUARD:GUARD + self.rows].view(self.shape)
        self.snap = None

    def snapshot(self):
        self.snap = self.big.clone()

    def touched(self, spans):
        d = self.big.view(torch.int16) != self.snap.view(torch.int16)
        w = d[GUARD:GUARD + self.rows].view(self.shape)
        for tok0, tokens in spans:
            w[:, :, tok0:tok0 + tokens] = False
        return [tuple(i) for i in d.nonzero()[:8].tolist()], int(d.sum())


def fresh_outputs(case, guarded, device):
    got = dict(C=[G.Out(s.M, case.N, BF, guarded, device) for s in case.streams])
    for c in got["C"]:
        c.snapshot()
    for name in "QKV":
        got[name] = Joint(case.batch, case.H, case.s_total, device)
        got[name].snapshot()
    return got


WORST = {}             # (kernel, input family, output) -> [per-element, per-row, per-column, rounding bias] as (ratio, case id)


def _compare(case, family, what, name, got, ref, det, rnd, failures, record, exact=False):
    if not bool(torch.isfinite(got).all()):
        failures.append(f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements")
        return
    r = G.ratios(got, ref, det, rnd)
    if record:
        w = WORST.setdefault((case.kernel, family, name), [(-1.0, "")] * 4)
        for i, k in enumerate(("el", "row", "col", "bias")):
            if r[k] is not None and r[k] > w[i][0]:
                w[i] = (r[k], f"{case.id} {what}")
    print(f"[qkv edges] {case.id} {family} {what}: elem {r['el']:.3f} @ ({r['at'][0]}, {r['at'][1]}) row {r['row']:.3f} @ {r['at'][2]} col {r['col']:.3f} @ {r['at'][3]}"
          + (f" bias {r['bias']:.3f}" if r["bias"] is not None else ""))
    bad = G.verdict(r)
    if bad:
        failures.append(f"{what}: {bad} over the bar: {r}")
    if exact:
        wrong, of = G.exact_mismatches(got, ref)
        if wrong:
            failures.append(f"{what}: {wrong} of {of} exactly representable elements differ from the float64 reference")


def judge(case, family, built, got, raw=True, base=None, tag="", record=True, eps=RMS_EPS):
    """Every check of one launch's outputs; returns the list of failures.  got: dict C (one G.Out per stream), Q, K, V (Joint).  raw = False (the
    C == NULL launch): C must be untouched and Q, K, V bit-identical to `base`, the windows of the C != NULL launch."""
    failures = []
    D = case.H * 64
    spans = [(s.tok0, s.tokens) for s in case.streams]
    for name in "QKV":
        where, count = got[name].touched(spans)
        if count:
            failures.append(f"{name}{tag}: {count} elements outside the written positions changed, first (row, feature) {where}")
    if not raw:
        for i, c in enumerate(got["C"]):
            if not torch.equal(c.big.view(torch.int16), c.snap.view(torch.int16)):
                failures.append(f"p{i}.C{tag}: written although C == NULL was passed")
        for name in "QKV":
            if not torch.equal(got[name].win.view(torch.int16), base[name].view(torch.int16)):
                failures.append(f"{name}{tag}: differs from the C != NULL launch ({int((got[name].win.view(torch.int16) != base[name].view(torch.int16)).sum())} elements)")
        return failures
    for i, (s, t, c) in enumerate(zip(case.streams, built, got["C"])):
        B, T, H = s.batch, s.tokens, case.H
        ref1, det1, rnd1 = stage1(case, t)
        where, count = c.touched()
        if count:
            failures.append(f"p{i}.C{tag}: {count} bytes outside the [M, N] window changed, first (row, byte) {where}")
        nv = int((c.win[:, 2 * D:].contiguous().view(torch.int16) != PATTERN).sum())
        if nv:
            failures.append(f"p{i}.C{tag}: {nv} elements of the v columns were written (mmdit_hip.h: not written)")
        qk_raw = c.win[:, :2 * D]
        _compare(case, family, f"p{i}.Cqk{tag}", "Cqk", qk_raw, ref1[:, :2 * D], det1[:, :2 * D], rnd1[:, :2 * D], failures, record, exact=family == "integer")
        v = lambda z: to_heads(z[:, 2 * D:].reshape(B, T, H, 64))      # noqa: E731
        pos = slice(s.tok0, s.tok0 + T)
        _compare(case, family, f"p{i}.V{tag}", "V", got["V"].win[:, :, pos].reshape(-1, 64), v(ref1), v(det1), v(rnd1), failures, record, exact=family == "integer")
        if not bool(torch.isfinite(qk_raw).all()):
            continue
        x = qk_raw.double().reshape(B, T, 2, H, 64)
        if family == "smallrow":
            qh = (x * x).mean(-1)
            assert float(qh.max().sqrt()) <= 1.2e-3, f"smallrow family: head rms {float(qh.max().sqrt())} above 1.2e-3"
            assert float((RMS_EPS / (qh + RMS_EPS)).min()) > 0.05, "smallrow family: eps is less than 5 % of the radicand"
        for part, name in ((0, "Q"), (1, "K")):
            ref2, det2, rnd2 = stage2(x[:, :, part], t["w" + name.lower()], t["cos"], t["sin"], eps)
            _compare(case, family, f"p{i}.{name}{tag}", name, got[name].win[:, :, pos].reshape(-1, 64), ref2, det2, rnd2, failures, record)
        if family == "smallrow":
            b, n = divmod(t["zero_row"], T)
            for name in "QKV":
                nz = int((got[name].win[b, :, s.tok0 + n].float() != 0).sum())
                if nz:
                    failures.append(f"p{i}.{name}{tag}: {nz} non-zero elements at the token of the all-zero A row")
    return failures


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\n[qkv epilogue edge sweep] worst ratio to the yardstick per kernel, input family and output (bars: per element 2.0, per row / column 1.0, rounding bias 1.0)")
    for (kf, fam, name), w in sorted(WORST.items()):
        print(f"  {kf:<5} {fam:<9} {name:<4} " + "  ".join(f"{n} {v:.3f} @ {cid}" for n, (v, cid) in zip(("elem", "row", "col", "bias"), w) if v >= 0))


@pytest.fixture(scope="module")
def workspace(ops):
    return torch.zeros(G.WS_BYTES, dtype=torch.uint8, device="cuda")


# ---------------------------------------------------------------------------------------------- the sweep
def _launch(ops, case, built, got, mode, raw, workspace):
    """One fused launch into `got` under (workspace, claiming) = mode; asserts the planner's code of the same problems without the epilogue
    immediately before it (bf16, claiming off) and returns the library's return code."""
    lib = ops._lib.lib()
    use_ws, claiming = mode
    n = len(case.streams)
    assert lib.mmdit_gemm_set_workspace(workspace.data_ptr() if use_ws else None, workspace.numel() if use_ws else 0) == 0
    assert lib.mmdit_gemm_set_claiming(int(claiming)) == 0 and lib.mmdit_gemm_get_claiming() == int(claiming)
    arr, qk = (ops.GemmArgs * n)(), (ops._lib.QkEpilogue * n)()
    for i, (s, t, c) in enumerate(zip(case.streams, built, got["C"])):
        ops._fill_gemm(arr[i], out=c.win, cu_budget=BUDGET, **t["kw"])
        assert (arr[i].M, arr[i].N, arr[i].K) == (s.M, case.N, case.K)
        qk[i].wq, qk[i].wk, qk[i].tokens, qk[i].tok0 = t["wq"].data_ptr(), t["wk"].data_ptr(), s.tokens, s.tok0
        if s.rope:
            qk[i].rope_cos, qk[i].rope_sin = t["cos"].data_ptr(), t["sin"].data_ptr()
    expect = fused_path(case, use_ws, claiming, raw)
    if case.kernel != "mx" and not claiming:
        plain = fused_path(case, use_ws, claiming)      # (with the raw columns: the plan of the problems themselves)
        plan = lib.mmdit_gemm_plan(arr, n)
        assert plan == (plain[2] if plain else 0), f"{case.id}: planned as {plan}, the restated planner says {plain}"
        if case.kernel == "wide":
            assert plan == 387, f"{case.id}: planned as {plan}, the wide-slot kernel needs 387"
    if not raw:
        for i in range(n):
            arr[i].C = None
    torch.cuda.synchronize()
    rc = lib.mmdit_gemm_qkv_norm_rope(arr, qk, n, case.H, case.s_total, got["Q"].win.data_ptr(), got["K"].win.data_ptr(), got["V"].win.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a HIP error ends the session: nothing more is started on a device that has reported one
        pytest.exit(f"HIP error behind {case.id} (mode {mode}, raw {raw}): {e}", returncode=3)
    assert (rc == ERR_SHAPE) if expect is None else (rc == 0), f"{case.id}: rc {rc}, the restated planner expects {expect}"
    return rc, expect


def _restore(ops, prev):
    lib = ops._lib.lib()
    torch.cuda.synchronize()
    assert lib.mmdit_gemm_set_claiming(0) == 0
    assert lib.mmdit_gemm_set_workspace(prev.data_ptr() if prev is not None else None, prev.numel() if prev is not None else 0) == 0


def _run_case(ops, workspace, c, family):
    """One case under one input family; returns the list of failures (a failed path assertion is one of them)."""
    prev = ops._GEMM_WS.get(torch.device("cuda", torch.cuda.current_device()))
    built = build(c, family, "cuda")
    failures, runs = [], []
    try:
        for mi, mode in enumerate(c.modes):
            tag = "" if len(c.modes) == 1 else f" ws={int(mode[0])} claim={int(mode[1])}"
            got = fresh_outputs(c, family == "poison", "cuda")
            rc, expect = _launch(ops, c, built, got, mode, True, workspace)
            assert expect[0] == c.kernel and (mi + 1 < len(c.modes) or expect[1] == c.walk), (c.id, expect)
            failures += judge(c, family, built, got, tag=tag)
            base = {name: got[name].win.clone() for name in "QKV"}
            runs.append(base)
            if c.noraw:
                got2 = fresh_outputs(c, family == "poison", "cuda")
                rc, expect = _launch(ops, c, built, got2, mode, False, workspace)
                assert expect[0] == c.kernel, (c.id, expect)
                failures += judge(c, family, built, got2, raw=False, base=base, tag=tag + " C=NULL")
    except AssertionError as e:
        failures.append(f"kernel path: {e}")
    finally:
        _restore(ops, prev)
    for other in runs[1:]:
        for name in "QKV":
            if not torch.equal(runs[0][name].view(torch.int16), other[name].view(torch.int16)):
                failures.append(f"{name} differs between {c.modes[0]} and a later mode")
    if int(workspace[:8192].view(torch.int32).abs().sum()) != 0:
        failures.append("tickets / queue heads are not left zero")
    return [f"{c.id} {family} [{c.path}] {f}" for f in failures]


GROUPS = sorted({(c.kernel, f) for c, f in CASES})      # one test per (kernel, input family): the cases of the table are its launches


@pytest.mark.parametrize("group", GROUPS, ids="-".join)
def test_qkv_epilogue_edge(ops, workspace, group):
    """Every case of one kernel under one input family (each a fraction of a second; a failure names its case): the kernel path asserted (planner
    code before the launch, the restated rules' answer, rc), the raw q / k columns and V within the bars of stage 1, the v columns of C and every
    unwritten position bit-identical, Q and K within the bars of stage 2 computed from the launch's own raw columns; the C == NULL launch
    bit-identical in Q, K, V; the static and the claimed walk bit-identical; the workspace's first 8 192 bytes left zero."""
    mine = [(c, f) for c, f in CASES if (c.kernel, f) == group]
    assert mine
    failures = [f for c, fam in mine for f in _run_case(ops, workspace, c, fam)]
    assert not failures, f"{len(failures)} failures in {len(mine)} cases:\n" + "\n".join(failures)


def test_refused_launch_returns_err_shape_and_writes_nothing(ops, workspace):
    """Small shapes the planner keeps on 128 x 128 tiles, and bf16 operands with C == NULL, with claiming off: MMDIT_ERR_SHAPE, and C, Q, K, V
    bit-identical afterwards (the caller runs mmdit_gemm_grouped + mmdit_qk_norm_rope_fwd instead)."""
    for c, raw in REFUSED:
        prev = ops._GEMM_WS.get(torch.device("cuda", torch.cuda.current_device()))
        built = build(c, "random", "cuda")
        got = fresh_outputs(c, True, "cuda")
        try:
            rc, expect = _launch(ops, c, built, got, WS_ON, raw, workspace)
        finally:
            _restore(ops, prev)
        assert rc == ERR_SHAPE and expect is None, (c.id, raw)
        for name in "QKV":
            assert got[name].touched([]) == ([], 0), (c.id, raw, name)
        for o in got["C"]:
            assert torch.equal(o.big.view(torch.int16), o.snap.view(torch.int16)), (c.id, raw)
