"""Tile-edge sweep of the GEMM kernels (csrc/gemm.hip, gemm_dma.hip, gemm_lean.hip, gemm8p.hip) with PER-ELEMENT, PER-ROW and PER-COLUMN
float64 parity through the C ABI.

test_kernels_gpu.py holds the GEMMs to whole-tensor Frobenius bars (1e-5 for fp32, 4e-3 .. 6e-3 for bf16 outputs) and reaches the 8-phase kernels at
workload size only (12 K tiles, M and N wherever the model puts them).  A row that lost one K tile, or a clamped row counted twice, passes there.
This file runs every kernel family

  register-staged gemm_kernel (plan 64)          bf16 and 3-term split fp32, all three layouts, K % 64 != 0
  LDS-DMA kernel 128 x 128 (plan 0)              all three layouts, fp32 / bf16 out, caller split-K, e4m3 per-tensor and MX operands
  LDS-DMA kernel 256 x 256 (plan 2)              fp32 out with the gate / residual / aux epilogue
  8-phase kernel, 256 rows (plan 386)            forward, bias + SiLU, data gradient, SwiGLU, SwiGLU backward, plain weight gradient, grouped, claimed
  8-phase kernel, 320 rows (plan 387)
  weight gradient, round + split tail (418)      K tails, atomics and workspace slots, balanced tail, grouped
  8-phase e4m3 kernel (plan 258)                 per-tensor and MX scales, SwiGLU
  implicit-GEMM 3x3 convolution                  LDS-DMA kernel at 128 x 128 (plan 0) and 256 x 256 (plan 2: the epilogues conv8 of gemm.hip refuses -- SiLU,
                                                 bf16 output + residual, aux) and the 8-phase CONV instantiation (plan 258 with conv_mode set: bf16 + bias,
                                                 fp32 + bias, fp32 + bias + residual), both modes, C = 64 / 128 / 192 (3 / 6 / 9 K tiles per kernel row),
                                                 image boundaries on, before and inside tiles, H = 1, a second and third tile per workgroup, grouped

at the smallest shapes that reach it, with M and N on, one before and one past a tile edge and 1 .. 5 K tiles (the two-tile prologue of the 8-phase
loop, its clamped "request the last K tile again" stagings, the odd trailing tile), and asserts the planner's code before every launch (the product
library ignores the environment switches: a kernel is reached through shapes and cu_budget only; tests/test_gemm_edges_cpu.py pins the same table
without a GPU).

Reference: plain float64 torch matmul of the operands exactly as the kernel receives them (bf16 values, e4m3 codes x scales, fp32 for the split mode),
epilogue in float64 (_reference: no ops.* call; the e4m3 / MX quantisers run before it, their outputs are inputs).  A convolution's A is the
zero-bordered NHWC operand (B, H + 2, W + 2, C); its float64 A (M, 9 C) is an explicit index gather written here (conv_gather: output row
(b, yo, xo), column (kh 3 + kw) C + c reads padded pixel (s yo + kh + o, s xo + kw + o), s = 1 | 2, o = 0 | 1 for mode 1 | 2), which
test_gemm_edges_cpu.py holds to torch.nn.functional.conv2d in float64; from there on it is the same product, epilogue and yardstick (K = 9 C).

Yardstick (derived from the kernels' rounding points, not tuned).  U = 2^-8 is the unit roundoff of bf16, products of bf16 and of e4m3 operands are
exact in fp32, an fp32 accumulation of K terms in any order errs by at most (K - 1) 2^-24 |A| |B|^T to first order; 2^-23 per term also covers
accumulators that truncate.  Componentwise, with c = (K + S + 8) 2^-23, S = the K slices of a caller split (split_k) or of a split tail (at most the
number of K tiles: empty slices add exact zeros), 8 = the epilogue's fp32 operations (bias, scale product, gate, residual, accumulate, activation):

  y_pre = c (|A| |B|^T + |bias|)  +  2^-22 |A| |B|^T                    (second term: split precision only, the dropped a1b2, a2b1, a2b2 passes of
                                                                          gemm.hip:15-16, each below 2^-24 |a| |b|)
  v     = residual + gate * pre + C_in:   y_det = |gate| y_pre + c (|residual| + |C_in|)        (the gate multiplies what it multiplies in the epilogue)
  bf16 output or bf16 aux:                y_rnd = U |ref|
  SiLU (|silu'| <= 1.1):                  y_det = 1.1 y_pre
  SwiGLU (mmdit_hip.h:40-44: h = silu(g) u from the bf16-ROUNDED [g | u]):
                                          y_det = 1.1 |u| y_pre,g + |silu(g)| y_pre,u,   y_rnd = U |h| + 1.1 |u| U |g| + |silu(g)| U |u|
                                          aux = [g | u] is a bf16 output of its own
  SwiGLU backward (mmdit_hip.h:46-52: d[g | u] from the bf16-ROUNDED dh = A B and the saved bf16 [g | u], which are exact inputs;
                   common.h swiglu_bwd_f: dg = dh u s (1 + g (1 - s)), du = dh g s, s = sigmoid(g)): with f_g = u s (1 + g (1 - s)), f_u = g s
                                          y_det = |f| c |A| |B|^T + 8 * 2^-23 (1 + |g|) |dh| |u or 1|      (second term: f itself evaluated in fp32)
                                          y_rnd = |f| U |dh| + U |ref|
                   dbias: the kernel sums the fp32 values BEFORE they are rounded to bf16 (gemm8p.hip epi8_swiglu_bwd: sg[e] += og[e]; the row kernel
                   mlp_act_bwd does the same), so it is held to the float64 column sum of the reference, not of the rounded outputs:
                                          y = colsum(y_det + |f| U |dh|) + M 2^-23 colsum |ref|
  y = y_det + y_rnd
  MX operands (E8M0 block scales) only: the random family exceeded y_pre on an fp32 output (3.16 per element at (257, 264, 128)) while the integer
  family was exact, so c |A| |B|^T is replaced by max(c, 2 kappa) |A| |B|^T with kappa = 9.8353e-5 = 2^-13.3, the accumulation error of ONE
  v_mfma_scale_f32_32x32x64_f8f6f4 on 64 products against float64 relative to sum |a_k| |b_k|, measured by tools/probes/mx_acc_probe.hip on
  operands like this file's (randn codes, block scales 2^-8 .. 2^8), never taken from the GEMM kernels.  Per-tensor e4m3 stays on c (worst 1.46).

and every output of every case must satisfy, for every element, every row and every column, with nothing exempt,

  |out - ref| <= 2.0 y          ||out_row - ref_row||_2 <= 1.0 ||y_row||_2          ||out_col - ref_col||_2 <= 1.0 ||y_col||_2

A float32-accumulating model rounded to bf16 reaches about 0.99 per element and 0.5 per row; a row that lost one K tile or was replaced by its
neighbour lands at tens to thousands (test_gemm_edges_cpu.py checks both statements on this comparator).  Those three bars cannot see a bf16 output
that is TRUNCATED instead of rounded (error below 2 U |ref| per element, about ||y|| per row), so bf16 outputs of 64 elements or more are also held to

  |sum_j sign(ref_j) (out_j - ref_j)| <= 6 ||y_rnd||_2 + ||y_det||_1

(round to nearest leaves zero-mean errors bounded by y_rnd: Hoeffding gives 2 exp(-18) for 6 ||y_rnd||_2; whatever is systematic is bounded by y_det
element by element; truncation gives about 0.75 ||y_rnd||_1).

Input families (seeded; each asserts its own precondition):
  random    randn operands; MX: block magnitudes 2^-8 .. 2^8 and one all-zero block.
  integer   operands in [-3, 3], integer bias / residual, power-of-two gate, power-of-two scales: every partial sum is exact in fp32 in any order
            (max |A| |B|^T < 2^24 units is asserted), so an fp32 output must EQUAL the float64 reference and a bf16 output must equal it wherever the
            reference is a bf16 number (every integer below 256 is).
  poison    the random operands as views into larger tensors the test owns: leading dimensions larger than the extent, 256 spare rows behind the last
            operand row, everything outside the operand NaN (e4m3 codes 0x7F, scale bytes 0xFF: padding rows and the 512 spare bytes); outputs with
            ldc / ld_aux > N and 256 guard rows before and behind, every byte outside [M, N] a bit pattern that must come back bit-identical.
            Every byte a clamped or over-wide access can touch lies inside a tensor the test allocated: this family checks values, not faults.
random runs on every case, integer and poison where M, N or K sits one step (1 row, 8 columns) before or past a tile edge.

Worst measured ratios per kernel family and input family: profiles/r09_gemm_edge_sweep.txt; the convolution families: profiles/conv_vae_edge_sweep.txt.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -8              # bf16 unit roundoff (round to nearest)
E23 = 2.0 ** -23
MX_KAPPA = 9.8353e-5       # accumulation error of one MX MFMA on 64 products (tools/probes/mx_acc_probe.hip, families 4 / 5; profiles/r09_gemm_edge_sweep.txt)
ELEM_BAR, ROW_BAR, BIAS_SIGMAS = 2.0, 1.0, 6.0
ACT_NONE, ACT_SILU, ACT_SWIGLU, ACT_SWIGLU_BWD = 0, 1, 2, 3
GUARD = 256                # guard rows before and behind an output, spare rows behind an operand
WS_BYTES = 8192 + 512 * 65536 * 4


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ---------------------------------------------------------------------------------------------- problems and launches
class P:
    """One problem of a launch.  lay: nt (A (M, K), B (N, K)), dgrad (B stored (K, N)), wgrad (A stored (K, M), B stored (K, N)); ab: operand format
    bf16 | split (fp32 operands, 3-term split) | e4m3 (per-tensor scales) | mx (E8M0 block scales); out: bf16 | f32; gate = rows_per_batch (implies
    a residual); aux: None | bf16 | f32 (ACT_SWIGLU_BWD: always the bf16 INPUT [g | u]); conv = (mode, B, H, W, C): implicit-GEMM 3x3
    convolution, mode 1 (stride 1, padding 1) or 2 (stride 2 after padding (0, 1, 0, 1)), A the zero-bordered NHWC operand (B, H + 2, W + 2, C):
    M = B Ho Wo and K = 9 C follow from it (PC), layout nt, bf16 operands."""

    def __init__(self, M, N, K, lay="nt", ab="bf16", out="bf16", bias=False, act=ACT_NONE, gate=0, residual=False, aux=None, acc=False, split_k=1,
                 stream_k=False, dbias=False, conv=None):
        self.M, self.N, self.K, self.lay, self.ab, self.out = M, N, K, lay, ab, out
        self.conv = conv
        if conv is not None:
            mode, B, H, W, C = conv
            assert mode in (1, 2) and (mode == 1 or (H % 2 == 0 and W % 2 == 0)) and lay == "nt" and ab == "bf16"
            assert (M, K) == (B * (H // mode) * (W // mode), 9 * C), (M, K, conv)
        self.bias, self.act, self.gate, self.residual, self.aux, self.acc = bias, act, gate, residual or gate > 0, aux, acc
        self.split_k, self.stream_k, self.dbias = split_k, stream_k, dbias
        if act == ACT_SWIGLU_BWD:
            self.lay, self.aux = "dgrad", "bf16"

    @property
    def a_km(self):
        return self.lay == "wgrad"

    @property
    def b_km(self):
        return self.lay != "nt"

    @property
    def c_cols(self):
        return self.N // 2 if self.act == ACT_SWIGLU else 2 * self.N if self.act == ACT_SWIGLU_BWD else self.N

    @property
    def aux_cols(self):
        return 2 * self.N if self.act == ACT_SWIGLU_BWD else self.N

    def tag(self):
        t = f"{self.M}x{self.N}x{self.K}-{self.lay}-{self.ab}-{self.out}"
        if self.conv is not None:
            t += "-conv{}.{}x{}x{}x{}".format(*self.conv)
        for on, s in ((self.bias, "b"), (self.act == ACT_SILU, "silu"), (self.act == ACT_SWIGLU, "swiglu"), (self.act == ACT_SWIGLU_BWD, "swiglubwd"),
                      (self.gate, f"g{self.gate}"), (self.residual and not self.gate, "r"), (self.aux and self.act != ACT_SWIGLU_BWD, f"aux{self.aux}"),
                      (self.acc, "acc"), (self.split_k > 1, f"sk{self.split_k}"), (self.stream_k, "stk"), (self.dbias, "db")):
            if on:
                t += "-" + s
        return t

    def is_edge(self):
        """M one row before or past a multiple of 32, or M, N or K 8 (the granularity of k-major rows and of N and K) before or past a multiple
        of 64: every tile edge of every kernel (32-row fragments and epilogue passes, 64-wide K tiles, 128 / 160-row wave tiles, 128 / 256 /
        320-row tiles) is one.  A convolution is judged by the M, N and K that follow from its geometry."""
        m = self.M % 32 in (1, 31) or self.M % 64 in (8, 56)
        return m or self.N % 64 in (8, 56) or self.K % 64 in (8, 56)


def PC(N, mode, B, H, W, C, **kw):
    """A convolution problem: M and K from the geometry."""
    return P(B * (H // mode) * (W // mode), N, 9 * C, conv=(mode, B, H, W, C), **kw)


STATIC, CLAIMED, NO_WS = (True, False), (True, True), (False, False)      # (workspace registered, tile claiming on)


class L:
    """One launch: kernel family (the record's key), expected mmdit_gemm_plan code, problems, cu_budget, the (workspace, claiming) modes it runs
    under (outputs bit-identical across modes when `same`), the expected zero mask per mode (None: not asserted)."""

    def __init__(self, family, plan, probs, budget=0, modes=(STATIC,), masks=None, same=False):
        self.family, self.plan, self.probs, self.budget = family, plan, probs if isinstance(probs, list) else [probs], budget
        self.modes, self.masks, self.same = modes, masks, same

    @property
    def id(self):
        return f"{self.family}:{self.plan}@{self.budget}:" + "+".join(p.tag() for p in self.probs)

    def is_edge(self):
        return any(p.is_edge() for p in self.probs)


K8 = (64, 128, 192, 256, 320)          # nk = 1 .. 5 of the 8-phase loop (two-tile prologue, odd and even trailing tile)
KF = (128, 256, 384, 512, 640)         # the same for e4m3 operands (128-wide K tiles)


def _launches():
    out = []
    add = out.append
    # ---- register-staged kernel (gemm.hip: BM = BN = 128, BK = 64, 64 x 64 wave tiles, 32-row fragments): K % 64 != 0, K below / past one and two tiles
    for ab, o in (("bf16", "bf16"), ("bf16", "f32"), ("split", "f32")):
        for lay, shapes in (("nt", [(129, 136, 72), (1, 8, 8), (127, 120, 56), (128, 128, 136), (257, 264, 136), (129, 136, 8)]),
                            ("dgrad", [(129, 136, 72), (1, 8, 8), (127, 120, 56), (257, 264, 136)]),
                            ("wgrad", [(136, 136, 72), (8, 8, 8), (120, 120, 56), (128, 128, 72), (264, 264, 136)])):      # (k-major A: M % 8 == 0)
            for M, N, K in shapes:
                add(L("reg", 64, P(M, N, K, lay, ab, o)))
    add(L("reg", 64, P(129, 136, 72, out="f32", bias=True, gate=50, aux="bf16")))               # gated residual, 50 rows per sample: 3 samples, the last ragged
    add(L("reg", 64, P(129, 136, 72, bias=True, act=ACT_SILU, aux="f32")))
    add(L("reg", 64, P(264, 520, 200, "wgrad", out="f32", acc=True)))                           # accumulate with k-major operands
    add(L("reg", 64, P(264, 520, 136, "wgrad", out="f32")))
    add(L("reg", 64, [P(129, 136, 72), P(1, 8, 72)]))                                           # grouped: locate_tile with a one-tile second problem
    # ---- LDS-DMA kernel, 128 x 128 tiles: K % 64 == 0, nk = 1 .. 5
    for o in ("f32", "bf16"):
        for lay, shapes in (("nt", [(1, 8, 64), (8, 120, 128), (127, 128, 192), (128, 136, 256), (129, 264, 320), (257, 264, 64), (129, 136, 64), (257, 8, 192), (128, 128, 128)]),
                            ("dgrad", [(1, 8, 64), (8, 120, 128), (127, 128, 192), (128, 136, 256), (129, 264, 320), (257, 264, 64)]),
                            ("wgrad", [(8, 8, 64), (120, 120, 128), (128, 136, 192), (136, 264, 256), (264, 128, 320), (264, 264, 64)])):
            for M, N, K in shapes:
                add(L("dma128", 0, P(M, N, K, lay, out=o)))
    add(L("dma128", 0, P(129, 136, 128, out="f32", bias=True, gate=50, aux="bf16")))
    add(L("dma128", 0, P(129, 136, 192, bias=True, act=ACT_SILU, aux="f32")))
    add(L("dma128", 0, P(257, 264, 64, out="f32", residual=True)))
    add(L("dma128", 0, P(136, 264, 128, "wgrad", out="f32", acc=True)))
    add(L("dma128", 0, [P(129, 136, 64), P(1, 8, 64), P(257, 264, 64)]))                       # 4 + 1 + 9 = 14 tiles: xcd_chunk with a work count not divisible by 8
    add(L("dma128", 0, P(129, 1032, 64)))                                                        # tiles_n = 9: the narrower last raster group at 128-column tiles
    # ... caller split-K (atomic slices into the pre-zeroed output: zero mask 1)
    add(L("dma128 split-K", 0, P(8, 264, 256, out="f32", split_k=4), masks=(1,)))
    add(L("dma128 split-K", 0, P(264, 520, 384, "wgrad", out="f32", split_k=3), masks=(1,)))
    add(L("dma128 split-K", 0, P(8, 264, 128, out="f32", split_k=4), masks=(1,)))               # more slices (4) than K tiles (2): empty slices
    add(L("dma128 split-K", 0, P(129, 136, 192, out="f32", bias=True, residual=True, split_k=3), masks=(1,)))      # bias and residual enter exactly once
    # ... e4m3 operands, small
    for ab in ("e4m3", "mx"):
        for o in ("bf16", "f32"):
            for K in (128, 256):
                add(L("dma128 " + ab, 0, P(257, 264, K, ab=ab, out=o)))
        add(L("dma128 " + ab, 0, P(129, 136, 384, ab=ab, out="f32", bias=True)))
    # ---- LDS-DMA kernel, 256 x 256 tiles, fp32 out (budget 64: 7 x 6 = 42 tiles; one row / 8 columns past the tile edge)
    for K in K8:
        add(L("dma256", 2, P(1537, 1288, K, out="f32"), budget=64))
    add(L("dma256", 2, P(1537, 1288, 128, "dgrad", out="f32"), budget=64))
    add(L("dma256", 2, P(1537, 1288, 192, out="f32", bias=True, gate=100), budget=64))          # 100 rows per sample: sample edges inside every row tile
    add(L("dma256", 2, P(1537, 1288, 64, out="f32", aux="bf16"), budget=64))
    for M, N in ((1536, 1288), (1535, 1288), (1537, 1280), (1537, 1272)):                       # on / one before the 256-row edge; N mod 256 = 0, 248
        add(L("dma256", 2, P(M, N, 128, out="f32"), budget=64))
    # ---- 8-phase kernel, 256 x 256 tiles, bf16 out
    for M, N in ((1537, 1288), (1793, 1032)):
        for K in K8:
            add(L("8p256", 386, P(M, N, K), budget=64))
    for K in (64, 192):
        add(L("8p256", 386, P(1537, 1288, K, bias=True, act=ACT_SILU), budget=64))
    for K in K8:
        add(L("8p256", 386, P(1537, 1288, K, "dgrad"), budget=64))
    for M, N in ((1536, 1288), (1535, 1288), (1537, 1280), (1537, 1272), (1567, 1288), (1569, 1288),      # ... the 32-row epilogue pass inside the last row tile,
                 (1663, 1288), (1665, 1288), (1537, 1336), (1537, 1352)):                                  # the 128-row / 64-column wave tile inside the last tile
        add(L("8p256", 386, P(M, N, 64), budget=64))
    add(L("8p256", 386, P(5441, 512, 64), budget=64))                                          # (N = 512 leaves the 320-row kernel: 22 x 2 tiles of 256 x 256)
    for K in (128, 192):
        add(L("8p256 grouped", 386, [P(1537, 1288, K), P(257, 1288, K)], budget=64))
    add(L("8p256 grouped", 386, [P(1537, 1288, 128), P(9, 520, 192)], budget=64))               # problems of different K (nk = 2 and 3) in one grid
    # ... more tiles than the budget: 12 x 9 = 108 tiles of (2817, 2056) (108 % 8 = 4: uneven xcd_chunk ranges), tiles_n = 9 -> a narrower last raster group; static walk, then claimed
    for K in (64, 128, 192):
        add(L("8p256 claimed", 386, P(2817, 2056, K), budget=64, modes=(STATIC, CLAIMED), same=True))
    add(L("8p256 claimed", 386, P(2817, 2056, 192, bias=True, act=ACT_SILU), budget=64, modes=(STATIC, CLAIMED), same=True))
    add(L("8p256 claimed", 386, P(2817, 2056, 128, "dgrad"), budget=64, modes=(STATIC, CLAIMED), same=True))
    # ... SwiGLU (N = 2h a multiple of 256; gate / up columns paired inside a 256-column tile)
    for aux in ("bf16", None):
        for M, N, K in ((1, 256, 64), (8, 256, 64)) + tuple((257, 512, K) for K in K8):
            add(L("8p256 swiglu", 386, P(M, N, K, bias=True, act=ACT_SWIGLU, aux=aux)))
    add(L("8p256 swiglu", 386, P(257, 512, 128, act=ACT_SWIGLU, aux="bf16")))                   # no bias
    add(L("8p256 swiglu", 386, P(2817, 4096, 64, bias=True, act=ACT_SWIGLU, aux="bf16"), budget=64, modes=(STATIC, CLAIMED), same=True))
    # ... SwiGLU backward (N = h; (255, 8): one 8-column chunk, every other chunk of the wave clamped to "the last 8")
    for db in (False, True):
        for M, N, K in ((257, 264, 64), (255, 8, 192), (257, 264, 128), (257, 264, 320)):
            add(L("8p256 swiglu_bwd", 386, P(M, N, K, act=ACT_SWIGLU_BWD, dbias=db)))
        add(L("8p256 swiglu_bwd", 386, P(2817, 2056, 64, act=ACT_SWIGLU_BWD, dbias=db), budget=64, modes=(STATIC, CLAIMED), same=True))
    # ... plain weight gradient (k-major x k-major, fp32 out, whole-K tiles only)
    for K in K8:
        add(L("8p256 wgrad", 386, P(1544, 1288, K, "wgrad", out="f32"), budget=64))
    # ---- 8-phase kernel, 320 x 256 tiles (budget 64; N = 768 or 520: (5441, 776) plans as 128 x 128, which is why the plan is asserted)
    for K in K8:
        add(L("8p320", 387, P(5441, 768, K), budget=64))                                         # 17 x 320 + 1
    for M, N, K in ((6719, 768, 64), (5377, 768, 64), (5441, 520, 64), (5761, 520, 128), (5440, 768, 64), (5439, 768, 64), (5441, 760, 64),
                    (5599, 768, 64), (5601, 768, 64)):
        add(L("8p320", 387, P(M, N, K), budget=64))                                              # 21 x 320 - 1; 16 x 320 + 257; N mod 256 = 8, 248 (N = 512 plans as 386: listed there); the 160-row wave tile
    add(L("8p320", 387, P(5441, 768, 128, "dgrad"), budget=64))
    add(L("8p320", 387, P(5441, 768, 192, bias=True, act=ACT_SILU), budget=64))
    # ---- weight gradient, round + tail schedule (stream_k): 72, 136, 200 are K tails (the k-rows beyond K are zero-filled on their way into LDS)
    for K in (64, 72, 136, 200):
        add(L("wgrad tail", 418, P(264, 520, K, "wgrad", out="f32", stream_k=True), masks=(0,)))
    add(L("wgrad tail", 418, [P(264, 520, 200, "wgrad", out="f32", stream_k=True), P(8, 8, 64, "wgrad", out="f32", stream_k=True),
                              P(256, 256, 136, "wgrad", out="f32", stream_k=True)], masks=(0,)))
    # ... a split tail that really adds: 81 / 90 tiles on 64 workgroups; fp32 atomics without the workspace (mask 1), per-slice slots with it (mask 0)
    for M, N, K in ((2056, 2056, 320), (2056, 2056, 328), (2056, 2312, 328)):
        add(L("wgrad split tail", 418, P(M, N, K, "wgrad", out="f32", stream_k=True), budget=64, modes=(NO_WS, STATIC), masks=(1, 0)))
    add(L("wgrad split tail", 418, [P(2048, 2048, 512, "wgrad", out="f32", stream_k=True), P(2048, 512, 192, "wgrad", out="f32", stream_k=True)],
          budget=64, modes=(NO_WS, STATIC), masks=(0, 0)))                                      # mixed K: 64 + 16 tiles, the balanced tail
    add(L("wgrad split tail", 418, [P(1792, 2048, 512, "wgrad", out="f32", stream_k=True), P(2048, 520, 200, "wgrad", out="f32", stream_k=True)],
          budget=64, modes=(NO_WS, STATIC)))
    for K in (320, 328):      # into an existing gradient: whole-K tiles, no decomposition ((2056, 2056) would plan as 128 x 128 at this budget: 64 tiles keep 256 x 256)
        add(L("wgrad accumulate", 386, P(2040, 2048, K, "wgrad", out="f32", acc=True, stream_k=True), budget=64))
    # ---- 8-phase e4m3 kernel (256 x 256 tiles, bf16 out)
    for ab in ("e4m3", "mx"):
        for K in KF:
            add(L("8p " + ab, 258, P(1537, 1288, K, ab=ab, bias=K in (256, 384)), budget=64))
        add(L("8p " + ab, 258, P(2817, 2056, 128, ab=ab), budget=64))
        add(L("8p " + ab, 258, P(2817, 2056, 256, ab=ab, bias=True), budget=64))
        for M, N in ((1536, 1288), (1535, 1288), (1537, 1280), (1537, 1272)):
            add(L("8p " + ab, 258, P(M, N, 128, ab=ab), budget=64))
    for K in (128, 256):
        add(L("8p mx swiglu", 258, P(257, 512, K, ab="mx", bias=True, act=ACT_SWIGLU)))
    # ---- implicit-GEMM 3x3 convolution (conv = (mode, B, H, W, C); K = 9 C: 9 / 18 / 27 K tiles, cseg_len = 3 / 6 / 9 K tiles per kernel row)
    # ... LDS-DMA kernel, 128 x 128 tiles: one pixel, one row, one column of pixels per image, image boundaries inside the 16-row pieces
    for N, kw in ((8, dict()), (40, dict(out="f32", bias=True))):
        for mode, B, H, W in ((1, 1, 1, 1), (1, 3, 5, 17), (1, 1, 1, 127), (1, 3, 1, 43), (1, 2, 8, 8), (2, 2, 2, 2), (2, 3, 10, 34)):
            add(L("conv dma128", 0, PC(N, mode, B, H, W, 64, **kw)))
    # ... LDS-DMA kernel, 256 x 256 tiles (budget 64): the epilogues conv8 (gemm.hip) refuses -- SiLU, bf16 output + residual, aux.  (A caller
    # split_k > 1 is refused for every convolution by plan_gemm -- test_gemm_edges_cpu.py pins that -- so the DMA cursor never starts inside a kernel row.)
    add(L("conv dma256", 2, PC(1288, 1, 1, 29, 53, 64, bias=True, act=ACT_SILU), budget=64))                  # M = 1537; W % 8 != 0: a 16-row piece wraps image rows
    add(L("conv dma256", 2, PC(1288, 1, 2, 24, 32, 128, bias=True, residual=True), budget=64))                # M = 1536: the image boundary on a tile boundary
    add(L("conv dma256", 2, PC(1288, 1, 5, 1, 307, 64, out="f32", aux="bf16"), budget=64))                    # M = 1535; H = 1: every kh = 0 / 2 tap is border
    add(L("conv dma256", 2, PC(1288, 2, 1, 58, 106, 192, residual=True), budget=64))                          # mode 2, M = 1537
    add(L("conv dma256", 2, PC(1288, 2, 2, 48, 64, 64, out="f32", act=ACT_SILU), budget=64))                  # mode 2, M = 1536
    add(L("conv dma256", 2, PC(1272, 1, 1, 29, 53, 128, out="f32", bias=True, aux="f32"), budget=64))
    add(L("conv dma256", 2, PC(1280, 2, 1, 58, 106, 64, bias=True, act=ACT_SILU), budget=64))                 # (N = 1280 / 1272 need M >= 1537: 12 x 10 tiles of 128 x 128 are one round and plan as 0)
    add(L("conv dma256", 2, [PC(1288, 1, 1, 29, 53, 64, act=ACT_SILU), PC(1288, 1, 1, 1, 257, 128, act=ACT_SILU)], budget=64))      # grouped: C and W differ
    # ... 8-phase kernel, CONV instantiation (budget 64): bf16 + bias, fp32 + bias, fp32 + bias + residual
    e_bf, e_f, e_fr = dict(bias=True), dict(out="f32", bias=True), dict(out="f32", bias=True, residual=True)
    for mode, B, H, W, C, N, kw in ((1, 1, 29, 53, 64, 1288, e_bf), (1, 1, 29, 53, 128, 1280, e_f), (1, 1, 29, 53, 192, 1272, e_fr),      # M = 1537
                                    (2, 1, 58, 106, 128, 1272, e_bf), (2, 1, 58, 106, 192, 1288, e_f), (2, 1, 58, 106, 64, 1280, e_fr),
                                    (1, 2, 24, 32, 64, 1288, e_f), (2, 2, 48, 64, 64, 1288, e_fr), (1, 2, 24, 32, 192, 1288, e_bf),       # M = 1536
                                    (1, 5, 1, 307, 64, 1288, e_bf), (2, 5, 2, 614, 128, 1288, e_f), (1, 5, 1, 307, 128, 1288, e_fr),      # M = 1535; H = 1
                                    (1, 1, 1, 1567, 64, 1288, e_bf), (1, 3, 1, 523, 64, 1288, e_f),                                       # M = 1567 / 1569: the 32-row epilogue pass
                                    (1, 1, 1, 1663, 64, 1288, e_fr), (2, 5, 18, 74, 64, 1288, e_bf),                                      # M = 1663 / 1665: the 128-row wave tile
                                    (1, 3, 3, 313, 64, 2056, e_bf), (1, 3, 3, 313, 128, 2056, e_fr), (2, 3, 6, 626, 192, 2056, e_f)):     # M = 2817: 108 tiles on 64 workgroups
        add(L("conv 8p", 258, PC(N, mode, B, H, W, C, **kw), budget=64))
    add(L("conv 8p", 258, [PC(1288, 1, 1, 29, 53, 64, bias=True), PC(1288, 1, 1, 1, 257, 128, bias=True)], budget=64))              # grouped: C and W differ in one grid
    add(L("conv 8p", 258, [PC(1288, 2, 1, 58, 106, 128, **e_fr), PC(520, 1, 3, 5, 17, 64, **e_fr)], budget=64))
    return out


CONV_FAMILIES = ("conv dma128", "conv dma256", "conv 8p")
LAUNCHES = _launches()
CASES = [(l, "random") for l in LAUNCHES] + [(l, f) for f in ("integer", "poison") for l in LAUNCHES if l.is_edge()]


def _case_id(case):
    return f"{case[0].id}-{case[1]}"


# ---------------------------------------------------------------------------------------------- planner arguments without a GPU
_F32, _BF16, _FP8 = 0, 1, 2


def fake_args(GemmArgs, launch):
    """The launch's mmdit_gemm_args on fake, aligned, far-apart device pointers (the planner never dereferences them), leading dimensions = extents."""
    nxt = [1 << 32]

    def ptr():
        nxt[0] += 1 << 28
        return nxt[0]
    arr = (GemmArgs * len(launch.probs))()
    for a, p in zip(arr, launch.probs):
        dt = {"bf16": _BF16, "split": _F32, "e4m3": _FP8, "mx": _FP8}[p.ab]
        a.A, a.a_dtype, a.a_kmajor, a.lda = ptr(), dt, int(p.a_km), p.M if p.a_km else p.K
        a.B, a.b_dtype, a.b_kmajor, a.ldb = ptr(), dt, int(p.b_km), p.N if p.b_km else p.K
        a.C, a.c_dtype, a.ldc = ptr(), _BF16 if p.out == "bf16" else _F32, p.c_cols
        a.M, a.N, a.K, a.act, a.accumulate, a.precision, a.split_k, a.stream_k = p.M, p.N, p.K, p.act, int(p.acc), int(p.ab == "split"), p.split_k, int(p.stream_k)
        if p.bias:
            a.bias = ptr()
        if p.gate:
            a.gate, a.ld_gate, a.rows_per_batch = ptr(), p.N, p.gate
        if p.residual:
            a.residual, a.ld_res = ptr(), p.N
        if p.aux:
            a.aux, a.aux_dtype, a.ld_aux = ptr(), _BF16 if p.aux == "bf16" else _F32, p.aux_cols
        if dt == _FP8:
            a.scale_a, a.scale_b, a.scale_mode = ptr(), ptr(), int(p.ab == "mx")
        if p.dbias:
            a.dbias = ptr()
        if p.conv is not None:      # (lda is ignored by the kernels and set to K, as ops._fill_gemm does)
            a.conv_mode, a.conv_H, a.conv_W, a.conv_C = p.conv[0], p.conv[2], p.conv[3], p.conv[4]
        a.cu_budget = launch.budget
    return arr


# ---------------------------------------------------------------------------------------------- MX scale layout (restated from mmdit_hip.h:111-117)
def mx_pack(rows_u8, pad_byte, spare_byte):
    """(rows, K / 32) scale bytes -> the GEMM's layout: per 64-wide K half the rows in groups of 128 (padded), inside a group the byte of (row,
    half-block h) at (row & 31) * 8 + h * 4 + ((row >> 5) & 3); 512 spare bytes behind."""
    rows, nb = rows_u8.shape
    rp = (rows + 127) // 128 * 128
    full = torch.full((rp, nb), pad_byte, dtype=torch.uint8, device=rows_u8.device)
    full[:rows] = rows_u8
    v = full.view(rp // 128, 4, 32, nb // 2, 2).permute(3, 0, 2, 4, 1).contiguous().view(-1)      # [group][rb][r31][k64][h] -> [k64][group][r31][h][rb]
    return torch.cat([v, torch.full((512,), spare_byte, dtype=torch.uint8, device=v.device)])


def mx_unpack(sc, rows, K):
    rp = (rows + 127) // 128 * 128
    return sc[:(K // 64) * rp * 2].view(K // 64, rp // 128, 32, 2, 4).permute(1, 4, 2, 0, 3).reshape(rp, K // 32)[:rows]


def mx_dequant(q, rows_u8):
    rows, K = q.shape
    return (q.float().double().view(rows, K // 32, 32) * torch.exp2(rows_u8.double() - 127.0).unsqueeze(-1)).view(rows, K)


# ---------------------------------------------------------------------------------------------- operands
def _place(x, poison):
    """x (storage-shaped, 2-D) as the kernel receives it: contiguous, or (poison) a view into a larger NaN-filled tensor with a wider leading
    dimension and GUARD spare rows behind the last row."""
    if not poison:
        return x.contiguous()
    r, c = x.shape
    if x.element_size() == 1:
        big = torch.full((r + GUARD, c + 16), 0x7F, dtype=torch.uint8, device=x.device)
        big[:r, :c] = x.view(torch.uint8)
        return big.view(torch.float8_e4m3fn)[:r, :c]
    big = torch.full((r + GUARD, c + 8), float("nan"), dtype=x.dtype, device=x.device)
    big[:r, :c] = x
    return big[:r, :c]


class Out:
    """An output the kernel writes: the [M, N] window of a tensor the test owns -- contiguous, or (guarded) with ld = N + 8 and GUARD rows before and
    behind.  Every byte starts as a NaN bit pattern; touched() lists the bytes outside the window that differ from the snapshot."""
    PATTERN = {torch.float32: (torch.int32, 0x7FC0A5A5), torch.bfloat16: (torch.int16, 0x7FA5)}

    def __init__(self, M, N, dtype, guarded, device):
        self.M, self.N, self.r0 = M, N, GUARD if guarded else 0
        self.big = torch.empty((M + 2 * self.r0, N + (8 if guarded else 0)), dtype=dtype, device=device)
        it, pat = self.PATTERN[dtype]
        self.big.view(it).fill_(pat)
        self.win = self.big[self.r0:self.r0 + M, :N]
        self.snap = None

    def snapshot(self):
        self.snap = self.big.clone()

    def touched(self):
        d = self.big.view(torch.uint8) != self.snap.view(torch.uint8)
        d[self.r0:self.r0 + self.M, :self.N * self.big.element_size()] = False
        return [tuple(i) for i in d.nonzero()[:8].tolist()], int(d.sum())


def conv_gather(xp, mode):
    """The implicit GEMM's A (M, 9 C) from the zero-bordered operand xp (B, H + 2, W + 2, C), by index: output row (b, yo, xo), column
    (kh 3 + kw) C + c = padded pixel (s yo + kh + o, s xo + kw + o) with s = 1, o = 0 (mode 1) or s = 2, o = 1 (mode 2)."""
    B, Hp, Wp, C = xp.shape
    s, o = (1, 0) if mode == 1 else (2, 1)
    Ho, Wo = (Hp - 2) // s, (Wp - 2) // s
    yo, xo = torch.arange(Ho, device=xp.device), torch.arange(Wo, device=xp.device)
    taps = []
    for kh in range(3):
        for kw in range(3):
            yi, xi = s * yo + kh + o, s * xo + kw + o
            taps.append(xp[:, yi[:, None], xi[None, :], :])              # (B, Ho, Wo, C)
    return torch.stack(taps, 3).reshape(B * Ho * Wo, 9 * C)


def conv_operand(p, x, poison):
    """x (B, H, W, C) bf16 -> the zero-bordered operand (B, H + 2, W + 2, C) the kernel receives: dense, border exactly zero in every family;
    poison: a view into a larger NaN tensor with GUARD spare NaN pixel rows behind (the clamped re-read min(m, M - 1) stays inside the operand)."""
    mode, B, H, W, C = p.conv
    n = B * (H + 2) * (W + 2) * C
    big = torch.full((n + (GUARD * C if poison else 0),), float("nan") if poison else 0.0, dtype=torch.bfloat16, device=x.device)
    xp = big[:n].view(B, H + 2, W + 2, C)
    xp.zero_()
    xp[:, 1:-1, 1:-1] = x
    border = xp.clone()
    border[:, 1:-1, 1:-1] = 0
    assert int((border.view(torch.int16) != 0).sum()) == 0 and (not poison or bool(torch.isnan(big[n:].float()).all()))
    return xp


def _seed(p, idx):
    return 1000003 * p.M + 1009 * p.N + 17 * p.K + 7 * idx + 1


def build(p, family, idx, device, ops=None):
    """Operands, epilogue inputs and float64 views of one problem.  Returns a dict: kw (keyword arguments of ops._fill_gemm without the outputs),
    A64 (M, K), B64 (N, K), bias / gate_rows / res / cin / gu in float64 (or None), unit (integer family: the spacing of every partial sum)."""
    integer, poison = family == "integer", family == "poison"
    g = torch.Generator().manual_seed(_seed(p, idx))
    rn = lambda *s: torch.randn(*s, generator=g)                                      # noqa: E731
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()         # noqa: E731
    val = (lambda *s: ri(-3, 3, *s)) if integer else rn
    A, B = (val(*p.conv[1:]) if p.conv is not None else val(p.M, p.K)), val(p.N, p.K)
    t = dict(unit=1.0)
    kw = {}
    if p.conv is not None:
        A, B = conv_operand(p, A.to(torch.bfloat16).to(device), poison), B.to(torch.bfloat16).to(device)
        t["A64"], t["B64"] = conv_gather(A.double(), p.conv[0]), B.double()
        assert tuple(t["A64"].shape) == (p.M, p.K)
        kw["conv"] = (p.conv[0],) + tuple(p.conv[2:])
    elif p.ab in ("bf16", "split"):
        dt = torch.bfloat16 if p.ab == "bf16" else torch.float32
        A, B = A.to(dt).to(device), B.to(dt).to(device)
        t["A64"], t["B64"] = A.double(), B.double()
        if p.ab == "split":
            kw["precision"] = 1
    elif p.ab == "e4m3":
        if integer:
            qa, qb = A.to(torch.float8_e4m3fn).to(device), B.to(torch.float8_e4m3fn).to(device)
            sa, sb = torch.tensor([0.5], device=device), torch.tensor([4.0], device=device)
        else:
            (qa, sa), (qb, sb) = ops.quant_fp8(A.to(torch.bfloat16).to(device)), ops.quant_fp8(B.to(torch.bfloat16).to(device))
        t["A64"], t["B64"] = qa.float().double() * sa.double(), qb.float().double() * sb.double()
        A, B = qa, qb
        kw.update(scale_a=sa, scale_b=sb, scale_mode=0)
    else:
        sc, q = [], []
        for name, x, rows in (("A64", A, p.M), ("B64", B, p.N)):
            nb = p.K // 32
            if integer:
                qx = x.to(torch.float8_e4m3fn).to(device)
                by = (127 + ri(-2, 2, rows, nb)).to(torch.uint8).to(device)
                packed = mx_pack(by, 127, 127)
            else:
                e = ri(-8, 8, rows, nb, 1)
                x = (x.view(rows, nb, 32) * torch.exp2(e)).view(rows, p.K)
                x[0, :32] = 0.0                                                         # one all-zero block: amax = 0 -> scale 2^-127, codes 0
                qx, packed = ops.quant_mxfp8(x.to(torch.bfloat16).to(device))
                by = mx_unpack(packed, rows, p.K).clone()
                if poison:
                    packed = mx_pack(by, 0xFF, 0xFF)
                assert int(by[0, 0]) == 0 and int((qx[0, :32].view(torch.uint8) & 0x7F).max()) == 0, "the all-zero block did not survive the quantiser"
            q.append(qx)
            sc.append(packed)
            t[name] = mx_dequant(qx, by)
        A, B = q
        kw.update(scale_a=sc[0], scale_b=sc[1], scale_mode=1)
        t["unit"] = 2.0 ** -4
    if p.ab == "e4m3":
        t["unit"] = 1.0          # (scales 0.5 * 4: every product an even integer)
    kw["A"] = A if p.conv is not None else _place(A.t() if p.a_km else A, poison)
    kw["B"] = _place(B.t() if p.b_km else B, poison)
    kw.update(a_kmajor=p.a_km, b_kmajor=p.b_km, act=p.act, split_k=p.split_k, stream_k=p.stream_k, accumulate=p.acc)
    t["bias"] = t["gate_rows"] = t["res"] = t["cin"] = t["gu"] = None
    if p.bias:
        kw["bias"] = val(p.N).to(device)
        t["bias"] = kw["bias"].double()
    if p.gate:
        nb = (p.M + p.gate - 1) // p.gate
        gate = (torch.exp2(ri(-2, 2, nb, p.N)) * (2 * ri(0, 1, nb, p.N) - 1) if integer else rn(nb, p.N)).to(device)
        kw.update(gate=gate, rows_per_batch=p.gate)
        t["gate_rows"] = gate.double().repeat_interleave(p.gate, 0)[:p.M]
    if p.residual:
        kw["residual"] = val(p.M, p.N).to(device)
        t["res"] = kw["residual"].double()
    if p.acc:
        t["cin32"] = val(p.M, p.N).to(device)
        t["cin"] = t["cin32"].double()
    if p.act == ACT_SWIGLU_BWD:
        gu = _place(val(p.M, 2 * p.N).to(torch.bfloat16).to(device), poison)
        kw["aux"] = gu
        t["gu"] = gu.double()
    t["kw"] = kw
    if integer:
        absP = t["A64"].abs() @ t["B64"].abs().T
        assert float(absP.max()) / t["unit"] < 2.0 ** 24, f"integer family: max |A||B|^T = {float(absP.max())} units of {t['unit']}"
    return t


# ---------------------------------------------------------------------------------------------- float64 reference + yardstick
def reference(p, t):
    """name -> (ref, y_det, y_rnd) in float64 for the outputs 'out', 'aux' (when written) and 'dbias'."""
    A, B = t["A64"], t["B64"]
    prod, absP = A @ B.T, A.abs() @ B.abs().T
    S = p.split_k if p.split_k > 1 else (p.K + 63) // 64 if p.stream_k else 0
    c = (p.K + S + 8) * E23
    zero = torch.zeros_like(prod)
    rnd = lambda ref, dt: U * ref.abs() if dt == "bf16" else torch.zeros_like(ref)      # noqa: E731
    res = {}
    if p.act == ACT_SWIGLU_BWD:
        h = p.N
        gv, uv = t["gu"][:, :h], t["gu"][:, h:]
        s = torch.sigmoid(gv)
        f = torch.cat([uv * s * (1 + gv * (1 - s)), gv * s], 1)
        dh, ydh = torch.cat([prod, prod], 1), torch.cat([c * absP, c * absP], 1)
        ref = dh * f
        feval = 8 * E23 * torch.cat([(1 + gv.abs()) * (prod * uv).abs(), (1 + gv.abs()) * prod.abs()], 1)
        det, carried = f.abs() * ydh + feval, f.abs() * U * dh.abs()
        res["out"] = (ref, det, carried + U * ref.abs())
        if p.dbias:
            res["dbias"] = (ref.sum(0), (det + carried).sum(0) + p.M * E23 * ref.abs().sum(0), torch.zeros_like(ref[0]))
        return res
    pre, ypre = prod, (max(c, 2 * MX_KAPPA) if p.ab == "mx" else c) * absP
    if p.ab == "split":
        ypre = ypre + 2.0 ** -22 * absP
    if t["bias"] is not None:
        pre, ypre = pre + t["bias"], ypre + c * t["bias"].abs()
    if p.aux:
        res["aux"] = (pre, ypre, rnd(pre, p.aux))
    if p.act == ACT_SILU:
        ref = pre * torch.sigmoid(pre)
        res["out"] = (ref, 1.1 * ypre, rnd(ref, p.out))
        return res
    if p.act == ACT_SWIGLU:
        h = p.N // 2
        gv, uv, yg, yu = pre[:, :h], pre[:, h:], ypre[:, :h], ypre[:, h:]
        sg = gv * torch.sigmoid(gv)
        ref = sg * uv
        res["out"] = (ref, 1.1 * uv.abs() * yg + sg.abs() * yu, U * ref.abs() + 1.1 * uv.abs() * U * gv.abs() + sg.abs() * U * uv.abs())
        return res
    ref, det = pre, ypre
    if t["gate_rows"] is not None:
        ref, det = t["gate_rows"] * ref, t["gate_rows"].abs() * det
    if t["res"] is not None:
        ref, det = ref + t["res"], det + c * t["res"].abs()
    if t["cin"] is not None:
        ref, det = ref + t["cin"], det + c * t["cin"].abs()
    res["out"] = (ref, det + zero, rnd(ref, p.out))
    return res


TINY = 1e-300


def ratios(out, ref, det, rnd):
    """Worst ratio to the yardstick y = det + rnd per element, per row and per column (2-D outputs; a vector is one row), the rounding-bias
    statistic (None where it does not apply), and where each worst sits.  y = 0 demands out == ref."""
    if ref.dim() == 1:
        out, ref, det, rnd = out[None], ref[None], det[None], rnd[None]
    diff = out.double() - ref
    y = det + rnd
    el = diff.abs() / y.clamp_min(TINY)
    row = diff.norm(dim=1) / y.norm(dim=1).clamp_min(TINY)
    col = diff.norm(dim=0) / y.norm(dim=0).clamp_min(TINY)
    bias = None
    if out.dtype == torch.bfloat16 and out.numel() >= 64:
        bias = float((torch.sign(ref) * diff).sum().abs() / (BIAS_SIGMAS * rnd.norm() + det.sum()).clamp_min(TINY))
    return dict(el=float(el.max()), row=float(row.max()), col=float(col.max()), bias=bias,
                at=(int(el.argmax()) // ref.shape[1], int(el.argmax()) % ref.shape[1], int(row.argmax()), int(col.argmax())))


def verdict(r):
    """The failed bars of one ratios() result (empty: pass)."""
    bad = [k for k, bar in (("el", ELEM_BAR), ("row", ROW_BAR), ("col", ROW_BAR)) if not r[k] <= bar]
    if r["bias"] is not None and not r["bias"] <= 1.0:
        bad.append("bias")
    return bad


def exact_mismatches(out, ref):
    """Integer family: elements that differ from the float64 reference although the reference is a number of the output's format."""
    representable = ref.to(out.dtype).double() == ref
    return int(((out.double() != ref) & representable).sum()), int(representable.sum())


WORST = {}             # (kernel family, input family) -> [per-element, per-row, per-column, rounding bias] as (ratio, case id)


def _record(launch, family, r, what):
    w = WORST.setdefault((launch.family, family), [(-1.0, "")] * 4)
    for i, k in enumerate(("el", "row", "col", "bias")):
        if r[k] is not None and r[k] > w[i][0]:
            w[i] = (r[k], f"{launch.id} {what}")


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\n[gemm edge sweep] worst ratio to the yardstick per kernel family and input family (bars: per element 2.0, per row / column 1.0, rounding bias 1.0)")
    for (kf, fam), w in sorted(WORST.items()):
        print(f"  {kf:<20} {fam:<8} " + "  ".join(f"{n} {v:.3f} @ {cid}" for n, (v, cid) in zip(("elem", "row", "col", "bias"), w) if v >= 0))


@pytest.fixture(scope="module")
def workspace(ops):
    return torch.zeros(WS_BYTES, dtype=torch.uint8, device="cuda")


# ---------------------------------------------------------------------------------------------- the sweep
def _run_mode(ops, launch, family, mode, mode_i, built, refs, workspace):
    lib = ops._lib.lib()
    use_ws, claiming = mode
    n = len(launch.probs)
    guarded = family == "poison"
    arr = (ops.GemmArgs * n)()
    outs = []
    assert lib.mmdit_gemm_set_workspace(workspace.data_ptr() if use_ws else None, workspace.numel() if use_ws else 0) == 0
    assert lib.mmdit_gemm_set_claiming(int(claiming)) == 0
    for i, (p, t) in enumerate(zip(launch.probs, built)):
        o = dict(out=Out(p.M, p.c_cols, torch.bfloat16 if p.out == "bf16" else torch.float32, guarded, "cuda"))
        kw = dict(t["kw"], out=o["out"].win, cu_budget=launch.budget)
        if p.aux and p.act != ACT_SWIGLU_BWD:
            o["aux"] = Out(p.M, p.aux_cols, torch.bfloat16 if p.aux == "bf16" else torch.float32, guarded, "cuda")
            kw["aux"] = o["aux"].win
        if p.dbias:
            o["dbias"] = torch.zeros(2 * p.N, device="cuda")
            kw["dbias"] = o["dbias"]
        ops._fill_gemm(arr[i], **kw)
        outs.append(o)
    plan = lib.mmdit_gemm_plan(arr, n)
    assert plan == launch.plan, f"{launch.id}: planned as {plan}, the sweep expects {launch.plan} (mode {mode})"
    mask = ctypes.c_uint(0)
    assert lib.mmdit_gemm_zero_mask(arr, n, ctypes.byref(mask)) == 0
    if launch.masks is not None:
        assert mask.value == launch.masks[mode_i], f"{launch.id}: zero mask {mask.value}, expected {launch.masks[mode_i]} (mode {mode})"
    for i, (p, t, o) in enumerate(zip(launch.probs, built, outs)):
        if p.acc:
            o["out"].win.copy_(t["cin32"])
        elif (mask.value >> i) & 1:
            o["out"].win.zero_()          # (every other output keeps its NaN pattern: an element the launch does not write fails the finite check)
        for k in ("out", "aux"):
            if k in o:
                o[k].snapshot()
    torch.cuda.synchronize()
    rc = lib.mmdit_gemm_grouped(arr, n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, (launch.id, rc)
    failures = []
    for i, (p, ref, o) in enumerate(zip(launch.probs, refs, outs)):
        for name, (rf, det, rnd) in ref.items():
            got = o[name] if name == "dbias" else o[name].win
            what = f"p{i}.{name}" + ("" if mode == STATIC else f" ws={int(use_ws)} claim={int(claiming)}")
            if name != "dbias":
                where, count = o[name].touched()
                if count:
                    failures.append(f"{what}: {count} bytes outside the [M, N] window changed, first (row, byte) {where}")
            if not bool(torch.isfinite(got).all()):
                failures.append(f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements")
                continue
            r = ratios(got, rf, det, rnd)
            _record(launch, family, r, what)
            print(f"[gemm edges] {launch.id} {family} {what}: elem {r['el']:.3f} @ ({r['at'][0]}, {r['at'][1]}) row {r['row']:.3f} @ {r['at'][2]} "
                  f"col {r['col']:.3f} @ {r['at'][3]}" + (f" bias {r['bias']:.3f}" if r["bias"] is not None else ""))
            bad = verdict(r)
            if bad:
                failures.append(f"{what}: {bad} over the bar: {r}")
            if family == "integer" and (p.act == ACT_NONE or name == "aux"):
                wrong, of = exact_mismatches(got, rf)
                if wrong:
                    failures.append(f"{what}: {wrong} of {of} exactly representable elements differ from the float64 reference")
    assert not failures, "\n".join([launch.id + " " + family] + failures)
    return [{k: (v if k == "dbias" else v.win).clone() for k, v in o.items()} for o in outs]


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_gemm_edge(ops, workspace, case):
    """One launch of the sweep under one input family: plan code (and zero mask) asserted, every output finite, within the three bars and the
    rounding-bias bar against float64, exact for the integer family, sentinels bit-identical for the poison family; bit-identical across the
    static and the claimed tile walk where the launch runs under both."""
    launch, family = case
    lib = ops._lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    prev = ops._GEMM_WS.get(dev)
    built = [build(p, family, i, "cuda", ops) for i, p in enumerate(launch.probs)]
    refs = [reference(p, t) for p, t in zip(launch.probs, built)]
    try:
        runs = [_run_mode(ops, launch, family, mode, i, built, refs, workspace) for i, mode in enumerate(launch.modes)]
    finally:
        torch.cuda.synchronize()
        assert lib.mmdit_gemm_set_claiming(0) == 0
        assert lib.mmdit_gemm_set_workspace(prev.data_ptr() if prev is not None else None, prev.numel() if prev is not None else 0) == 0
    if launch.same:
        for a, b in zip(runs[0], runs[1]):
            for k in a:
                if k != "dbias":          # (fp32 atomics: equal to rounding, held to float64 above)
                    assert torch.equal(a[k], b[k]), f"{launch.id}: {k} differs between {launch.modes[0]} and {launch.modes[1]}"
    assert int(workspace[:8192].view(torch.int32).abs().sum()) == 0, "tickets / queue heads are left zero by every launch"
