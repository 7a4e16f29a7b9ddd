"""Edge sweep of the FLUX-VAE kernels (csrc/vae.hip) with PER-ELEMENT, PER-ROW and PER-COLUMN float64 parity through the C ABI.

tests/test_vae.py holds these kernels to whole-tensor rel-L2 bars (1e-5 .. 5e-3) at one shape each, and the encode / decode tests to 3e-2 through 26
convolutions.  A GroupNorm whose straddling channel takes its neighbour's statistics, a statistics chunk that loses its last row, eps = 1e-5, a
softmax that forgets its last column, an im2col tap off by one pixel on the upsampling path or a producer that writes one border pixel of a recycled
conv operand all pass there.  This file runs the seven kernels

  mmdit_vae_nchw_to_nhwc      fp32 / bf16 source, channel padding 3 -> 8 / 64, 9 -> 16, none; scale / shift off and on
  mmdit_vae_nhwc_to_nchw      row pitch ld = C and C + 5, clamp inactive and active (values on both sides of and exactly on the bounds)
  mmdit_vae_im2col3x3         modes 0 / 1 / 2, H, W in {1, 2, 3, 5, 6}
  mmdit_vae_pad_cast          fp32 / bf16 input, nearest x2 upsampling off / on, sentinel border
  mmdit_vae_groupnorm         the (C, G) table below x HW around the 128-row statistics chunk and the 128-pixel apply chunk, fp32 / bf16 input,
                              SiLU, padded output with a sentinel border, the rows_per_block doubling
  mmdit_vae_softmax_rows      rows % 4 = 0 .. 3 (idle waves), cols around the 64 lanes, ld = cols rounded up to 8 and cols + 8, a saturating family

at the smallest shapes that reach each path, and each grid-stride kernel once past its 65535-block cap.  The library has no query for the shape of
these launches, so the launch arithmetic is RESTATED below (grid_cap, gn_rpb, PPB, gn_nty) and every case carries the paths it reaches (paths());
tests/test_vae_edges_cpu.py asserts on that restatement that every path is present.  The restated C++ lines in vae.hip carry a comment that points here.

Reference: plain float64 torch of the operands exactly as the kernel receives them (bf16 values widened, fp32 as is), no ops.* call inside.  For the
pure gather / copy kernels (nhwc_to_nchw, im2col, pad_cast, and nchw_to_nhwc from bf16 with scale 1, shift 0) the output must be BIT-IDENTICAL to a
torch index gather (yardstick 0: ratios() then demands out == ref; the past-the-cap cases compare bit patterns on the device).

Yardstick (derived from the kernels as written, not tuned).  u = 2^-24, U = 2^-8 (bf16 round to nearest), |.| elementwise.

  nchw_to_nhwc   (x + shift) * scale in fp32:  y_det = 2 u (|x| + |shift|) |scale|,  y_rnd = U |ref|;  padded channels: ref = 0, y = 0
  groupnorm      the kernel computes a ONE-PASS variance from fp32 sums.  n = HW cpg elements per group, m = mean x, q = mean x^2, v = q - m^2,
                 r = (v + eps)^-1/2 and  S = serial adds per lane (ceil(min(rpb, HW) / nty))  +  (thread, channel) pairs added into one LDS slot
                 (nty cpg)  +  workgroups added into one global slot (ceil(HW / rpb))  +  2:
                   dm = S u mean|x|      dq = S u q      dv = dq + 2 |m| dm + 2 u (q + m^2)      dr = r (0.5 dv / (v + eps) + 2 u)
                 apply is fma(x, sc, of) with sc = r gamma, of = beta - m sc; the same rounded sc multiplies x and m, so its error enters as |x - m|:
                   y_det = |x - m| (|gamma| dr + u |sc|) + |sc| dm + u (|x sc| + |m sc| + |of|) + u |ref|
                 SiLU (o the pre-activation): y_det = 1.1 y_det + 8 * 2^-23 (1 + |o|) |ref|  (the row-kernel sweep's sigmoid term);  y_rnd = U |ref|
  softmax_rows   t = scale x - max, p = exp(t) / sum:  y_det = p (8 * 2^-23 (1 + |t|) + (ceil(cols / 64) + 8) u) + 2^-126,  y_rnd = U p;
                 padding columns: ref = 0, y = 0.  The 2^-126 is not in the issue's form and is derived, not fitted: __expf flushes results below
                 the smallest normal fp32 to zero, which the relative terms cannot cover (the saturating family has t down to -160, p ~ 1e-70 in
                 float64 against 0 from the kernel); it is the FLUSH term of the row-kernel sweep and is far below every bf16 value the other
                 families produce.

and every output of every case must satisfy, for every element, every row and every column, with nothing exempt (test_gemm_edges_gpu.ratios / verdict),

  |out - ref| <= 2.0 y          ||out_row - ref_row||_2 <= 1.0 ||y_row||_2          ||out_col - ref_col||_2 <= 1.0 ||y_col||_2
  bf16 outputs of >= 64 elements:  |sum_j sign(ref_j) (out_j - ref_j)| <= 6 ||y_rnd||_2 + ||y_det||_1

Every output sits between GUARD sentinel rows (and, for the padded outputs of pad_cast / groupnorm, inside a sentinel BORDER: vae.py recycles those
buffers and relies on producers writing the interior only) whose bit pattern must come back identical; every input has NaN rows behind it.

Input families (seeded; each asserts its own precondition):
  random      GroupNorm x = 0.5 + 2 N(0, 1); N(0, 1) elsewhere.  Every case.
  offset      (groupnorm) x = 16 + N(0, 1).  Also recorded: the worst ||out_row - ref_row|| / (U ||ref_row||) and the worst |out - ref| / (U |ref|) over the
              elements with |ref| >= the row's rms -- how far the one-pass variance is from a pure bf16-rounding result.
  smallvar    (groupnorm) x = 0.03 + 8e-4 N(0, 1) clipped to 3 sigma, a group's spread scaled back to 9e-4 where it drew more: group standard deviation <= 1e-3, so eps = 1e-6 carries about half of rstd; group 0
              of every image is constant 2.0: its output must be beta to within y.  eps = 1e-5 fails here (test_vae_edges_cpu.py).
  poison      (groupnorm) the random data; named because the issue names it: the NaN rows behind x and the guard rows around y are on in EVERY family.
  saturating  (softmax) scale x spread over [-80, 60] with one column per row at exactly +80: most terms underflow; the output must be finite, within the
              bars, and the argmax column 1 to within U.

Worst measured ratios per kernel and input family, and the offset figures: profiles/conv_vae_edge_sweep.txt.
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
FLUSH = 2.0 ** -126
GUARD = 256
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DT = {"bf16": BF, "f32": F32}
CODE = {"bf16": G._BF16, "f32": G._F32}
GN_EPS = 1e-6


def f32(v):
    """The fp32 number a float argument of the C ABI arrives as."""
    return float(torch.tensor(v, dtype=F32))


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ---------------------------------------------------------------------------------------------- the launch arithmetic, restated (see the docstring)
CAP_BLOCKS, THREADS = 65535, 256
PPB = 128                                         # vae.hip mmdit_vae_groupnorm: pixels per apply workgroup


def grid_cap(n, bs=THREADS):                      # vae.hip grid_cap
    return max(1, min(CAP_BLOCKS, (n + bs - 1) // bs))


def past_cap(n):
    """A grid-stride kernel whose n work items need a second trip of the loop."""
    return n > grid_cap(n) * THREADS


def gn_rpb(HW, B):                                # vae.hip mmdit_vae_groupnorm: rows per statistics workgroup
    rpb = 128
    while ((HW + rpb - 1) // rpb) * B > 2048 and rpb < HW:
        rpb *= 2
    return rpb


def gn_nty(C):                                    # vae.hip gn_stats_kernel / gn_apply_kernel: row lanes of a 256-thread workgroup
    return 256 // (C // 8)


def gn_depth(C, Gn, HW, B):
    """S of the yardstick."""
    rpb, nty, cpg = gn_rpb(HW, B), gn_nty(C), C // Gn
    return -(-min(rpb, HW) // nty) + nty * cpg + -(-HW // rpb) + 2


HW_SHAPE = {1: (1, 1), 3: (1, 3), 15: (3, 5), 77: (7, 11), 127: (1, 127), 128: (8, 16), 129: (3, 43), 257: (1, 257), 262145: (5, 52429)}


class Case:
    """One launch of one kernel under one input family; the keyword arguments are the kernel's shape parameters."""

    def __init__(self, kind, fam="random", exact_only=False, **kw):
        self.kind, self.fam, self.exact_only, self.kw = kind, fam, exact_only, kw
        self.__dict__.update(kw)

    @property
    def id(self):
        return f"{self.kind}-{self.fam}-" + "-".join(f"{k}{v}" for k, v in self.kw.items())

    def work(self):
        """Work items of the grid-stride kernels (one thread each)."""
        k = self.kind
        if k == "nchw_to_nhwc":
            return self.B * self.HW * (self.Cp // 8)
        if k == "nhwc_to_nchw":
            return self.B * self.C * self.HW
        if k == "im2col":
            Ho, Wo = im2col_out(self.mode, self.H, self.W)
            return self.B * Ho * Wo * 9 * (self.C // 8)
        if k == "pad_cast":
            return self.B * (self.H << self.up) * (self.W << self.up) * (self.C // 8)
        return 0

    def paths(self):
        k, s = self.kind, set()
        if past_cap(self.work()):
            s.add(f"{k}:past_cap")
        if k == "nchw_to_nhwc":
            s |= {f"{k}:{self.dt}", f"{k}:pad{self.Cp - self.C > 0}", f"{k}:affine{self.aff}", f"{k}:partial_group{self.C % 8 != 0}"}
        if k == "nhwc_to_nchw":
            s |= {f"{k}:ld>C{self.ld > self.C}", f"{k}:clamp{self.clamp}"}
        if k == "im2col":
            s |= {f"{k}:mode{self.mode}", f"{k}:H1" if self.H == 1 else f"{k}:H>1", f"{k}:W1" if self.W == 1 else f"{k}:W>1"}
        if k == "pad_cast":
            s |= {f"{k}:{self.dt}", f"{k}:up{self.up}"}
        if k == "groupnorm":
            C, Gn, HW, B = self.C, self.Gn, self.HW, self.B
            cg, cpg, nty, rpb = C // 8, C // Gn, gn_nty(C), gn_rpb(HW, B)
            s |= {f"{k}:{self.dt}", f"{k}:silu{self.silu}", f"{k}:pad{self.pad}", f"{k}:{self.fam}"}
            if rpb > 128:
                s.add(f"{k}:rpb_doubles")
            if 256 % cg:
                s.add(f"{k}:idle_threads")
            if cpg % 8:
                s.add(f"{k}:thread_spans_groups")
            if cpg < 8:
                s.add(f"{k}:cpg<8")
            if cpg > 8 and cpg % 8:
                s.add(f"{k}:straddle")
            if cpg == 1:
                s.add(f"{k}:cpg1")
            if Gn == 1:
                s.add(f"{k}:one_group")
            if Gn == 64:
                s.add(f"{k}:G64")
            if nty == 1:
                s.add(f"{k}:nty1")
            if HW < nty:
                s.add(f"{k}:fewer_rows_than_nty")
            last = min(rpb, HW - (HW - 1) // rpb * rpb)          # rows of the last statistics chunk
            if last % (4 * nty):
                s.add(f"{k}:rows_in_flight_beyond_end")          # the four-rows-in-flight clamp
            if HW > rpb:
                s.add(f"{k}:second_stats_chunk")
            if HW > PPB:
                s.add(f"{k}:second_apply_chunk")
            if HW % PPB in (1, PPB - 1) or HW == PPB:
                s.add(f"{k}:apply_chunk_edge{HW % PPB}")
            if (min(PPB, HW) // nty) % 2 or min(PPB, HW) % nty:
                s.add(f"{k}:second_pixel_in_flight_absent")
        if k == "softmax":
            s |= {f"{k}:rows%4={self.rows % 4}", f"{k}:cols{'<' if self.cols < 64 else '=' if self.cols == 64 else '>'}64", f"{k}:ld-cols>=8{self.ld - self.cols >= 8}",
                  f"{k}:{self.fam}", f"{k}:scale1{self.scale == 1.0}"}
            if self.ld == self.cols:
                s.add(f"{k}:no_padding")
            if self.cols % 64 == 1:
                s.add(f"{k}:one_lane_second_trip")
        return s


def im2col_out(mode, H, W):
    return (H // 2, W // 2) if mode == 1 else (2 * H, 2 * W) if mode == 2 else (H, W)


def _cases():
    out = []
    add = out.append
    # ---- NCHW -> NHWC
    for dt in ("f32", "bf16"):
        for C, Cp in ((3, 8), (3, 64), (16, 16), (16, 64), (9, 16), (8, 8)):
            for HW in (1, 15, 77):
                for B in (1, 3):
                    for aff in (0, 1):
                        add(Case("nchw_to_nhwc", dt=dt, C=C, Cp=Cp, HW=HW, B=B, aff=aff))
    add(Case("nchw_to_nhwc", exact_only=True, dt="bf16", C=3, Cp=64, HW=2097200, B=1, aff=0))                 # 16,777,600 threads' worth: 640 past 65535 x 256
    # ---- NHWC -> NCHW
    for C in (3, 32):
        for ld in (C, C + 5):
            for clamp in (0, 1):
                for HW in (1, 15, 77):
                    for B in (1, 3):
                        add(Case("nhwc_to_nchw", C=C, ld=ld, HW=HW, B=B, clamp=clamp))
    add(Case("nhwc_to_nchw", exact_only=True, C=32, ld=32, HW=524300, B=1, clamp=1))
    # ---- im2col
    for mode, hw in ((0, ((1, 1), (1, 5), (2, 3), (3, 2), (5, 6), (6, 1), (2, 2), (3, 3), (6, 5))), (2, ((1, 1), (1, 5), (2, 3), (3, 2), (5, 6), (6, 1), (2, 2), (3, 3), (6, 5))),
                     (1, ((2, 2), (2, 6), (6, 2), (6, 6)))):
        for H, W in hw:
            for C in (8, 24, 64):
                for B in (1, 3):
                    add(Case("im2col", mode=mode, H=H, W=W, C=C, B=B))
    add(Case("im2col", exact_only=True, mode=0, H=1366, W=1366, C=8, B=1))
    # ---- pad / cast / upsample
    for dt in ("f32", "bf16"):
        for up in (0, 1):
            for H, W in ((1, 1), (1, 6), (3, 3), (6, 1), (3, 6), (6, 6)):
                for C in (8, 24, 128):
                    for B in (1, 3):
                        add(Case("pad_cast", dt=dt, up=up, H=H, W=W, C=C, B=B))
    add(Case("pad_cast", exact_only=True, dt="bf16", up=1, H=2049, W=2049, C=8, B=1))
    # ---- GroupNorm: the (C, G) table of the docstring x HW x B; input dtype, SiLU and pad rotate so that every pair meets every option
    table = ((128, 32), (512, 32), (32, 32), (64, 32), (96, 8), (24, 1), (512, 64), (2048, 32))
    n = 0
    for C, Gn in table:
        for HW in (1, 3, 127, 128, 129, 257):
            for B in (1, 3):
                o = n + n // 8      # (walks all 8 option combinations under every (C, G) and every HW)
                n += 1
                opt = dict(dt=("f32", "bf16")[o & 1], silu=(o >> 1) & 1, pad=(o >> 2) & 1)
                add(Case("groupnorm", C=C, Gn=Gn, HW=HW, B=B, **opt))
                if B == 3 and HW in (1, 128, 129):
                    for fam in ("offset", "smallvar", "poison"):
                        add(Case("groupnorm", fam, C=C, Gn=Gn, HW=HW, B=B, **opt))
    for C, Gn in ((128, 32), (96, 8)):      # ... and every option combination at the two shapes where a thread's channels span groups
        for o in range(8):
            add(Case("groupnorm", "smallvar" if o & 1 else "offset", C=C, Gn=Gn, HW=129, B=2, dt=("f32", "bf16")[o & 1], silu=(o >> 1) & 1, pad=(o >> 2) & 1))
    add(Case("groupnorm", C=8, Gn=2, HW=262145, B=1, dt="bf16", silu=1, pad=0))                                  # ceil(HW / 128) B = 2049 > 2048: rpb doubles
    # ---- row softmax
    for rows in (1, 2, 3, 4, 5, 37):
        for cols in (1, 63, 64, 65, 100, 129):
            for ld in ((cols + 7) // 8 * 8, cols + 8):
                for scale in (1.0, 512 ** -0.5):
                    add(Case("softmax", rows=rows, cols=cols, ld=ld, scale=scale))
                if rows in (3, 37):
                    add(Case("softmax", "saturating", rows=rows, cols=cols, ld=ld, scale=512 ** -0.5))
    return out


CASES = _cases()
KINDS = ("nchw_to_nhwc", "nhwc_to_nchw", "im2col", "pad_cast", "groupnorm", "softmax")


# ---------------------------------------------------------------------------------------------- sentinels
class Win(G.Out):
    """The GEMM sweep's sentinel output for a DENSE tensor of any rank: `t` (what the kernel receives) lies between GUARD rows of the NaN bit
    pattern; pad: t is (B, H + 2, W + 2, C) and the kernel may write the interior only -- the border keeps the (non-zero) pattern too.
    touched() counts the sentinel elements that changed."""

    def __init__(self, shape, dtype, device, pad=False):
        self.it, self.pat = self.PATTERN[dtype]
        self.n, self.g, self.pad = math.prod(shape), GUARD * ((shape[-1] + 7) // 8 * 8), pad
        self.big = torch.empty(self.n + 2 * self.g, dtype=dtype, device=device)
        self.big.view(self.it).fill_(self.pat)
        self.t = self.big[self.g:self.g + self.n].view(shape)
        self.win = self.t[:, 1:-1, 1:-1] if pad else self.t

    def sentinels(self):
        s = [self.big[:self.g], self.big[self.g + self.n:]]
        return s + [self.t[:, 0], self.t[:, -1], self.t[:, 1:-1, 0], self.t[:, 1:-1, -1]] if self.pad else s

    def touched(self):
        return sum(int((s.view(self.it) != self.pat).sum()) for s in self.sentinels())


def nan_tailed(x):
    """x as the kernel receives it: dense, with GUARD NaN rows (of the last dimension's width, at least 8 elements) behind."""
    if x.numel() > 1 << 24:
        return x.contiguous()
    n, g = x.numel(), GUARD * max(8, x.shape[-1])
    big = torch.full((n + g,), float("nan"), dtype=x.dtype, device=x.device)
    big[:n] = x.reshape(-1)
    return big[:n].view(x.shape)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ---------------------------------------------------------------------------------------------- inputs, float64 references, yardsticks
def _gen(c):
    return torch.Generator().manual_seed(sum((i + 1) * b for i, b in enumerate(c.id.encode())) % (1 << 31))      # (a seed per case id, stable across processes)


def build(c, device):
    """The case's inputs as the kernel receives them (dict), on `device`."""
    g = _gen(c)
    rn = lambda *s: torch.randn(*s, generator=g)                                      # noqa: E731
    k, t = c.kind, {}
    if k == "nchw_to_nhwc":
        if c.exact_only:
            x = (torch.arange(c.B * c.C * c.HW, dtype=torch.int32) % 251 - 125).float().view(c.B, c.C, c.HW)
        else:
            x = rn(c.B, c.C, c.HW)
        t["x"] = nan_tailed(x.to(DT[c.dt]).to(device))
        t["scale"], t["shift"] = (f32(1 / 0.3611), f32(0.1159)) if c.aff else (1.0, 0.0)
    elif k == "nhwc_to_nchw":
        if c.exact_only:
            x = ((torch.arange(c.B * c.HW * c.ld, dtype=torch.int32) % 509 - 254).float() / 128).view(c.B * c.HW, c.ld)
        else:
            x = rn(c.B * c.HW, c.ld) * 1.5
            x.view(-1)[::7] = 1.0              # values exactly on the bounds
            x.view(-1)[3::11] = -1.0
            x[:, c.C:] = float("nan")        # the columns between C and ld are never read
        t["x"] = nan_tailed(x.to(device))
        t["lo"], t["hi"] = (-1.0, 1.0) if c.clamp else (-float("inf"), float("inf"))
        if c.clamp and not c.exact_only and c.B * c.HW * c.C >= 45:
            v = x[:, :c.C]
            assert bool((v > 1).any()) and bool((v < -1).any()) and bool((v == 1).any()) and bool((v == -1).any()) and bool((v.abs() < 1).any())
    elif k == "im2col":
        x = (torch.arange(c.B * c.H * c.W * c.C, dtype=torch.int32) % 32749 - 16000).float().view(c.B, c.H, c.W, c.C) if c.exact_only else rn(c.B, c.H, c.W, c.C)
        t["x"] = nan_tailed(x.to(BF).to(device))
    elif k == "pad_cast":
        x = (torch.arange(c.B * c.H * c.W * c.C, dtype=torch.int32) % 32749 - 16000).float().view(c.B * c.H * c.W, c.C) if c.exact_only else rn(c.B * c.H * c.W, c.C)
        t["x"] = nan_tailed(x.to(DT[c.dt]).to(device))
    elif k == "groupnorm":
        rows, cpg = c.B * c.HW, c.C // c.Gn
        if c.HW > 1 << 16:
            x = 0.5 + 2 * torch.randn(rows, c.C, generator=torch.Generator(device=device).manual_seed(5), device=device)      # (2 M elements: drawn on the device)
        elif c.fam == "offset":
            x = 16 + rn(rows, c.C)
        elif c.fam == "smallvar":
            d = (8e-4 * rn(rows, c.C).clamp(-3, 3)).view(c.B, c.HW, c.Gn, cpg)
            sd = (d - d.mean((1, 3), keepdim=True)).pow(2).mean((1, 3), keepdim=True).sqrt()
            x = (0.03 + d * (9e-4 / sd.clamp_min(9e-4))).reshape(rows, c.C)          # (a group of few elements can draw a larger spread: scaled back to 9e-4)
            x.view(c.B, c.HW, c.Gn, cpg)[:, :, 0, :] = 2.0
        else:
            x = 0.5 + 2 * rn(rows, c.C)
        t["x"] = nan_tailed(x.to(DT[c.dt]).to(device))
        t["gamma"], t["beta"] = rn(c.C).to(device), rn(c.C).to(device)
        t["eps"] = f32(GN_EPS)
        if c.fam == "smallvar":
            xg = t["x"].double().view(c.B, c.HW, c.Gn, cpg)
            sd = (xg - xg.mean((1, 3), keepdim=True)).pow(2).mean((1, 3)).sqrt()
            assert float(sd.max()) <= 1e-3 and float(sd[:, 0].max()) == 0.0, float(sd.max())
    elif k == "softmax":
        sc = f32(c.scale)
        if c.fam == "saturating":
            x = (torch.rand(c.rows, c.ld, generator=g) * 140 - 80) / sc
            top = torch.randint(0, c.cols, (c.rows,), generator=g)
            x[torch.arange(c.rows), top] = 80 / sc
            t["top"] = top.to(device)
        else:
            x = rn(c.rows, c.ld) * 3
        x[:, c.cols:] = float("nan")       # padding columns are never read
        t["x"], t["scale"] = nan_tailed(x.to(device)), sc
    return t


def im2col_gather(x, mode):
    """x (B, H, W, C) -> (B Ho Wo, 9 C) by index, from an explicitly padded (mode 0 / 2: one zero pixel all round; mode 1: one zero row below and one
    zero column right) and, for mode 2, explicitly upsampled tensor."""
    B, H, W, C = x.shape
    if mode == 2:
        x = x[:, torch.arange(2 * H, device=x.device) // 2][:, :, torch.arange(2 * W, device=x.device) // 2]
        H, W = 2 * H, 2 * W
    Ho, Wo = (H // 2, W // 2) if mode == 1 else (H, W)
    s, lead = (2, 0) if mode == 1 else (1, 1)
    xp = torch.zeros((B, H + 2, W + 2, C), dtype=x.dtype, device=x.device)
    xp[:, lead:lead + H, lead:lead + W] = x
    yo, xo = s * torch.arange(Ho, device=x.device), s * torch.arange(Wo, device=x.device)
    return torch.stack([xp[:, (yo + kh)[:, None], (xo + kw)[None, :]] for kh in range(3) for kw in range(3)], 3).reshape(B * Ho * Wo, 9 * C)


def gn_reference(x, gamma, beta, B, HW, C, Gn, eps, silu):
    cpg, S = C // Gn, gn_depth(C, Gn, HW, B)
    x64 = x.double().view(B, HW, Gn, cpg)
    red = lambda v: v.mean((1, 3), keepdim=True)                                     # noqa: E731
    m, q, a1 = red(x64), red(x64 * x64), red(x64.abs())
    v = red((x64 - m) ** 2)
    r = (v + eps) ** -0.5
    dm, dq = S * u * a1, S * u * q
    dv = dq + 2 * m.abs() * dm + 2 * u * (q + m * m)
    dr = r * (0.5 * dv / (v + eps) + 2 * u)
    ga, be = gamma.double().view(1, 1, Gn, cpg), beta.double().view(1, 1, Gn, cpg)
    sc = r * ga
    of = be - m * sc
    ref = (x64 - m) * sc + be
    det = (x64 - m).abs() * (ga.abs() * dr + u * sc.abs()) + sc.abs() * dm + u * ((x64 * sc).abs() + (m * sc).abs() + of.abs()) + u * ref.abs()
    if silu:
        o = ref
        ref = o * torch.sigmoid(o)
        det = 1.1 * det + 8 * E23 * (1 + o.abs()) * ref.abs()
    shape = (B * HW, C)
    return ref.reshape(shape), det.reshape(shape), (U * ref.abs()).reshape(shape)


def reference(c, t):
    """(ref, y_det, y_rnd) in float64, 2-D, laid out like view2d() of the output."""
    k, x = c.kind, t["x"]
    if k == "nchw_to_nhwc":
        x64 = x.double()
        ref = torch.zeros((c.B, c.HW, c.Cp), dtype=F64, device=x.device)
        det = torch.zeros_like(ref)
        ref[:, :, :c.C] = ((x64 + t["shift"]) * t["scale"]).transpose(1, 2)
        if not (c.dt == "bf16" and not c.aff):
            det[:, :, :c.C] = (2 * u * (x64.abs() + abs(t["shift"])) * abs(t["scale"])).transpose(1, 2)
            rnd = U * ref.abs()
        else:
            rnd = torch.zeros_like(ref)
        return ref.view(-1, c.Cp), det.view(-1, c.Cp), rnd.view(-1, c.Cp)
    if k == "nhwc_to_nchw":
        ref = x[:, :c.C].double().clamp(t["lo"], t["hi"]).view(c.B, c.HW, c.C).transpose(1, 2).reshape(c.B * c.C, c.HW)
    elif k == "im2col":
        ref = im2col_gather(x, c.mode).double()
    elif k == "pad_cast":
        xb = x.to(BF).view(c.B, c.H, c.W, c.C)
        if c.up:
            xb = xb[:, torch.arange(2 * c.H, device=x.device) // 2][:, :, torch.arange(2 * c.W, device=x.device) // 2]
        ref = xb.reshape(-1, c.C).double()
    elif k == "groupnorm":
        return gn_reference(x, t["gamma"], t["beta"], c.B, c.HW, c.C, c.Gn, t["eps"], c.silu)
    elif k == "softmax":
        tt = t["scale"] * x[:, :c.cols].double()
        tt = tt - tt.amax(1, keepdim=True)
        p = torch.exp(tt)
        p = p / p.sum(1, keepdim=True)
        ref, det, rnd = (torch.zeros((c.rows, c.ld), dtype=F64, device=x.device) for _ in range(3))
        ref[:, :c.cols] = p
        det[:, :c.cols] = p * (8 * E23 * (1 + tt.abs()) + ((c.cols + 63) // 64 + 8) * u) + FLUSH
        rnd[:, :c.cols] = U * p
        return ref, det, rnd
    return ref, torch.zeros_like(ref), torch.zeros_like(ref)


def out_shape(c):
    """(shape of the tensor the kernel receives, dtype, padded)."""
    k = c.kind
    if k == "nchw_to_nhwc":
        return (c.B * c.HW, c.Cp), BF, False
    if k == "nhwc_to_nchw":
        return (c.B * c.C, c.HW), F32, False
    if k == "im2col":
        Ho, Wo = im2col_out(c.mode, c.H, c.W)
        return (c.B * Ho * Wo, 9 * c.C), BF, False
    if k == "pad_cast":
        return (c.B, (c.H << c.up) + 2, (c.W << c.up) + 2, c.C), BF, True
    if k == "groupnorm":
        H, W = HW_SHAPE[c.HW]
        return ((c.B, H + 2, W + 2, c.C), BF, True) if c.pad else ((c.B * c.HW, c.C), BF, False)
    return (c.rows, c.ld), BF, False


def view2d(c, win):
    """The written window as the 2-D matrix reference() describes."""
    return win.reshape(-1, win.shape[-1]) if win.dim() == 4 else win


def launch(lib, c, t, o, stream):
    k, x = c.kind, t["x"]
    if k == "nchw_to_nhwc":
        H, W = HW_SHAPE.get(c.HW, (1, c.HW))
        return lib.mmdit_vae_nchw_to_nhwc(x.data_ptr(), CODE[c.dt], c.B, c.C, H, W, c.Cp, t["scale"], t["shift"], o.t.data_ptr(), stream)
    if k == "nhwc_to_nchw":
        H, W = HW_SHAPE.get(c.HW, (1, c.HW))
        return lib.mmdit_vae_nhwc_to_nchw(x.data_ptr(), c.B, c.C, H, W, c.ld, t["lo"], t["hi"], o.t.data_ptr(), stream)
    if k == "im2col":
        return lib.mmdit_vae_im2col3x3(x.data_ptr(), c.B, c.H, c.W, c.C, c.mode, o.t.data_ptr(), stream)
    if k == "pad_cast":
        return lib.mmdit_vae_pad_cast(x.data_ptr(), CODE[c.dt], c.B, c.H, c.W, c.C, c.up, o.t.data_ptr(), stream)
    if k == "groupnorm":
        H, W = HW_SHAPE[c.HW]
        t["sums"] = torch.zeros(c.B * c.Gn * 2, dtype=F32, device=x.device)
        return lib.mmdit_vae_groupnorm(x.data_ptr(), CODE[c.dt], t["gamma"].data_ptr(), t["beta"].data_ptr(), c.B, H, W, c.C, c.Gn, t["eps"], c.silu,
                                       t["sums"].data_ptr(), o.t.data_ptr(), c.pad, stream)
    return lib.mmdit_vae_softmax_rows(x.data_ptr(), c.rows, c.cols, c.ld, t["scale"], o.t.data_ptr(), stream)


def offset_figures(out, ref):
    """(worst row ||out - ref|| / (U ||ref||), worst |out - ref| / (U |ref|) over the elements with |ref| >= the row's rms)."""
    d = (out.double() - ref).abs()
    rms = ref.pow(2).mean(1, keepdim=True).sqrt()
    big = ref.abs() >= rms
    el = float((d / (U * ref.abs()).clamp_min(G.TINY))[big].max()) if bool(big.any()) else 0.0
    return float((d.norm(dim=1) / (U * ref.norm(dim=1)).clamp_min(G.TINY)).max()), el


def check(c, t, out2d, ref, det, rnd):
    """The failures of one output against its reference beyond the three bars: the kernel's own extra promises."""
    bad = []
    if c.kind == "softmax":
        o = out2d.double()
        if bool((o[:, c.cols:] != 0).any()):
            bad.append("a padding column is not zero")
        dev = float((o[:, :c.cols].sum(1) - 1).abs().max())
        if not dev <= c.cols * U:
            bad.append(f"a row sum is {dev} from 1, more than cols U = {c.cols * U}")
        if c.fam == "saturating":
            top = o[torch.arange(c.rows, device=o.device), t["top"]]
            if not float((top - 1).abs().max()) <= U:
                bad.append(f"argmax column {top.tolist()[:4]} is not 1 to within U")
    if c.kind == "nchw_to_nhwc" and bool((bits(out2d[:, c.C:]) != 0).any()):
        bad.append("a padded channel is not (+) zero")
    if c.kind == "groupnorm" and c.fam == "smallvar":      # the constant group: beta to within y (it is inside the bars already; stated on its own)
        cpg = c.C // c.Gn
        d = (out2d.double() - ref)[:, :cpg].abs()
        if bool((d > G.ELEM_BAR * (det + rnd)[:, :cpg]).any()):
            bad.append("the constant group is not beta (after SiLU) to within y")
    return bad


WORST = {}             # (kernel, input family) -> [per-element, per-row, per-column, rounding bias] as (ratio, case id)
OFFSET = [0.0, 0.0, "", ""]


def _record(c, r):
    w = WORST.setdefault((c.kind, c.fam), [(-1.0, "")] * 4)
    for i, k in enumerate(("el", "row", "col", "bias")):
        if r[k] is not None and r[k] > w[i][0]:
            w[i] = (r[k], c.id)


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\n[vae edge sweep] worst ratio to the yardstick per kernel and input family (bars: per element 2.0, per row / column 1.0, rounding bias 1.0)")
    for (kf, fam), w in sorted(WORST.items()):
        print(f"  {kf:<14} {fam:<10} " + "  ".join(f"{n} {v:.3f} @ {cid}" for n, (v, cid) in zip(("elem", "row", "col", "bias"), w) if v >= 0))
    print(f"[vae edge sweep] groupnorm, offset family, distance from a pure bf16 rounding: worst row ||out - ref|| / (U ||ref||) = {OFFSET[0]:.3f} @ {OFFSET[2]}; "
          f"worst |out - ref| / (U |ref|) over |ref| >= row rms = {OFFSET[1]:.3f} @ {OFFSET[3]}")


# ---------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_vae_edge(ops, c):
    """One launch: sentinels (guard rows, border of a padded output) bit-identical, every output finite and within the three bars and the rounding-bias
    bar against float64 (yardstick 0 for the gather / copy kernels: bit-identical), the kernel's own promises (zero padding, row sums, argmax)."""
    lib = ops._lib.lib()
    t = build(c, "cuda")
    shape, dtype, pad = out_shape(c)
    o = Win(shape, dtype, "cuda", pad)
    torch.cuda.synchronize()
    rc = launch(lib, c, t, o, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, (c.id, rc)
    failures = []
    if o.touched():
        failures.append(f"{o.touched()} sentinel elements (guard rows{' / border' if pad else ''}) changed")
    got = view2d(c, o.win)
    ref, det, rnd = reference(c, t)
    if c.exact_only:      # past the cap: bit patterns, on the device
        want = ref.to(dtype)
        assert bool((want.double() == ref).all())
        wrong = int((bits(got) != bits(want)).sum())
        print(f"[vae edges] {c.id}: {wrong} of {want.numel()} elements differ")
        assert not failures and wrong == 0, (c.id, failures, wrong)
        return
    if not bool(torch.isfinite(got).all()):
        failures.append(f"{int((~torch.isfinite(got)).sum())} non-finite elements")
    else:
        r = G.ratios(got, ref, det, rnd)
        _record(c, r)
        print(f"[vae edges] {c.id}: elem {r['el']:.3f} @ ({r['at'][0]}, {r['at'][1]}) row {r['row']:.3f} @ {r['at'][2]} col {r['col']:.3f} @ {r['at'][3]}"
              + (f" bias {r['bias']:.3f}" if r["bias"] is not None else ""))
        bad = G.verdict(r)
        if bad:
            failures.append(f"{bad} over the bar: {r}")
        failures += check(c, t, got, ref, det, rnd)
        if c.kind == "groupnorm" and c.fam == "offset":
            ro, el = offset_figures(got, ref)
            print(f"[vae edges] {c.id}: offset figures row {ro:.3f} elem {el:.3f}")
            if ro > OFFSET[0]:
                OFFSET[0], OFFSET[2] = ro, c.id
            if el > OFFSET[1]:
                OFFSET[1], OFFSET[3] = el, c.id
    assert not failures, "\n".join([c.id] + failures)
