"""positional_encoding="RoPE2dV2" on the GPU (reference: rotary_embedding_2d_v2.py, Attention.py:105-107, 220-239): channel triples of the
normalised image queries / keys are rotated by a row angle theta and a column angle alpha, and the three rotated components are written as
three concatenated groups.

  1, 2  mmdit_qk_norm_rope3_fwd / _bwd at head width 64 and 128                  (csrc/rowops_rope3.hip)
  3     argument checks of the ops wrappers and of the entry points: nothing is launched
  4     the model against the reference's own golden (tests/golden/forward_micro_rope2dv2*.npz, tools/make_goldens_rope2dv2.py), both routes
  5     head width 128: one block against float64 autograd of this file's restatement of a block; the parity forward of the model
  6     sample_imgs against a plain loop over net.forward; three optimizer steps, eager and replayed from a captured graph

References inside this file are plain float64 torch on the operands as the kernel sees them (the bf16- or fp32-stored qkv, the fp32 tables cast
to float64); none of them calls ops.*.  rotate3 / rotate3_t below are the yardstick; tests/test_rope2dv2_abi.py holds them to the reference
module's recorded outputs on the CPU.

The kernels have one layout for every row and head count (a head vector is head_dim / 8 lanes, the vectors of a problem are dealt to 256-thread
workgroups in a grid-stride loop): include/mmdit_hip_rope3.h defines no switch constant, so there is no threshold to straddle.  The shapes are
the smallest at which that indexing can go wrong: 1, 2, 3, 19 and 24 heads (head counts that do and do not divide the 32 / 16 vectors of a
workgroup, the trained model's 19, one past the 21-head cap of the hd128 / merge kernels), grids of one row and of one column, fewer vectors
than one workgroup holds and several workgroups with a ragged last one.

Bound of the forward (1), derived as tests/test_kv_merge_gpu.py (1) derives its own.  The kernel evaluates, in fp32 from the loaded row x,
z = w * x / sqrt(mean(x^2) + eps) and the rotation of the module docstring's three lines, and rounds ONCE to bf16.  Every fp32 step is a relative
perturbation of at most 2^-24 of its result: the hd-term sum of squares at most hd - 1 of them on a sum of positive terms (any order), i.e.
(hd - 1) / 2 on 1 / sqrt; the reciprocal square root 2; the two norm products 2; the rotation 4 (two for a three-factor term, two for the
three-term sum) on the magnitude m = the sum of the absolute values of an output's (up to three) rotation terms of the exact chain (m = |z| for
text rows and the tail channels, m = |v| for V).  (hd - 1) / 2 + 2 + 2 + 4 = hd / 2 + 7.5 < C = hd / 2 + 8, so the fp32 value f satisfies
|f - ref| <= C * 2^-24 * m and the stored bf16(f)
    |out - ref| <= u |ref| + (1 + u) * C * 2^-24 * m,      u = 2^-8,
for EVERY element.  The kernel's operation order is the counted one (rowops_rope3.hip: x * rinv * w, then a * c - b * s * c' + d * s * s'; a
contraction into fused multiply-adds only removes roundings).  V is the rounded copy of the raw row: bit-equal.

Bound of the backward (2): tests/test_kv_merge_gpu.py (2) with the head width in place of 64.  The rotation is orthogonal, so the Jacobian
R diag(w) (I - x x^T / (hd r^2)) / r enlarges a row by at most max|w| / r, and per output row (one token: 3 * heads * hd gradients)
    G_row = sqrt(sum_heads (max|wq| / r_q)^2 ||dQ||^2 + (max|wk| / r_k)^2 ||dK||^2 + ||dV||^2),
    err_row <= u_out ||ref_row|| + 2 * hd * 2^-24 * G_row          (two hd-term reductions; u_out = 2^-8 for bf16 dqkv, 0 for fp32).
The norm-weight gradients are fp32 sums of n = rows * heads terms t = dz * xhat per feature, added atomically on top of the caller's value:
|dw - (init + ref)| <= (n + hd) * 2^-24 * (sum |t| + |init|).

Measured figures: profiles/rope2dv2_parity.txt.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import mmdit_oracle as O  # noqa: E402
from oracle.weights import make_inputs as model_inputs, make_state_dict  # noqa: E402

U = 2.0 ** -8          # bf16 unit roundoff (round to nearest)
E32 = 2.0 ** -24       # fp32 unit roundoff
BF16, F32 = torch.bfloat16, torch.float32
EPS = torch.finfo(torch.float32).eps
MICRO = dict(dim=128, num_heads=2, num_blocks=3)
HD128 = dict(dim=256, num_heads=2, num_blocks=1)


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------- the yardstick: the rotation in float64
def _split3(z, cs, sn):
    T = cs.shape[-1] // 2
    return T, (z[..., 0:3 * T:3], z[..., 1:3 * T:3], z[..., 2:3 * T:3]), (cs[..., :T], sn[..., :T], cs[..., T:], sn[..., T:])


def rotate3(z, cs, sn):
    """z (..., tokens, hd); cs / sn (tokens, 2T) = [theta part | alpha part].  Triples (3j, 3j+1, 3j+2) in, groups j, T+j, 2T+j out; tail kept."""
    T, (a, b, d), (ct, st, ca, sa) = _split3(z, cs, sn)
    return torch.cat([a * ct - b * st * ca + d * st * sa, a * st + b * ct * ca - d * ct * sa, b * sa + d * ca, z[..., 3 * T:]], dim=-1)


def rotate3_mag(z, cs, sn):
    """The sum of the absolute values of the terms of each output of rotate3 (the m of the forward bound)."""
    T, (a, b, d), (ct, st, ca, sa) = _split3(z.abs(), cs.abs(), sn.abs())
    return torch.cat([a * ct + b * st * ca + d * st * sa, a * st + b * ct * ca + d * ct * sa, b * sa + d * ca, z.abs()[..., 3 * T:]], dim=-1)


def rotate3_t(g, cs, sn, mag=False):
    """The transpose of rotate3 (its backward): groups in, interleaved triples out.  mag: the sum of the absolute values of the terms."""
    T = cs.shape[-1] // 2
    if mag:
        g, cs, sn = g.abs(), cs.abs(), sn.abs()
    s = 1.0 if mag else -1.0
    g0, g1, g2 = g[..., :T], g[..., T:2 * T], g[..., 2 * T:3 * T]
    ct, st, ca, sa = cs[..., :T], sn[..., :T], cs[..., T:], sn[..., T:]
    da = g0 * ct + g1 * st
    db = s * g0 * st * ca + g1 * ct * ca + g2 * sa
    dd = g0 * st * sa + s * g1 * ct * sa + g2 * ca
    return torch.cat([torch.stack([da, db, dd], dim=-1).reshape(*g.shape[:-1], 3 * T), g[..., 3 * T:]], dim=-1)


def _tables(hd, h2, w2, f=1):
    import sd3_amd  # noqa: F401
    from sd3_amd.blocks.rotary_embedding_2d_v2 import RoPE2D
    return RoPE2D(hd, interpolate_factor=f).tables(h2, w2, torch.device("cuda:0"))


# ---------------------------------------------------------------------------------------------- 1, 2: the row kernels
# (batch, heads, (grid rows, grid columns), text tokens)
_SHAPES = [(2, 1, (3, 5), 6), (2, 3, (5, 3), 6), (1, 2, (1, 4), 2), (1, 2, (4, 1), 2), (1, 19, (2, 2), 2), (1, 24, (2, 2), 2)]


class _Case:
    """Seeded operands of one (batch, heads, grid, Mt, hd, dtype, f) and the float64 chain norm -> rotation."""

    def __init__(self, Bt, H, hw, Mt, hd, dtype, f):
        self.Bt, self.H, self.hw, self.N, self.Mt, self.hd, self.dtype, self.f = Bt, H, hw, hw[0] * hw[1], Mt, hd, dtype, f
        self.S, self.d = self.N + Mt, H * hd
        g = torch.Generator().manual_seed(9176 * self.S + 31 * Bt * H + 7 * hw[0] + hd + f)
        rn = lambda *sh: torch.randn(*sh, generator=g)
        self.cos, self.sin = _tables(hd, hw[0], hw[1], f)
        self.w = [(1 + 0.1 * rn(hd)).cuda() for _ in range(4)]                      # wq_x, wk_x, wq_c, wk_c: not all ones
        self.qkv_x, self.qkv_c = rn(Bt * self.N, 3 * self.d).to(dtype).cuda(), rn(Bt * Mt, 3 * self.d).to(dtype).cuda()

    def img(self, *extra):
        return (self.qkv_x, self.w[0], self.w[1], self.cos, self.sin, self.N, 0) + extra

    def txt(self, *extra):
        return (self.qkv_c, self.w[2], self.w[3], None, None, self.Mt, self.N) + extra

    def chain(self, qkv, L, rope, wq, wk):
        """float64: (q, k, v) per token after norm / rotation and the magnitudes m of the docstring, each (Bt, H, L, hd)."""
        q, k, v = qkv.reshape(self.Bt, L, 3, self.H, self.hd).permute(2, 0, 3, 1, 4)
        q, k = F.rms_norm(q, (self.hd,), wq.double(), EPS), F.rms_norm(k, (self.hd,), wk.double(), EPS)
        mq, mk = q.abs(), k.abs()
        if rope:
            c, s = self.cos.double(), self.sin.double()
            mq, mk = rotate3_mag(q, c, s), rotate3_mag(k, c, s)
            q, k = rotate3(q, c, s), rotate3(k, c, s)
        return (q, k, v), (mq, mk, v.abs())

    def reference(self, xr, cr, w=None):
        w = self.w if w is None else w
        (qx, kx, vx), (mqx, mkx, mvx) = self.chain(xr, self.N, True, w[0], w[1])
        (qc, kc, vc), (mqc, mkc, mvc) = self.chain(cr, self.Mt, False, w[2], w[3])
        cat = lambda a, b: torch.cat([a, b], 2)
        return dict(Q=cat(qx, qc), K=cat(kx, kc), V=cat(vx, vc)), dict(Q=cat(mqx, mqc), K=cat(mkx, mkc), V=cat(mvx, mvc))


def _case_id(p):
    (Bt, H, hw, Mt), hd, f = p
    return f"b{Bt}h{H}-{hw[0]}x{hw[1]}-txt{Mt}-hd{hd}-f{f}"


_KERNEL_CASES = [(s, hd, f) for s in _SHAPES for hd in (64, 128) for f in (1, 2)]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", _KERNEL_CASES, ids=_case_id)
def test_rope3_fwd(case, dtype, ops):
    """Q, K, V of both streams in one launch against the float64 chain, EVERY element under the bound of the module docstring; each stream
    alone at its tok0 writes the same bits and nothing outside its token range; V bit-equal to the rounded raw rows; text rows in natural
    channel order; the tail channels not rotated; image token (0, 0) the pure permutation of z."""
    (Bt, H, hw, Mt), hd, f = case
    c = _Case(Bt, H, hw, Mt, hd, dtype, f)
    T, sent = hd // 3, 123.0
    Q, K, V = (torch.full((Bt, H, c.S, hd), sent, dtype=BF16, device="cuda") for _ in range(3))
    ops.qk_norm_rope3_fwd_pair(c.img(), c.txt(), Bt, H, c.S, Q, K, V)
    with torch.no_grad():
        ref, mag = c.reference(c.qkv_x.double(), c.qkv_c.double())
    C = hd / 2 + 8
    worst = {}
    for name, out in (("Q", Q), ("K", K), ("V", V)):
        assert bool(torch.isfinite(out).all()) and not bool((out == sent).all(-1).any()), (name, "a row was not written")
        bound = U * ref[name].abs() + (1 + U) * C * E32 * mag[name]
        ratio = (out.double() - ref[name]).abs() / bound
        worst[name] = float(ratio.max())
        # the parts of the claim, each on its own slice: text rows (natural order), tail channels (not rotated)
        worst[name + " text"], worst[name + " tail"] = float(ratio[:, :, c.N:].max()), float(ratio[..., 3 * T:].max())
    print(f"[rope3 fwd {'bf16' if dtype == BF16 else 'fp32'}] {_case_id(case)}: worst |out - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= 1.0, (name, v)
    # V: the rounded copy of the raw rows
    vx = c.qkv_x.reshape(Bt, c.N, 3, H, hd)[:, :, 2].permute(0, 2, 1, 3).to(BF16)
    vc = c.qkv_c.reshape(Bt, Mt, 3, H, hd)[:, :, 2].permute(0, 2, 1, 3).to(BF16)
    assert torch.equal(V, torch.cat([vx, vc], 2)), "V is not the rounded copy of the v columns"
    # each stream alone at its tok0: the same bits, and the other stream's rows untouched
    for streams in ((c.img(),), (c.txt(),)):
        Q1, K1, V1 = (torch.full((Bt, H, c.S, hd), sent, dtype=BF16, device="cuda") for _ in range(3))
        qkv, wq, wk, rc, rs, tokens, tok0 = streams[0]
        ops.qk_norm_rope3_fwd(qkv, wq, wk, rc, rs, Bt, tokens, H, c.S, tok0, Q1, K1, V1)
        for a, b in ((Q1, Q), (K1, K), (V1, V)):
            assert torch.equal(a[:, :, tok0:tok0 + tokens], b[:, :, tok0:tok0 + tokens]), "a single-stream launch differs from the pair launch"
            rest = torch.cat([a[:, :, :tok0], a[:, :, tok0 + tokens:]], 2)
            assert bool((rest == sent).all()), "a single-stream launch wrote outside its token range"
    # image token (0, 0): both angles are zero, the output is the de-interleaving permutation of z -- the same launch without tables gives z
    Qn, Kn, Vn = (torch.full((Bt, H, c.S, hd), sent, dtype=BF16, device="cuda") for _ in range(3))
    ops.qk_norm_rope3_fwd(c.qkv_x, c.w[0], c.w[1], None, None, Bt, c.N, H, c.S, 0, Qn, Kn, Vn)
    perm = torch.cat([torch.arange(0, 3 * T, 3), torch.arange(1, 3 * T, 3), torch.arange(2, 3 * T, 3), torch.arange(3 * T, hd)]).cuda()
    assert torch.equal(Q[:, :, 0], Qn[:, :, 0][..., perm]) and torch.equal(K[:, :, 0], Kn[:, :, 0][..., perm]), "token (0, 0) is not the pure permutation of z"
    if c.N > 1:
        assert not torch.equal(Q[:, :, 1:c.N], Qn[:, :, 1:c.N][..., perm]), "no token of the image stream was rotated"


_BWD_CASES = [(s, hd, 1) for s in _SHAPES for hd in (64, 128)] + [(_SHAPES[1], 64, 2), (_SHAPES[1], 128, 2)]


@pytest.mark.parametrize("gdtype,dtype", [(BF16, BF16), (F32, F32), (BF16, F32)], ids=["bf16", "fp32", "mixed"])
@pytest.mark.parametrize("case", _BWD_CASES, ids=_case_id)
def test_rope3_bwd(case, gdtype, dtype, ops):
    """dqkv rows against float64 autograd through norm -> rotation, per row under the bound of the module docstring; the norm-weight gradients
    are ADDED to a non-zero initial value.  The three dtype combinations of mmdit_qk_norm_rope_bwd; each stream alone gives the same dqkv bits."""
    (Bt, H, hw, Mt), hd, f = case
    c = _Case(Bt, H, hw, Mt, hd, dtype, f)
    g = torch.Generator().manual_seed(4441 * c.S + H + hd)
    dQ, dK, dV = (torch.randn(Bt, H, c.S, hd, generator=g).to(gdtype).cuda() for _ in range(3))
    init = [(0.5 * torch.randn(hd, generator=g)).cuda() for _ in range(4)]
    dw = [t.clone() for t in init]
    dx, dc = ops.qk_norm_rope3_bwd_pair(dQ, dK, dV, c.img(dw[0], dw[1]), c.txt(dw[2], dw[3]), Bt, H, c.S, dtype)
    assert dx.dtype == dtype and dx.shape == c.qkv_x.shape and dc.shape == c.qkv_c.shape

    xr, cr = c.qkv_x.double().requires_grad_(True), c.qkv_c.double().requires_grad_(True)
    w64 = [t.double().requires_grad_(True) for t in c.w]
    ref, _ = c.reference(xr, cr, w64)
    ((ref["Q"] * dQ.double()).sum() + (ref["K"] * dK.double()).sum() + (ref["V"] * dV.double()).sum()).backward()

    def row_bound(qkv, L, tok0, wq, wk):
        x = qkv.double().reshape(Bt, L, 3, H, hd)
        r = (x.pow(2).mean(-1) + EPS).sqrt()                                            # (Bt, L, 3, H)
        nrm = lambda t: t.double()[:, :, tok0:tok0 + L].norm(dim=-1).permute(0, 2, 1)      # (Bt, L, H)
        fq, fk = float(wq.abs().max()) / r[:, :, 0], float(wk.abs().max()) / r[:, :, 1]
        return ((fq * nrm(dQ)) ** 2 + (fk * nrm(dK)) ** 2 + nrm(dV) ** 2).sum(-1).sqrt().reshape(Bt * L)

    tag = "bf16" if dtype == BF16 else "fp32" if gdtype == F32 else "mixed"
    u_out = U if dtype == BF16 else 0.0
    for name, out, rg, G in (("dqkv_x", dx, xr.grad, row_bound(c.qkv_x, c.N, 0, c.w[0], c.w[1])), ("dqkv_c", dc, cr.grad, row_bound(c.qkv_c, Mt, c.N, c.w[2], c.w[3]))):
        assert bool(torch.isfinite(out).all())
        err, bound = (out.double() - rg).norm(dim=-1), u_out * rg.norm(dim=-1) + 2 * hd * E32 * G
        ratio = err / bound
        print(f"[rope3 bwd {tag}] {_case_id(case)} {name}: worst row {float(ratio.max()):.3f} of the bound (row {int(ratio.argmax())})")
        assert float(ratio.max()) <= 1.0, (name, int(ratio.argmax()), float(ratio.max()))

    # norm-weight gradients: sum |t| from a second float64 pass with |.| taken per term (t = dz * xhat of one (row, head))
    def abs_terms(qkv, L, tok0, rope, part):
        x = qkv.double().reshape(Bt, L, 3, H, hd).permute(2, 0, 3, 1, 4)[part]
        xhat = x / (x.pow(2).mean(-1, keepdim=True) + EPS).sqrt()
        gz = (dQ if part == 0 else dK).double()[:, :, tok0:tok0 + L]
        gz = rotate3_t(gz, c.cos.double(), c.sin.double(), mag=True) if rope else gz.abs()
        return (gz * xhat.abs()).sum((0, 1, 2))
    plan = [(0, c.qkv_x, c.N, 0, True, 0), (1, c.qkv_x, c.N, 0, True, 1), (2, c.qkv_c, Mt, c.N, False, 0), (3, c.qkv_c, Mt, c.N, False, 1)]
    for i, qkv, L, tok0, rope, part in plan:
        n = Bt * L * H
        bound = (n + hd) * E32 * (abs_terms(qkv, L, tok0, rope, part) + init[i].double().abs())
        err = (dw[i].double() - (init[i].double() + w64[i].grad)).abs()
        print(f"[rope3 bwd {tag}] {_case_id(case)} dw[{i}]: worst {float((err / bound).max()):.3f} of the bound")
        assert bool((err <= bound).all()), (i, float((err / bound).max()))
        assert float((dw[i] - init[i]).abs().max()) > 0

    scratch = [torch.zeros(hd, device="cuda") for _ in range(4)]
    dx1 = ops.qk_norm_rope3_bwd(dQ, dK, dV, *c.img()[:5], Bt, c.N, H, c.S, 0, scratch[0], scratch[1], dtype)
    dc1 = ops.qk_norm_rope3_bwd(dQ, dK, dV, *c.txt()[:5], Bt, Mt, H, c.S, c.N, scratch[2], scratch[3], dtype)
    assert torch.equal(dx1, dx) and torch.equal(dc1, dc), "a single-stream launch differs from the pair launch"


# ---------------------------------------------------------------------------------------------- 3: argument checks
def test_argument_checks_raise_before_a_launch(ops):
    from sd3_amd import _lib
    Bt, H, hw, Mt = 2, 3, (2, 3), 4
    c = _Case(Bt, H, hw, Mt, 64, BF16, 1)
    sent = 7.0
    new = lambda hd=64, S=c.S: [torch.full((Bt, H, S, hd), sent, dtype=BF16, device="cuda") for _ in range(3)]
    outs = []

    def refused(fn, *a):
        with pytest.raises(RuntimeError):
            fn(*a)
    Q, K, V = new(96)                                                                  # a head width the kernels are not built for
    refused(ops.qk_norm_rope3_fwd_pair, c.img(), c.txt(), Bt, H, c.S, Q, K, V)
    outs += [Q, K, V]
    Q, K, V = new(128)                                                                 # qkv rows, weights and tables of width 64 with a 128-wide Q
    refused(ops.qk_norm_rope3_fwd_pair, c.img(), c.txt(), Bt, H, c.S, Q, K, V)
    outs += [Q, K, V]
    Q, K, V = new()
    wide = torch.zeros(c.N, 64, device="cuda")                                         # the table of the pair kernels: (tokens, 64), not (tokens, 42)
    refused(ops.qk_norm_rope3_fwd_pair, (c.qkv_x, c.w[0], c.w[1], wide, wide, c.N, 0), c.txt(), Bt, H, c.S, Q, K, V)
    refused(ops.qk_norm_rope3_fwd_pair, (c.qkv_x, c.w[0], c.w[1], c.cos[:-1], c.sin[:-1], c.N, 0), c.txt(), Bt, H, c.S, Q, K, V)
    refused(ops.qk_norm_rope3_fwd_pair, (c.qkv_x, c.w[0], c.w[1], c.cos, None, c.N, 0), c.txt(), Bt, H, c.S, Q, K, V)
    refused(ops.qk_norm_rope3_fwd_pair, c.img(), (c.qkv_c, c.w[2], c.w[3], None, None, Mt, c.N + 1), Bt, H, c.S, Q, K, V)      # tokens past s_total
    refused(ops.qk_norm_rope3_fwd, c.qkv_x, c.w[0][:32], c.w[1], c.cos, c.sin, Bt, c.N, H, c.S, 0, Q, K, V)                   # norm weight length
    dw = [torch.full((64,), sent, device="cuda") for _ in range(4)]
    dQ = torch.zeros(Bt, H, c.S, 64, device="cuda")
    refused(ops.qk_norm_rope3_bwd_pair, dQ, dQ, dQ, c.img(dw[0], dw[1]), (c.qkv_c, c.w[2], c.w[3], None, None, Mt, c.N + 1, dw[2], dw[3]), Bt, H, c.S, BF16)
    refused(ops.qk_norm_rope3_bwd_pair, dQ, dQ, dQ, c.img(dw[0][:32], dw[1]), c.txt(dw[2], dw[3]), Bt, H, c.S, BF16)
    outs += [Q, K, V] + dw

    # the entry points themselves: error codes of the header, nothing launched
    probs = (_lib.QkProblem * 2)()
    dx, dc = torch.full_like(c.qkv_x, sent), torch.full_like(c.qkv_c, sent)

    def fill(tok0_txt=c.N):
        for q, (qkv, wq, wk, rc, rs, tokens, tok0, dq, dwq, dwk) in zip(probs, (c.img(dx, dw[0], dw[1]), (c.qkv_c, c.w[2], c.w[3], None, None, Mt, tok0_txt, dc, dw[2], dw[3]))):
            q.qkv, q.wq, q.wk, q.tokens, q.tok0 = qkv.data_ptr(), wq.data_ptr(), wk.data_ptr(), tokens, tok0
            q.rope_cos, q.rope_sin = (rc.data_ptr(), rs.data_ptr()) if rc is not None else (None, None)
            q.dqkv, q.dwq, q.dwk = dq.data_ptr(), dwq.data_ptr(), dwk.data_ptr()
    fill()
    st, L = torch.cuda.current_stream().cuda_stream, _lib.lib()
    q3 = [t.data_ptr() for t in (Q, K, V)]
    fwd = lambda count=2, dt=_lib.BF16, hd=64, S=c.S, q3=q3: L.mmdit_qk_norm_rope3_fwd(probs, count, dt, Bt, H, hd, S, *q3, st)
    bwd = lambda count=2, dts=(_lib.BF16,) * 3, hd=64, S=c.S: L.mmdit_qk_norm_rope3_bwd(probs, count, *q3, *dts, Bt, H, hd, S, st)
    for hd in (32, 96, 63, 256):
        assert fwd(hd=hd) == _lib.ERR_SHAPE and bwd(hd=hd) == _lib.ERR_SHAPE
    assert fwd(dt=_lib.FP8) == _lib.ERR_DTYPE and bwd(dts=(_lib.F32, _lib.BF16, _lib.BF16)) == _lib.ERR_DTYPE and bwd(dts=(_lib.BF16, _lib.BF16, _lib.F32)) == _lib.ERR_DTYPE
    assert fwd(count=0) == _lib.ERR_ARG and fwd(count=3) == _lib.ERR_ARG and bwd(count=3) == _lib.ERR_ARG
    assert fwd(q3=[q3[0], None, q3[2]]) == _lib.ERR_ARG and fwd(S=c.S - 1) == _lib.ERR_ARG and bwd(S=c.S - 1) == _lib.ERR_ARG
    fill(tok0_txt=c.N + 1)
    assert fwd() == _lib.ERR_ARG and bwd() == _lib.ERR_ARG
    probs[0].rope_sin = None
    assert fwd(count=1) == _lib.ERR_ARG and bwd(count=1) == _lib.ERR_ARG
    torch.cuda.synchronize()
    for t in outs + [dx, dc]:
        assert bool((t == sent).all()), "a refused launch wrote to its outputs"


# ---------------------------------------------------------------------------------------------- 4: the model against the reference's golden
_net = {}


def _state_dict(net, cfg):
    """oracle.weights.make_state_dict minus the rotary_emb.freqs keys; the inv_freq buffers stay as constructed (tools/make_goldens_rope2dv2.py)."""
    sd = {k: v for k, v in make_state_dict(0, MLP_type="swiglu", **cfg).items() if not k.endswith("rotary_emb.freqs")}
    sd.update({k: v.detach().cpu().clone() for k, v in net.state_dict().items() if k.endswith("rotary_emb.inv_freq")})
    return sd


def _new_model(cfg, **kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    net = diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=torch.device("cuda:0"),
                     positional_encoding="RoPE2dV2", **cfg, **kw)
    net.load_state_dict(_state_dict(net, cfg), strict=True)
    return net


def build(precision, which="micro"):
    if which not in _net:
        _net[which] = _new_model(MICRO if which == "micro" else HD128, checkpoint_MLP=False, checkpoint_attn=False)
    return _net[which].set_precision(precision)


def _checksum(*ts):
    return [float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts]


# tests/test_model_gpu.py on `micro_plain`: parity mode rel-L2 < 1e-3 against the reference golden (the project's bar for every configuration);
# fast mode < 1.5 x FAST_MEASURED["micro_plain"][1] = 1.5 x 6.893e-3 against the same fp32 golden: the same network with another orthogonal map at
# the same rounding points
FWD_BAR = {"parity": 1e-3, "fast": 1.5 * 6.893e-03}
_FWD_CASES = [("square", "forward_micro_rope2dv2.npz", 0, 16, 16, 1.0, [0.3, 0.7], None),
              ("16x24", "forward_micro_rope2dv2_nonsquare.npz", 2, 16, 24, 30.0, [0.5, 0.5], ([0, 0], [1, 0], [0, 0]))]


@pytest.mark.parametrize("precision", ["parity", "fast"])
@pytest.mark.parametrize("case", _FWD_CASES, ids=[c[0] for c in _FWD_CASES])
def test_model_forward_vs_reference_golden(case, precision, golden_dir):
    """diff_model.forward (the engine route) against the reference run with positional_encoding="RoPE2dV2"."""
    name, file, seed, h, w, tscale, tvals, nulls = case
    gold = np.load(os.path.join(golden_dir, file))
    x, c, cp = model_inputs(seed, 2, h, w, text_scale=tscale)
    assert np.allclose(gold["inputs_checksum"], _checksum(x, c, cp), rtol=1e-9), "seeded inputs drifted from the fixture"
    nl = [] if nulls is None else [torch.tensor(n).bool() for n in nulls]
    net = build(precision)
    assert all(b.attn.rope3 for b in net.blocks)
    with torch.no_grad():
        v = net(x.cuda(), torch.tensor(tvals), c.cuda(), cp.cuda(), *nl)
    r = rel(v, torch.from_numpy(gold["v"]))
    print(f"[rope2dv2 {precision}] {name}: forward rel-L2 vs reference golden = {r:.3e} (bar {FWD_BAR[precision]:.2e}) = {r / FWD_BAR[precision]:.3f} of the bar")
    assert bool(torch.isfinite(v).all()) and r < FWD_BAR[precision], r


# the RoPE2d micro model in fast mode against grads_micro.npz (tests/test_kv_merge_gpu.py PLAIN_FAST_MEASURED, profiles/kv_merge_parity.txt): worst
# stored-tensor rel-L2, worst tensor gradient-norm error, worst sample error / typical element
PLAIN_FAST_MEASURED = (2.507e-02, 1.531e-02, 7.391e-02)


@pytest.mark.parametrize("precision", ["parity", "fast"])
def test_model_gradients_vs_reference_golden(precision, golden_dir):
    """loss = v.pow(2).mean() on the inputs of grads_micro.npz, gradients against the reference's (RoPE2dV2) own, in the structure of
    tests/test_kv_merge_gpu.py::test_model_gradients_vs_reference_golden:
      parity  loss within 2e-3 relative, 8 seeded samples per tensor within 6e-2 of a typical element, the stored (<= 4096-element) tensors
              rel-L2 < 3e-2, gradient norms of the tensors < 3e-2 and of the three scalar parameters < 1e-1;
      fast    bf16 rounding of the whole path against an fp32 reference: the yardstick is that rounding itself, the RoPE2d model in fast mode,
              same weights and inputs, against ITS reference golden (grads_micro.npz), measured here and pinned to 1.5 x its recorded figures.
              The encoding must not move the model farther from its reference than 1.5 x that: worst stored-tensor rel-L2, worst tensor
              gradient-norm error, worst sample error; the scalar parameters' norms < 1e-1.
    Every figure is printed before anything is asserted."""
    gold = np.load(os.path.join(golden_dir, "forward_micro_rope2dv2.npz"))
    x, c, cp = model_inputs(5, 2, 16, 16, text_scale=30.0)
    nl = [torch.tensor(n).bool() for n in ([0, 1], [0, 0], [1, 0])]

    def measure(net, gold):
        """(loss, v, rows): rows = (name, numel, relative norm error, worst sample error / typical element, rel-L2 of a stored tensor or None)"""
        net.zero_grad()
        v = net(x.cuda(), torch.tensor([0.4, 0.9]), c.clone().cuda(), cp.clone().cuda(), *nl)
        loss = v.pow(2).mean()
        loss.backward()
        grads = dict((n, p.grad) for n, p in net.named_parameters() if p.grad is not None)
        names = [str(n) for n in gold["grad_names"]]
        assert set(names) == set(grads.keys())
        gs = torch.Generator().manual_seed(11)
        params = dict(net.named_parameters())
        rows = []
        for i, n in enumerate(names):
            p = params[n]
            idx = torch.randint(0, p.numel(), (8,), generator=gs)
            gn = float(grads[n].double().norm())
            rn = abs(gn - gold["grad_norms"][i]) / (gold["grad_norms"][i] + 1e-12)
            samp = grads[n].flatten()[idx.cuda()].cpu().numpy()
            typical = max(float(np.abs(gold["grad_samples"][i]).max()), gold["grad_norms"][i] / np.sqrt(p.numel()))
            rs = float(np.abs(samp - gold["grad_samples"][i]).max()) / (typical + 1e-30)
            rows.append((n, p.numel(), rn, rs, rel(grads[n], torch.from_numpy(gold["grad__" + n])) if "grad__" + n in gold.files else None))
        net.zero_grad()
        return float(loss.detach()), v.detach(), rows

    loss, v, rows = measure(build(precision), gold)
    assert len(rows) == 109
    tens = [r for r in rows if r[1] > 1]
    worst = lambda rws, k: max(r[k] for r in rws if r[k] is not None)
    print(f"[rope2dv2 {precision}] gradient case: loss {loss:.6f} vs {float(gold['grad_loss']):.6f} (rel {abs(loss - float(gold['grad_loss'])) / abs(float(gold['grad_loss'])):.3e}), "
          f"v rel-L2 {rel(v, torch.from_numpy(gold['grad_v'])):.3e}; "
          f"{len(rows)} parameters: worst relative grad-norm error {worst(tens, 2):.3e} ({max(tens, key=lambda r: r[2])[0]}), "
          f"worst sample / typical {worst(tens, 3):.3e} ({max(tens, key=lambda r: r[3])[0]}), "
          f"worst stored-tensor rel-L2 {worst(tens, 4):.3e} ({max((r for r in tens if r[4] is not None), key=lambda r: r[4])[0]}); "
          "scalars (norm error): " + ", ".join(f"{r[0]} {r[2]:.3e}" for r in rows if r[1] == 1))
    if precision == "parity":
        assert abs(loss - float(gold["grad_loss"])) < 2e-3 * abs(float(gold["grad_loss"]))
        for n, numel, rn, rs, rl in rows:
            assert rn < (1e-1 if numel == 1 else 3e-2), (n, rn)
            if numel > 1:
                assert rs < 6e-2, (n, rs)
                assert rl is None or rl < 3e-2, (n, rl)
    else:
        from sd3_amd.models.diff_model import diff_model
        plain = diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=torch.device("cuda:0"),
                           positional_encoding="RoPE2d", checkpoint_MLP=False, checkpoint_attn=False, **MICRO)
        plain.load_state_dict(make_state_dict(0, MLP_type="swiglu", **MICRO), strict=True)
        gm = np.load(os.path.join(golden_dir, "grads_micro.npz"))
        _, _, base = measure(plain.set_precision("fast"), gm)
        bt = [r for r in base if r[1] > 1]
        print(f"[rope2dv2 fast] the RoPE2d model in fast mode against grads_micro.npz: worst relative grad-norm error {worst(bt, 2):.3e}, worst sample / typical {worst(bt, 3):.3e}, "
              f"worst stored-tensor rel-L2 {worst(bt, 4):.3e}")
        print(f"[rope2dv2 fast] RoPE2dV2 / RoPE2d: stored-tensor rel-L2 {worst(tens, 4) / worst(bt, 4):.3f}, grad-norm error {worst(tens, 2) / worst(bt, 2):.3f}, "
              f"sample error {worst(tens, 3) / worst(bt, 3):.3f} (bar 1.5)")
        for k, recorded in ((4, PLAIN_FAST_MEASURED[0]), (2, PLAIN_FAST_MEASURED[1]), (3, PLAIN_FAST_MEASURED[2])):
            assert worst(bt, k) <= 1.5 * recorded, ("the RoPE2d yardstick moved", k, worst(bt, k), recorded)
        assert worst(tens, 4) <= 1.5 * worst(bt, 4), (worst(tens, 4), worst(bt, 4))
        assert worst(tens, 2) <= 1.5 * worst(bt, 2), (worst(tens, 2), worst(bt, 2))
        assert worst(tens, 3) <= 1.5 * worst(bt, 3), (worst(tens, 3), worst(bt, 3))
        for n, numel, rn, rs, rl in rows:
            if numel == 1:
                assert rn < 1e-1, (n, rn)


@pytest.mark.parametrize("precision", ["parity", "fast"])
def test_attention_module_route_vs_golden_and_engine_route(precision, golden_dir, monkeypatch):
    """The stand-alone Attention module (blocks/Attention.py, the autograd route) of block 0:
      * on the reference's own block-0 inputs (forward_micro_plain.npz's norm1 taps: nothing in front of the first attention depends on the
        positional encoding) against the reference's attention taps: parity mode < 1e-3 (fast mode: held to the forward's fast-mode bar);
      * on the engine route's OWN block-0 inputs (captured from diff_model.forward) the attention core's outputs of the two routes agree to the
        bar test_graph_replay_matches_eager_steps applies to two launch modes of one step: rel-L2 < 1e-3, max-abs <= 2e-3 max|b| + 1e-6;
      * BACKWARD, the same bar: block 0's gradient of the two out-projection outputs is captured from the model's backward and fed to the
        stand-alone module's backward; the two routes' gradients of the attention inputs and of every attention parameter of block 0 agree."""
    from sd3_amd import engine, ops
    gold = np.load(os.path.join(golden_dir, "forward_micro_rope2dv2.npz"))
    plain = np.load(os.path.join(golden_dir, "forward_micro_plain.npz"))
    net = build(precision)
    b0 = net.blocks[0]
    assert b0.attn.rope3 and b0.attn.precision == precision
    x, c, cp = model_inputs(0, 2, 16, 16, text_scale=1.0)
    n1x, n1c = torch.from_numpy(plain["tap_norm1_x"]).cuda(), torch.from_numpy(plain["tap_norm1_c"]).cuda()
    with torch.no_grad():
        ax, ac = b0.attn(n1x, n1c, x.shape)
    rx, rc = rel(ax, torch.from_numpy(gold["tap_attn_x"])), rel(ac, torch.from_numpy(gold["tap_attn_c"]))
    print(f"[rope2dv2 {precision}] stand-alone Attention vs reference taps: attn_x {rx:.3e}, attn_c {rc:.3e} (bar {FWD_BAR[precision]:.2e})")
    assert rx < FWD_BAR[precision] and rc < FWD_BAR[precision]

    seen, groups, real_block_fwd, real_group = [], [], engine.block_fwd, engine._group
    launches, real3f, real3b = [], ops.qk_norm_rope3_fwd_pair, ops.qk_norm_rope3_bwd_pair

    def spy(*a, **kw):
        out = real_block_fwd(*a, **kw)
        if not seen:          # (clones: the step's buffers go back to the pool)
            sv = out[2]
            seen.append({k: getattr(sv, k).clone() for k in ("ln1x", "ln1c", "Ox", "Oc", "lse")})
        return out

    def spy_group(m, problems, **kw):
        outs = real_group(m, problems, **kw)
        groups.append(([(p["A"].clone(), p["B"].data_ptr(), bool(p.get("b_kmajor")), bool(p.get("a_kmajor"))) for p in problems], [o.clone() for o in outs]))
        return outs
    B, N, Mt, d = 2, 64, 154, 128
    net.zero_grad()
    monkeypatch.setattr(engine, "block_fwd", spy)
    monkeypatch.setattr(engine, "_group", spy_group)
    monkeypatch.setattr(ops, "qk_norm_rope3_fwd_pair", lambda *a, **kw: (launches.append("fwd"), real3f(*a, **kw))[1])
    monkeypatch.setattr(ops, "qk_norm_rope3_bwd_pair", lambda *a, **kw: (launches.append("bwd"), real3b(*a, **kw))[1])
    v = net(x.cuda(), torch.tensor([0.3, 0.7]), c.cuda(), cp.cuda())
    v.pow(2).sum().backward()
    monkeypatch.undo()
    assert launches == ["fwd"] * 3 + ["bwd"] * 3, launches      # every block took the new pair launches, in both directions
    sv = seen[0]
    attn_params = [(n, p) for n, p in b0.attn.named_parameters() if p.requires_grad]
    eng_grads = {n: p.grad.detach().clone() for n, p in attn_params}
    assert len(eng_grads) == 12 and all(float(gr.abs().max()) > 0 for gr in eng_grads.values())
    w0 = b0.attn.weights(net._mode())
    dgrad = lambda ptr: [(ins, outs) for ins, outs in groups if ins[0][1] == ptr and ins[0][2] and not ins[0][3]]
    (do_in, _), = dgrad(w0.Wo_x.data_ptr())              # block 0's dO launch: A = d(out-projection outputs)
    (_, dln1), = dgrad(w0.Wqkv_x.data_ptr())             # block 0's dln1 launch: the gradients of the attention inputs
    dacc_x, dacc_c = do_in[0][0], do_in[1][0]
    net.zero_grad()

    cores, real_attn_fwd = [], ops.attn_fwd
    monkeypatch.setattr(ops, "attn_fwd", lambda *a, **kw: (cores.append(real_attn_fwd(*a, **kw)), cores[-1])[1])
    xin, cin = sv["ln1x"].float().view(B, N, d).requires_grad_(True), sv["ln1c"].float().view(B, Mt, d).requires_grad_(True)
    ox, oc = b0.attn(xin, cin, x.shape)
    torch.autograd.backward([ox, oc], [dacc_x.float().view(B, N, d), dacc_c.float().view(B, Mt, d)])
    monkeypatch.undo()
    Ox, Oc, lse = cores[0]
    pairs = [("Ox", Ox, sv["Ox"]), ("Oc", Oc, sv["Oc"]), ("lse", lse, sv["lse"]),
             ("dX", xin.grad.reshape(B * N, d).to(dln1[0].dtype), dln1[0]), ("dC", cin.grad.reshape(B * Mt, d).to(dln1[1].dtype), dln1[1])]
    pairs += [("grad " + n, p.grad, eng_grads[n]) for n, p in attn_params]
    res = [(name, rel(a, b), float((a.double() - b.double()).abs().max()), float(b.double().abs().max())) for name, a, b in pairs]
    for name, r, mx, bmax in res:
        print(f"[rope2dv2 {precision}] autograd route vs engine route, block 0 {name}: rel-L2 {r:.3e}, max-abs {mx:.3e} (max|b| {bmax:.3e})")
    for name, r, mx, bmax in res:
        assert bmax > 0 and r < 1e-3 and mx <= 2e-3 * bmax + 1e-6, (name, r, mx)
    net.zero_grad()


def test_inference_forward_and_refusals():
    """The inference forward schedule (no_grad: no saved tensors) takes the new route in both supported precisions; the e4m3 ones are refused and
    leave the precision as it was."""
    x, c, cp = model_inputs(0, 2, 16, 16, text_scale=1.0)
    outs = {}
    for precision in ("parity", "fast"):
        net = build(precision)
        with torch.no_grad():
            outs[precision] = net(x.cuda(), torch.tensor([0.3, 0.7]), c.cuda(), cp.cuda())
    assert rel(outs["fast"], outs["parity"]) < FWD_BAR["fast"]
    for precision in ("fp8", "mxfp8"):
        with pytest.raises(RuntimeError, match="RoPE2dV2"):
            build(precision)
        assert _net["micro"].precision == "fast"


# ---------------------------------------------------------------------------------------------- 5: head width 128
def _attention_v2(x, c, sd, prefix, cfg, hw, last, taps=None):
    """oracle.attention with the RoPE2dV2 branch (Attention.py:220-239) in place of the RoPE2d one: this file's restatement, on the oracle's leaf
    functions (their rounding points are the HIP path's in the rounding-matched configurations).  tests/test_rope2dv2_abi.py holds the oracle with
    this function in place of its own to the reference's golden at width 64, where one exists."""
    B, N, d = x.shape
    M, H, hd = c.shape[1], cfg.num_heads, cfg.head_dim
    heads = lambda t, L: t.reshape(B, L, H, hd).permute(0, 2, 1, 3)
    qkv_x = O._lin8(cfg, x, [sd[prefix + n + "_proj_x.weight"] for n in ("query", "key", "value")])
    qkv_c = O._lin8(cfg, c, [sd[prefix + n + "_proj_c.weight"] for n in ("query", "key", "value")])
    q_x = O.rms_norm(heads(O._act(cfg, qkv_x[0]), N), sd[prefix + "q_norm_x.weight"])
    k_x = O.rms_norm(heads(O._act(cfg, qkv_x[1]), N), sd[prefix + "k_norm_x.weight"])
    v_x = heads(O._act(cfg, qkv_x[2]), N)
    q_c = O.rms_norm(heads(O._act(cfg, qkv_c[0]), M), sd[prefix + "q_norm_c.weight"])
    k_c = O.rms_norm(heads(O._act(cfg, qkv_c[1]), M), sd[prefix + "k_norm_c.weight"])
    v_c = heads(O._act(cfg, qkv_c[2]), M)
    h2, w2 = hw[0] // 2, hw[1] // 2
    fr = sd[prefix + "rotary_emb.inv_freq"].float()
    n = torch.arange(h2 * w2)
    ang = torch.cat([(n // w2).float()[:, None] * fr, (n % w2).float()[:, None] * fr], dim=-1)      # (interpolate_factor 1)
    cs, sn = ang.cos().to(q_x.dtype), ang.sin().to(q_x.dtype)
    q = torch.cat([rotate3(q_x, cs, sn), q_c], dim=2)
    k = torch.cat([rotate3(k_x, cs, sn), k_c], dim=2)
    v = torch.cat([v_x, v_c], dim=2)
    o = O._rg(cfg, O.attention_core(q, k, v, hd ** -0.5, cfg.attn_core))
    o_x = o[:, :, :N].permute(0, 2, 1, 3).reshape(B, N, -1)
    o_c = o[:, :, N:].permute(0, 2, 1, 3).reshape(B, M, -1)
    a_x = O._lin8(cfg, o_x, [sd[prefix + "out_proj_x.weight"]])[0]
    a_c = o_c if last else O._lin8(cfg, o_c, [sd[prefix + "out_proj_c.weight"]])[0]
    return a_x, a_c


def test_hd128_model_parity_forward(monkeypatch):
    """diff_model(dim 256, 2 heads, 1 block) in parity mode against the fp32 oracle with the restated attention: rel-L2 < 1e-3, the bar of
    tests/test_hd128_model_gpu.py::test_parity_forward_vs_oracle."""
    net = build("parity", "hd128")
    assert net.blocks[0].attn.head_dim == 128 and net.blocks[0].attn.rope3
    sd = _state_dict(net, HD128)
    monkeypatch.setattr(O, "attention", _attention_v2)
    for name, h, w, seed in (("sq", 16, 16, 80), ("nonsq", 12, 20, 81)):
        x, c, cp = model_inputs(seed, 2, h, w, text_scale=30.0)
        t = torch.tensor([0.3, 0.8])
        with torch.no_grad():
            v = net(x.cuda(), t, c.clone().cuda(), cp.clone().cuda())
            ref = O.forward(sd, O.OracleConfig(**HD128), x.clone(), t, c.clone(), cp.clone())
        r = rel(v, ref)
        print(f"[rope2dv2 hd128 parity] {name} {h}x{w}: rel-L2 vs the fp32 oracle with the restated attention = {r:.3e} (bar 1e-3)")
        assert bool(torch.isfinite(v).all()) and r < 1e-3


def test_hd128_block_forward_and_gradients(monkeypatch):
    """One block at head width 128 (blocks.0 of the 1-block model, the engine's block_fwd / block_bwd through Transformer_Block_Dual) in fast mode:
    both outputs, the three input gradients and every parameter gradient against torch autograd through oracle.block with the restated attention
    at the HIP path's rounding points (flash_bf16 core, bf16 GEMMs, rounded gradients); bar max(5e-3, 2 x the restatement's own fp32-vs-float64
    distance), the rule of tests/test_hd128_model_gpu.py.  A 4 x 6 grid and 7 text tokens: 31 keys, one key tile of the 128-wide attention
    kernel, so the untiled flash_bf16 core rounds where the kernel rounds (that file's docstring on the tiled / untiled difference)."""
    net = build("fast", "hd128")
    blk = net.blocks[0]
    sd = _state_dict(net, HD128)
    B, hw, Mt, d = 2, (8, 12), 7, 256
    N = (hw[0] // 2) * (hw[1] // 2)
    g = torch.Generator().manual_seed(17)
    X, Ct, y = torch.randn(B, N, d, generator=g), torch.randn(B, Mt, d, generator=g), torch.randn(B, d, generator=g)
    gX = torch.randn(B, N, d, generator=g) * 1e-2
    blk.zero_grad()
    Xi, Ci, yi = (t.cuda().clone().requires_grad_(True) for t in (X, Ct, y))
    X2, C2 = blk(Xi, Ci, yi, (B, 16) + hw)
    assert torch.equal(C2.detach().cpu(), Ct), "the last block passes the text stream through"
    torch.autograd.backward([X2], [gX.cuda()])
    mine = {"X2": X2.detach(), "dX": Xi.grad, "dC": Ci.grad, "dy": yi.grad}
    mine.update({n: p.grad for n, p in blk.named_parameters() if p.grad is not None})
    names = [k for k in sd if k.startswith("blocks.0.") and not k.endswith("inv_freq")]
    monkeypatch.setattr(O, "attention", _attention_v2)

    def oracle_run(dt):
        cfg = O.OracleConfig(**HD128, attn_core="flash_bf16", gemm="bf16", grad_round=True, dtype=dt)
        sdr = {k: (v.to(dt).clone().requires_grad_(k in names) if v.is_floating_point() else v) for k, v in sd.items()}
        xi, ci, yy = (t.to(dt).clone().requires_grad_(True) for t in (X, Ct, y))
        x2, _ = O.block(xi, ci, yy, sdr, 0, cfg, hw)
        torch.autograd.backward([x2], [gX.to(dt)])
        out = {"X2": x2.detach(), "dX": xi.grad, "dC": ci.grad, "dy": yy.grad}
        out.update({k[len("blocks.0."):]: sdr[k].grad for k in names if sdr[k].grad is not None})
        return out

    g32, g64 = oracle_run(torch.float32), oracle_run(torch.float64)
    assert set(mine) == set(g32), sorted(set(mine) ^ set(g32))
    res = sorted(((rel(mine[n].float(), g32[n]) / max(5e-3, 2 * rel(g64[n], g32[n])), rel(mine[n].float(), g32[n]), rel(g64[n], g32[n]), n) for n in g32), reverse=True)
    print("[rope2dv2 hd128 block] fast: worst by ratio to max(5e-3, 2 x self-distance) (rel-L2 vs the restated block | its float64 self-distance): "
          + "; ".join(f"{n} {r:.2e} | {f:.2e} = {q:.2f}" for q, r, f, n in res[:6]))
    blk.zero_grad()
    for q, r, f, n in res:
        assert bool(torch.isfinite(mine[n]).all()) and q < 1.0, (n, r, f)


# ---------------------------------------------------------------------------------------------- 6: sampler, training step
def test_sampler_equals_a_plain_loop_over_forward():
    """sample_imgs, two Euler steps with guidance and a stub text encoder, against the same two steps written as a loop over net.forward on the
    (2B) guidance batch: the resident-buffer schedule of the sampler launches the same kernels on the same values, bit for bit."""
    class _Cfg:
        latent_channels, shift_factor, scaling_factor = 16, 0.0, 8.0

    class _VAE:
        config, dtype = _Cfg(), torch.float32

        def decode(self, z):
            class D:
                sample = z
            return D

    class _Enc:
        VAE = _VAE()

        def __init__(self, th, tp):
            self.th, self.tp = th, tp

        def text_to_embedding(self, text):
            return self.th.clone(), self.tp.clone()

    _, th, tp = model_inputs(40, 1, 16, 16, text_scale=30.0)
    B, steps, cfg_scale = 2, 2, 3.0
    for precision in ("parity", "fast"):
        net = build(precision)
        net.text_encoders = _Enc(th, tp)
        try:
            img = net.sample_imgs(B, steps, ["x"], cfg_scale=cfg_scale, width=128, height=128, sampler="euler", generator=torch.Generator().manual_seed(99))
        finally:
            del net.text_encoders
        xl = torch.randn((B, 16, 16, 16), generator=torch.Generator().manual_seed(99)).cuda()
        cc = torch.cat([th.expand(B, -1, -1), torch.zeros(B, *th.shape[1:])]).contiguous().cuda()
        pp = torch.cat([tp.expand(B, -1), torch.zeros(B, tp.shape[-1])]).contiguous().cuda()
        with torch.no_grad():
            for t_now in torch.linspace(1, 1.0 / steps, steps).tolist():
                v = net(torch.cat([xl, xl]), torch.full((2 * B,), t_now), cc.clone(), pp.clone())
                xl = xl.sub(((1 + cfg_scale) * v[:B] - cfg_scale * v[B:]), alpha=1 / steps)
        net.train()
        ref = (xl / 8.0).clamp(-1, 1).float()
        print(f"[rope2dv2 sampler] {precision}: rel-L2 vs the plain loop = {rel(img, ref):.3e}")
        assert img.shape == (B, 16, 16, 16) and bool(torch.isfinite(img).all())
        assert torch.equal(img, ref), (precision, rel(img, ref))


def test_graph_replay_matches_eager_steps():
    """tests/test_model_gpu.py::test_graph_replay_matches_eager_steps with the encoding on: three eager warm-up steps, snapshot, steps 4-6 eager,
    restore, capture, steps 4-6 replayed.  The loss of step 4 is bit-identical, the later losses and the final parameters agree to the
    run-to-run noise of the backward pass (that test's bars: rel-L2 < 1e-3, max-abs <= 2e-3 max|b| + 1e-6)."""
    import sd3_amd  # noqa: F401
    from sd3_amd import engine, packing
    from sd3_amd.model_trainer import model_trainer

    overlap = engine._WG_OVERLAP
    try:
        engine._WG_OVERLAP = False
        torch.manual_seed(0)
        net = _new_model(MICRO)
        tr = model_trainer(net, batchSize=4, accumulation_steps=1, totalSteps=100, lr=1e-3, ema_update_freq=1, ema_decay=0.9, warmup_steps=8,
                           use_lr_scheduler=False, device=torch.device("cuda:0"), saveDir="/tmp/_t_rope2dv2", numSaveSteps=100, null_prob_pooled=0.1,
                           null_prob_gemma=0.316, null_prob_bert=0.316, max_res=128, device_rng=True, use_ema=False)
        for s in (1, 2, 3):
            tr.train_step(s)
        torch.cuda.synchronize()
        params = [p for p in net.parameters()]
        snap_p = [p.detach().clone() for p in params]
        snap_o = {id(p): {k: v.clone() for k, v in tr.optim.state[p].items()} for p in params if p in tr.optim.state}
        snap_s = (tr.grad_scaler._scale.clone(), tr.grad_scaler._growth_tracker.clone())
        snap_r = (torch.cuda.get_rng_state(), tr._gen.get_state(), tr.data_source.g.get_state())

        def three_steps():
            losses = [float(tr.train_step(s)) for s in (4, 5, 6)]
            torch.cuda.synchronize()
            return losses, [p.detach().clone() for p in params], tr.optim.param_groups[0]["lr"]

        l0, p0, lr0 = three_steps()
        with torch.no_grad():
            for p, q in zip(params, snap_p):
                p.copy_(q)
                for k, v in snap_o.get(id(p), {}).items():
                    tr.optim.state[p][k].copy_(v)
            tr.grad_scaler._scale.copy_(snap_s[0])
            tr.grad_scaler._growth_tracker.copy_(snap_s[1])
        packing.bump_epoch()
        torch.cuda.set_rng_state(snap_r[0])
        tr._gen.set_state(snap_r[1])
        tr.data_source.g.set_state(snap_r[2])
        tr.scheduler.step(3)
        net(*[a.cuda() for a in model_inputs(3, 2, 16, 16)][:1], torch.tensor([0.3, 0.7]), *[a.cuda() for a in model_inputs(3, 2, 16, 16)][1:]).sum().backward()
        tr.optim.zero_grad()
        torch.cuda.set_rng_state(snap_r[0])
        tr.capture_graph(4)
        assert tr._graph is not None
        l1, p1, lr1 = three_steps()
    finally:
        engine._WG_OVERLAP = overlap
    worst = max((rel(a, b), float((a - b).abs().max()) / (2e-3 * float(b.abs().max()) + 1e-6)) for a, b in zip(p0, p1))
    print(f"[rope2dv2 graph] eager losses {l0}  replayed {l1}; parameters: worst rel-L2 {worst[0]:.3e} (bar 1e-3)")
    assert all(math.isfinite(v) for v in l0 + l1)
    assert lr0 == lr1 and l0[0] == l1[0] and np.allclose(l0, l1, rtol=1e-3)
    for a, b in zip(p0, p1):
        assert rel(a, b) < 1e-3 and float((a - b).abs().max()) <= 2e-3 * float(b.abs().max()) + 1e-6
    assert abs(l0[2] - l0[0]) > 1e-4 * abs(l0[0])
