"""attn_type="cosine2" on the GPU: the L2-norm / RoPE row kernels, the linear-time attention kernels (include/mmdit_hip_cos2.h) and the model.

Every reference is plain float64 torch on the operands AS STORED (bf16 or fp32 values widened exactly); none of them calls ops.*.  The
attention reference is the reference implementation's own quadratic expression (Attention.py:330-339)
    prod = q @ k.mT + 1;  out = (prod / prod.sum(-1, keepdim=True)) @ v
and tests/test_cosine2_abi.py shows on the CPU that this restatement, and its linear form, reproduce the real reference's attention taps.

Bounds (u = 2^-24, u_out = 2^-8 for a bf16 output and 0 for an fp32 one; all per ELEMENT unless said otherwise)

Row kernel, forward.  z = x / max(||x||, 1e-12): the sum of 64 squares is 8 sequential terms per lane and a 3-step tree (products and sums:
<= 11 u relative, every term positive), its square root halves that and adds its own rounding (<= 7.5 u with a 1-ulp sqrt), the quotient adds
<= 2 u: z carries <= 9.5 u relative.  The rotation a c - b s is two more roundings relative to m = |a||c| + |b||s| (the text stream: m = |z|):
    |out - ref| <= u_out |ref| + (1 + u_out) 14 u m                                    (counted 11.5; V: the rounded copy, bit-equal)
A row of zeros has ||x|| = 0 < 1e-12 and gives exact zeros.

Row kernel, backward, per output ROW (one token: 3 * heads * 64 gradients).  With n = max(||x||, 1e-12) and r = R^T dz the un-rotated gradient,
dx = (r - z (z . r)) / n.  r carries 2 u ||dz|| (norm-wise), z 9.5 u, the 64-term sum z . r <= 11 u sum |z||r| <= 11 u ||dz|| of its own and
11.5 u ||dz|| from its operands, the numerator therefore <= 2 + 22.5 + 9.5 + 4 = 38 u ||dz||, and the quotient by n (7.5 u) adds <= 9.5 u:
    err_row <= u_out ||ref_row|| + 48 u G_row,   G_row = sqrt(sum_heads ||dQ||^2 / n_q^2 + ||dK||^2 / n_k^2 + ||dV||^2)       (counted 47.5)

Attention forward.  KV, ksum, vsum are sums of T = MMDIT_ATTN_COS2_TOKEN_CHUNK sequential fp32 FMAs per chunk and of the chunks in order:
<= (T + nchunks) u relative to the sums of absolute values.  A row adds 64 FMAs over the channels and one addition (vsum, or S) to the
numerator and to the denominator, and one division:
    |out - ref| <= u_out |ref| + (1 + u_out) (T + nchunks + 70) u (m_n + |ref| m_d) / den
    m_n = sum_j (|q| . |k_j| + 1) |v_j|,   m_d = sum_j |q| . |k_j| + S
which the test holds to be inside the cap 2^-14 (m_n + |ref| m_d) / den (+ u_out |ref|) that fp32 sums satisfy and a state rounded to bf16
(2^-9 m) does not (tests/test_cosine2_abi.py).  den itself: |den - ref| <= (S + 70) u m_d.  On the reference, den >= S / 2 on every row of every
case (asserted: the quotient is well conditioned; random unit vectors give >= 0.9 S beyond the shortest sequences).

Attention backward (the formulas of the header on the stored o and den; dn = g / den one rounding, dd = -(g . o) / den a 64-term sum and a
division: <= 12 u relative to A = sum |g||o| / den).  With |dn| = |g| / den:
    dq: m = |dn| (|K|^T |V|)^T + A sum_j |k_j|      dk: m = |v| (|Q|^T |dN|)^T + sum_i A_i |q_i|      dv: m = |k| (|Q|^T |dN|) + sum_i |dn_i|
    |out - ref| <= u_out |ref| + (1 + u_out) (T + nchunks + 80) u m                     (inside the same cap 2^-14 m)

Model: parity mode rel-L2 < 1e-3 against the real reference's fp32 goldens (the project's bar for every configuration); fast mode no worse than
the reference's OWN torch.autocast("cpu", bfloat16) distance from its fp32 output, read from tests/golden/generation_report_cosine2.json.

Measured figures: profiles/cosine2_attention.txt.
"""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle.weights import make_inputs as model_inputs, make_state_dict  # noqa: E402

HD = 64                # MMDIT_COS2_HEAD_DIM (tests/test_cosine2_abi.py checks the three against the header)
T, RT = 128, 64        # MMDIT_ATTN_COS2_TOKEN_CHUNK, MMDIT_ATTN_COS2_ROW_TILE
U = 2.0 ** -8          # bf16 unit roundoff (round to nearest)
E32 = 2.0 ** -24       # fp32 unit roundoff
CAP = 2.0 ** -14       # the cap of the attention bounds
L2_EPS = 1e-12         # F.normalize(eps=1e-12)
BF16, F32 = torch.bfloat16, torch.float32
MICRO = dict(dim=128, num_heads=2, num_blocks=3)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


WORST = {}             # kernel -> output -> (worst ratio to its bound, case id)


def _record(kernel, name, ratio, cid):
    cur = WORST.setdefault(kernel, {}).get(name)
    if cur is None or ratio > cur[0]:
        WORST[kernel][name] = (ratio, cid)


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    for kernel in sorted(WORST):
        print(f"\n[cosine2 worst] {kernel}: " + ", ".join(f"{k} {v[0]:.3f} (@ {v[1]})" for k, v in WORST[kernel].items()))


# ---------------------------------------------------------------------------------------------- float64 restatements (shared with the CPU file)
def l2n(x):
    """x / max(||x||_2, 1e-12) over the last axis (F.normalize)."""
    return x / x.norm(dim=-1, keepdim=True).clamp_min(L2_EPS)


def rotate2(z, cs, sn):
    """z (..., tokens, 64); cs / sn (tokens, 64).  Pairs (2p, 2p + 1): out[2p] = a c[2p] - b s[2p], out[2p+1] = b c[2p+1] + a s[2p+1]."""
    a, b = z[..., 0::2], z[..., 1::2]
    return torch.stack([a * cs[..., 0::2] - b * sn[..., 0::2], b * cs[..., 1::2] + a * sn[..., 1::2]], -1).flatten(-2)


def rotate2_mag(z, cs, sn):
    """The sum of the absolute values of the two terms of each output of rotate2."""
    a, b, cs, sn = z[..., 0::2].abs(), z[..., 1::2].abs(), cs.abs(), sn.abs()
    return torch.stack([a * cs[..., 0::2] + b * sn[..., 0::2], b * cs[..., 1::2] + a * sn[..., 1::2]], -1).flatten(-2)


def rotate2_t(g, cs, sn):
    """The transpose of rotate2 applied to g."""
    g0, g1 = g[..., 0::2], g[..., 1::2]
    return torch.stack([g0 * cs[..., 0::2] + g1 * sn[..., 1::2], g1 * cs[..., 1::2] - g0 * sn[..., 0::2]], -1).flatten(-2)


def cos2_quadratic(q, k, v):
    """The reference's expression (Attention.py:330-339).  Returns out and the row sums den."""
    prod = q @ k.mT + 1
    den = prod.sum(-1, keepdim=True)
    return (prod / den) @ v, den.squeeze(-1)


def cos2_linear(q, k, v):
    """out_i = (q_i KV + vsum) / (q_i . ksum + S)."""
    KV, ksum, vsum = k.mT @ v, k.sum(-2, keepdim=True), v.sum(-2, keepdim=True)
    den = (q * ksum).sum(-1, keepdim=True) + k.shape[-2]
    return (q @ KV + vsum) / den, den.squeeze(-1)


def cos2_backward(q, k, v, o, den, g):
    """The backward formulas of include/mmdit_hip_cos2.h on the given o and den (batch, heads, S, 64) / (batch, heads, S)."""
    d = den.unsqueeze(-1)
    dn, dd = g / d, -(g * o).sum(-1, keepdim=True) / d
    KV, ksum = k.mT @ v, k.sum(-2, keepdim=True)
    dKV, dvsum, dksum = q.mT @ dn, dn.sum(-2, keepdim=True), (dd * q).sum(-2, keepdim=True)
    return dn @ KV.mT + dd * ksum, v @ dKV.mT + dksum, k @ dKV + dvsum


def cos2_backward_mag(q, k, v, o, den, g):
    """The sums of absolute values behind cos2_backward (the m of the bounds)."""
    q, k, v, d = q.abs(), k.abs(), v.abs(), den.unsqueeze(-1)
    dn, A = g.abs() / d, (g.abs() * o.abs()).sum(-1, keepdim=True) / d
    KV, ksum = k.mT @ v, k.sum(-2, keepdim=True)
    dKV, dvsum, dksum = q.mT @ dn, dn.sum(-2, keepdim=True), (A * q).sum(-2, keepdim=True)
    return dn @ KV.mT + A * ksum, v @ dKV.mT + dksum, k @ dKV + dvsum


# ---------------------------------------------------------------------------------------------- 1: the row kernels
def _tables(h2, w2, f=1):
    import sd3_amd  # noqa: F401
    from sd3_amd.blocks.rotary_embedding import RotaryEmbedding
    return RotaryEmbedding(HD // 2, use_xpos=False, interpolate_factor=f).tables(h2, w2, torch.device("cuda:0"))


# (batch, heads, (grid rows, grid columns), text tokens): the list of tests/test_rope2dv2_gpu.py -- 1, 2, 3, 19, 24 heads; one-row and one-column
# grids; fewer chunks (24 * heads per row) than a workgroup of 256 holds; a ragged last workgroup
_SHAPES = [(2, 1, (3, 5), 6), (2, 3, (5, 3), 6), (1, 2, (1, 4), 2), (1, 2, (4, 1), 2), (1, 19, (2, 2), 2), (1, 24, (2, 2), 2)]


class _RowCase:
    """Seeded operands of one (batch, heads, grid, Mt, dtype) and the float64 chain normalise -> rotate.  One query vector of the image stream and
    one key vector of the text stream are rows of zeros (the max(||x||, 1e-12) branch)."""

    def __init__(self, Bt, H, hw, Mt, dtype):
        self.Bt, self.H, self.hw, self.N, self.Mt, self.dtype = Bt, H, hw, hw[0] * hw[1], Mt, dtype
        self.S, self.row = self.N + Mt, 3 * H * HD
        g = torch.Generator().manual_seed(7331 * self.S + 31 * Bt * H + 7 * hw[0])
        rn = lambda *sh: torch.randn(*sh, generator=g)      # noqa: E731
        self.cos, self.sin = _tables(hw[0], hw[1])
        assert self.cos.shape == (self.N, HD) and self.cos.dtype == F32
        qkv_x, qkv_c = rn(Bt * self.N, self.row), rn(Bt * Mt, self.row)
        self.zero_q = (self.N - 1, H - 1)               # (row of the image stream, head): its q vector is zero
        self.zero_k = (Bt * Mt - 1, 0)                  # (row of the text stream, head): its k vector is zero
        qkv_x[self.zero_q[0], self.zero_q[1] * HD:(self.zero_q[1] + 1) * HD] = 0
        qkv_c[self.zero_k[0], (H + self.zero_k[1]) * HD:(H + self.zero_k[1] + 1) * HD] = 0
        self.qkv_x, self.qkv_c = qkv_x.to(dtype).cuda(), qkv_c.to(dtype).cuda()

    def img(self):
        return (self.qkv_x, self.cos, self.sin, self.N, 0)

    def txt(self):
        return (self.qkv_c, None, None, self.Mt, self.N)

    def parts(self, qkv, L):
        """(q, k, v) of rows [q | k | v]: (Bt, H, L, 64) each."""
        return tuple(qkv[:, i * self.H * HD:(i + 1) * self.H * HD].reshape(self.Bt, L, self.H, HD).permute(0, 2, 1, 3) for i in range(3))

    def chain(self, qkv, L, rope):
        q, k, v = self.parts(qkv, L)
        q, k = l2n(q), l2n(k)
        mq, mk = q.abs(), k.abs()
        if rope:
            c, s = self.cos.double(), self.sin.double()
            mq, mk = rotate2_mag(q, c, s), rotate2_mag(k, c, s)
            q, k = rotate2(q, c, s), rotate2(k, c, s)
        return (q, k, v), (mq, mk, v.abs())

    def reference(self):
        (qx, kx, vx), (mqx, mkx, mvx) = self.chain(self.qkv_x.double(), self.N, True)
        (qc, kc, vc), (mqc, mkc, mvc) = self.chain(self.qkv_c.double(), self.Mt, False)
        cat = lambda a, b: torch.cat([a, b], 2)      # noqa: E731
        return dict(Q=cat(qx, qc), K=cat(kx, kc), V=cat(vx, vc)), dict(Q=cat(mqx, mqc), K=cat(mkx, mkc), V=cat(mvx, mvc))

    def outputs(self, sent, dtype):
        return [torch.full((self.Bt, self.H, self.S, HD), sent, dtype=dtype, device="cuda") for _ in range(3)]


def _row_id(s):
    Bt, H, hw, Mt = s
    return f"b{Bt}h{H}-{hw[0]}x{hw[1]}-txt{Mt}"


def _tn(dt):
    return "bf16" if dt == BF16 else "fp32"


@pytest.mark.parametrize("dtype,odtype", [(BF16, BF16), (F32, F32), (F32, BF16), (BF16, F32)], ids=["bf16", "fp32", "fp32-bf16", "bf16-fp32"])
@pytest.mark.parametrize("shape", _SHAPES, ids=_row_id)
def test_rows_fwd(shape, dtype, odtype, ops):
    """Q, K, V of both streams in one launch against the float64 chain, EVERY element under the bound of the module docstring; the rows of zeros give
    zeros; each stream alone at its tok0 writes the same bits and nothing outside its token range; V bit-equal to the rounded raw rows; image
    token (0, 0) is not rotated."""
    Bt, H, hw, Mt = shape
    c = _RowCase(Bt, H, hw, Mt, dtype)
    sent = 123.0
    Q, K, V = c.outputs(sent, odtype)
    ops.qk_l2norm_rope_fwd_pair(c.img(), c.txt(), Bt, H, c.S, Q, K, V)
    ref, mag = c.reference()
    u_out = U if odtype == BF16 else 0.0
    worst = {}
    for name, out in (("Q", Q), ("K", K), ("V", V)):
        assert bool(torch.isfinite(out).all()) and not bool((out == sent).all(-1).any()), (name, "a row was not written")
        bound = u_out * ref[name].abs() + (1 + u_out) * 14 * E32 * mag[name]
        ratio = (out.double() - ref[name]).abs() / bound.clamp_min(1e-300)
        worst[name], worst[name + " text"] = float(ratio.max()), float(ratio[:, :, c.N:].max())
        _record(f"qk_l2norm_rope_fwd {_tn(dtype)}->{_tn(odtype)}", name, worst[name], _row_id(shape))
    print(f"[cosine2 rows fwd {_tn(dtype)}->{_tn(odtype)}] {_row_id(shape)}: worst |out - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= 1.0, (name, v)
    vx, vc = c.parts(c.qkv_x, c.N)[2].to(odtype), c.parts(c.qkv_c, Mt)[2].to(odtype)
    assert torch.equal(V, torch.cat([vx, vc], 2)), "V is not the rounded copy of the v columns"
    rq, hq = c.zero_q
    rk, hk = c.zero_k
    assert bool((Q[rq // c.N, hq, rq % c.N] == 0).all()) and bool((K[rk // Mt, hk, c.N + rk % Mt] == 0).all()), "a row of zeros did not give zeros"
    assert float(Q.double().norm(dim=-1).mean()) > 0.9      # (the rest are unit vectors)
    for st in (c.img(), c.txt()):
        Q1, K1, V1 = c.outputs(sent, odtype)
        tokens, tok0 = st[3], st[4]
        ops.qk_l2norm_rope_fwd_pair(st, None, Bt, H, c.S, Q1, K1, V1)
        for a, b in ((Q1, Q), (K1, K), (V1, V)):
            assert torch.equal(a[:, :, tok0:tok0 + tokens], b[:, :, tok0:tok0 + tokens]), "a single-stream launch differs from the pair launch"
            rest = torch.cat([a[:, :, :tok0], a[:, :, tok0 + tokens:]], 2)
            assert bool((rest == sent).all()), "a single-stream launch wrote outside its token range"
    # image token (0, 0): both angles are zero -- the same launch without tables gives the same bits there and other bits elsewhere
    Qn, Kn, Vn = c.outputs(sent, odtype)
    ops.qk_l2norm_rope_fwd_pair((c.qkv_x, None, None, c.N, 0), None, Bt, H, c.S, Qn, Kn, Vn)
    assert torch.equal(Q[:, :, 0], Qn[:, :, 0]) and torch.equal(K[:, :, 0], Kn[:, :, 0]), "token (0, 0) was rotated"
    if c.N > 1:
        assert not torch.equal(Q[:, :, 1:c.N], Qn[:, :, 1:c.N]), "no token of the image stream was rotated"


@pytest.mark.parametrize("gdtype,dtype", [(BF16, BF16), (F32, F32), (BF16, F32)], ids=["bf16", "fp32", "mixed"])
@pytest.mark.parametrize("shape", _SHAPES, ids=_row_id)
def test_rows_bwd(shape, gdtype, dtype, ops):
    """dqkv rows against the float64 formula dx = (r - z (z . r)) / max(||x||, 1e-12), r = R^T dz, per row under the bound of the module
    docstring (the v columns pass through: bit-equal to the rounded dV); the formula equals float64 autograd through F.normalize -> rotation
    (checked here on the same operands); the three dtype combinations of the entry point; each stream alone gives the same dqkv bits."""
    Bt, H, hw, Mt = shape
    c = _RowCase(Bt, H, hw, Mt, dtype)
    g = torch.Generator().manual_seed(4441 * c.S + H)
    dQ, dK, dV = (torch.randn(Bt, H, c.S, HD, generator=g).to(gdtype).cuda() for _ in range(3))
    dx, dc = ops.qk_l2norm_rope_bwd_pair(dQ, dK, dV, c.img(), c.txt(), Bt, H, c.S, dtype)
    assert dx.dtype == dtype and dx.shape == c.qkv_x.shape and dc.shape == c.qkv_c.shape

    def formula(qkv, L, tok0, rope):
        """(float64 dqkv rows, G_row)"""
        q, k, _ = c.parts(qkv.double(), L)
        outs, G2 = [], 0.0
        for x, dz in ((q, dQ), (k, dK)):
            dz = dz.double()[:, :, tok0:tok0 + L]
            r = rotate2_t(dz, c.cos.double(), c.sin.double()) if rope else dz
            n = x.norm(dim=-1, keepdim=True).clamp_min(L2_EPS)
            z = x / n
            outs.append((r - z * (z * r).sum(-1, keepdim=True)) / n)
            G2 = G2 + (dz.norm(dim=-1) / n.squeeze(-1)) ** 2
        dv = dV.double()[:, :, tok0:tok0 + L]
        outs.append(dv)
        G2 = G2 + dv.norm(dim=-1) ** 2
        rows = torch.cat([t.permute(0, 2, 1, 3).reshape(Bt * L, H * HD) for t in outs], 1)
        return rows, G2.sum(1).sqrt().reshape(Bt * L)

    # the formula is autograd's, wherever the vector is not a row of zeros (there F.normalize's clamp has the gradient dz / eps as well)
    xr, cr = c.qkv_x.double().requires_grad_(True), c.qkv_c.double().requires_grad_(True)
    qx, kx, vx = c.parts(xr, c.N)
    qc, kc, vc = c.parts(cr, Mt)
    cs, sn = c.cos.double(), c.sin.double()
    Qr = torch.cat([rotate2(F.normalize(qx, dim=-1), cs, sn), F.normalize(qc, dim=-1)], 2)
    Kr = torch.cat([rotate2(F.normalize(kx, dim=-1), cs, sn), F.normalize(kc, dim=-1)], 2)
    ((Qr * dQ.double()).sum() + (Kr * dK.double()).sum() + (torch.cat([vx, vc], 2) * dV.double()).sum()).backward()

    tag = "bf16" if dtype == BF16 else "fp32" if gdtype == F32 else "mixed"
    u_out = U if dtype == BF16 else 0.0
    for name, out, qkv, L, tok0, rope, auto in (("dqkv_x", dx, c.qkv_x, c.N, 0, True, xr.grad), ("dqkv_c", dc, c.qkv_c, Mt, c.N, False, cr.grad)):
        rg, G = formula(qkv, L, tok0, rope)
        assert float(((rg - auto).norm(dim=-1) / auto.norm(dim=-1)).max()) < 1e-11, "the backward formula is not autograd's"
        assert bool(torch.isfinite(out).all())
        err, bound = (out.double() - rg).norm(dim=-1), u_out * rg.norm(dim=-1) + 48 * E32 * G
        ratio = err / bound
        print(f"[cosine2 rows bwd {tag}] {_row_id(shape)} {name}: worst row {float(ratio.max()):.3f} of the bound (row {int(ratio.argmax())})")
        _record("qk_l2norm_rope_bwd " + tag, name, float(ratio.max()), _row_id(shape))
        assert float(ratio.max()) <= 1.0, (name, int(ratio.argmax()), float(ratio.max()))
        assert torch.equal(out[:, 2 * H * HD:], rg[:, 2 * H * HD:].to(dtype)), "the v columns did not pass through"
    dx1, = ops.qk_l2norm_rope_bwd_pair(dQ, dK, dV, c.img(), None, Bt, H, c.S, dtype)
    dc1, = ops.qk_l2norm_rope_bwd_pair(dQ, dK, dV, c.txt(), None, Bt, H, c.S, dtype)
    assert torch.equal(dx1, dx) and torch.equal(dc1, dc), "a single-stream launch differs from the pair launch"


# ---------------------------------------------------------------------------------------------- 2: attention
_S = [1, T - 1, T, T + 1, 2 * T + 3, 5 * T + 1]
_BH = [(1, 1), (1, 3), (2, 4), (1, 19)]                 # batch * heads = 1, 3, 8, 19
ATTN_CASES = [(S, bh) for S in _S for bh in _BH]


def n_img_values(S):
    """0, 1, a value inside a chunk and inside a row tile (S / 2 + 5: 68, 69, 69, 134, 325 for the lengths of _S), S - 1, S."""
    inside = S // 2 + 5 if S > 12 else S // 2
    assert S <= 12 or (inside % T and inside % RT and 1 < inside < S - 1)
    return sorted({0, 1, inside, S - 1, S} & set(range(S + 1)))


def _attn_id(case):
    S, (Bt, H) = case
    return f"S{S}-b{Bt}h{H}"


@functools.lru_cache(maxsize=None)
def attn_inputs(S, Bt, H, dtype):
    """Seeded unit-norm q, k (as the row kernel leaves them), v, dO, stored in `dtype`; CPU tensors."""
    g = torch.Generator().manual_seed(1009 * S + 17 * Bt + H)
    rn = lambda: torch.randn(Bt, H, S, HD, generator=g)      # noqa: E731
    q, k, v, dO = l2n(rn()), l2n(rn()), rn(), rn()
    return tuple(t.to(dtype) for t in (q, k, v, dO))


@functools.lru_cache(maxsize=None)
def attn_reference(S, Bt, H, dtype):
    """float64, from the stored operands: out and den of the reference's quadratic expression, the magnitude sums m_n, m_d, and the o / den a
    backward launch is given (the reference's, rounded to the storage dtypes).  Computed once per case and never modified."""
    q, k, v, _ = (t.double() for t in attn_inputs(S, Bt, H, dtype))
    out, den = cos2_quadratic(q, k, v)
    m_n = q.abs() @ (k.abs().mT @ v.abs()) + v.abs().sum(-2, keepdim=True)
    m_d = (q.abs() * k.abs().sum(-2, keepdim=True)).sum(-1) + S
    assert float((den / S).min()) >= 0.5, ("den < S / 2 on the reference: choose another seed", float((den / S).min()))
    lin, lden = cos2_linear(q, k, v)
    assert float((lin - out).abs().max()) < 1e-12 and float((lden - den).abs().max() / S) < 1e-13      # (the linear form is the same function)
    return dict(out=out, den=den, m_n=m_n, m_d=m_d, o_st=out.to(dtype), den_st=den.float())


def _split(x, n_img):
    """(Bt, H, S, 64) -> head-merged Ox (Bt, n_img, H * 64), Oc (Bt, S - n_img, H * 64) (None when empty)."""
    Bt, H, S, _ = x.shape
    m = x.permute(0, 2, 1, 3).reshape(Bt, S, H * HD)
    return (m[:, :n_img].contiguous() if n_img else None), (m[:, n_img:].contiguous() if n_img < S else None)


def _merge(Ox, Oc, H):
    parts = [t for t in (Ox, Oc) if t is not None]
    m = torch.cat(parts, 1)
    return m.reshape(m.shape[0], m.shape[1], H, HD).permute(0, 2, 1, 3)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", ATTN_CASES, ids=_attn_id)
def test_attn_fwd(case, dtype, ops):
    """Every element of O under the bound of the module docstring (itself inside the 2^-14 cap), den to (S + 70) u m_d, for every split n_img of the
    joint sequence (the outputs of all splits hold the same bits); a second launch on the same operands is bit-equal."""
    S, (Bt, H) = case
    ref = attn_reference(S, Bt, H, dtype)
    Q, K, V, _ = (t.cuda() for t in attn_inputs(S, Bt, H, dtype))
    nchunks = (S + T - 1) // T
    Kf = T + nchunks + 70
    assert Kf * E32 <= CAP
    u_out = U if dtype == BF16 else 0.0
    first = None
    for n_img in n_img_values(S):
        Ox, Oc, den = ops.attn_cos2_fwd(Q, K, V, n_img)
        assert (Ox is None) == (n_img == 0) and (Oc is None) == (n_img == S) and den.dtype == F32
        assert all(t is None or t.dtype == dtype for t in (Ox, Oc))
        O = _merge(Ox, Oc, H)
        if first is None:
            first = (O.clone(), den.clone())
            o, d = O.double().cpu(), den.double().cpu()
            assert bool(torch.isfinite(o).all())
            core = (ref["m_n"] + ref["out"].abs() * ref["m_d"].unsqueeze(-1)) / ref["den"].unsqueeze(-1)
            ratio = (o - ref["out"]).abs() / (u_out * ref["out"].abs() + (1 + u_out) * Kf * E32 * core)
            rcap = ((o - ref["out"]).abs() - u_out * ref["out"].abs()).clamp_min(0) / (CAP * core)
            rden = (d - ref["den"]).abs() / ((S + 70) * E32 * ref["m_d"])
            print(f"[cosine2 attn fwd {_tn(dtype)}] {_attn_id(case)}: worst |O - ref| / bound {float(ratio.max()):.3f}, / cap {float(rcap.max()):.4f}, "
                  f"|den - ref| / bound {float(rden.max()):.4f}; min den / S {float((ref['den'] / S).min()):.3f}")
            _record("attn_cos2_fwd " + _tn(dtype), "O", float(ratio.max()), _attn_id(case))
            _record("attn_cos2_fwd " + _tn(dtype), "O / cap", float(rcap.max()), _attn_id(case))
            _record("attn_cos2_fwd " + _tn(dtype), "den", float(rden.max()), _attn_id(case))
            assert float(ratio.max()) <= 1.0 and float(rden.max()) <= 1.0, (float(ratio.max()), float(rden.max()))
        else:
            assert torch.equal(O, first[0]) and torch.equal(den, first[1]), f"n_img = {n_img} changed the values"
    n_img = n_img_values(S)[len(n_img_values(S)) // 2]
    a, b = ops.attn_cos2_fwd(Q, K, V, n_img), ops.attn_cos2_fwd(Q, K, V, n_img)
    assert all(x is y is None or torch.equal(x, y) for x, y in zip(a, b)), "two launches on the same operands differ"


@pytest.mark.parametrize("dtype,gdtype", [(BF16, BF16), (BF16, F32), (F32, F32)], ids=["bf16", "bf16-fp32grad", "fp32"])
@pytest.mark.parametrize("case", ATTN_CASES, ids=_attn_id)
def test_attn_bwd(case, dtype, gdtype, ops):
    """dQ, dK, dV, every element under the bound of the module docstring (inside the 2^-14 m cap), from the reference's o and den as stored, with
    dOc given (every split n_img: the same bits) and dOc = NULL (the last block: zero gradient for the text rows, every split); two launches
    are bit-equal."""
    S, (Bt, H) = case
    ref = attn_reference(S, Bt, H, dtype)
    Q, K, V, dO = attn_inputs(S, Bt, H, dtype)
    q, k, v, g_all = (t.double() for t in (Q, K, V, dO))
    o, den = ref["o_st"].double(), ref["den_st"].double()
    Qc, Kc, Vc = Q.cuda(), K.cuda(), V.cuda()
    den_c = ref["den_st"].cuda()
    nchunks = (S + T - 1) // T
    Kb = T + nchunks + 80
    assert Kb * E32 <= CAP
    u_out = U if gdtype == BF16 else 0.0
    tag = f"{_tn(dtype)}/{_tn(gdtype)}"

    def check(outs, g, what):
        refs, mags = cos2_backward(q, k, v, o, den, g), cos2_backward_mag(q, k, v, o, den, g)
        res = []
        for name, out, r, m in zip(("dQ", "dK", "dV"), outs, refs, mags):
            out = out.double().cpu()
            assert bool(torch.isfinite(out).all()), name
            err = (out - r).abs()
            ratio = float((err / (u_out * r.abs() + (1 + u_out) * Kb * E32 * m).clamp_min(1e-300)).max())
            res.append((name, ratio))
            _record("attn_cos2_bwd " + tag, name, ratio, f"{_attn_id(case)} {what}")
        print(f"[cosine2 attn bwd {tag}] {_attn_id(case)} {what}: worst |out - ref| / bound " + ", ".join(f"{n} {r:.3f}" for n, r in res))
        for n, r in res:
            assert r <= 1.0, (n, r, what)

    first = None
    for n_img in n_img_values(S):
        Ox, Oc = _split(ref["o_st"].cuda(), n_img)
        dOx, dOc = _split(dO.cuda(), n_img)
        outs = ops.attn_cos2_bwd(Qc, Kc, Vc, Ox, Oc, dOx, dOc, den_c, n_img, gdtype)
        assert all(t.dtype == gdtype and t.shape == Qc.shape for t in outs)
        if first is None:
            first = [t.clone() for t in outs]
            check(outs, g_all, "dOc given")
            again = ops.attn_cos2_bwd(Qc, Kc, Vc, Ox, Oc, dOx, dOc, den_c, n_img, gdtype)
            assert all(torch.equal(a, b) for a, b in zip(outs, again)), "two launches on the same operands differ"
        else:
            assert all(torch.equal(a, b) for a, b in zip(outs, first)), f"n_img = {n_img} changed the values"
        if n_img < S:      # the last block: dOc = NULL means zeros
            g = g_all.clone()
            g[:, :, n_img:] = 0
            check(ops.attn_cos2_bwd(Qc, Kc, Vc, Ox, Oc, dOx, None, den_c, n_img, gdtype), g, f"dOc NULL n_img {n_img}")


def test_backward_formulas_are_autograd_of_the_quadratic_form():
    """On the reference alone (float64, exact o and den): the header's backward formulas are the gradients of the reference's expression."""
    q, k, v, dO = (t.double() for t in attn_inputs(T + 1, 2, 4, F32))
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, den = cos2_quadratic(q, k, v)
    (out * dO).sum().backward()
    for name, a, b in zip(("dq", "dk", "dv"), cos2_backward(q.detach(), k.detach(), v.detach(), out.detach(), den.detach(), dO), (q.grad, k.grad, v.grad)):
        assert float((a - b).abs().max() / b.abs().max()) < 1e-12, name


# ---------------------------------------------------------------------------------------------- 3: argument checks
def test_argument_checks_leave_the_outputs_untouched(ops):
    from sd3_amd import _lib
    Bt, H, hw, Mt = 2, 3, (2, 3), 4
    c = _RowCase(Bt, H, hw, Mt, BF16)
    sent = 7.0

    def refused(fn, *a):
        with pytest.raises(RuntimeError):
            fn(*a)
    Q, K, V = c.outputs(sent, BF16)
    Q32 = torch.full((Bt, H, c.S, 32), sent, dtype=BF16, device="cuda")
    refused(ops.qk_l2norm_rope_fwd_pair, c.img(), c.txt(), Bt, H, c.S, Q32, K, V)                            # a 32-wide Q
    refused(ops.qk_l2norm_rope_fwd_pair, c.img(), c.txt(), Bt, H, c.S, Q, K, V.float())                      # mixed output dtypes
    narrow = torch.zeros(c.N, 32, device="cuda")                                                              # the table of the qk_half kernels
    refused(ops.qk_l2norm_rope_fwd_pair, (c.qkv_x, narrow, narrow, c.N, 0), c.txt(), Bt, H, c.S, Q, K, V)
    refused(ops.qk_l2norm_rope_fwd_pair, (c.qkv_x, c.cos[:-1], c.sin[:-1], c.N, 0), c.txt(), Bt, H, c.S, Q, K, V)
    refused(ops.qk_l2norm_rope_fwd_pair, (c.qkv_x, c.cos, None, c.N, 0), c.txt(), Bt, H, c.S, Q, K, V)
    refused(ops.qk_l2norm_rope_fwd_pair, c.img(), (c.qkv_c, None, None, Mt, c.N + 1), Bt, H, c.S, Q, K, V)   # tokens past s_total
    refused(ops.qk_l2norm_rope_fwd_pair, (c.qkv_x[:, :2 * H * HD].contiguous(), c.cos, c.sin, c.N, 0), c.txt(), Bt, H, c.S, Q, K, V)      # qk_half rows
    dQ = torch.zeros(Bt, H, c.S, HD, device="cuda")
    refused(ops.qk_l2norm_rope_bwd_pair, dQ, dQ, dQ, c.img(), (c.qkv_c, None, None, Mt, c.N + 1), Bt, H, c.S, BF16)
    refused(ops.qk_l2norm_rope_bwd_pair, dQ, dQ, dQ[..., :32].contiguous(), c.img(), c.txt(), Bt, H, c.S, BF16)
    # the attention wrappers
    Sa, na = 40, 33
    Qa, Ka, Va, dOa = (t.cuda() for t in attn_inputs(Sa, 1, 2, BF16))
    refused(ops.attn_cos2_fwd, Qa[..., :32].contiguous(), Ka, Va, na)
    refused(ops.attn_cos2_fwd, Qa, Ka.float(), Va, na)
    refused(ops.attn_cos2_fwd, Qa, Ka, Va, Sa + 1)
    refused(ops.attn_cos2_fwd, Qa, Ka, Va, -1)
    refused(ops.attn_cos2_fwd, Qa.to(torch.float16), Ka.to(torch.float16), Va.to(torch.float16), na)
    outs = [Q, K, V]

    # the entry points themselves: error codes of the header, nothing launched
    probs = (_lib.QkProblem * 2)()
    dx, dc = torch.full_like(c.qkv_x, sent), torch.full_like(c.qkv_c, sent)

    def fill(tok0_txt=c.N):
        for q, (qkv, rc, rs, tokens, tok0), dq in zip(probs, (c.img(), (c.qkv_c, None, None, Mt, tok0_txt)), (dx, dc)):
            q.qkv, q.wq, q.wk, q.tokens, q.tok0 = qkv.data_ptr(), None, None, tokens, tok0      # (no norm weights: NULL)
            q.rope_cos, q.rope_sin = (rc.data_ptr(), rs.data_ptr()) if rc is not None else (None, None)
            q.dqkv, q.dwq, q.dwk = dq.data_ptr(), None, None
    fill()
    st, L = torch.cuda.current_stream().cuda_stream, _lib.lib()
    q3 = [t.data_ptr() for t in (Q, K, V)]
    fwd = lambda count=2, dt=_lib.BF16, ot=_lib.BF16, S=c.S, q3=q3, b=Bt, h=H: L.mmdit_qk_l2norm_rope_fwd(probs, count, dt, ot, b, h, S, *q3, st)      # noqa: E731
    bwd = lambda count=2, dts=(_lib.BF16,) * 3, S=c.S, q3=q3, b=Bt, h=H: L.mmdit_qk_l2norm_rope_bwd(probs, count, *q3, *dts, b, h, S, st)      # noqa: E731
    assert fwd(dt=_lib.FP8) == _lib.ERR_DTYPE and fwd(ot=_lib.FP8) == _lib.ERR_DTYPE
    assert bwd(dts=(_lib.F32, _lib.BF16, _lib.BF16)) == _lib.ERR_DTYPE and bwd(dts=(_lib.BF16, _lib.BF16, _lib.F32)) == _lib.ERR_DTYPE
    assert fwd(count=0) == _lib.ERR_ARG and fwd(count=3) == _lib.ERR_ARG and bwd(count=3) == _lib.ERR_ARG and fwd(b=0) == _lib.ERR_ARG and bwd(h=0) == _lib.ERR_ARG
    assert fwd(q3=[q3[0], None, q3[2]]) == _lib.ERR_ARG and bwd(q3=[q3[0], q3[1], None]) == _lib.ERR_ARG
    assert fwd(S=c.S - 1) == _lib.ERR_ARG and bwd(S=c.S - 1) == _lib.ERR_ARG
    fill(tok0_txt=c.N + 1)
    assert fwd() == _lib.ERR_ARG and bwd() == _lib.ERR_ARG
    probs[0].rope_sin = None
    assert fwd(count=1) == _lib.ERR_ARG and bwd(count=1) == _lib.ERR_ARG
    fill()
    probs[1].dqkv = None
    assert bwd() == _lib.ERR_ARG
    # attention
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    Ox, Oc = torch.full((1, na, 2 * HD), sent, dtype=BF16, device="cuda"), torch.full((1, Sa - na, 2 * HD), sent, dtype=BF16, device="cuda")
    den = torch.full((1, 2, Sa), sent, device="cuda")
    assert L.mmdit_attn_cos2_ws_bytes(1, 2, Sa) == 2 * 2 * ((2 * 64 * 64 + 128) + 1 * (64 * 64 + 128)) * 4
    assert L.mmdit_attn_cos2_ws_bytes(0, 2, Sa) == 0 and L.mmdit_attn_cos2_ws_bytes(1, 2, 0) == 0
    assert L.mmdit_attn_cos2_ws_bytes(3, 5, T + 1) == 2 * 15 * ((2 * 64 * 64 + 128) + 2 * (64 * 64 + 128)) * 4
    ws = torch.full((L.mmdit_attn_cos2_ws_bytes(1, 2, Sa) // 4,), sent, device="cuda")
    af = lambda **kw: L.mmdit_attn_cos2_fwd(*[kw.get(k, v) for k, v in (("Q", p(Qa)), ("K", p(Ka)), ("V", p(Va)), ("dt", _lib.BF16), ("batch", 1), ("heads", 2), ("S", Sa),      # noqa: E731
                                                                        ("n_img", na), ("Ox", p(Ox)), ("Oc", p(Oc)), ("ot", _lib.BF16), ("den", p(den)), ("ws", p(ws)), ("stream", st))])
    assert af(Q=None) == _lib.ERR_ARG and af(den=None) == _lib.ERR_ARG and af(ws=None) == _lib.ERR_ARG and af(batch=0) == _lib.ERR_ARG and af(heads=-1) == _lib.ERR_ARG
    assert af(Oc=None) == _lib.ERR_ARG and af(Ox=None) == _lib.ERR_ARG          # (a stream without its output)
    assert af(S=0) == _lib.ERR_SHAPE and af(n_img=-1) == _lib.ERR_SHAPE and af(n_img=Sa + 1) == _lib.ERR_SHAPE
    assert af(dt=_lib.F32) == _lib.ERR_DTYPE and af(ot=_lib.F32) == _lib.ERR_DTYPE and af(dt=_lib.FP8, ot=_lib.FP8) == _lib.ERR_DTYPE
    dOx, dOc = _split(dOa, na)
    gQ, gK, gV = (torch.full(t.shape, sent, dtype=BF16, device="cuda") for t in (Qa, Ka, Va))
    ab = lambda **kw: L.mmdit_attn_cos2_bwd(*[kw.get(k, v) for k, v in (("Q", p(Qa)), ("K", p(Ka)), ("V", p(Va)), ("dt", _lib.BF16), ("Ox", p(Ox)), ("Oc", p(Oc)), ("dOx", p(dOx)),      # noqa: E731
                                                                        ("dOc", p(dOc)), ("ot", _lib.BF16), ("den", p(den)), ("batch", 1), ("heads", 2), ("S", Sa), ("n_img", na),
                                                                        ("dQ", p(gQ)), ("dK", p(gK)), ("dV", p(gV)), ("gt", _lib.BF16), ("ws", p(ws)), ("stream", st))])
    assert ab(gt=2) == _lib.ERR_DTYPE and ab(gt=-1) == _lib.ERR_DTYPE and ab(dt=_lib.F32) == _lib.ERR_DTYPE and ab(dt=_lib.F32, ot=_lib.F32) == _lib.ERR_DTYPE
    assert ab(dQ=None) == _lib.ERR_ARG and ab(den=None) == _lib.ERR_ARG and ab(ws=None) == _lib.ERR_ARG and ab(Oc=None) == _lib.ERR_ARG and ab(dOx=None) == _lib.ERR_ARG
    assert ab(S=0) == _lib.ERR_SHAPE and ab(n_img=Sa + 1) == _lib.ERR_SHAPE and ab(n_img=-1) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    for t in outs + [dx, dc, Ox, Oc, den, ws, gQ, gK, gV]:
        assert bool((t == sent).all()), "a refused launch wrote to its outputs"


# ---------------------------------------------------------------------------------------------- 4: the model against the reference's golden
_net = {}


def own_state_dict(net, cfg=MICRO):
    """The seeded synthetic weights of oracle/weights.py restricted to the model's own keys (tools/make_goldens_cosine2.py): the plain model's
    minus the q_norm_* / k_norm_* weights."""
    sd = make_state_dict(0, MLP_type="swiglu", **cfg)
    return {k: sd[k].clone() for k in net.state_dict()}


def _new_model(**kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    net = diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="cosine2", MLP_type="swiglu", device=torch.device("cuda:0"),
                     positional_encoding="RoPE2d", **MICRO, **kw)
    net.load_state_dict(own_state_dict(net), strict=True)
    return net


def build(precision):
    if "micro" not in _net:
        _net["micro"] = _new_model(checkpoint_MLP=False, checkpoint_attn=False)
    return _net["micro"].set_precision(precision)


def _checksum(*ts):
    return [float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts]


def fwd_bar(precision, case):
    """parity: rel-L2 < 1e-3 against the reference golden (the project's bar for every configuration); fast: the reference's own
    torch.autocast("cpu", bfloat16) distance from its fp32 output on that case, as tools/make_goldens_cosine2.py recorded it."""
    if precision == "parity":
        return 1e-3
    with open(os.path.join(GOLD, "generation_report_cosine2.json")) as f:
        return json.load(f)[{"square": "forward", "16x24": "forward_nonsquare"}[case]]["bf16_autocast_vs_fp32"]


_FWD_CASES = [("square", "forward_micro_cosine2.npz", 0, 16, 16, 1.0, [0.3, 0.7], None),
              ("16x24", "forward_micro_cosine2_nonsquare.npz", 2, 16, 24, 30.0, [0.5, 0.5], ([0, 0], [1, 0], [0, 0]))]


@pytest.mark.parametrize("precision", ["parity", "fast"])
@pytest.mark.parametrize("case", _FWD_CASES, ids=[c[0] for c in _FWD_CASES])
def test_model_forward_vs_reference_golden(case, precision, golden_dir):
    """diff_model.forward (the engine route) against the reference run with attn_type="cosine2"."""
    name, file, seed, h, w, tscale, tvals, nulls = case
    gold = np.load(os.path.join(golden_dir, file))
    x, c, cp = model_inputs(seed, 2, h, w, text_scale=tscale)
    assert np.allclose(gold["inputs_checksum"], _checksum(x, c, cp), rtol=1e-9), "seeded inputs drifted from the fixture"
    nl = [] if nulls is None else [torch.tensor(n).bool() for n in nulls]
    net = build(precision)
    assert all(b.attn.cos2 and not hasattr(b.attn, "q_norm_x") and not hasattr(b.attn, "scale") for b in net.blocks)
    with torch.no_grad():
        v = net(x.cuda(), torch.tensor(tvals), c.cuda(), cp.cuda(), *nl)
    r, bar = rel(v, torch.from_numpy(gold["v"])), fwd_bar(precision, name)
    print(f"[cosine2 {precision}] {name}: forward rel-L2 vs reference golden = {r:.3e} (bar {bar:.3e}) = {r / bar:.3f} of the bar")
    assert bool(torch.isfinite(v).all()) and r <= bar, r


@pytest.mark.parametrize("precision", ["parity", "fast"])
def test_model_gradients_vs_reference_golden(precision, golden_dir):
    """loss = v.pow(2).mean() on the inputs of grads_micro.npz, gradients against the reference's (cosine2) own, in the structure and with the bars
    of tests/test_qk_half_gpu.py::test_model_gradients_vs_reference_golden:
      parity  loss within 2e-3 relative, 8 seeded samples per tensor within 6e-2 of a typical element, the stored (<= 4096-element) tensors
              rel-L2 < 3e-2, gradient norms of the tensors < 3e-2 and of the three scalar parameters < 1e-1;
      fast    bf16 rounding of the whole path against an fp32 reference: the yardstick is that rounding itself, the plain RoPE2d softmax model in
              fast mode, same seeded weights and inputs, against ITS reference golden (grads_micro.npz), measured in this run.  The option must
              not move the model farther from its reference than 1.5 x that: worst stored-tensor rel-L2, worst tensor gradient-norm error, worst
              sample error, and the worst gradient-norm error of the three scalar parameters (worst against worst).
    Every figure is printed before anything is asserted."""
    gold = np.load(os.path.join(golden_dir, "forward_micro_cosine2.npz"))
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
    assert len(rows) == 97      # (the plain model's 109 minus the twelve norm weights)
    tens = [r for r in rows if r[1] > 1]
    worst = lambda rws, k: max(r[k] for r in rws if r[k] is not None)      # noqa: E731
    print(f"[cosine2 {precision}] gradient case: loss {loss:.6f} vs {float(gold['grad_loss']):.6f} (rel {abs(loss - float(gold['grad_loss'])) / abs(float(gold['grad_loss'])):.3e}), "
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
        print(f"[cosine2 fast] the plain RoPE2d model in fast mode against grads_micro.npz: worst relative grad-norm error {worst(bt, 2):.3e}, worst sample / typical {worst(bt, 3):.3e}, "
              f"worst stored-tensor rel-L2 {worst(bt, 4):.3e}; scalars (norm error): " + ", ".join(f"{r[0]} {r[2]:.3e}" for r in base if r[1] == 1))
        print(f"[cosine2 fast] cosine2 / plain: stored-tensor rel-L2 {worst(tens, 4) / worst(bt, 4):.3f}, grad-norm error {worst(tens, 2) / worst(bt, 2):.3f}, "
              f"sample error {worst(tens, 3) / worst(bt, 3):.3f} (bar 1.5)")
        sc, bsc = max(r[2] for r in rows if r[1] == 1), max(r[2] for r in base if r[1] == 1)
        print(f"[cosine2 fast] scalars, worst gradient-norm error: {sc:.3e} against the plain model's {bsc:.3e} = {sc / bsc:.3f} (bar 1.5)")
        assert worst(tens, 4) <= 1.5 * worst(bt, 4), (worst(tens, 4), worst(bt, 4))
        assert worst(tens, 2) <= 1.5 * worst(bt, 2), (worst(tens, 2), worst(bt, 2))
        assert worst(tens, 3) <= 1.5 * worst(bt, 3), (worst(tens, 3), worst(bt, 3))
        assert sc <= 1.5 * bsc, (sc, bsc)


@pytest.mark.parametrize("precision", ["parity", "fast"])
def test_attention_module_route_vs_golden_and_engine_route(precision, golden_dir, monkeypatch):
    """The stand-alone Attention module (blocks/Attention.py, the autograd route) of block 0:
      * on the reference's own block-0 inputs (forward_micro_plain.npz's norm1 taps: nothing in front of the first attention depends on the
        option) against the reference's attention taps: parity mode < 1e-3 (fast mode: held to the forward's fast-mode bar);
      * on the engine route's OWN block-0 inputs (captured from diff_model.forward) the attention core's outputs of the two routes agree:
        rel-L2 < 1e-3, max-abs <= 2e-3 max|b| + 1e-6;
      * BACKWARD, the same bar: block 0's gradient of the two out-projection outputs is captured from the model's backward and fed to the
        stand-alone module's backward; the two routes' gradients of the attention inputs and of every attention parameter of block 0 agree.
    Spies: every block took the new row-kernel and attention launches in both directions and none of the fused or plain ones."""
    from sd3_amd import engine, ops
    gold = np.load(os.path.join(golden_dir, "forward_micro_cosine2.npz"))
    plain = np.load(os.path.join(golden_dir, "forward_micro_plain.npz"))
    net = build(precision)
    b0 = net.blocks[0]
    assert b0.attn.cos2 and b0.attn.precision == precision
    x, c, cp = model_inputs(0, 2, 16, 16, text_scale=1.0)
    n1x, n1c = torch.from_numpy(plain["tap_norm1_x"]).cuda(), torch.from_numpy(plain["tap_norm1_c"]).cuda()
    with torch.no_grad():
        ax, ac = b0.attn(n1x, n1c, x.shape)
    rx, rc = rel(ax, torch.from_numpy(gold["tap_attn_x"])), rel(ac, torch.from_numpy(gold["tap_attn_c"]))
    bar = fwd_bar(precision, "square")
    print(f"[cosine2 {precision}] stand-alone Attention vs reference taps: attn_x {rx:.3e}, attn_c {rc:.3e} (bar {bar:.2e})")
    assert rx <= bar and rc <= bar

    seen, groups, real_block_fwd, real_group = [], [], engine.block_fwd, engine._group
    launches = []

    def spy(*a, **kw):
        out = real_block_fwd(*a, **kw)
        if not seen:          # (clones: the step's buffers go back to the pool)
            sv = out[2]
            seen.append({k: getattr(sv, k).clone() for k in ("ln1x", "ln1c", "Ox", "Oc", "den")})
        return out

    def spy_group(m, problems, **kw):
        outs = real_group(m, problems, **kw)
        groups.append(([(p["A"].clone(), p["B"].data_ptr(), bool(p.get("b_kmajor")), bool(p.get("a_kmajor"))) for p in problems], [o.clone() for o in outs]))
        return outs

    def tag(name):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, **kw: (launches.append(name), real(*a, **kw))[1])
    B, N, Mt, d = 2, 64, 154, 128
    net.zero_grad()
    monkeypatch.setattr(engine, "block_fwd", spy)
    monkeypatch.setattr(engine, "_group", spy_group)
    new = ["qk_l2norm_rope_fwd_pair", "attn_cos2_fwd", "attn_cos2_bwd", "qk_l2norm_rope_bwd_pair"]
    old = ["gemm_qkv_norm_rope", "attn_bwd_qk", "attn_fwd", "attn_bwd", "qk_norm_rope_fwd_pair", "qk_norm_rope_bwd_pair", "qk_norm_rope_fwd", "qk_norm_rope_bwd",
           "qk_norm_rope3_fwd_pair", "qk_norm_rope3_bwd_pair", "qk_norm_rope_fwd_merge_pair", "qk_norm_rope_bwd_merge_pair", "qk_norm_rope_fwd_qkhalf_pair",
           "qk_norm_rope_bwd_qkhalf_pair", "attn_fwd_qkhalf", "attn_bwd_qkhalf", "attn_fwd_e4m3", "attn_fwd_mx"]
    for name in new + old:
        tag(name)
    v = net(x.cuda(), torch.tensor([0.3, 0.7]), c.cuda(), cp.cuda())
    v.pow(2).sum().backward()
    monkeypatch.undo()
    assert launches == new[:2] * 3 + new[2:] * 3, launches      # every block took the new launches, in both directions, and none of the others
    sv = seen[0]
    T_act = torch.bfloat16 if precision == "fast" else torch.float32
    assert sv["Ox"].dtype == sv["Oc"].dtype == T_act and sv["den"].dtype == torch.float32
    attn_params = [(n, p) for n, p in b0.attn.named_parameters() if p.requires_grad]
    eng_grads = {n: p.grad.detach().clone() for n, p in attn_params}
    assert len(eng_grads) == 8 and all(float(gr.abs().max()) > 0 for gr in eng_grads.values())
    w0 = b0.attn.weights(net._mode())
    assert w0.Wqkv_x.shape == (3 * d, d) and w0.cos2 and not hasattr(w0, "wq_x")
    dgrad = lambda ptr: [(ins, outs) for ins, outs in groups if ins[0][1] == ptr and ins[0][2] and not ins[0][3]]      # noqa: E731
    (do_in, _), = dgrad(w0.Wo_x.data_ptr())              # block 0's dO launch: A = d(out-projection outputs)
    (_, dln1), = dgrad(w0.Wqkv_x.data_ptr())             # block 0's dln1 launch: the gradients of the attention inputs
    dacc_x, dacc_c = do_in[0][0], do_in[1][0]
    net.zero_grad()

    cores, real_attn_fwd = [], ops.attn_cos2_fwd
    monkeypatch.setattr(ops, "attn_cos2_fwd", lambda *a, **kw: (cores.append(real_attn_fwd(*a, **kw)), cores[-1])[1])
    xin, cin = sv["ln1x"].float().view(B, N, d).requires_grad_(True), sv["ln1c"].float().view(B, Mt, d).requires_grad_(True)
    ox, oc = b0.attn(xin, cin, x.shape)
    torch.autograd.backward([ox, oc], [dacc_x.float().view(B, N, d), dacc_c.float().view(B, Mt, d)])
    monkeypatch.undo()
    Ox, Oc, den = cores[0]
    pairs = [("Ox", Ox, sv["Ox"]), ("Oc", Oc, sv["Oc"]), ("den", den, sv["den"]),
             ("dX", xin.grad.reshape(B * N, d).to(dln1[0].dtype), dln1[0]), ("dC", cin.grad.reshape(B * Mt, d).to(dln1[1].dtype), dln1[1])]
    pairs += [("grad " + n, p.grad, eng_grads[n]) for n, p in attn_params]
    res = [(name, rel(a, b), float((a.double() - b.double()).abs().max()), float(b.double().abs().max())) for name, a, b in pairs]
    for name, r, mx, bmax in res:
        print(f"[cosine2 {precision}] autograd route vs engine route, block 0 {name}: rel-L2 {r:.3e}, max-abs {mx:.3e} (max|b| {bmax:.3e})")
    for name, r, mx, bmax in res:
        assert bmax > 0 and r < 1e-3 and mx <= 2e-3 * bmax + 1e-6, (name, r, mx)
    net.zero_grad()


def test_inference_forward_and_refusals():
    """The inference forward schedule (no_grad: no saved tensors) takes the new route in both supported precisions; the e4m3 ones are refused, name
    the option and leave the precision as it was; the other options are refused at construction on the GPU model as well."""
    from sd3_amd.models.diff_model import diff_model
    x, c, cp = model_inputs(0, 2, 16, 16, text_scale=1.0)
    outs = {}
    for precision in ("parity", "fast"):
        net = build(precision)
        with torch.no_grad():
            outs[precision] = net(x.cuda(), torch.tensor([0.3, 0.7]), c.cuda(), cp.cuda())
    assert rel(outs["fast"], outs["parity"]) < 1.5 * fwd_bar("fast", "square")
    for args, kw in ((("fp8",), {}), (("mxfp8",), {}), (("fp8",), dict(attention="e4m3"))):
        with pytest.raises(RuntimeError, match="cosine2"):
            _net["micro"].set_precision(*args, **kw)
        assert _net["micro"].precision == "fast"
    base = dict(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="cosine2", MLP_type="swiglu", device=torch.device("cuda:0"), positional_encoding="RoPE2d", **MICRO)
    for bad in (dict(kv_merge_attn=True), dict(qk_half_dim=True), dict(text_loss=True), dict(positional_encoding="RoPE2dV2"), dict(dim=256)):
        with pytest.raises(RuntimeError, match="cosine2"):
            diff_model(**{**base, **bad})
    with pytest.raises(RuntimeError, match="attn_type must be"):
        diff_model(**{**base, "attn_type": "cosine"})


# ---------------------------------------------------------------------------------------------- 5: sampler, training step
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
        print(f"[cosine2 sampler] {precision}: rel-L2 vs the plain loop = {rel(img, ref):.3e}")
        assert img.shape == (B, 16, 16, 16) and bool(torch.isfinite(img).all())
        assert torch.equal(img, ref), (precision, rel(img, ref))


def test_graph_replay_matches_eager_steps(tmp_path):
    """tests/test_model_gpu.py::test_graph_replay_matches_eager_steps with the option on: three eager warm-up steps, snapshot, steps 4-6 eager,
    restore, capture, steps 4-6 replayed.  The loss of step 4 is bit-identical, the later losses and the final parameters agree to the
    run-to-run noise of the backward pass (that test's bars: rel-L2 < 1e-3, max-abs <= 2e-3 max|b| + 1e-6)."""
    import sd3_amd  # noqa: F401
    from sd3_amd import engine, packing
    from sd3_amd.model_trainer import model_trainer

    overlap = engine._WG_OVERLAP
    try:
        engine._WG_OVERLAP = False
        torch.manual_seed(0)
        net = _new_model()
        tr = model_trainer(net, batchSize=4, accumulation_steps=1, totalSteps=100, lr=1e-3, ema_update_freq=1, ema_decay=0.9, warmup_steps=8,
                           use_lr_scheduler=False, device=torch.device("cuda:0"), saveDir=str(tmp_path), numSaveSteps=100, null_prob_pooled=0.1,
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
    print(f"[cosine2 graph] eager losses {l0}  replayed {l1}; parameters: worst rel-L2 {worst[0]:.3e} (bar 1e-3)")
    assert all(math.isfinite(v) for v in l0 + l1)
    assert lr0 == lr1 and l0[0] == l1[0] and np.allclose(l0, l1, rtol=1e-3)
    for a, b in zip(p0, p1):
        assert rel(a, b) < 1e-3 and float((a - b).abs().max()) <= 2e-3 * float(b.abs().max()) + 1e-6
    assert abs(l0[2] - l0[0]) > 1e-4 * abs(l0[0])
