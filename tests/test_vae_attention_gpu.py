"""VAE mid-block attention, one batched flash kernel at head width 512 (csrc/vae_attn.hip) through ops.vae_attention.

Reference: float64 softmax(q k^T scale) v of the bf16-rounded operands on the CPU, per image.  Error: rel-L2 of EACH output row, the worst
row of a case counts, no row is left out.  Bar: not a number fixed in advance -- the same per-row error of the three-launch path the
kernel replaces (ops.gemm -> ops.vae_softmax_rows -> ops.gemm per image, as AutoencoderKL._attn runs it) against the same reference; the
fused kernel's worst row must be <= 2 x that path's worst row.  The 2 covers the one rounding point that differs: the fused kernel rounds
the unnormalised P to bf16 and divides by the fp32 row sum at the end, the three-launch path rounds the normalised P.

Shapes: tokens on, one before and one past the 16-query wave, the 32-key tile and the 64-query workgroup, 1 to 32 key tiles, batch 1 and 3
(plain block order) and batch 8 (the XCD-interleaved block order, 1, 2 and 3 query blocks).

Measured, all pairs (worst row of the fused kernel, of the three-launch path): profiles/r08_vae_attention_edge_sweep.txt.  Largest fused worst
row of the sweep 2.709e-03 beside 3.550e-03 (tokens 32, batch 3); largest ratio 0.93 (tokens 65, batch 1: 2.594e-03 beside 2.798e-03).
"""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 512
SCALE = 1.0 / math.sqrt(C)
MARGIN = 2.0


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _reference(q, k, v, batch, tokens):
    """float64 attention of the bf16-rounded operands, per image."""
    qd, kd, vd = (t.double().view(batch, tokens, C) for t in (q, k, v))
    return (torch.softmax(qd @ kd.transpose(1, 2) * SCALE, -1) @ vd).view(batch * tokens, C)


_cases = {}


def _case(tokens, batch):
    """Seeded unit-variance operands (the logits then have unit variance after the 1/sqrt(512) scale) and their reference, computed once."""
    key = (tokens, batch)
    if key not in _cases:
        g = torch.Generator().manual_seed(1000 * tokens + batch)
        q, k, v = (torch.randn(batch * tokens, C, generator=g).to(torch.bfloat16) for _ in range(3))
        _cases[key] = (q, k, v, _reference(q, k, v, batch, tokens))
    return _cases[key]


def _three_launch(ops, q, k, v, batch, tokens):
    """The path the fused kernel replaces, as AutoencoderKL._attn runs it: per image, keys / values zero-padded to a multiple of 8 tokens."""
    o = torch.empty((batch * tokens, C), dtype=torch.bfloat16, device=q.device)
    tp = (tokens + 7) // 8 * 8
    kp, vp = (torch.zeros((tp, C), dtype=torch.bfloat16, device=q.device) for _ in range(2))
    for i in range(batch):
        kp[:tokens].copy_(k[i * tokens:(i + 1) * tokens])
        vp[:tokens].copy_(v[i * tokens:(i + 1) * tokens])
        s = ops.gemm(q[i * tokens:(i + 1) * tokens], kp, out_dtype=torch.float32)
        p = ops.vae_softmax_rows(s, SCALE, cols=tokens)
        ops.gemm(p, vp, b_kmajor=True, out=o[i * tokens:(i + 1) * tokens])
    return o


def _worst_row(out, ref):
    out = out.double().cpu()
    assert bool(torch.isfinite(out).all())
    err = (out - ref).norm(dim=1) / ref.norm(dim=1)
    return float(err.max())


def _check(ops, q, k, v, ref, batch, tokens, tag):
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    fused = _worst_row(ops.vae_attention(qc, kc, vc, batch, tokens, SCALE), ref)
    three = _worst_row(_three_launch(ops, qc, kc, vc, batch, tokens), ref)
    print(f"[vae_attn] {tag} tokens={tokens} batch={batch}: worst row fused {fused:.3e}, three-launch {three:.3e}, ratio {fused / max(three, 1e-300):.2f}")
    assert fused <= MARGIN * three, (tag, tokens, batch, fused, three)


TOKENS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 257, 1000]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("tokens", TOKENS)
def test_tile_edge_sweep(ops, tokens, batch):
    """Largest measured worst-row pair of the sweep (fused, three-launch): 2.709e-03, 3.550e-03 at tokens 32, batch 3; every pair:
    profiles/r08_vae_attention_edge_sweep.txt."""
    q, k, v, ref = _case(tokens, batch)
    _check(ops, q, k, v, ref, batch, tokens, "sweep")


@pytest.mark.parametrize("tokens", [33, 65, 129])
def test_tile_edge_sweep_interleaved_block_order(ops, tokens):
    """batch % 8 == 0 takes the XCD-interleaved block order: 1, 2 and 3 query blocks per image, each with a partial key tile."""
    q, k, v, ref = _case(tokens, 8)
    _check(ops, q, k, v, ref, 8, tokens, "sweep8")


@pytest.mark.parametrize("dominant", [5, 128])
def test_online_softmax_stress(ops, dominant):
    """Logits spanning -40 .. +40 at tokens = 129: every query has one dominant key (+40) -- in the first key tile, or at index 128, the only key
    of the last tile, where the running maximum jumps by ~40 and everything accumulated before it is rescaled to ~0 -- and one key at -40."""
    tokens, batch = 129, 1
    g = torch.Generator().manual_seed(77 + dominant)
    q, k, v = (torch.randn(tokens, C, generator=g) for _ in range(3))
    u = torch.randn(C, generator=g)
    q = q + u
    k[dominant] = 4.0 * u
    k[64] = -4.0 * u
    q = q * (40.0 / float((q @ k.t() * SCALE).abs().max()))
    q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
    logits = q.double() @ k.double().t() * SCALE
    assert float(logits.max()) > 38 and float(logits.min()) < -30 and bool((logits.argmax(1) == dominant).all())
    _check(ops, q, k, v, _reference(q, k, v, batch, tokens), batch, tokens, f"stress dom={dominant}")


def test_batch_isolation(ops):
    """K and V of images 0 and 2 are NaN: image 1 must not see them (its clamped tail rows stay inside its own range, the zeroed V rows of
    its partial tile are zeros whatever lies behind them) and must equal the batch-1 run bit for bit."""
    tokens, batch = 17, 3
    q, k, v, _ = _case(tokens, batch)
    q, k, v = q.cuda(), k.clone().cuda(), v.clone().cuda()
    for t in (k, v):
        t[:tokens] = float("nan")
        t[2 * tokens:] = float("nan")
    out = ops.vae_attention(q, k, v, batch, tokens, SCALE)[tokens:2 * tokens]
    alone = ops.vae_attention(q[tokens:2 * tokens].contiguous(), k[tokens:2 * tokens].contiguous(), v[tokens:2 * tokens].contiguous(), 1, tokens, SCALE)
    assert bool(torch.isfinite(out.float()).all())
    assert torch.equal(out.view(torch.int16), alone.view(torch.int16))


def test_row_pitch(ops):
    """q, k, v as column slices of one contiguous (batch * tokens, 1536) matrix (ld = 1536): bit-identical to the contiguous call."""
    tokens, batch = 65, 2
    q, k, v, _ = _case(tokens, batch)
    qkv = torch.cat([q, k, v], 1).cuda()
    assert qkv.is_contiguous() and qkv.shape == (batch * tokens, 3 * C)
    sliced = ops.vae_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], batch, tokens, SCALE)
    plain = ops.vae_attention(q.cuda(), k.cuda(), v.cuda(), batch, tokens, SCALE)
    assert torch.equal(sliced.view(torch.int16), plain.view(torch.int16))


def test_shape_refusal(ops):
    """C = 256 (and a bad pitch, and tokens < 1) through the raw entry point: MMDIT_ERR_SHAPE, nothing launched (the output keeps its fill)."""
    from sd3_amd import _lib
    fn = _lib.lib().mmdit_vae_attn_fwd
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(64, 512).to(torch.bfloat16).cuda()
    o = torch.full((64, 512), 7.0, dtype=torch.bfloat16, device="cuda")
    assert fn(x.data_ptr(), x.data_ptr(), x.data_ptr(), 256, 1, 64, 256, 0.0625, o.data_ptr(), st) == _lib.ERR_SHAPE
    assert fn(x.data_ptr(), x.data_ptr(), x.data_ptr(), 508, 1, 64, 512, SCALE, o.data_ptr(), st) == _lib.ERR_SHAPE
    assert fn(x.data_ptr(), x.data_ptr(), x.data_ptr(), 516, 1, 32, 512, SCALE, o.data_ptr(), st) == _lib.ERR_SHAPE
    assert fn(x.data_ptr(), x.data_ptr(), x.data_ptr(), 512, 1, 0, 512, SCALE, o.data_ptr(), st) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    with pytest.raises(RuntimeError):
        ops.vae_attention(x[:, :256], x[:, :256], x[:, :256], 1, 64, 0.0625)


_CHILD = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
import sd3_amd  # noqa: F401
from sd3_amd import ops, vae
from oracle import vae_oracle as V
calls = [0]
_orig = ops.vae_attention
def _counted(*a, **k):
    calls[0] += 1
    return _orig(*a, **k)
ops.vae_attention = _counted
net = vae.AutoencoderKL(device="cuda")
net.load_state_dict(V.make_state_dict(0), strict=True)
zs = torch.load(sys.argv[2])
outs = [net.decode(z.cuda()).sample.float().cpu() for z in zs]
torch.cuda.synchronize()
torch.save({"outs": outs, "calls": calls[0], "fused": vae._ATTN_FUSED}, sys.argv[3])
"""


def test_model_level_decode_fused_vs_gemm_path(tmp_path):
    """AutoencoderKL (default channels) decodes a latent with 30 mid-block tokens (5 x 6) and one with a single full key tile (4 x 8 = 32) at B = 2,
    once with the fused kernel and once with MMDIT_VAE_ATTN=gemm (the switch is read at import: a fresh child process each).  The two agree to
    2 x the distance between the three-launch path and oracle/vae_oracle.py, and both stay under the 3e-2 bar of tests/test_vae.py."""
    from oracle import vae_oracle as V
    g = torch.Generator().manual_seed(11)
    zs = [torch.randn(2, 16, 5, 6, generator=g), torch.randn(2, 16, 4, 8, generator=g)]
    zin = str(tmp_path / "z.pt")
    torch.save(zs, zin)
    got = {}
    for mode in ("fused", "gemm"):
        env = dict(os.environ, MMDIT_EXPERIMENTS="1", MMDIT_VAE_ATTN=mode)
        out = str(tmp_path / f"{mode}.pt")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, zin, out], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        got[mode] = torch.load(out)
    assert got["fused"]["fused"] is True and got["fused"]["calls"] == len(zs)        # one call per decode for the whole batch
    assert got["gemm"]["fused"] is False and got["gemm"]["calls"] == 0
    sd, cfg = V.make_state_dict(0), V.VAEConfig()

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    for z, yf, yg in zip(zs, got["fused"]["outs"], got["gemm"]["outs"]):
        yo = V.decode(z, sd, cfg)
        rf, rg, d = rel(yf, yo), rel(yg, yo), rel(yf, yg)
        print(f"[vae_attn] decode {tuple(z.shape)}: fused vs oracle {rf:.3e}, three-launch vs oracle {rg:.3e}, fused vs three-launch {d:.3e}")
        assert yf.shape == yo.shape and rf < 3e-2 and rg < 3e-2
        assert d <= 2.0 * rg
