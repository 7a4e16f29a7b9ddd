"""Attention micro-benchmark on the MMDiT-B shape (batch 64, 12 heads, 256 image + 154 text tokens, head_dim 64) or `reps B H N M`.
Times forward and backward (prep + dQ + dK/dV launches) with HIP events; checks the outputs against a torch fp32 reference.
python tools/attn_bench.py [reps]
python tools/attn_bench.py --e4m3 [--out=FILE] [reps [B H N M]]: the forward of the e4m3 inference modes instead -- mmdit_attn_fwd_e4m3 (bf16 and MX
outputs) beside mmdit_attn_fwd mode 0 and mmdit_attn_fwd_mx, by default at the sampler's MMDiT-L shape (batch 16, 16 heads, 1024 image + 154 text
tokens); the kernels alternate inside every round, the table gives median and min / max over the rounds and is appended to FILE.
python tools/attn_bench.py --hd128 [--out=FILE] [reps [B H N M]]: forward (mode 0) and backward (bf16 gradients) of the 128-wide kernels (mmdit_attn_fwd_hd128 /
mmdit_attn_bwd_hd128) at B x H x 128 beside the 64-wide kernels at B x 2H x 64 -- the same d and the same FLOPs; default batch 16, 8 heads x 128 against
16 x 64, 1024 image + 154 text tokens.  Same table as --e4m3."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sd3_amd  # noqa: E402,F401
from sd3_amd import ops  # noqa: E402

E4M3 = "--e4m3" in sys.argv
HD128 = "--hd128" in sys.argv
OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), None)
sys.argv = [a for a in sys.argv if not a.startswith("--")]
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B, H, N, M, hd = (16, 16, 1024, 154, 64) if E4M3 else (16, 8, 1024, 154, 128) if HD128 else (64, 12, 256, 154, 64)
if len(sys.argv) > 5:      # python tools/attn_bench.py reps B H N M   (e.g. 20 16 16 1024 154: MMDiT-L 512^2 batch 16)
    B, H, N, M = (int(v) for v in sys.argv[2:6])
S = N + M
g = torch.Generator(device="cuda").manual_seed(0)
rnd = lambda *s: torch.randn(s, generator=g, device="cuda").to(torch.bfloat16)
Q, K, V = rnd(B, H, S, hd), rnd(B, H, S, hd), rnd(B, H, S, hd)
dOx, dOc = rnd(B, N, H * hd), rnd(B, M, H * hd)
scale = hd ** -0.5


def timed(fn):
    for _ in range(3):
        out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / reps * 1e-3


def e4m3_table(rounds=7):
    """Forward kernels of the e4m3 inference modes, alternating inside each round (same inputs, same box, same minute)."""
    import platform
    import statistics
    import time
    kernels = [("mmdit_attn_fwd mode 0 (bf16 MFMA, bf16 out)", lambda: ops.attn_fwd(Q, K, V, N, scale, 0)),
               ("mmdit_attn_fwd_mx (bf16 MFMA, MX out)", lambda: ops.attn_fwd_mx(Q, K, V, N, scale)),
               ("mmdit_attn_fwd_e4m3 (e4m3 MFMA, bf16 out)", lambda: ops.attn_fwd_e4m3(Q, K, V, N, scale)),
               ("mmdit_attn_fwd_e4m3 (e4m3 MFMA, MX out)", lambda: ops.attn_fwd_e4m3(Q, K, V, N, scale, mx=True))]
    t = {name: [] for name, _ in kernels}
    for _ in range(rounds):
        for name, fn in kernels:
            t[name].append(timed(fn)[1] * 1e6)
    fl = 4.0 * B * H * S * S * hd
    lines = [f"{time.strftime('%Y-%m-%d %H:%M')}  {torch.cuda.get_device_name(0)} ({platform.node()})  attention forward, B={B} H={H} S={S} (n_img={N}) head 64, "
             f"{rounds} rounds x {reps} launches per kernel, HIP events; the two existing kernels are the parent commit's (csrc/attention.hip is unchanged)",
             f"{'kernel':<46} {'median us':>10} {'min':>8} {'max':>8} {'TF (median)':>12}"]
    for name, _ in kernels:
        med = statistics.median(t[name])
        lines.append(f"{name:<46} {med:10.1f} {min(t[name]):8.1f} {max(t[name]):8.1f} {fl / med / 1e6:12.1f}")
    # accuracy on a slice of the batch: relative L2 against fp32 attention of the bf16 inputs
    nb = min(B, 2)
    ref = torch.softmax(Q[:nb].float() @ K[:nb].float().transpose(-1, -2) * scale, dim=-1) @ V[:nb].float()
    cat = lambda ox, oc: torch.cat([ox[:nb].view(nb, N, H, hd), oc[:nb].view(nb, M, H, hd)], 1).permute(0, 2, 1, 3).float()
    o0, o8 = cat(*ops.attn_fwd(Q, K, V, N, scale, 0)[:2]), cat(*ops.attn_fwd_e4m3(Q, K, V, N, scale))
    lines.append(f"rel-L2 of O against fp32 attention: bf16 kernel {float((o0 - ref).norm() / ref.norm()):.2e}, e4m3 kernel {float((o8 - ref).norm() / ref.norm()):.2e}")
    print("\n".join(lines))
    if OUT:
        with open(OUT, "a") as f:
            f.write("\n".join(lines) + "\n")


def hd128_table(rounds=7):
    """The 128-wide kernels at (B, H, S, 128) and the 64-wide ones at (B, 2 H, S, 64), alternating inside each round."""
    import platform
    import statistics
    import time
    Q6, K6, V6 = rnd(B, 2 * H, S, 64), rnd(B, 2 * H, S, 64), rnd(B, 2 * H, S, 64)
    f128, f64 = ops.attn_fwd(Q, K, V, N, scale, 0), ops.attn_fwd(Q6, K6, V6, N, 0.125, 0)
    kernels = [(f"mmdit_attn_fwd mode 0        {2 * H:>3} x  64", 1.0, lambda: ops.attn_fwd(Q6, K6, V6, N, 0.125, 0)),
               (f"mmdit_attn_fwd_hd128 mode 0  {H:>3} x 128", 1.0, lambda: ops.attn_fwd(Q, K, V, N, scale, 0)),
               (f"mmdit_attn_bwd -> bf16       {2 * H:>3} x  64", 2.5, lambda: ops.attn_bwd(Q6, K6, V6, f64[0], f64[1], dOx, dOc, f64[2], N, 0.125, torch.bfloat16)),
               (f"mmdit_attn_bwd_hd128 -> bf16 {H:>3} x 128", 2.5, lambda: ops.attn_bwd(Q, K, V, f128[0], f128[1], dOx, dOc, f128[2], N, scale, torch.bfloat16))]
    t = {name: [] for name, _, _ in kernels}
    for _ in range(rounds):
        for name, _, fn in kernels:
            t[name].append(timed(fn)[1] * 1e6)
    fl = 4.0 * B * H * S * S * hd
    lines = [f"{time.strftime('%Y-%m-%d %H:%M')}  {torch.cuda.get_device_name(0)} ({platform.node()})  attention, B={B} S={S} (n_img={N}) d={H * hd}, "
             f"{rounds} rounds x {reps} launches per kernel, HIP events; the 64-wide kernels are the parent commit's (csrc/attention.hip is unchanged)",
             f"{'kernel':<46} {'median us':>10} {'min':>8} {'max':>8} {'TF (median)':>12}"]
    for name, mult, _ in kernels:
        med = statistics.median(t[name])
        lines.append(f"{name:<46} {med:10.1f} {min(t[name]):8.1f} {max(t[name]):8.1f} {mult * fl / med / 1e6:12.1f}")
    nb = min(B, 2)
    ref = torch.softmax(Q[:nb].float() @ K[:nb].float().transpose(-1, -2) * scale, dim=-1) @ V[:nb].float()
    o = torch.cat([f128[0][:nb].view(nb, N, H, hd), f128[1][:nb].view(nb, M, H, hd)], 1).permute(0, 2, 1, 3).float()
    lines.append(f"rel-L2 of O (128 wide) against fp32 attention: {float((o - ref).norm() / ref.norm()):.2e}")
    print("\n".join(lines))
    if OUT:
        with open(OUT, "a") as f:
            f.write("\n".join(lines) + "\n")


if E4M3:
    e4m3_table()
    sys.exit(0)
if HD128:
    hd128_table()
    sys.exit(0)

(Ox, Oc, lse), tf = timed(lambda: ops.attn_fwd(Q, K, V, N, scale, 0))
(dQ, dK, dV), tb = timed(lambda: ops.attn_bwd(Q, K, V, Ox, Oc, dOx, dOc, lse, N, scale, torch.bfloat16))
fl = 4.0 * B * H * S * S * hd
print(f"attn fwd {tf * 1e6:8.1f} us  {fl / tf / 1e12:7.1f} TF   bwd {tb * 1e6:8.1f} us  {2.5 * fl / tb / 1e12:7.1f} TF")

# reference on a slice of the batch (fp32 math on the bf16 inputs)
nb = 4
q, k, v = (t[:nb].float().requires_grad_(True) for t in (Q, K, V))
p = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
o = p @ v                                                     # (nb, H, S, hd)
do = torch.cat([dOx[:nb].view(nb, N, H, hd), dOc[:nb].view(nb, M, H, hd)], 1).permute(0, 2, 1, 3).float()
o.backward(do)
of = torch.cat([Ox[:nb].view(nb, N, H, hd), Oc[:nb].view(nb, M, H, hd)], 1).permute(0, 2, 1, 3).float()
rel = lambda a, b: float((a - b).norm() / b.norm())
print(f"rel err: O {rel(of, o.detach()):.2e}  dQ {rel(dQ[:nb].float(), q.grad):.2e}  dK {rel(dK[:nb].float(), k.grad):.2e}  dV {rel(dV[:nb].float(), v.grad):.2e}")

# attention backward + QK-RMSNorm / RoPE backward: two passes (mmdit_attn_bwd + mmdit_qk_norm_rope_bwd) vs the fused epilogues
d = H * hd
qkv_x, qkv_c = rnd(B * N, 3 * d), rnd(B * M, 3 * d)
wts = [1 + 0.1 * torch.randn(64, generator=g, device="cuda") for _ in range(4)]
ang = torch.rand(N, 64, generator=g, device="cuda") * 6.28
cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
dw = [torch.zeros(64, device="cuda") for _ in range(4)]
dw4 = torch.zeros(256, device="cuda")


def two_pass():
    a, b_, c = ops.attn_bwd(Q, K, V, Ox, Oc, dOx, dOc, lse, N, scale, torch.bfloat16)
    return ops.qk_norm_rope_bwd_pair(a, b_, c, (qkv_x, wts[0], wts[1], cos, sin, N, 0, dw[0], dw[1]), (qkv_c, wts[2], wts[3], None, None, M, N, dw[2], dw[3]), B, H, S, torch.bfloat16)


_, t2 = timed(two_pass)
_, t1 = timed(lambda: ops.attn_bwd_qk(Q, K, V, Ox, Oc, dOx, dOc, lse, N, scale, qkv_x, qkv_c, *wts, cos, sin, dw4))
print(f"attn bwd + qk-norm/rope bwd: two passes {t2 * 1e6:8.1f} us   fused {t1 * 1e6:8.1f} us")
