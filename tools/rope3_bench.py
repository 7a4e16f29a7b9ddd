"""RoPE2dV2 row kernels at the MMDiT-B block shape (batch 64, 12 heads, N = 256 image + 154 text tokens, bf16): the image + text pair launches
of mmdit_qk_norm_rope3_fwd / _bwd next to the plain mmdit_qk_norm_rope_fwd / _bwd pair launches, which move the same bytes.
python tools/rope3_bench.py [reps] [--cold]
--cold: a 1.5 GB copy runs before every timed call, so the operands come from HBM as they do inside a training step (tools/row_bench.py)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sd3_amd  # noqa: E402,F401
from sd3_amd import ops  # noqa: E402
from sd3_amd.blocks.rotary_embedding_2d_v2 import RoPE2D  # noqa: E402

COLD = "--cold" in sys.argv
_args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(_args[0]) if _args else 50
_flush_src = torch.empty(768 * 2 ** 20, dtype=torch.uint8, device="cuda") if COLD else None
_flush_dst = torch.empty_like(_flush_src) if COLD else None
BF, F32 = torch.bfloat16, torch.float32
B, H, hd, N, Mt = 64, 12, 64, 256, 154
S, d = N + Mt, H * hd
g = torch.Generator(device="cuda").manual_seed(0)
rnd = lambda *s, dt=F32: torch.randn(s, generator=g, device="cuda").to(dt)


def timed(name, fn, nbytes):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        if COLD:
            _flush_dst.copy_(_flush_src)
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) * 1e-3 for e0, e1 in ev)
    t = ts[len(ts) // 2]
    print(f"{name:<40}{t * 1e6:9.1f} us median ({ts[0] * 1e6:.1f} .. {ts[-1] * 1e6:.1f}) {nbytes / t / 1e9:8.0f} GB/s  ({nbytes / 1e6:.0f} MB)", flush=True)
    return t


qkv_x, qkv_c = rnd(B * N, 3 * d, dt=BF), rnd(B * Mt, 3 * d, dt=BF)
w = [1 + 0.1 * rnd(hd) for _ in range(4)]
cos2, sin2 = rnd(N, hd), rnd(N, hd)
cos3, sin3 = RoPE2D(hd).tables(16, 16, torch.device("cuda"))
Q, K, V = (torch.empty(B, H, S, hd, dtype=BF, device="cuda") for _ in range(3))
dQ, dK, dV = (rnd(B, H, S, hd, dt=BF) for _ in range(3))
dw = [torch.zeros(hd, device="cuda") for _ in range(4)]
rows = B * S
fwd_bytes, bwd_bytes = rows * 3 * d * 4, rows * 3 * d * 6      # bf16 read + bf16 write; + the saved projection read again
img = lambda cs, sn, *e: (qkv_x, w[0], w[1], cs, sn, N, 0) + e
txt = lambda *e: (qkv_c, w[2], w[3], None, None, Mt, N) + e
print(f"MMDiT-B block shape: batch {B}, {H} heads x {hd}, {N} image + {Mt} text tokens, bf16; {reps} calls each{', cold operands' if COLD else ''}")
a = timed("qk_norm_rope_fwd  (RoPE2d, pair)", lambda: ops.qk_norm_rope_fwd_pair(img(cos2, sin2), txt(), B, H, S, Q, K, V), fwd_bytes)
b = timed("qk_norm_rope3_fwd (RoPE2dV2, pair)", lambda: ops.qk_norm_rope3_fwd_pair(img(cos3, sin3), txt(), B, H, S, Q, K, V), fwd_bytes)
c = timed("qk_norm_rope_bwd  (RoPE2d, pair)", lambda: ops.qk_norm_rope_bwd_pair(dQ, dK, dV, img(cos2, sin2, dw[0], dw[1]), txt(dw[2], dw[3]), B, H, S, BF), bwd_bytes)
e = timed("qk_norm_rope3_bwd (RoPE2dV2, pair)", lambda: ops.qk_norm_rope3_bwd_pair(dQ, dK, dV, img(cos3, sin3, dw[0], dw[1]), txt(dw[2], dw[3]), B, H, S, BF), bwd_bytes)
print(f"RoPE2dV2 / RoPE2d: forward {b / a:.2f} x, backward {e / c:.2f} x")
