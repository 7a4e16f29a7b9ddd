"""attn_type="cosine2": the linear-time attention launches (mmdit_attn_cos2_fwd + _bwd, include/mmdit_hip_cos2.h) beside the softmax flash launches
(mmdit_attn_fwd mode 0 + mmdit_attn_bwd) of the same tree, on the same seeded bf16 operands, with HIP events.

python tools/cosine2_bench.py [--out=FILE] [reps]

Shapes: batch 64 x 12 heads (batch * heads = 768) at S = 410 (256 image + 154 text tokens: the MMDiT-B training shape of tools/attn_bench.py) and,
at the same batch, the 1024^2 stage's S = 4250 (4096 + 154).  Per shape the four launches alternate inside every round (same inputs, same box, same
minute); the table gives median and min / max over the rounds, the FLOPs each algorithm needs (softmax: 4 S^2 64 per (batch, head) forward, 2.5 x
that backward; cosine2: the two passes of the forward are 2 x 2 S 64^2, the five of the backward 5 x 2 S 64^2) over the median, and the bytes the
cosine2 launches move at the least (operands, outputs and the workspace's partial states, once each) over the median.  The outputs of the cosine2
launches are compared with fp32 torch on a slice of the batch first.  Reads nothing outside the tree; needs a GPU (no fallback)."""
import os
import platform
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sd3_amd  # noqa: E402,F401
from sd3_amd import _lib, ops  # noqa: E402

OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), None)
argv = [a for a in sys.argv if not a.startswith("--")]
REPS = int(argv[1]) if len(argv) > 1 else 10
ROUNDS = 5
BF16 = torch.bfloat16
HD = _lib.COS2_HEAD_DIM
if not torch.cuda.is_available():
    raise SystemExit("tools/cosine2_bench.py measures on a GPU; none is visible")


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us per call


def shape_table(B, H, N, M, reps):
    S, bh = N + M, B * H
    g = torch.Generator(device="cuda").manual_seed(S)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda")      # noqa: E731
    unit = lambda t: (t / t.norm(dim=-1, keepdim=True)).to(BF16)      # noqa: E731  (what the L2-norm row kernel leaves)
    Q, K, V = unit(rnd(B, H, S, HD)), unit(rnd(B, H, S, HD)), rnd(B, H, S, HD).to(BF16)
    dOx, dOc = rnd(B, N, H * HD).to(BF16), rnd(B, M, H * HD).to(BF16)
    Ox, Oc, den = ops.attn_cos2_fwd(Q, K, V, N)
    dQ, dK, dV = ops.attn_cos2_bwd(Q, K, V, Ox, Oc, dOx, dOc, den, N, BF16)
    # fp32 torch on a slice of the batch: the quadratic form and its autograd
    nb = 1
    q, k, v = (t[:nb].float().requires_grad_(True) for t in (Q, K, V))
    prod = q @ k.mT + 1
    o = (prod / prod.sum(-1, keepdim=True)) @ v
    do = torch.cat([dOx[:nb].view(nb, N, H, HD), dOc[:nb].view(nb, M, H, HD)], 1).permute(0, 2, 1, 3).float()
    o.backward(do)
    of = torch.cat([Ox[:nb].view(nb, N, H, HD), Oc[:nb].view(nb, M, H, HD)], 1).permute(0, 2, 1, 3).float()
    rel = lambda a, b: float((a - b).norm() / b.norm())      # noqa: E731
    check = f"rel-L2 against fp32 torch (quadratic form, autograd; {nb} of {B} samples): O {rel(of, o.detach()):.2e}  dQ {rel(dQ[:nb].float(), q.grad):.2e}  " \
            f"dK {rel(dK[:nb].float(), k.grad):.2e}  dV {rel(dV[:nb].float(), v.grad):.2e}"
    del q, k, v, prod, o, do, of

    scale = HD ** -0.5
    sOx, sOc, lse = ops.attn_fwd(Q, K, V, N, scale, 0)
    fl_soft, fl_pass = 4.0 * bh * S * S * HD, 2.0 * bh * S * HD * HD
    nchunks = -(-S // _lib.ATTN_COS2_TOKEN_CHUNK)
    state = (HD * HD + 2 * HD) * 4
    by_fwd = bh * (3 * S * HD * 2 + S * HD * 2 + S * 4 + 2 * nchunks * state)                      # Q K V in, O and den out, partial states out and in
    by_bwd = bh * (3 * S * HD * 2 * 3 + 2 * S * HD * 2 * 2 + 2 * S * 4 + 3 * S * HD * 2 + 4 * nchunks * state)      # operands per pass, O / dO twice, den, gradients, partials
    kernels = [("mmdit_attn_fwd mode 0 (softmax, flash)", fl_soft, None, lambda: ops.attn_fwd(Q, K, V, N, scale, 0)),
               ("mmdit_attn_cos2_fwd (3 launches)", 2 * fl_pass, by_fwd, lambda: ops.attn_cos2_fwd(Q, K, V, N)),
               ("mmdit_attn_bwd -> bf16 (softmax)", 2.5 * fl_soft, None, lambda: ops.attn_bwd(Q, K, V, sOx, sOc, dOx, dOc, lse, N, scale, BF16)),
               ("mmdit_attn_cos2_bwd -> bf16 (4 launches)", 5 * fl_pass, by_bwd, lambda: ops.attn_cos2_bwd(Q, K, V, Ox, Oc, dOx, dOc, den, N, BF16))]
    t = {name: [] for name, *_ in kernels}
    for _ in range(ROUNDS):
        for name, _, _, fn in kernels:
            t[name].append(timed(fn, reps))
    ws_mb = _lib.lib().mmdit_attn_cos2_ws_bytes(B, H, S) / 2 ** 20
    lines = [f"B={B} H={H} (batch * heads = {bh}) S={S} (n_img={N}) head 64, bf16 operands and outputs; {ROUNDS} rounds x {reps} launches per kernel, HIP events; "
             f"cosine2 workspace {ws_mb:.0f} MiB ({nchunks} chunks of {_lib.ATTN_COS2_TOKEN_CHUNK} tokens)",
             f"{'kernel':<44} {'median us':>10} {'min':>9} {'max':>9} {'TFLOP/s':>9} {'TB/s':>7}"]
    med = {}
    for name, fl, by, _ in kernels:
        med[name] = m = statistics.median(t[name])
        lines.append(f"{name:<44} {m:10.1f} {min(t[name]):9.1f} {max(t[name]):9.1f} {fl / m / 1e6:9.1f} {'' if by is None else f'{by / m / 1e6:7.2f}'}")
    names = [k[0] for k in kernels]
    soft, cos2 = med[names[0]] + med[names[2]], med[names[1]] + med[names[3]]
    lines.append(f"forward + backward: softmax {soft:.1f} us, cosine2 {cos2:.1f} us: cosine2 takes {cos2 / soft:.3f} of the softmax time "
                 f"(forward {med[names[1]] / med[names[0]]:.3f}, backward {med[names[3]] / med[names[2]]:.3f}); algorithmic FLOPs softmax / cosine2 = {3.5 * fl_soft / (7 * fl_pass):.1f}")
    lines.append(check)
    return lines


def main():
    lines = [f"{time.strftime('%Y-%m-%d %H:%M')}  {torch.cuda.get_device_name(0)} ({platform.node()})  tools/cosine2_bench.py: cosine2 (linear-time, fp32 FMA) attention "
             "beside the softmax flash kernels of the same tree"]
    for B, H, N, M, reps in ((64, 12, 256, 154, REPS), (64, 12, 4096, 154, max(2, REPS // 3))):
        lines += [""] + shape_table(B, H, N, M, reps)
        torch.cuda.empty_cache()
    print("\n".join(lines))
    if OUT:
        with open(OUT, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
