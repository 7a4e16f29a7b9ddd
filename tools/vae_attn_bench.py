"""VAE mid-block attention (one head of width 512): the fused flash kernel (ops.vae_attention, csrc/vae_attn.hip) against the three-launch path it
replaces (per image: Q K^T GEMM -> row softmax -> P V GEMM, as AutoencoderKL._attn runs it) on the same random bf16 operands.
Cases (tokens, batch): (1024, 16) = 16 images at 256^2, (4096, 16) = 16 images at 512^2, (16384, 2) = 2 images at 1024^2.
Warm-up, then HIP-event timing over enough repeats for >= ~50 ms of work; peak memory of each path with torch.cuda.max_memory_allocated
(operands excluded).  One JSON line per case.
python tools/vae_attn_bench.py [tokens batch]"""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sd3_amd  # noqa: E402,F401
from sd3_amd import ops  # noqa: E402

C = 512
SCALE = 1.0 / math.sqrt(C)
CASES = [(1024, 16), (4096, 16), (16384, 2)]
if len(sys.argv) > 2:
    CASES = [(int(sys.argv[1]), int(sys.argv[2]))]


def three_launch(q, k, v, batch, tokens):
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


def timed(fn):
    """(last output, seconds per call, peak bytes allocated by a call beyond what was live before it)."""
    for _ in range(3):
        out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(5, min(200, int(50.0 / max(e0.elapsed_time(e1), 1e-3))))
    del out
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / reps * 1e-3, torch.cuda.max_memory_allocated() - base


for tokens, batch in CASES:
    g = torch.Generator(device="cuda").manual_seed(tokens + batch)
    q, k, v = (torch.randn(batch * tokens, C, generator=g, device="cuda").to(torch.bfloat16) for _ in range(3))
    of, tf, mf = timed(lambda: ops.vae_attention(q, k, v, batch, tokens, SCALE))
    og, tg, mg = timed(lambda: three_launch(q, k, v, batch, tokens))
    fl = 4.0 * batch * tokens * tokens * C
    diff = float((of.float() - og.float()).norm() / og.float().norm())
    print(json.dumps({"tokens": tokens, "batch": batch, "fused_ms": round(tf * 1e3, 4), "three_launch_ms": round(tg * 1e3, 4),
                      "fused_tflops": round(fl / tf / 1e12, 1), "three_launch_tflops": round(fl / tg / 1e12, 1),
                      "fused_peak_bytes": int(mf), "three_launch_peak_bytes": int(mg), "rel_l2_between_paths": diff}), flush=True)
    del q, k, v, of, og
