"""Attention with pair-averaged keys (kv_merge_attn, mmdit_attn_fwd_kv / mmdit_attn_bwd_kv) next to the unmerged launch at the same S.

Times, with HIP events on one box in one run, at (S, s_kv) = (410, 205), (1178, 589) and (4250, 2125) -- the 256^2, 512^2 and 1024^2
stages plus 154 text tokens, MMDiT-B heads, batch sized to ~26 k tokens --
  the forward (mode 0) and the bf16 backward (one call = the dQ kernel + the dK/dV kernel; the per-kernel split is read from a
  `rocprofv3 --kernel-trace --stats -- python tools/kv_merge_bench.py --shape ...` run of its own: attn_bwd_dq_kernel / attn_bwd_dkv_kernel rows),
  the merging norm / RoPE row kernels next to the plain pair kernels,
each merged launch beside the unmerged one, and the ratio.

  python tools/kv_merge_bench.py [--reps 20] [--rounds 3] [--parent-lib path/to/libmmdit_hip.so]

--parent-lib: alternate the UNMERGED mmdit_attn_fwd / mmdit_attn_bwd of this tree's library and of another build (the parent commit's) at
S = 410 and 4250, `rounds` times each, and print both numbers with the spread between rounds: the existing launches must cost nothing.
Each shape runs in a child process of its own under `timeout` (a fault or a hang in one ends the run there).
"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(410, 205, 256, 64), (1178, 589, 1024, 22), (4250, 2125, 4096, 6)]      # (S, s_kv, n_img, batch)
H, HD = 12, 64


def timed(torch, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def child(args):
    import torch
    sys.path.insert(0, ROOT)
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib, ops
    S, s_kv, N, B = args.shape
    M, d, scale = S - N, H * HD, HD ** -0.5
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda").to(torch.bfloat16)
    Q, K, V, Km, Vm = rnd(B, H, S, HD), rnd(B, H, S, HD), rnd(B, H, S, HD), rnd(B, H, s_kv, HD), rnd(B, H, s_kv, HD)
    dOx, dOc = rnd(B, N, d), rnd(B, M, d)
    bf = torch.bfloat16
    if args.parent_lib:
        # the unmerged launches of two builds, alternating; raw C ABI calls (the other build has no binding of its own)
        libs = {"this": _lib.lib(), "parent": ctypes.CDLL(args.parent_lib)}
        for L in libs.values():
            L.mmdit_attn_fwd.argtypes, L.mmdit_attn_fwd.restype = _lib._SIGNATURES["mmdit_attn_fwd"]
            L.mmdit_attn_bwd.argtypes, L.mmdit_attn_bwd.restype = _lib._SIGNATURES["mmdit_attn_bwd"]
        Ox, Oc, lse = ops.attn_fwd(Q, K, V, N, scale, 0)
        delta, dQ, dK, dV = torch.empty_like(lse), torch.empty_like(Q), torch.empty_like(Q), torch.empty_like(Q)
        st = torch.cuda.current_stream().cuda_stream
        p = lambda t: t.data_ptr()
        res = {k: {"fwd": [], "bwd": []} for k in libs}
        for _ in range(args.rounds):
            for name, L in libs.items():
                def fwd():
                    assert L.mmdit_attn_fwd(p(Q), p(K), p(V), B, H, S, N, scale, 0, p(Ox), p(Oc), p(lse), st) == 0

                def bwd():
                    assert L.mmdit_attn_bwd(p(Q), p(K), p(V), p(Ox), p(Oc), p(dOx), p(dOc), p(lse), p(delta), B, H, S, N, scale, p(dQ), p(dK), p(dV), _lib.BF16, st) == 0
                res[name]["fwd"].append(timed(torch, fwd, args.reps))
                res[name]["bwd"].append(timed(torch, bwd, args.reps))
        for kind in ("fwd", "bwd"):
            a, b = res["this"][kind], res["parent"][kind]
            fmt = lambda v: " ".join(f"{x:8.1f}" for x in v)
            print(f"unmerged {kind} S={S} B={B}: this tree [{fmt(a)}] us   parent [{fmt(b)}] us   medians {sorted(a)[len(a) // 2]:.1f} / {sorted(b)[len(b) // 2]:.1f}   "
                  f"spread between rounds: this {max(a) - min(a):.1f}, parent {max(b) - min(b):.1f} us")
        return
    Ox, Oc, lse = ops.attn_fwd(Q, K, V, N, scale, 0)
    Oxm, Ocm, lsem = ops.attn_fwd(Q, Km, Vm, N, scale, 0, s_kv=s_kv)
    rows = []
    for _ in range(args.rounds):
        rows.append((timed(torch, lambda: ops.attn_fwd(Q, K, V, N, scale, 0), args.reps),
                     timed(torch, lambda: ops.attn_fwd(Q, Km, Vm, N, scale, 0, s_kv=s_kv), args.reps),
                     timed(torch, lambda: ops.attn_bwd(Q, K, V, Ox, Oc, dOx, dOc, lse, N, scale, bf), args.reps),
                     timed(torch, lambda: ops.attn_bwd(Q, Km, Vm, Oxm, Ocm, dOx, dOc, lsem, N, scale, bf, s_kv=s_kv), args.reps)))
    med = [sorted(r[i] for r in rows)[len(rows) // 2] for i in range(4)]
    print(f"S={S} s_kv={s_kv} n_img={N} batch={B} heads={H}: forward unmerged {med[0]:8.1f} us  merged {med[1]:8.1f} us  ratio {med[1] / med[0]:.3f}   "
          f"backward (dQ + dK/dV) unmerged {med[2]:8.1f} us  merged {med[3]:8.1f} us  ratio {med[3] / med[2]:.3f}")
    # the row kernels in front of / behind the attention: plain pair launches vs the merging ones
    qkv_x, qkv_c = rnd(B * N, 3 * d), rnd(B * M, 3 * d)
    w = [1 + 0.1 * torch.randn(64, generator=g, device="cuda") for _ in range(4)]
    ang = torch.rand(N, 64, generator=g, device="cuda") * 6.28
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    dw = [torch.zeros(64, device="cuda") for _ in range(4)]
    img, txt = (qkv_x, w[0], w[1], cos, sin, N, 0), (qkv_c, w[2], w[3], None, None, M, N)
    dQ, dK, dV = rnd(B, H, S, HD), rnd(B, H, S, HD), rnd(B, H, S, HD)
    dKm, dVm = rnd(B, H, s_kv, HD), rnd(B, H, s_kv, HD)
    t = (timed(torch, lambda: ops.qk_norm_rope_fwd_pair(img, txt, B, H, S, Q, K, V), args.reps),
         timed(torch, lambda: ops.qk_norm_rope_fwd_merge_pair(img, txt, B, H, S, Q, Km, Vm), args.reps),
         timed(torch, lambda: ops.qk_norm_rope_bwd_pair(dQ, dK, dV, img + (dw[0], dw[1]), txt + (dw[2], dw[3]), B, H, S, bf), args.reps),
         timed(torch, lambda: ops.qk_norm_rope_bwd_merge_pair(dQ, dKm, dVm, img + (dw[0], dw[1]), txt + (dw[2], dw[3]), B, H, S, bf), args.reps))
    print(f"    norm / RoPE rows: forward plain {t[0]:8.1f} us  merging {t[1]:8.1f} us   backward plain {t[2]:8.1f} us  merging {t[3]:8.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per shape (child process)")
    ap.add_argument("--shape", type=int, nargs=4, default=None, metavar=("S", "S_KV", "N_IMG", "BATCH"), help="one shape in this process (what the parent starts per shape; also the form to put behind rocprofv3 --)")
    args = ap.parse_args()
    if args.shape:
        return child(args)
    shapes = [s for s in SHAPES if s[0] in (410, 4250)] if args.parent_lib else SHAPES
    for s in shapes:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--rounds", str(args.rounds), "--shape"] + [str(v) for v in s]
        if args.parent_lib:
            cmd += ["--parent-lib", args.parent_lib]
        rc = subprocess.run(cmd).returncode
        if rc != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
            print(f"shape {s}: child ended with status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
