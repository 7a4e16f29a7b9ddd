"""What text_loss costs: the MMDiT-B 256^2 batch-64 training step (bench.py's workload: 12 blocks, d = 768, 12 heads, SwiGLU, RoPE2d, synthetic
data, device RNG, HIP optimizer, the step replayed from a hipGraph) with the option off and on, and the loss kernel alone.

  python tools/text_loss_bench.py [--steps 20] [--rounds 3] [--parent-tree DIR]

step   `off`  = diff_model(text_loss=False), text_loss_weight 0: this tree must launch what the parent commit launches;
       `on`   = diff_model(text_loss=True), text_loss_weight 0.1: a full last block, the text head (forward, data and weight gradient GEMMs over
                9856 x 2304), the loss kernel and the draw of the mask;
       `parent` (--parent-tree DIR: a checkout of the parent commit with its library built) = `off` run from that tree.
       Every configuration is a child process of its own under `timeout` (a fault or a hang in one ends the run there: nothing more is started on
       the GPU); the configurations alternate, `rounds` times each.  A child warms up with 5 eager steps, captures the step, replays 2 steps untimed and
       times `steps` replays between device synchronisations.  Printed: every round, the median and the spread between rounds per configuration --
       a difference between two configurations means something only when it is larger than the spreads.
kernel mmdit_text_loss at 9856 x 2304 (batch 64 x 154 tokens), fp32 prediction, bf16 labels, fp32 gradient, with 0 %, 8 % (= 25 % of the tokens of the
       31.6 % null-conditioned halves), 25 % and 100 % of the rows masked: time per call (HIP events around 10 replays of a hipGraph of 20 calls) and effective GB/s = the bytes the
       algorithm needs (every gradient row stored, the masked rows of prediction and labels loaded) over that time.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_CFG = dict(dim=768, num_heads=12, num_blocks=12)      # bench.py's MMDiT-B
ROWS, COLS = 64 * 154, 2304


def child_step(args):
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import contextlib
    import tempfile
    import time
    import torch
    import sd3_amd  # noqa: F401
    from sd3_amd.model_trainer import model_trainer
    from sd3_amd.models.diff_model import diff_model
    on = args.child == "on"
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    net = diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=dev,
                     positional_encoding="RoPE2d", checkpoint_MLP=False, checkpoint_attn=False, **({"text_loss": True} if on else {}), **B_CFG)
    with contextlib.redirect_stdout(sys.stderr):
        tr = model_trainer(net, batchSize=64, accumulation_steps=1, totalSteps=10 ** 9, lr=1e-4, ema_update_freq=10 ** 9, ema_decay=0.999, warmup_steps=1000,
                           use_lr_scheduler=False, device=dev, saveDir=tempfile.mkdtemp(prefix="text_loss_bench_"), numSaveSteps=10 ** 9, null_prob_pooled=0.1,
                           null_prob_gemma=0.316, null_prob_bert=0.316, use_amp=True, max_res=256, device_rng=True, use_ema=False,
                           **({"text_loss_weight": 0.1} if on else {}))
    net.train()
    step = 0
    for _ in range(5):
        step += 1
        tr.train_step(step)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        step += 1
        tr.train_step(step)
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t0) / 5 * 1e3
    tr.capture_graph(step + 1)
    for _ in range(2):
        step += 1
        tr.train_step(step)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = []
    for _ in range(args.steps):
        step += 1
        losses.append(tr.train_step(step).clone())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    rec = {"config": args.child, "ms_per_step": round(ms, 3), "ms_per_step_eager": round(eager_ms, 3), "images_per_s": round(64 / ms * 1e3, 1),
           "loss_first": float(losses[0]), "loss_last": float(losses[-1])}
    if on:
        rec["last_img_loss"], rec["last_text_loss"] = float(tr.last_img_loss), float(tr.last_text_loss)
    print("STEP " + json.dumps(rec), flush=True)


def child_kernel(args):
    sys.path.insert(0, ROOT)
    import torch
    import sd3_amd  # noqa: F401
    from sd3_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.randn(ROWS, COLS, generator=g, device="cuda")
    label = (torch.randn(ROWS, COLS, generator=g, device="cuda") * 30).to(torch.bfloat16)
    coef = 0.1 / (ROWS * COLS)
    for frac in (0.0, 0.08, 0.25, 1.0):
        mask = torch.rand(ROWS, generator=g, device="cuda") < frac
        n = int(mask.sum())
        # 20 calls captured into one hipGraph and replayed: a call from Python costs more host time than the kernel runs, so a loop of eager calls would
        # time the enqueue
        calls, reps = 20, 10
        ops.text_loss(pred, label, mask, coef, grad_dtype=torch.float32)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(calls):
                ops.text_loss(pred, label, mask, coef, grad_dtype=torch.float32)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / (reps * calls) * 1e3
        nbytes = ROWS * COLS * 4 + n * COLS * (4 + 2) + ROWS
        print(f"KERNEL mmdit_text_loss {ROWS} x {COLS} (pred fp32, label bf16, dpred fp32), {n} of {ROWS} rows masked ({frac:.0%} drawn): "
              f"{us:8.1f} us per call (both launches), {nbytes / 1e6:7.1f} MB needed -> {nbytes / us / 1e3:7.1f} GB/s effective", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: its `off` step alternates with this tree's")
    ap.add_argument("--child", default=None, choices=["off", "on", "kernel"], help="one configuration in this process (what the parent process starts)")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.child == "kernel":
        return child_kernel(args)
    if args.child:
        return child_step(args)
    plan = [("off", ROOT), ("on", ROOT)] + ([("parent", args.parent_tree)] if args.parent_tree else [])
    res = {name: [] for name, _ in plan}
    runs = [(name, tree) for _ in range(args.rounds) for name, tree in plan] + [("kernel", ROOT)]
    for name, tree in runs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--child", "off" if name == "parent" else name, "--tree", tree]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if out.returncode != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
            print(f"{name}: child ended with status {out.returncode}; stopping", flush=True)
            return out.returncode
        for line in out.stdout.splitlines():
            if line.startswith("STEP "):
                rec = json.loads(line[5:])
                res[name].append(rec["ms_per_step"])
                print(f"{name:7s} {json.dumps(rec)}", flush=True)
            elif line.startswith("KERNEL "):
                print(line[7:], flush=True)
    for name, v in res.items():
        if v:
            print(f"{name:7s} ms per step over {len(v)} rounds: {v}  median {sorted(v)[len(v) // 2]:.3f}  spread {max(v) - min(v):.3f}")
    if res["off"] and res["on"]:
        a, b = sorted(res["off"])[len(res["off"]) // 2], sorted(res["on"])[len(res["on"]) // 2]
        print(f"text_loss on / off: {b / a:.4f} ({b - a:+.3f} ms per step)")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
