"""Golden fixtures of attn_type="cosine2" (Attention.py:153-162, 330-339: L2-normalised queries / keys, weights (q k + 1) / sum) from the REAL
reference.

Runs only in the build container (needs the reference checkout, tools/ref_import.py).  Writes, data only:

tests/golden/forward_micro_cosine2.npz -- the micro configuration of tools/make_goldens.py (dim 128, 2 heads, 3 blocks, 154 text tokens) built
with attn_type="cosine2", dual stream, "RoPE2d".  Weights: the state dict is the plain model's minus the twelve q_norm_* / k_norm_* weights
(nothing is added); every tensor is the seeded synthetic tensor of oracle/weights.py (make_state_dict(0, MLP_type="swiglu", **CFG)[key]) of
the model's own keys, loaded with strict=True.  tests/test_cosine2_abi.py and tests/test_cosine2_gpu.py rebuild the same weights by the same rule.
  inputs_checksum, v               the forward on the `micro_plain` inputs (16 x 16 latents, seed 0, t = [0.3, 0.7], no nulls)
  tap_attn_x, tap_attn_c           block 0's attention outputs on those inputs (its inputs are forward_micro_plain.npz's tap_norm1_x /
                                   tap_norm1_c: nothing in front of the first attention depends on the option)
  grad_loss, grad_v, grad_names,   loss = v.pow(2).mean() on the inputs of grads_micro.npz (seed 5, t = [0.4, 0.9], nulls), every
  grad_norms, grad_samples,        parameter's gradient norm and 8 seeded samples, and the whole gradient of the parameters with at most
  grad__<name>                     4096 elements -- the record of forward_micro_kvmerge.npz

tests/golden/forward_micro_cosine2_nonsquare.npz -- the same network on 16 x 24 latents:
  inputs_checksum, v               seed 2, t = [0.5, 0.5], text scale 30, nulls ([0,0], [1,0], [0,0])

tests/golden/state_dict_spec_micro_swiglu_cosine2.json -- state-dict keys / shapes / dtypes, parameter order, no_grad list, parameter count.

tests/golden/generation_report_cosine2.json -- the figures above, and per forward case `bf16_autocast_vs_fp32`: the rel-L2 distance of the
reference's own torch.autocast("cpu", bfloat16) output from its fp32 output (the bar of the "fast" precision in tests/test_cosine2_gpu.py).

No file may be larger than forward_micro_kvmerge.npz (asserted).

Usage:  python tools/make_goldens_cosine2.py
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle.weights import make_inputs, make_state_dict  # noqa: E402
from ref_import import import_reference  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CFG = dict(dim=128, num_heads=2, num_blocks=3)
torch.set_num_threads(8)


def build_ref(refmod, attn_type):
    with contextlib.redirect_stdout(io.StringIO()):
        return refmod.diff_model(inCh=16, class_dim=768, patch_size=2, dim=CFG["dim"], hidden_scale=4.0, num_heads=CFG["num_heads"],
                                 attn_type=attn_type, MLP_type="swiglu", num_blocks=CFG["num_blocks"], device="cpu",
                                 positional_encoding="RoPE2d", checkpoint_MLP=False, checkpoint_attn=False)


def build_cos2(refmod):
    net = build_ref(refmod, "cosine2")
    sd = make_state_dict(0, MLP_type="swiglu", **CFG)
    own = list(net.state_dict().keys())
    plain = list(build_ref(refmod, "softmax_flash").state_dict().keys())
    dropped = [k for k in plain if k not in own]
    assert [k for k in plain if k in own] == own and list(sd.keys()) == plain, "cosine2 added or reordered state-dict keys"
    net.load_state_dict({k: sd[k].clone() for k in own}, strict=True)
    return net, dropped


def checksum(*ts):
    return [float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def autocast_distance(net, v, x, t, c, cp, nl=()):
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        vb = net(x.clone(), t, c.clone(), cp.clone(), *nl)
    return rel_l2(vb.float(), v)


def main():
    refmod = import_reference()
    report = {}
    limit = os.path.getsize(os.path.join(GOLD, "forward_micro_kvmerge.npz"))

    # ---- state-dict layout
    net, dropped = build_cos2(refmod)
    assert net.defaults["attn_type"] == "cosine2"
    spec = [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu_cosine2.json"), "w") as f:
        json.dump({"state_dict": spec, "named_parameters": [n for n, _ in net.named_parameters()],
                   "no_grad": [n for n, p in net.named_parameters() if not p.requires_grad],
                   "num_params": sum(p.numel() for p in net.parameters())}, f)
    report["state_dict_keys_dropped"] = dropped

    # ---- forward on the micro_plain inputs
    out = {}
    x, c, cp = make_inputs(0, 2, 16, 16, text_scale=1.0)
    t = torch.tensor([0.3, 0.7])
    out["inputs_checksum"] = np.array(checksum(x, c, cp))
    taps = {}
    hk = net.blocks[0].attn.register_forward_hook(lambda m, i, o: taps.update(attn_x=o[0].detach().clone(), attn_c=o[1].detach().clone()))
    with torch.no_grad():
        v = net(x.clone(), t, c.clone(), cp.clone())
    hk.remove()
    out["v"] = v.numpy()
    out["tap_attn_x"], out["tap_attn_c"] = taps["attn_x"].numpy(), taps["attn_c"].numpy()
    plain = np.load(os.path.join(GOLD, "forward_micro_plain.npz"))
    assert np.allclose(plain["inputs_checksum"], out["inputs_checksum"], rtol=1e-12), "not the micro_plain inputs"
    report["forward"] = {"v_std": float(v.std()), "cosine2_vs_plain": rel_l2(v, torch.from_numpy(plain["v"])),
                         "attn_x_cosine2_vs_plain": rel_l2(taps["attn_x"], torch.from_numpy(plain["tap_attn_x"])),
                         "bf16_autocast_vs_fp32": autocast_distance(net, v, x, t, c, cp)}

    # ---- forward on a non-square input
    x, c, cp = make_inputs(2, 2, 16, 24, text_scale=30.0)
    nl = [torch.tensor(n).bool() for n in ([0, 0], [1, 0], [0, 0])]
    t = torch.tensor([0.5, 0.5])
    with torch.no_grad():
        v = net(x.clone(), t, c.clone(), cp.clone(), *nl)
    path = os.path.join(GOLD, "forward_micro_cosine2_nonsquare.npz")
    np.savez_compressed(path, inputs_checksum=np.array(checksum(x, c, cp)), v=v.numpy())
    report["forward_nonsquare"] = {"v_std": float(v.std()), "bytes": os.path.getsize(path),
                                   "bf16_autocast_vs_fp32": autocast_distance(net, v, x, t, c, cp, nl)}
    assert report["forward_nonsquare"]["bytes"] <= limit, "fixture larger than forward_micro_kvmerge.npz"

    # ---- gradients on the inputs of grads_micro.npz
    x, c, cp = make_inputs(5, 2, 16, 16, text_scale=30.0)
    t = torch.tensor([0.4, 0.9])
    nl = [torch.tensor(n).bool() for n in ([0, 1], [0, 0], [1, 0])]
    net.zero_grad()
    v = net(x.clone(), t, c.clone(), cp.clone(), *nl)
    loss = v.pow(2).mean()
    loss.backward()
    out["grad_loss"], out["grad_v"] = np.array(float(loss.detach())), v.detach().numpy()
    names, norms, samples = [], [], []
    gs = torch.Generator().manual_seed(11)
    for n, p in net.named_parameters():
        if p.grad is None:
            continue
        names.append(n)
        norms.append(float(p.grad.double().norm()))
        idx = torch.randint(0, p.numel(), (8,), generator=gs)
        samples.append(p.grad.flatten()[idx].numpy())
        if p.numel() <= 4096:
            out["grad__" + n] = p.grad.numpy()
    out["grad_names"], out["grad_norms"], out["grad_samples"] = np.array(names), np.array(norms), np.stack(samples)
    gm = np.load(os.path.join(GOLD, "grads_micro.npz"))
    assert names == [str(n) for n in gm["grad_names"] if not any(s in str(n) for s in ("q_norm_", "k_norm_"))], "parameter list differs from grads_micro.npz minus the norm weights"
    report["gradients"] = {"loss": float(loss.detach()), "loss_plain": float(gm["loss"]), "parameters": len(names),
                           "parameters_total": len(list(net.parameters())), "whole_gradients_kept": sum(k.startswith("grad__") for k in out)}

    path = os.path.join(GOLD, "forward_micro_cosine2.npz")
    np.savez_compressed(path, **out)
    report["bytes"] = os.path.getsize(path)
    assert report["bytes"] <= limit, "fixture larger than forward_micro_kvmerge.npz"
    with open(os.path.join(GOLD, "generation_report_cosine2.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
