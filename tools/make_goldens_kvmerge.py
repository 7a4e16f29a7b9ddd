"""Golden fixture of the kv_merge_attn option (Attention.py:243-251) from the REAL reference: tests/golden/forward_micro_kvmerge.npz.

Runs only in the build container (needs the reference checkout, tools/ref_import.py).  The micro configuration of tools/make_goldens.py
(dim 128, 2 heads, 3 blocks, 16 x 16 latents, 154 text tokens) is built with kv_merge_attn=True and loaded with the seeded synthetic
weights of oracle/weights.py -- the option adds no parameter, so the state dict is the one `micro_plain` uses.  Recorded, data only:

  inputs_checksum, v              the forward on the `micro_plain` inputs (seed 0, t = [0.3, 0.7], no nulls)
  tap_attn_x, tap_attn_c          block 0's attention outputs on those inputs (its inputs are forward_micro_plain.npz's tap_norm1_x /
                                  tap_norm1_c: nothing in front of the first attention depends on the option)
  grad_loss, grad_v, grad_names,  loss = v.pow(2).mean() on the inputs of grads_micro.npz (seed 5, t = [0.4, 0.9], nulls), every
  grad_norms, grad_samples,       parameter's gradient norm and 8 seeded samples, and the whole gradient of the parameters with at most
  grad__<name>                    4096 elements -- the subset grads_micro.npz keeps

Usage:  python tools/make_goldens_kvmerge.py            (writes tests/golden/forward_micro_kvmerge.npz, generation_report_kvmerge.json)
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


def build_ref(refmod, kv_merge_attn):
    with contextlib.redirect_stdout(io.StringIO()):
        net = refmod.diff_model(inCh=16, class_dim=768, patch_size=2, dim=CFG["dim"], hidden_scale=4.0, num_heads=CFG["num_heads"],
                                attn_type="softmax_flash", MLP_type="swiglu", num_blocks=CFG["num_blocks"], device="cpu",
                                positional_encoding="RoPE2d", kv_merge_attn=kv_merge_attn, checkpoint_MLP=False, checkpoint_attn=False)
    sd = make_state_dict(0, MLP_type="swiglu", **CFG)
    assert list(net.state_dict().keys()) == list(sd.keys()), "kv_merge_attn changed the state-dict keys"
    net.load_state_dict(sd, strict=True)
    return net


def checksum(*ts):
    return [float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    refmod = import_reference()
    net = build_ref(refmod, True)
    assert net.defaults["kv_merge_attn"] is True
    out, report = {}, {}

    # ---- forward on the micro_plain inputs
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
    with torch.no_grad():
        v_off = build_ref(refmod, False)(x.clone(), t, c.clone(), cp.clone())
    report["forward"] = {"v_std": float(v.std()), "merged_vs_unmerged": rel_l2(v, torch.from_numpy(plain["v"])),
                         "unmerged_rebuilt_vs_micro_plain_golden": rel_l2(v_off, torch.from_numpy(plain["v"])),
                         "attn_x_merged_vs_unmerged": rel_l2(taps["attn_x"], torch.from_numpy(plain["tap_attn_x"]))}

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
    assert [str(n) for n in gm["grad_names"]] == names, "parameter list differs from grads_micro.npz"
    assert sorted(k for k in gm.files if k.startswith("grad__")) == sorted(k for k in out if k.startswith("grad__"))
    report["gradients"] = {"loss": float(loss), "loss_unmerged": float(gm["loss"]), "parameters": len(names),
                           "whole_gradients_kept": sum(k.startswith("grad__") for k in out)}

    path = os.path.join(GOLD, "forward_micro_kvmerge.npz")
    np.savez_compressed(path, **out)
    report["bytes"] = os.path.getsize(path)
    with open(os.path.join(GOLD, "generation_report_kvmerge.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
