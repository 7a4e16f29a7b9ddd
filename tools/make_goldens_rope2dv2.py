"""Golden fixtures of positional_encoding="RoPE2dV2" (rotary_embedding_2d_v2.py, Attention.py:105-107, 220-239) from the REAL reference.

Runs only in the build container (needs the reference checkout, tools/ref_import.py).  Writes, data only:

tests/golden/leaf_rope2dv2.npz -- the reference's RoPE2D module on seeded fp32 inputs:
  in_64, in_128                    (2, 2, 3, 5, 64) and (1, 2, 4, 3, 128), seed 7
  out_64_f1, out_64_f2, ...        the module's output at interpolate_factor 1 and 2
  inv_freq_64, inv_freq_128        its buffer

tests/golden/forward_micro_rope2dv2.npz -- the micro configuration of tools/make_goldens.py (dim 128, 2 heads, 3 blocks, 154 text tokens)
built with positional_encoding="RoPE2dV2" and loaded with the seeded synthetic weights of oracle/weights.py minus the `rotary_emb.freqs`
keys (the `inv_freq` buffers stay as the reference constructs them):
  inputs_checksum, v               the forward on the `micro_plain` inputs (16 x 16 latents, seed 0, t = [0.3, 0.7], no nulls)
  tap_attn_x, tap_attn_c           block 0's attention outputs on those inputs (its inputs are forward_micro_plain.npz's tap_norm1_x /
                                   tap_norm1_c: nothing in front of the first attention depends on the positional encoding)
  grad_loss, grad_v, grad_names,   loss = v.pow(2).mean() on the inputs of grads_micro.npz (seed 5, t = [0.4, 0.9], nulls), every
  grad_norms, grad_samples,        parameter's gradient norm and 8 seeded samples, and the whole gradient of the parameters with at most
  grad__<name>                     4096 elements -- the record of forward_micro_kvmerge.npz

tests/golden/forward_micro_rope2dv2_nonsquare.npz -- the same network on 16 x 24 latents (a file of its own: with it the file above would be
larger than forward_micro_kvmerge.npz, the size every fixture here is held to):
  inputs_checksum, v               seed 2, t = [0.5, 0.5], text scale 30, nulls ([0,0], [1,0], [0,0])

tests/golden/state_dict_spec_micro_swiglu_rope2dv2.json -- state-dict keys / shapes / dtypes, parameter order, parameter count.

Usage:  python tools/make_goldens_rope2dv2.py       (also writes tests/golden/generation_report_rope2dv2.json)
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


def build_ref(refmod, positional_encoding):
    with contextlib.redirect_stdout(io.StringIO()):
        return refmod.diff_model(inCh=16, class_dim=768, patch_size=2, dim=CFG["dim"], hidden_scale=4.0, num_heads=CFG["num_heads"],
                                 attn_type="softmax_flash", MLP_type="swiglu", num_blocks=CFG["num_blocks"], device="cpu",
                                 positional_encoding=positional_encoding, checkpoint_MLP=False, checkpoint_attn=False)


def build_v2(refmod):
    net = build_ref(refmod, "RoPE2dV2")
    sd = make_state_dict(0, MLP_type="swiglu", **CFG)
    # the state dicts differ only in the rotary module's entry: the `freqs` parameter of RoPE2d is the `inv_freq` buffer here
    keys_v1, keys_v2 = list(build_ref(refmod, "RoPE2d").state_dict().keys()), list(net.state_dict().keys())
    assert keys_v1 == list(sd.keys())
    assert [k.replace("rotary_emb.freqs", "rotary_emb.inv_freq") for k in keys_v1] == keys_v2, "RoPE2dV2 changed more than freqs -> inv_freq"
    own = net.state_dict()
    sd = {k: (own[k].clone() if k.endswith("rotary_emb.inv_freq") else sd[k]) for k in keys_v2}
    net.load_state_dict(sd, strict=True)
    return net


def checksum(*ts):
    return [float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    refmod = import_reference()
    from src.blocks.rotary_embedding_2d_v2 import RoPE2D
    report = {}

    # ---- leaf: the rotary module alone
    leaf = {}
    g = torch.Generator().manual_seed(7)
    for hd, shape in ((64, (2, 2, 3, 5, 64)), (128, (1, 2, 4, 3, 128))):
        x = torch.randn(shape, generator=g)
        leaf[f"in_{hd}"] = x.numpy().copy()
        for f in (1, 2):
            mod = RoPE2D(hd, interpolate_factor=f)
            leaf[f"out_{hd}_f{f}"] = mod(x.clone()).detach().numpy()
            leaf[f"inv_freq_{hd}"] = mod.inv_freq.numpy().copy()
    path = os.path.join(GOLD, "leaf_rope2dv2.npz")
    np.savez_compressed(path, **leaf)
    report["leaf_bytes"] = os.path.getsize(path)

    # ---- state-dict layout
    net = build_v2(refmod)
    assert net.defaults["positional_encoding"] == "RoPE2dV2"
    spec = [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu_rope2dv2.json"), "w") as f:
        json.dump({"state_dict": spec, "named_parameters": [n for n, _ in net.named_parameters()],
                   "no_grad": [n for n, p in net.named_parameters() if not p.requires_grad],
                   "num_params": sum(p.numel() for p in net.parameters())}, f)

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
    report["forward"] = {"v_std": float(v.std()), "v2_vs_rope2d": rel_l2(v, torch.from_numpy(plain["v"])),
                         "attn_x_v2_vs_rope2d": rel_l2(taps["attn_x"], torch.from_numpy(plain["tap_attn_x"]))}

    # ---- forward on a non-square input
    x, c, cp = make_inputs(2, 2, 16, 24, text_scale=30.0)
    nl = [torch.tensor(n).bool() for n in ([0, 0], [1, 0], [0, 0])]
    with torch.no_grad():
        v = net(x.clone(), torch.tensor([0.5, 0.5]), c.clone(), cp.clone(), *nl)
    path = os.path.join(GOLD, "forward_micro_rope2dv2_nonsquare.npz")
    np.savez_compressed(path, inputs_checksum=np.array(checksum(x, c, cp)), v=v.numpy())
    report["forward_nonsquare"] = {"v_std": float(v.std()), "bytes": os.path.getsize(path)}

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
    assert [str(n) for n in gm["grad_names"] if not str(n).endswith("rotary_emb.freqs")] == names, "parameter list differs from grads_micro.npz"
    report["gradients"] = {"loss": float(loss.detach()), "loss_rope2d": float(gm["loss"]), "parameters": len(names),
                           "whole_gradients_kept": sum(k.startswith("grad__") for k in out)}

    path = os.path.join(GOLD, "forward_micro_rope2dv2.npz")
    np.savez_compressed(path, **out)
    report["bytes"] = os.path.getsize(path)
    assert report["bytes"] <= os.path.getsize(os.path.join(GOLD, "forward_micro_kvmerge.npz")), "fixture larger than forward_micro_kvmerge.npz"
    assert report["leaf_bytes"] <= os.path.getsize(os.path.join(GOLD, "forward_micro_kvmerge.npz"))
    with open(os.path.join(GOLD, "generation_report_rope2dv2.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
