"""Golden fixtures of text_loss=True (diff_model.py:149-151, 215-217, 344-346; model_trainer.py:399-454) from the REAL reference.

Runs only in the build container (needs the reference checkout, tools/ref_import.py).  Writes, data only:

tests/golden/state_dict_spec_micro_swiglu_textloss.json -- state-dict keys / shapes / dtypes, parameter order, no_grad list, parameter count of
the micro configuration of tools/make_goldens.py (dim 128, 2 heads, 3 blocks) built with text_loss=True: the 112 keys of the plain model, the
nine keys a full last block adds (blocks.2: MLP_c w12 / w3 weights and biases, attn.out_proj_c, norm2_c c_shift / c_scale, scale1_c, scale2_c)
and out_text_proj.weight / .bias.

Weights rule (textloss_state_dict below; tests/test_text_loss_abi.py and tests/test_text_loss_gpu.py rebuild the same weights by the same rule):
  * the keys the plain model shares: make_state_dict(0, MLP_type="swiglu", dim=128, num_heads=2, num_blocks=3) of oracle/weights.py;
  * the nine extra blocks.2.* keys: the tensors of those names in make_state_dict(1, ..., num_blocks=4) (block 2 of four is not a last block);
  * the head: g = Generator().manual_seed(4242); weight = randn(2304, 128, generator=g) * 128 ** -0.5; bias = 0.02 * randn(2304, generator=g);
loaded with strict=True.  The 11 extra tensors cannot influence v: asserted here bit for bit against forward_micro_plain.npz["v"] and
grads_micro.npz, which is what lets the GPU tests hold v and its gradients to the EXISTING goldens.

tests/golden/forward_micro_textloss.npz (no larger than forward_micro_kvmerge.npz, asserted):
  inputs_checksum                 the `micro_plain` inputs (16 x 16 latents, seed 0, t = [0.3, 0.7], no nulls)
  txt_norms, txt_rows_idx,        txt_pred on those inputs: the L2 norm of every token's prediction (2, 154), and 16 seeded token rows
  txt_rows                        (flat token indices, then (16, 2304)) in full
  txt_bf16_rel                    rel-L2 of the reference's own txt_pred under torch.autocast("cpu", torch.bfloat16) against its fp32 one
  mask, mask_counts               gradient records: inputs seed 5, text scale 30, t = [0.4, 0.9]; nulls pooled [0,1], gemma [0,1], bert [1,0];
                                  mask = rand(2, 154, generator=manual_seed(99)) < 0.25 ANDed with the gemma nulls on tokens < 77 and the bert
                                  nulls on the others; labels = the text, input = text * ~mask; txt = (MSE(txt_pred, labels) * mask[:, :, None]).mean()
  T_loss, T_names, T_norms,       record (T), loss = txt alone: every parameter's gradient norm and 8 seeded samples, the whole gradient of the
  T_samples, T__<name>            parameters with at most 4096 elements (out_norm / out_proj and the last block's image-only half are not in this graph: no entry)
  S_loss, S_names, S_norms,       record (S), loss = v.pow(2).mean() + 4.0 * txt: norms and samples
  S_samples
  T_bf16_rel, T_bf16_norm_err,    per parameter, the reference's own bf16 distance: the same computation under torch.autocast("cpu", torch.bfloat16)
  S_bf16_rel, S_bf16_norm_err     against fp32, as rel-L2 of the gradient and as relative error of its norm (NaN where the fp32 gradient is zero)

Usage:  python tools/make_goldens_textloss.py       (also writes tests/golden/generation_report_textloss.json)
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
TEXT_DIM = 2304
torch.set_num_threads(8)


def build_ref(refmod, text_loss=True):
    with contextlib.redirect_stdout(io.StringIO()):
        return refmod.diff_model(inCh=16, class_dim=768, patch_size=2, dim=CFG["dim"], hidden_scale=4.0, num_heads=CFG["num_heads"],
                                 attn_type="softmax_flash", MLP_type="swiglu", num_blocks=CFG["num_blocks"], device="cpu",
                                 positional_encoding="RoPE2d", text_loss=text_loss, checkpoint_MLP=False, checkpoint_attn=False)


def textloss_state_dict(keys, shared):
    """The weights rule of the docstring: `keys` = the text_loss model's state-dict keys, `shared` = the seeded plain state dict."""
    last = CFG["num_blocks"] - 1
    four = make_state_dict(1, MLP_type="swiglu", dim=CFG["dim"], num_heads=CFG["num_heads"], num_blocks=CFG["num_blocks"] + 1)
    g = torch.Generator().manual_seed(4242)
    head = {"out_text_proj.weight": torch.randn(TEXT_DIM, CFG["dim"], generator=g) * CFG["dim"] ** -0.5}
    head["out_text_proj.bias"] = 0.02 * torch.randn(TEXT_DIM, generator=g)
    sd, extra = {}, []
    for k in keys:
        if k in shared:
            sd[k] = shared[k].clone()
        elif k in head:
            sd[k] = head[k]
            extra.append(k)
        else:
            assert k.startswith(f"blocks.{last}."), k
            sd[k] = four[k].clone()
            extra.append(k)
    return sd, extra


def checksum(*ts):
    return [float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def grad_inputs():
    x, c, cp = make_inputs(5, 2, 16, 16, text_scale=30.0)
    t = torch.tensor([0.4, 0.9])
    nulls = [torch.tensor(n).bool() for n in ([0, 1], [0, 1], [1, 0])]
    mask = torch.rand(2, 154, generator=torch.Generator().manual_seed(99)) < 0.25
    mask[:, :77] = mask[:, :77] & nulls[1][:, None]
    mask[:, 77:] = mask[:, 77:] & nulls[2][:, None]
    return x, c, cp, t, nulls, mask


def run_record(net, which, autocast):
    """Gradients of record (T) or (S); returns (loss, {name: grad})."""
    x, c, cp, t, nulls, mask = grad_inputs()
    labels = c.clone()
    net.zero_grad()
    ctx = torch.autocast("cpu", torch.bfloat16) if autocast else contextlib.nullcontext()
    with ctx:
        v, txt_pred = net(x.clone(), t, c * ~mask[:, :, None], cp.clone(), *[n.clone() for n in nulls])
        txt = (torch.nn.MSELoss(reduction="none")(txt_pred, labels) * mask[:, :, None]).mean()
        loss = txt if which == "T" else v.pow(2).mean() + 4.0 * txt
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


def main():
    refmod = import_reference()
    report = {}
    limit = os.path.getsize(os.path.join(GOLD, "forward_micro_kvmerge.npz"))
    shared = make_state_dict(0, MLP_type="swiglu", **CFG)

    # ---- state-dict layout and the weights rule
    net = build_ref(refmod)
    assert net.defaults["text_loss"] is True
    plain_keys = list(build_ref(refmod, False).state_dict().keys())
    assert plain_keys == list(shared.keys())
    sd, extra = textloss_state_dict(list(net.state_dict().keys()), shared)
    assert len(extra) == 11 and [k for k in net.state_dict() if k not in extra] == plain_keys, "text_loss adds other keys than expected"
    assert all(sd[k].shape == v.shape for k, v in net.state_dict().items())
    net.load_state_dict(sd, strict=True)
    spec = [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu_textloss.json"), "w") as f:
        json.dump({"state_dict": spec, "named_parameters": [n for n, _ in net.named_parameters()],
                   "no_grad": [n for n, p in net.named_parameters() if not p.requires_grad],
                   "num_params": sum(p.numel() for p in net.parameters())}, f)
    report["extra_keys"] = extra

    # ---- forward on the micro_plain inputs: v is the plain golden's, bit for bit
    out = {}
    x, c, cp = make_inputs(0, 2, 16, 16, text_scale=1.0)
    t = torch.tensor([0.3, 0.7])
    out["inputs_checksum"] = np.array(checksum(x, c, cp))
    plain = np.load(os.path.join(GOLD, "forward_micro_plain.npz"))
    assert np.allclose(plain["inputs_checksum"], out["inputs_checksum"], rtol=1e-12), "not the micro_plain inputs"
    with torch.no_grad():
        v, txt = net(x.clone(), t, c.clone(), cp.clone())
        with torch.autocast("cpu", torch.bfloat16):
            _, txt_bf = net(x.clone(), t, c.clone(), cp.clone())
    assert np.array_equal(v.numpy(), plain["v"]), "v of the text_loss model differs from forward_micro_plain.npz"
    assert tuple(txt.shape) == (2, 154, TEXT_DIM) and txt.dtype == torch.float32
    idx = torch.randperm(2 * 154, generator=torch.Generator().manual_seed(7))[:16].sort().values
    out["txt_norms"] = txt.double().norm(dim=-1).numpy()
    out["txt_rows_idx"], out["txt_rows"] = idx.numpy(), txt.reshape(-1, TEXT_DIM)[idx].numpy()
    out["txt_bf16_rel"] = np.array(rel_l2(txt_bf.float(), txt))
    report["forward"] = {"v_bit_equal_to_micro_plain": True, "txt_pred_std": float(txt.std()), "txt_pred_bf16_rel": float(out["txt_bf16_rel"])}

    # ---- the image-only gradients are those of grads_micro.npz (deviation 0.0)
    gm = np.load(os.path.join(GOLD, "grads_micro.npz"))
    xg, cg, cpg = make_inputs(5, 2, 16, 16, text_scale=30.0)
    net.zero_grad()
    vg, _ = net(xg.clone(), torch.tensor([0.4, 0.9]), cg.clone(), cpg.clone(), *[torch.tensor(n).bool() for n in ([0, 1], [0, 0], [1, 0])])
    vg.pow(2).mean().backward()
    grads = dict(net.named_parameters())
    dev = max(float((grads[k[6:]].grad.double() - torch.from_numpy(gm[k]).double()).abs().max()) for k in gm.files if k.startswith("grad__"))
    assert dev == 0.0 and np.array_equal(vg.detach().numpy(), gm["v"]), dev
    report["image_only_gradients_vs_grads_micro_max_abs_dev"] = dev

    # ---- gradient records (T) and (S), fp32 and the reference's own bf16-autocast run
    mask = grad_inputs()[5]
    counts = [int(mask[:, :77].sum()), int(mask[:, 77:].sum())]
    assert min(counts) >= 8, counts
    out["mask"], out["mask_counts"] = mask.numpy(), np.array(counts)
    report["mask_counts"] = counts
    for which in ("T", "S"):
        gs = torch.Generator().manual_seed(11)
        loss, g32 = run_record(net, which, False)
        loss_bf, gbf = run_record(net, which, True)
        names = [n for n, _ in net.named_parameters() if n in g32]
        norms, samples, rels, nerrs = [], [], [], []
        for n in names:
            a = g32[n]
            norms.append(float(a.double().norm()))
            idx = torch.randint(0, a.numel(), (8,), generator=gs)
            samples.append(a.flatten()[idx].numpy())
            if which == "T" and a.numel() <= 4096:
                out["T__" + n] = a.numpy()
            zero = norms[-1] == 0.0
            rels.append(float("nan") if zero else rel_l2(gbf[n].float(), a))
            nerrs.append(float("nan") if zero else abs(float(gbf[n].double().norm()) - norms[-1]) / norms[-1])
        out[which + "_loss"] = np.array(loss)
        out[which + "_names"], out[which + "_norms"], out[which + "_samples"] = np.array(names), np.array(norms), np.stack(samples)
        out[which + "_bf16_rel"], out[which + "_bf16_norm_err"] = np.array(rels), np.array(nerrs)
        worst = int(np.nanargmax(rels))
        report["record_" + which] = {"loss": loss, "loss_bf16": loss_bf, "parameters": len(names), "zero_gradients": [n for n, z in zip(names, norms) if z == 0.0],
                                     "bf16_rel_median": float(np.nanmedian(rels)), "bf16_rel_worst": [names[worst], rels[worst]],
                                     "bf16_norm_err_worst": [names[int(np.nanargmax(nerrs))], float(np.nanmax(nerrs))]}
    # (under (T) the image head -- out_norm, out_proj -- and the last block's image-only half are not part of the graph: the reference leaves
    #  those gradients None; the HIP path returns zeros for them)
    report["record_T"]["no_gradient"] = [n for n, p in net.named_parameters() if p.requires_grad and n not in set(str(k) for k in out["T_names"])]
    assert all(n.startswith(("out_norm.", "out_proj.", "blocks.%d." % (CFG["num_blocks"] - 1))) for n in report["record_T"]["no_gradient"])
    assert [str(n) for n in out["S_names"]] == [n for n, p in net.named_parameters() if p.requires_grad], "a parameter received no gradient under (S)"

    path = os.path.join(GOLD, "forward_micro_textloss.npz")
    np.savez_compressed(path, **out)
    report["bytes"] = os.path.getsize(path)
    assert report["bytes"] <= limit, "fixture larger than forward_micro_kvmerge.npz"
    with open(os.path.join(GOLD, "generation_report_textloss.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
