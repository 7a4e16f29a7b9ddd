"""text_loss=True on the GPU: the masked text-reconstruction loss kernel, the text head through the engine, the trainer and the sampler.

1  mmdit_text_loss (include/mmdit_hip_textloss.h) against float64 over the edges of its launch shape.  ROWS = MMDIT_TEXT_LOSS_ROWS_PER_WG rows per
   workgroup (one per wave), at most PARTS = MMDIT_TEXT_LOSS_MAX_PARTIALS workgroups:
     rows   1; ROWS - 1, ROWS, ROWS + 1; ROWS * PARTS - 1, ROWS * PARTS, ROWS * PARTS + 1 (the grid-stride wraps at the last one)
     cols   8, 16 (a fraction of one 512-wide wave step), 2056 (four steps and a ragged fifth), 2304 (the model's)
     masks  none, all, first row only, last row only, alternating, seeded 25 %;  every pred / label / dpred dtype combination.
   Bars, from the evaluation the header documents (u = 2^-24, U = 2^-8 the bf16 unit roundoff):
     dpred  out = fl_out(fl32(c2 * fl32(p - l))) with c2 = 2 * coef exact: two fp32 roundings, then the output's, so
            |out - ref| <= u_out |ref| + 4 u |ref| per element (u_out = U for bf16, 0 for fp32; half of the 4 u is slack for the products of the
            error terms);  rows the mask excludes: all bits zero.
     loss   every term d^2 is >= 0, so the relative error of the sum is at most (1 + u)^n - 1 <= n u / (1 - n u) with n the number of roundings a
            term can pass through: 2 (d is rounded once, squared) + L (serial fma chain of a lane, L = ceil(ceil(rows / ROWS) / grid) *
            ceil(cols / 512) * 8) + 6 (wave butterfly) + 3 (wave sums) + ceil(grid / 64) (serial over the partials) + 6 (butterfly) + 1 (* coef).
            That is 59 u for a single 2304-wide row and 102 u for 1025 of them (the wrapped grid); the any-order bound rows * cols * u would be
            2.4e6 u.  The float64 reference's own error (<= rows * cols * 2^-53 < 3e-10) is below 1e-3 of the smallest bar.
     none   loss is exactly 0 and every dpred bit is zero.
2  the model against the reference (tools/make_goldens_textloss.py): v on the EXISTING goldens under their existing bars (the 11 extra tensors
   cannot influence v), txt_pred and the gradients of records (T) and (S) against forward_micro_textloss.npz.
3  the engine's route, 4 the trainer (eager step against a float64 restatement, graph replay), 5 the sampler.
Every figure is printed before anything is asserted (collected in profiles/text_loss_parity.txt).
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.weights import make_inputs as model_inputs, make_state_dict  # noqa: E402

ROWS, PARTS = 4, 256           # MMDIT_TEXT_LOSS_ROWS_PER_WG, MMDIT_TEXT_LOSS_MAX_PARTIALS (tests/test_text_loss_abi.py checks them against the header)
LANE_COLS, WAVE_COLS = 8, 512  # MMDIT_TEXT_LOSS_LANE_COLS, MMDIT_TEXT_LOSS_WAVE_COLS
U = 2.0 ** -8                  # bf16 unit roundoff (round to nearest)
E32 = 2.0 ** -24               # fp32 unit roundoff
BF16, F32 = torch.bfloat16, torch.float32
MICRO = dict(dim=128, num_heads=2, num_blocks=3)
TEXT_DIM, TOKENS = 2304, 154

ROW_SIZES = [1, ROWS - 1, ROWS, ROWS + 1, ROWS * PARTS - 1, ROWS * PARTS, ROWS * PARTS + 1]
COL_SIZES = [8, 16, 2056, 2304]
MASKS = ["none", "all", "first", "last", "alternating", "seeded25"]
DTYPES = [(p, l, o) for p in (BF16, F32) for l in (BF16, F32) for o in (BF16, F32)]
SHAPES = [(r, c) for r in ROW_SIZES for c in COL_SIZES]


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------- 1: the kernel
def grid_of(rows):
    return min((rows + ROWS - 1) // ROWS, PARTS)


def serial_length(rows, cols):
    """Longest fma chain of one lane (the header's step 1)."""
    groups = (rows + ROWS - 1) // ROWS
    return -(-groups // grid_of(rows)) * -(-cols // WAVE_COLS) * LANE_COLS


def loss_roundings(rows, cols):
    return 2 + serial_length(rows, cols) + 6 + (ROWS - 1) + -(-grid_of(rows) // 64) + 6 + 1


def loss_bar(rows, cols):
    n = loss_roundings(rows, cols)
    return n * E32 / (1 - n * E32)


def make_mask(kind, rows, device="cpu"):
    m = torch.zeros(rows, dtype=torch.bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind == "seeded25":
        m = torch.rand(rows, generator=torch.Generator().manual_seed(rows)) < 0.25
    else:
        assert kind == "none"
    return m.to(device)


def make_case(rows, cols):
    """pred, label (fp32, seeded; the bf16 cases take their roundings) and coef."""
    g = torch.Generator().manual_seed(1000 * rows + cols)
    pred = torch.randn(rows, cols, generator=g)
    label = pred * 0.5 + torch.randn(rows, cols, generator=g) * 3.0
    return pred, label, float(np.float32(0.37 / (rows * cols)))


def reference(pred, label, mask, coef):
    """float64: (loss, dpred) of the values as stored."""
    d = (pred.double() - label.double()) * mask[:, None].double()
    return coef * (d * d).sum(), 2.0 * coef * d


WORST = {}


def _note(key, val, where):
    if val > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (val, where)


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    if WORST:
        print("\n[text_loss kernel] worst ratio to the bar over the sweep: " + "; ".join(f"{k} {v[0]:.3f} (@ {v[1]})" for k, v in sorted(WORST.items())))


def _bits_zero(t):
    return not bool(t.view(torch.int16 if t.dtype == BF16 else torch.int32).any())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "r%d-c%d" % s)
def test_kernel_sweep_vs_float64(shape, ops):
    rows, cols = shape
    p32, l32, coef = make_case(rows, cols)
    p32, l32 = p32.cuda(), l32.cuda()
    ins = {F32: (p32, l32), BF16: (p32.to(BF16), l32.to(BF16))}
    bar = loss_bar(rows, cols)
    worst_loss, worst_d = 0.0, 0.0
    fails = []
    for kind in MASKS:
        mask = make_mask(kind, rows, "cuda")
        for pdt, ldt, odt in DTYPES:
            pred, label = ins[pdt][0], ins[ldt][1]
            ref_loss, ref_d = reference(pred, label, mask, coef)
            loss, d = ops.text_loss(pred, label, mask, coef, grad_dtype=odt)
            assert loss.shape == () and loss.dtype == F32 and d.shape == pred.shape and d.dtype == odt
            where = f"r{rows}-c{cols}-{kind}-{str(pdt)[6:]}/{str(ldt)[6:]}/{str(odt)[6:]}"
            if not bool(mask.any()):      # "none" (and a seeded draw of a tiny case that masks nothing)
                if not (float(loss) == 0.0 and _bits_zero(loss.view(1)) and _bits_zero(d)):
                    fails.append((where, "all-zero mask: loss or dpred not exactly +0"))
                continue
            rl = abs(float(loss.double() - ref_loss)) / float(ref_loss)
            uo = U if odt == BF16 else 0.0
            lim = (uo + 4 * E32) * ref_d.abs()
            rd = float(((d.double() - ref_d).abs() / lim.clamp_min(1e-300))[mask].max())
            worst_loss, worst_d = max(worst_loss, rl / bar), max(worst_d, rd)
            _note("loss", rl / bar, where)
            _note("dpred " + ("bf16" if odt == BF16 else "fp32"), rd, where)
            if not _bits_zero(d[~mask]):
                fails.append((where, "an excluded dpred row is not +0"))
            if not (math.isfinite(float(loss)) and rl <= bar):
                fails.append((where, f"loss rel {rl:.3e} > bar {bar:.3e}"))
            if not rd <= 1.0:
                fails.append((where, f"dpred ratio {rd:.3f}"))
    print(f"[text_loss kernel] rows {rows} cols {cols}: {loss_roundings(rows, cols)} roundings, loss bar {bar:.3e}; worst loss error / bar {worst_loss:.3f}, "
          f"worst dpred error / bar {worst_d:.3f} over {len(MASKS) - 1} masks x {len(DTYPES)} dtype combinations")
    assert not fails, fails[:5]


@pytest.mark.parametrize("shape,kind", [((ROWS * PARTS + 1, 2304), "seeded25"), ((ROWS + 1, 16), "alternating")], ids=["r1025-c2304", "r5-c16"])
def test_excluded_rows_are_never_read(shape, kind, ops):
    """NaN poison: with every excluded row of pred and label filled with NaN the loss is finite and has the clean run's bits, the masked dpred rows
    have the clean run's bits and the excluded ones are +0."""
    rows, cols = shape
    p32, l32, coef = make_case(rows, cols)
    mask = make_mask(kind, rows, "cuda")
    assert 0 < int(mask.sum()) < rows
    for pdt, ldt, odt in DTYPES:
        pred, label = p32.cuda().to(pdt), l32.cuda().to(ldt)
        loss0, d0 = ops.text_loss(pred, label, mask, coef, grad_dtype=odt)
        pred[~mask] = float("nan")
        label[~mask] = float("nan")
        loss1, d1 = ops.text_loss(pred, label, mask, coef, grad_dtype=odt)
        fwd_only, none = ops.text_loss(pred, label, mask, coef)
        assert none is None
        assert math.isfinite(float(loss1)) and float(loss1) > 0 and torch.equal(loss0.view(1).view(torch.int32), loss1.view(1).view(torch.int32))
        assert torch.equal(fwd_only.view(1).view(torch.int32), loss1.view(1).view(torch.int32))
        assert _bits_zero(d1[~mask]) and bool(torch.isfinite(d1.float()).all()) and torch.equal(d0, d1)


def test_two_calls_give_equal_bits(ops):
    rows, cols = ROWS * PARTS + 1, 2304
    p32, l32, coef = make_case(rows, cols)
    pred, label, mask = p32.cuda(), l32.cuda().to(BF16), make_mask("alternating", rows, "cuda")
    a = [ops.text_loss(pred, label, mask, coef, grad_dtype=F32) for _ in range(3)]
    for loss, d in a[1:]:
        assert torch.equal(loss.view(1).view(torch.int32), a[0][0].view(1).view(torch.int32)) and torch.equal(d, a[0][1])


def test_refused_arguments_leave_the_outputs_untouched(ops):
    from sd3_amd import _lib
    rows, cols, sent = 6, 16, 7.0
    pred, label = torch.randn(rows, cols, device="cuda"), torch.randn(rows, cols, device="cuda")
    mask = make_mask("all", rows, "cuda")
    for bad in (lambda: ops.text_loss(pred, label[:, :8], mask, 1.0), lambda: ops.text_loss(pred, label, mask[:-1], 1.0),
                lambda: ops.text_loss(pred, label, mask.to(torch.uint8), 1.0), lambda: ops.text_loss(pred[:, :12], label[:, :12], mask, 1.0),
                lambda: ops.text_loss(pred[:, :4].contiguous(), label[:, :4].contiguous(), mask, 1.0), lambda: ops.text_loss(pred.half(), label, mask, 1.0),
                lambda: ops.text_loss(pred, label.double(), mask, 1.0), lambda: ops.text_loss(pred, label, mask, 1.0, grad_dtype=torch.float16),
                lambda: ops.text_loss(pred.cpu(), label.cpu(), mask.cpu(), 1.0), lambda: ops.text_loss(pred.t(), label.t(), mask[:cols].repeat(3)[:cols], 1.0),
                lambda: ops.text_loss(pred.flatten(), label.flatten(), mask, 1.0)):
        with pytest.raises(RuntimeError):
            bad()
    # the entry point itself: error codes of the header, nothing launched
    d = torch.full((rows, cols), sent, device="cuda")
    part = torch.full((PARTS,), sent, device="cuda")
    loss = torch.full((1,), sent, device="cuda")
    st, L = torch.cuda.current_stream().cuda_stream, _lib.lib()
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    base = (("pred", p(pred)), ("pdt", _lib.F32), ("label", p(label)), ("ldt", _lib.F32), ("mask", p(mask)), ("rows", rows), ("cols", cols), ("coef", 1.0),
            ("dpred", p(d)), ("odt", _lib.F32), ("partials", p(part)), ("loss", p(loss)), ("stream", st))
    call = lambda **kw: L.mmdit_text_loss(*[kw.get(k, v) for k, v in base])      # noqa: E731
    for k in ("pred", "label", "mask", "partials", "loss"):
        assert call(**{k: None}) == _lib.ERR_ARG, k
    assert call(pred=p(pred) + 4) == _lib.ERR_ARG and call(dpred=p(d) + 8) == _lib.ERR_ARG      # 16-byte loads and stores
    for k in ("pdt", "ldt", "odt"):
        assert call(**{k: _lib.FP8}) == _lib.ERR_DTYPE and call(**{k: -1}) == _lib.ERR_DTYPE, k
    assert call(rows=0) == _lib.ERR_SHAPE and call(rows=-3) == _lib.ERR_SHAPE
    assert call(cols=0) == _lib.ERR_SHAPE and call(cols=4) == _lib.ERR_SHAPE and call(cols=12) == _lib.ERR_SHAPE
    assert call(dpred=None, odt=-1) == 0 and float(loss) != sent      # forward only: the output dtype is not looked at
    loss.fill_(sent)
    part.fill_(sent)
    for kw in (dict(pred=None), dict(pdt=5), dict(cols=12), dict(rows=0)):
        assert call(**kw) < 0
    torch.cuda.synchronize()
    for t in (d, part, loss):
        assert bool((t == sent).all()), "a refused launch wrote to its outputs"


# ---------------------------------------------------------------------------------------------- 2: the model against the reference
_net = {}


def textloss_state_dict(net, MLP_type="swiglu", **cfg):
    """The weights rule of tools/make_goldens_textloss.py for a text_loss model of configuration cfg: the keys the plain model shares from
    make_state_dict(0, ...) (cut to the LEADING slice where the option has smaller tensors: qk_half_dim, tools/make_goldens_qkhalf.py; buffers the seeded
    dict does not have -- RoPE2dV2's inv_freq -- stay as constructed: tools/make_goldens_rope2dv2.py), the nine extra keys of the last block from
    make_state_dict(1, ..., num_blocks + 1), the head from Generator().manual_seed(4242)."""
    shared = make_state_dict(0, MLP_type=MLP_type, **cfg)
    four = make_state_dict(1, MLP_type=MLP_type, **{**cfg, "num_blocks": cfg["num_blocks"] + 1})
    g = torch.Generator().manual_seed(4242)
    head = {"out_text_proj.weight": torch.randn(TEXT_DIM, cfg["dim"], generator=g) * cfg["dim"] ** -0.5}
    head["out_text_proj.bias"] = 0.02 * torch.randn(TEXT_DIM, generator=g)
    sd, extra = {}, []
    for k, own in net.state_dict().items():
        if k in shared:
            sd[k] = shared[k][tuple(slice(0, n) for n in own.shape)].clone()
        elif k in head:
            sd[k] = head[k]
            extra.append(k)
        elif k.endswith("rotary_emb.inv_freq"):
            sd[k] = own.detach().cpu().clone()
        else:
            assert k.startswith("blocks.%d." % (cfg["num_blocks"] - 1)), k
            sd[k] = four[k][tuple(slice(0, n) for n in own.shape)].clone()
            extra.append(k)
    assert len(extra) == 11, extra
    return sd, extra


def _new_model(cfg=MICRO, MLP_type="swiglu", device="cuda:0", **kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    kw.setdefault("positional_encoding", "RoPE2d")
    net = diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type=MLP_type, device=torch.device(device),
                     text_loss=True, checkpoint_MLP=False, checkpoint_attn=False, **cfg, **kw)
    sd, extra = textloss_state_dict(net, MLP_type=MLP_type, **cfg)
    net.load_state_dict(sd, strict=True)
    net.text_only = extra
    return net


def build(precision):
    if "micro" not in _net:
        _net["micro"] = _new_model()
    return _net["micro"].set_precision(precision)


def _checksum(*ts):
    return [float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts]


# tests/test_qk_half_gpu.py FWD_BAR: parity mode rel-L2 < 1e-3 against the reference golden (the project's bar for every configuration); fast mode
# < 1.5 x FAST_MEASURED["micro_plain"][1] = 1.5 x 6.893e-3 of tests/test_model_gpu.py against the same fp32 golden
FWD_BAR = {"parity": 1e-3, "fast": 1.5 * 6.893e-03}
TXT_BAR = {"parity": 1e-3}      # fast: 1.5 x the reference's own bf16-autocast distance, stored with the fixture


@pytest.mark.parametrize("precision", ["parity", "fast"])
def test_forward_v_on_the_plain_golden_and_txt_pred(precision, golden_dir):
    """v against forward_micro_plain.npz (the text head and the last block's text half cannot influence it) and txt_pred against the reference's:
    per-token norms and the 16 stored rows, parity rel-L2 < 1e-3, fast < 1.5 x the reference's own bf16 distance (2.1e-2)."""
    plain = np.load(os.path.join(golden_dir, "forward_micro_plain.npz"))
    gold = np.load(os.path.join(golden_dir, "forward_micro_textloss.npz"))
    x, c, cp = model_inputs(0, 2, 16, 16, text_scale=1.0)
    assert np.allclose(gold["inputs_checksum"], _checksum(x, c, cp), rtol=1e-9) and np.allclose(plain["inputs_checksum"], gold["inputs_checksum"], rtol=1e-12)
    net = build(precision)
    assert not any(b.last for b in net.blocks)
    with torch.no_grad():
        out = net(x.cuda(), torch.tensor([0.3, 0.7]), c.cuda(), cp.cuda())
    assert isinstance(out, tuple) and len(out) == 2
    v, txt = out
    assert txt.shape == (2, TOKENS, TEXT_DIM) and txt.dtype == F32 and v.dtype == F32
    rv = rel(v, torch.from_numpy(plain["v"]))
    rows = txt.reshape(-1, TEXT_DIM)[torch.from_numpy(gold["txt_rows_idx"]).cuda()]
    rr, rn = rel(rows, torch.from_numpy(gold["txt_rows"])), rel(txt.double().norm(dim=-1), torch.from_numpy(gold["txt_norms"]))
    bar = TXT_BAR.get(precision, 1.5 * float(gold["txt_bf16_rel"]))
    print(f"[text_loss {precision}] forward: v rel-L2 vs forward_micro_plain.npz {rv:.3e} (bar {FWD_BAR[precision]:.2e}); txt_pred 16 stored rows rel-L2 {rr:.3e}, "
          f"per-token norms rel-L2 {rn:.3e} (bar {bar:.3e}; the reference's own bf16 distance {float(gold['txt_bf16_rel']):.3e})")
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(txt).all())
    assert rv < FWD_BAR[precision] and rr < bar and rn < bar


def _measure(net, gold, names, norms, samples, run, prefix):
    """rows = (name, numel, relative norm error, worst sample error / typical element, rel-L2 of a stored tensor or None, reference norm)."""
    net.zero_grad()
    loss, v = run(net)
    grads = dict((n, p.grad) for n, p in net.named_parameters() if p.grad is not None)
    params = dict(net.named_parameters())
    gs = torch.Generator().manual_seed(11)
    rows = []
    for i, n in enumerate(names):
        p = params[n]
        idx = torch.randint(0, p.numel(), (8,), generator=gs)
        gn = float(grads[n].double().norm())
        rn = abs(gn - norms[i]) / (norms[i] + 1e-12)
        samp = grads[n].flatten()[idx.cuda()].cpu().numpy()
        typical = max(float(np.abs(samples[i]).max()), norms[i] / np.sqrt(p.numel()))
        rs = float(np.abs(samp - samples[i]).max()) / (typical + 1e-30)
        rows.append((n, p.numel(), rn, rs, rel(grads[n], torch.from_numpy(gold[prefix + n])) if prefix + n in gold.files else None, norms[i]))
    return float(loss.detach()), v.detach(), rows, grads


@pytest.mark.parametrize("precision", ["parity", "fast"])
def test_image_only_gradients_vs_grads_micro(precision, golden_dir):
    """loss = v.pow(2).mean() on the inputs of grads_micro.npz: the reference's gradients of a text_loss model with these weights ARE those of
    grads_micro.npz (deviation 0.0, tools/make_goldens_textloss.py).  Structure and bars of tests/test_qk_half_gpu.py::test_model_gradients_vs_reference_golden:
    parity fixed bars; fast 1.5 x the plain RoPE2d model in fast mode against the same golden, measured in this run.  txt_pred receives no gradient
    (dtxt=None): the 11 text-only tensors get gradient tensors, all zero."""
    gm = np.load(os.path.join(golden_dir, "grads_micro.npz"))
    names = [k[6:] for k in gm.files if k.startswith("grad__")]
    x, c, cp = model_inputs(5, 2, 16, 16, text_scale=30.0)
    nl = [torch.tensor(n).bool() for n in ([0, 1], [0, 0], [1, 0])]

    def run(net):
        out = net(x.cuda(), torch.tensor([0.4, 0.9]), c.clone().cuda(), cp.clone().cuda(), *nl)
        v = out[0] if isinstance(out, tuple) else out
        loss = v.pow(2).mean()
        loss.backward()
        return loss, v

    def measure(net):
        net.zero_grad()
        loss, v = run(net)
        grads = dict((n, p.grad) for n, p in net.named_parameters() if p.grad is not None)
        ref = {n: float(np.linalg.norm(gm["grad__" + n].astype(np.float64))) for n in names}
        rows = [(n, grads[n].numel(), abs(float(grads[n].double().norm()) - ref[n]) / ref[n], rel(grads[n], torch.from_numpy(gm["grad__" + n]))) for n in names if ref[n] > 0.0]
        # the reference's exact zeros (the last block's text queries reach only the text stream, which v does not see): the bar of the text records
        zeros = [n for n in names if ref[n] == 0.0]
        assert zeros == ["blocks.2.attn.q_norm_c.weight"]
        for n in zeros:
            assert float(grads[n].abs().max()) <= 1e-6 * max(ref[k] for k in names if k.startswith("blocks.2.")), n
        return float(loss.detach()), v.detach(), rows, grads

    net = build(precision)
    loss, v, rows, grads = measure(net)
    assert set(grads) == {n for n, p in net.named_parameters() if p.requires_grad}, "a parameter received no gradient tensor"
    for n in net.text_only:
        assert float(grads[n].abs().max()) == 0.0, n
    tens = [r for r in rows if r[1] > 1]
    print(f"[text_loss {precision}] image-only gradients vs grads_micro.npz: loss {loss:.6f} vs {float(gm['loss']):.6f}, v rel-L2 {rel(v, torch.from_numpy(gm['v'])):.3e}; "
          f"{len(rows)} stored tensors: worst rel-L2 {max(r[3] for r in tens):.3e} ({max(tens, key=lambda r: r[3])[0]}), worst norm error {max(r[2] for r in tens):.3e}; "
          "scalars (norm error): " + ", ".join(f"{r[0]} {r[2]:.3e}" for r in rows if r[1] == 1))
    if precision == "parity":
        assert abs(loss - float(gm["loss"])) < 2e-3 * abs(float(gm["loss"]))
        for n, numel, rn, rl in rows:
            assert rn < (1e-1 if numel == 1 else 3e-2), (n, rn)
            assert numel == 1 or rl < 3e-2, (n, rl)
    else:
        from sd3_amd.models.diff_model import diff_model
        plain = diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=torch.device("cuda:0"),
                           positional_encoding="RoPE2d", checkpoint_MLP=False, checkpoint_attn=False, **MICRO)
        plain.load_state_dict(make_state_dict(0, MLP_type="swiglu", **MICRO), strict=True)
        _, _, base, _ = measure(plain.set_precision("fast"))
        bt = [r for r in base if r[1] > 1]
        sc, bsc = max(r[2] for r in rows if r[1] == 1), max(r[2] for r in base if r[1] == 1)
        print(f"[text_loss fast] the plain model in fast mode against grads_micro.npz: worst rel-L2 {max(r[3] for r in bt):.3e}, worst norm error {max(r[2] for r in bt):.3e}, scalars {bsc:.3e}; "
              f"text_loss / plain: rel-L2 {max(r[3] for r in tens) / max(r[3] for r in bt):.3f}, norm error {max(r[2] for r in tens) / max(r[2] for r in bt):.3f}, scalars {sc / bsc:.3f} (bar 1.5)")
        assert max(r[3] for r in tens) <= 1.5 * max(r[3] for r in bt)
        assert max(r[2] for r in tens) <= 1.5 * max(r[2] for r in bt)
        assert sc <= 1.5 * bsc


def grad_inputs():
    """The inputs of records (T) and (S) (tools/make_goldens_textloss.py)."""
    x, c, cp = model_inputs(5, 2, 16, 16, text_scale=30.0)
    nulls = [torch.tensor(n).bool() for n in ([0, 1], [0, 1], [1, 0])]
    mask = torch.rand(2, TOKENS, generator=torch.Generator().manual_seed(99)) < 0.25
    mask[:, :77] = mask[:, :77] & nulls[1][:, None]
    mask[:, 77:] = mask[:, 77:] & nulls[2][:, None]
    return x, c, cp, torch.tensor([0.4, 0.9]), nulls, mask


@pytest.mark.parametrize("record", ["T", "S"])
@pytest.mark.parametrize("precision", ["parity", "fast"])
def test_text_gradients_vs_reference_golden(precision, record, golden_dir):
    """Records (T): loss = txt, and (S): loss = v.pow(2).mean() + 4 txt, with txt = (MSE(txt_pred, labels) * mask[:, :, None]).mean() written in torch on
    the model's outputs (the HIP loss kernel has its own tests).
      parity  the fixed bars of tests/test_qk_half_gpu.py::test_model_gradients_vs_reference_golden: loss within 2e-3 relative, 8 seeded samples per
              tensor within 6e-2 of a typical element, the stored (<= 4096-element) tensors rel-L2 < 3e-2, gradient norms of the tensors < 3e-2
              and of the three scalar parameters < 1e-1.  Where the reference's gradient is exactly zero ((T): blocks.2.attn.query_proj_x /
              q_norm_x -- the last block's image queries reach only v) or None ((T): the image head and the last block's image-only half):
              max|grad| <= 1e-6 x the largest gradient norm of the block (of the model for the head).
      fast    the yardstick is the reference's OWN bf16 distance, stored with the fixture: the same computation under torch.autocast("cpu",
              bfloat16) against fp32.  The fast path keeps fp32 residual streams and fp32 accumulation -- fewer rounding points than autocast --
              so it should not be farther from fp32 than that: worst stored-tensor rel-L2 ((T) only: (S) stores none), worst tensor
              gradient-norm error and worst scalar-parameter error, worst against worst over the same parameters, each <= 1.5 x the
              reference's (the factor covers which tensor happens to be worst)."""
    gold = np.load(os.path.join(golden_dir, "forward_micro_textloss.npz"))
    x, c, cp, t, nulls, mask = grad_inputs()
    assert np.array_equal(gold["mask"], mask.numpy()) and [int(mask[:, :77].sum()), int(mask[:, 77:].sum())] == [19, 13]
    names = [str(n) for n in gold[record + "_names"]]

    def run(net):
        labels = c.cuda()
        v, txt_pred = net(x.cuda(), t, (c * ~mask[:, :, None]).cuda(), cp.clone().cuda(), *[n.clone() for n in nulls])
        txt = ((txt_pred - labels) ** 2 * mask.cuda()[:, :, None]).mean()
        loss = txt if record == "T" else v.pow(2).mean() + 4.0 * txt
        loss.backward()
        return loss, v

    net = build(precision)
    loss, v, rows, grads = _measure(net, gold, names, gold[record + "_norms"], gold[record + "_samples"], run, "T__" if record == "T" else "none__")
    assert set(grads) == {n for n, p in net.named_parameters() if p.requires_grad}, "a parameter received no gradient tensor"
    gloss = float(gold[record + "_loss"])
    live = [r for r in rows if r[5] > 0.0]
    tens = [r for r in live if r[1] > 1]
    scal = [r for r in live if r[1] == 1]
    worst = lambda rws, k: max(r[k] for r in rws if r[k] is not None)      # noqa: E731
    stored = [r for r in tens if r[4] is not None]
    print(f"[text_loss {precision}] record ({record}): loss {loss:.6f} vs {gloss:.6f} (rel {abs(loss - gloss) / abs(gloss):.3e}); {len(rows)} parameters: "
          f"worst relative grad-norm error {worst(tens, 2):.3e} ({max(tens, key=lambda r: r[2])[0]}), worst sample / typical {worst(tens, 3):.3e} ({max(tens, key=lambda r: r[3])[0]})"
          + (f", worst stored-tensor rel-L2 {worst(stored, 4):.3e} ({max(stored, key=lambda r: r[4])[0]})" if stored else "")
          + "; scalars (norm error): " + ", ".join(f"{r[0]} {r[2]:.3e}" for r in scal))
    # gradients the reference has as exact zeros / None
    block_norm = lambda n: max([r[5] for r in rows if r[0].split(".")[:2] == n.split(".")[:2]] if n.startswith("blocks.") else [r[5] for r in rows])      # noqa: E731
    dead = [r[0] for r in rows if r[5] == 0.0] + [n for n, p in net.named_parameters() if p.requires_grad and n not in names]
    for n in dead:
        mx = float(grads[n].abs().max())
        print(f"[text_loss {precision}] record ({record}): {n}: reference gradient zero / None, max|grad| {mx:.3e} (bar {1e-6 * block_norm(n):.3e})")
    if record == "T":
        assert {"blocks.2.attn.query_proj_x.weight", "blocks.2.attn.q_norm_x.weight", "out_proj.weight"} <= set(dead)
        for n in net.text_only:
            assert float(grads[n].abs().max()) > 0.0, n      # the 11 text-only tensors are trained by this loss
    for n in dead:
        assert float(grads[n].abs().max()) <= 1e-6 * block_norm(n), n
    if precision == "parity":
        assert abs(loss - gloss) < 2e-3 * abs(gloss)
        for n, numel, rn, rs, rl, _ in live:
            assert rn < (1e-1 if numel == 1 else 3e-2), (n, rn)
            if numel > 1:
                assert rs < 6e-2, (n, rs)
                assert rl is None or rl < 3e-2, (n, rl)
    else:
        ref_rel = dict(zip(names, gold[record + "_bf16_rel"]))
        ref_nrm = dict(zip(names, gold[record + "_bf16_norm_err"]))
        mine = {"norm": worst(tens, 2), "scalar": worst(scal, 2)}
        ref = {"norm": max(ref_nrm[r[0]] for r in tens), "scalar": max(ref_nrm[r[0]] for r in scal)}
        if stored:
            mine["stored rel-L2"], ref["stored rel-L2"] = worst(stored, 4), max(ref_rel[r[0]] for r in stored)
        print(f"[text_loss fast] record ({record}) against the reference's own bf16-autocast distance: "
              + ", ".join(f"{k} {mine[k]:.3e} / {ref[k]:.3e} = {mine[k] / ref[k]:.3f}" for k in mine) + " (bar 1.5)")
        for k in mine:
            assert mine[k] <= 1.5 * ref[k], (k, mine[k], ref[k])
    net.zero_grad()


_COMPOSE = [("gelu", dict(MLP_type="gelu"), MICRO, ("forward_micro_gelu.npz", 3, 30.0, [0.1, 0.6])),
            ("RoPE2dV2", dict(positional_encoding="RoPE2dV2"), MICRO, ("forward_micro_rope2dv2.npz", 0, 1.0, [0.3, 0.7])),
            ("qk_half_dim", dict(qk_half_dim=True), MICRO, ("forward_micro_qkhalf.npz", 0, 1.0, [0.3, 0.7])),
            ("hd128", dict(), dict(dim=256, num_heads=2, num_blocks=2), None)]


@pytest.mark.parametrize("case", _COMPOSE, ids=[c[0] for c in _COMPOSE])
def test_composes_with_the_other_options(case, golden_dir):
    """One forward per option: v against the option's own existing golden at the micro shape (parity bar 1e-3; weights by that option's rule + the
    text_loss rule), txt_pred finite and of the right shape, and a fast-mode forward + backward of v.pow(2).mean() + txt_pred.pow(2).mean() that
    gives every parameter a finite gradient.  Head width 128 (dim 256, 2 heads) has no micro golden: its fast forward is held to the parity one."""
    name, kw, cfg, gold_case = case
    net = _new_model(cfg, **kw).set_precision("parity")
    file, seed, tscale, tvals = gold_case if gold_case else (None, 0, 1.0, [0.3, 0.7])
    x, c, cp = model_inputs(seed, 2, 16, 16, text_scale=tscale)
    with torch.no_grad():
        v, txt = net(x.cuda(), torch.tensor(tvals), c.clone().cuda(), cp.cuda())
    assert txt.shape == (2, TOKENS, TEXT_DIM) and bool(torch.isfinite(txt).all()) and float(txt.std()) > 0.1
    if file is not None:
        gold = np.load(os.path.join(golden_dir, file))
        assert np.allclose(gold["inputs_checksum"], _checksum(x, c, cp), rtol=1e-9), "seeded inputs drifted from the fixture"
        r = rel(v, torch.from_numpy(gold["v"]))
        print(f"[text_loss compose] {name}: parity v rel-L2 vs {file} = {r:.3e} (bar 1e-3)")
        assert r < 1e-3, r
    net.set_precision("fast")
    vf, tf = net(x.cuda(), torch.tensor(tvals), c.clone().cuda(), cp.cuda())
    (vf.pow(2).mean() + tf.pow(2).mean()).backward()
    rv, rt = rel(vf, v), rel(tf, txt)
    tbar = 1.5 * float(np.load(os.path.join(golden_dir, "forward_micro_textloss.npz"))["txt_bf16_rel"])      # 1.5 x the reference's own bf16 distance of txt_pred
    print(f"[text_loss compose] {name}: fast vs parity forward: v {rv:.3e} (bar {FWD_BAR['fast']:.2e}), txt_pred {rt:.3e} (bar {tbar:.3e})")
    assert rv < FWD_BAR["fast"] and rt < tbar
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    for n in net.text_only:
        assert float(dict(net.named_parameters())[n].grad.abs().max()) > 0.0, n


# ---------------------------------------------------------------------------------------------- 3: the engine's route
def test_every_block_takes_the_pair_forms(monkeypatch):
    """With text_loss the last block is a full dual block: all three blocks launch the image + text pair forms of the adaLN kernels in both directions
    (the single-stream forms run once each, for the output head's norm), the text head materialises the pending text stream with ONE gated-residual
    forward and its backward forms that update's gradient with ONE gated-residual backward; the head's GEMMs are a forward, a data gradient and a
    deferred weight gradient."""
    from sd3_amd import ops
    net = build("fast")
    launches = []

    def tag(name):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, **kw: (launches.append(name), real(*a, **kw))[1])
    names = ["ln_modulate_fwd_pair", "ln_modulate_fwd_res", "ln_modulate_fwd", "ln_modulate_bwd_pair", "ln_modulate_bwd", "gate_residual_fwd", "gate_residual_bwd",
             "qk_norm_rope_fwd", "qk_norm_rope_bwd", "mlp_act_bwd", "text_loss"]
    for n in names:
        tag(n)
    x, c, cp = model_inputs(0, 2, 16, 16, text_scale=1.0)
    net.zero_grad()
    v, txt = net(x.cuda(), torch.tensor([0.3, 0.7]), c.cuda(), cp.cuda())
    (v.pow(2).mean() + txt.pow(2).mean()).backward()
    monkeypatch.undo()
    count = {n: launches.count(n) for n in names}
    print(f"[text_loss route] launches of one forward + backward: {count}")
    nb = len(net.blocks)
    assert count["ln_modulate_fwd_pair"] == 2 * nb and count["ln_modulate_bwd_pair"] == 2 * nb
    assert count["ln_modulate_fwd_res"] == 1 and count["ln_modulate_fwd"] == 0 and count["ln_modulate_bwd"] == 1
    assert count["gate_residual_fwd"] == 1 and count["gate_residual_bwd"] == 1
    assert count["qk_norm_rope_fwd"] == 0 and count["qk_norm_rope_bwd"] == 0 and count["mlp_act_bwd"] == 0 and count["text_loss"] == 0
    # a plain model on the same inputs: its last block is the image-only form (one single-stream adaLN more per direction, no gated-residual launches)
    from sd3_amd.models.diff_model import diff_model
    plain = diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu", device=torch.device("cuda:0"),
                       positional_encoding="RoPE2d", checkpoint_MLP=False, checkpoint_attn=False, **MICRO)
    plain.load_state_dict(make_state_dict(0, MLP_type="swiglu", **MICRO), strict=True)
    launches.clear()
    for n in names:
        tag(n)
    plain(x.cuda(), torch.tensor([0.3, 0.7]), c.cuda(), cp.cuda()).pow(2).mean().backward()
    monkeypatch.undo()
    assert launches.count("ln_modulate_fwd_pair") == 2 * nb - 1 and launches.count("ln_modulate_fwd_res") == 2 and launches.count("gate_residual_fwd") == 0
    assert launches.count("gate_residual_bwd") == 0
    net.zero_grad()


def _flatten(g, pre=""):
    """Every gradient tensor of engine.model_bwd's result, top level and blocks, as (name, tensor) in a fixed order."""
    out = []
    for k, v in vars(g).items():
        if k == "arenas":
            continue
        if torch.is_tensor(v):
            out.append((pre + k, v))
        elif isinstance(v, list):
            for i, b in enumerate(v):
                out += _flatten(b, f"{pre}{k}[{i}].")
        elif v is not None:
            out += _flatten(v, pre + k + ".")
    return out


def test_dtxt_none_equals_explicit_zeros(monkeypatch):
    """engine.model_bwd(dtxt=None) against dtxt = an explicit zero tensor, on one saved forward state each (two forwards of the same inputs: a backward
    consumes its state).  The two paths differ only in FRONT of the launch sequence they share: None builds the zero operand in the activation dtype,
    an explicit tensor is cast.  Bit for bit, therefore, where bits can hold -- what model_bwd hands to that shared sequence, all of it from
    launches without atomics:
      the head's GEMM operand dtxt_a, g.btxt right after its column sum, dC, and what the first block_bwd receives: dX2, dC2, and both halves of dacc
      (dacc_c is the explicit gated-residual backward of the last block's text MLP update);
    and from the first block_bwd on the two runs issue the same list of launches (every public function of ops, in order).  The gradients of the text
    head and of the last block's text half have all bits zero in both runs.  No bit claim is made on the other gradients: they sit downstream of fp32
    atomic column sums whose order is not fixed, and bf16 roundings of those (tests/test_model_gpu.py::test_graph_replay_matches_eager_steps), so
    two runs of the SAME call already differ there; they are held to that test's run-to-run bars (rel-L2 < 1e-3, max-abs <= 2e-3 max|b| + 1e-6)."""
    import types
    from sd3_amd import engine, ops
    net = build("fast")
    m = net._mode()
    W = net.weights(m)
    x, c, cp = model_inputs(5, 2, 16, 16, text_scale=30.0)
    rope = net.blocks[0].attn.rotary_emb.tables(8, 8, torch.device("cuda:0"))
    dv = torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(3)).cuda()
    cur = {}

    def wrap(name, real):
        def f(*a, **kw):
            if "launches" in cur:
                cur["launches"].append(name)
            out = real(*a, **kw)
            if name == "colsum" and a[1].numel() == TEXT_DIM and "btxt" not in cur:
                cur["btxt"] = a[1].clone()
            return out
        return f
    for name, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_"):
            monkeypatch.setattr(ops, name, wrap(name, fn))
    real_dgrad, real_block_bwd = engine._dgrad, engine.block_bwd

    def spy_dgrad(mm, dY, Wt, out_dtype, **kw):
        out = real_dgrad(mm, dY, Wt, out_dtype, **kw)
        if Wt is W.Wtxt:
            cur["dtxt_a"], cur["dC"] = dY.clone(), out.clone()
        return out

    def spy_block_bwd(mm, w, sv, dX2, dC2, *a, **kw):
        if "launches" not in cur:      # the first block: what the head handed over; the shared launch sequence starts here
            cur["dX2"], cur["dC2"], cur["dacc_x"], cur["dacc_c"] = dX2.clone(), dC2.clone(), kw["dacc"][0].clone(), kw["dacc"][1].clone()
            cur["launches"] = []
        return real_block_bwd(mm, w, sv, dX2, dC2, *a, **kw)
    monkeypatch.setattr(engine, "_dgrad", spy_dgrad)
    monkeypatch.setattr(engine, "block_bwd", spy_block_bwd)
    out = []
    for dtxt in (None, torch.zeros(2 * TOKENS, TEXT_DIM, device="cuda")):
        cur.clear()
        v, sv = engine.model_fwd(m, W, x.cuda(), torch.tensor([0.4, 0.9]).cuda(), c.cuda(), cp.cuda(), rope)
        assert sv.txt.shape == (2 * TOKENS, TEXT_DIM)
        g = engine.model_bwd(m, W, sv, dv, rope, dtxt=dtxt)
        torch.cuda.synchronize()
        out.append((v, sv.txt, _flatten(g), dict(cur)))
    monkeypatch.undo()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)      # noqa: E731
    ha, hb = out[0][3], out[1][3]
    handed = ["dtxt_a", "btxt", "dC", "dX2", "dC2", "dacc_x", "dacc_c"]
    assert set(handed) <= set(ha) and set(handed) <= set(hb)
    for k in handed:
        assert ha[k].dtype == hb[k].dtype and ha[k].shape == hb[k].shape and torch.equal(bits(ha[k]), bits(hb[k])), k
    assert ha["dtxt_a"].dtype == BF16 and not bool(bits(ha["dtxt_a"]).any()) and not bool(bits(ha["btxt"]).any()) and float(ha["dX2"].abs().max()) > 0
    assert torch.equal(bits(ha["dC"]), bits(ha["dC2"]))
    assert ha["launches"] == hb["launches"] and len(ha["launches"]) > 50 and "gate_residual_bwd" not in ha["launches"]
    assert [n for n, _ in out[0][2]] == [n for n, _ in out[1][2]] and len(out[0][2]) > 50
    pairs = [(n, a, b) for (n, a), (_, b) in zip(out[0][2], out[1][2])]
    differ = [n for n, a, b in pairs if not torch.equal(a, b)]
    live = [(n, a, b) for n, a, b in pairs if float(b.abs().max()) > 0]
    worst = max((rel(a, b), n) for n, a, b in live)
    print(f"[text_loss route] dtxt=None vs explicit zeros: the {len(handed)} tensors handed to the shared sequence bit-equal, {len(ha['launches'])} launches from the first block on, "
          f"the same list; of {len(pairs)} gradient tensors {len(differ)} differ in bits downstream of the atomics (worst rel-L2 {worst[0]:.3e} @ {worst[1]}, run-to-run bar 1e-3)")
    for n, a, b in pairs:
        assert rel(a, b) < 1e-3 and float((a - b).abs().max()) <= 2e-3 * float(b.abs().max()) + 1e-6, n
    last = "blocks[%d]." % (len(net.blocks) - 1)
    zero = [n for n, a, b in pairs if n in ("Wtxt", "btxt") or n.startswith(last + "mlp_c.") or n == last + "Wo_c"]
    assert len(zero) == 7, zero
    for n, a, b in pairs:
        if n in zero:
            assert not bool(bits(a).any()) and not bool(bits(b).any()), n
    # forward without the head (the sampler's call): nothing to run a backward from
    v2, sv2 = engine.model_fwd(m, W, x.cuda(), torch.tensor([0.4, 0.9]).cuda(), c.cuda(), cp.cuda(), rope, keep=False, text_head=False)
    assert sv2.txt is None and torch.equal(v2, out[0][0])


# ---------------------------------------------------------------------------------------------- 4: the trainer
def _trainer(net, tmp_path, weight, **kw):
    from sd3_amd.model_trainer import model_trainer
    args = dict(batchSize=4, accumulation_steps=1, totalSteps=100, lr=1e-3, ema_update_freq=1, ema_decay=0.9, warmup_steps=8, use_lr_scheduler=False,
                device=torch.device("cuda:0"), saveDir=str(tmp_path), numSaveSteps=100, null_prob_pooled=0.1, null_prob_gemma=0.316, null_prob_bert=0.316,
                max_res=128, device_rng=True, use_ema=False, text_loss_weight=weight)
    args.update(kw)
    return model_trainer(net, **args)


def test_trainer_eager_step_against_a_float64_restatement(tmp_path, monkeypatch):
    """One eager step with text_loss_weight = 0.5 on the trainer's seeded synthetic data.  The draw obeys model_trainer.py:400-414 (mask only on
    null-conditioned halves, input = labels * ~mask, labels untouched by the model's in-place null masking); last_text_loss equals
    (MSE(txt_pred, labels) * mask[:, :, None]).mean() restated in float64 on the prediction the kernel saw, within the kernel's loss bound (+ 2 u for
    the two scalar products that undo the weight); the step's loss is img + w * txt (exact in fp32: both factors are powers of two)."""
    from sd3_amd import ops
    torch.manual_seed(0)
    net = _new_model()
    w = 0.5
    tr = _trainer(net, tmp_path, w, null_prob_gemma=0.6, null_prob_bert=0.6, warmup_steps=0)      # (warm-up 0: the first step already has a learning rate)
    assert tr.text_loss and tr.text_loss_weight == w
    inp = tr._draw()
    assert len(inp) == 9
    x0, masked, pooled, t, n_pooled, n_gemma, n_bert, labels, mask = inp
    assert mask.dtype == torch.bool and mask.shape == (4, TOKENS) and labels.shape == (4, TOKENS, TEXT_DIM)
    assert not bool((mask[:, :77] & ~n_gemma[:, None]).any()) and not bool((mask[:, 77:] & ~n_bert[:, None]).any())
    assert int(mask[:, :77].sum()) > 0 and int(mask[:, 77:].sum()) > 0, "the seeded draw masks nothing: choose another seed"
    assert torch.equal(masked, labels * ~mask[:, :, None]) and bool((masked[mask] == 0).all()) and float(labels[mask].abs().max()) > 0
    labels0 = labels.clone()
    seen = {}
    real = ops.text_loss
    monkeypatch.setattr(ops, "text_loss", lambda pred, label, mk, coef, grad_dtype=None: (seen.update(pred=pred.clone(), label=label.clone(), mask=mk.clone(), coef=coef),
                                                                                         real(pred, label, mk, coef, grad_dtype=grad_dtype))[1])
    before = [p.detach().clone() for p in net.parameters()]
    total = tr._eager_step(1, inputs=[inp])
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.equal(labels, labels0) and torch.equal(seen["label"], labels0) and torch.equal(seen["mask"], mask)
    assert seen["coef"] == w / (4 * TOKENS * TEXT_DIM)
    ref = float((((seen["pred"].double() - labels0.double()) ** 2) * mask[:, :, None]).mean())
    rows = 4 * TOKENS
    bar = (loss_roundings(rows, TEXT_DIM) + 2) * E32 / (1 - (loss_roundings(rows, TEXT_DIM) + 2) * E32)
    txt, img = float(tr.last_text_loss), float(tr.last_img_loss)
    print(f"[text_loss trainer] eager step: img {img:.6f}, txt {txt:.6f} (float64 restatement {ref:.6f}, rel {abs(txt - ref) / ref:.3e}, bar {bar:.3e}), total {float(total):.6f}; "
          f"masked tokens {int(mask[:, :77].sum())} + {int(mask[:, 77:].sum())} of {rows}")
    assert tr.last_text_loss.is_cuda and tr.last_img_loss.is_cuda and ref > 0
    assert abs(txt - ref) <= bar * ref
    assert float(np.float32(img) + np.float32(w) * np.float32(txt)) == float(total)
    moved = [n for (n, p), q in zip(net.named_parameters(), before) if p.requires_grad and not torch.equal(p, q)]
    assert set(net.text_only) <= set(moved), "the step did not train the text head"
    # weight 0 on a text_loss model: v alone, the 7-tuple draw
    tr0 = _trainer(_new_model(), tmp_path, 0.0)
    assert len(tr0._draw()) == 7 and not tr0.text_loss and tr0.last_text_loss is None
    assert math.isfinite(float(tr0.train_step(1)))


def test_graph_replay_matches_eager_steps(tmp_path):
    """tests/test_model_gpu.py::test_graph_replay_matches_eager_steps with text_loss_weight = 0.5 (two more static inputs in the captured step: the
    labels and the mask, drawn inside the graph with device_rng): three eager warm-up steps, snapshot, steps 4-6 eager, restore, capture, steps 4-6
    replayed.  The loss of step 4 is bit-identical, the later losses and the final parameters agree to the run-to-run noise of the backward pass (that
    test's bars: rel-L2 < 1e-3, max-abs <= 2e-3 max|b| + 1e-6).  null_prob_gemma = null_prob_bert = 0.316: at least one step has a text term."""
    import sd3_amd  # noqa: F401
    from sd3_amd import engine, packing

    overlap = engine._WG_OVERLAP
    try:
        engine._WG_OVERLAP = False
        torch.manual_seed(0)
        net = _new_model()
        tr = _trainer(net, tmp_path, 0.5)
        for s in (1, 2, 3):
            tr.train_step(s)
        torch.cuda.synchronize()
        params = [p for p in net.parameters()]
        snap_p = [p.detach().clone() for p in params]
        snap_o = {id(p): {k: v.clone() for k, v in tr.optim.state[p].items()} for p in params if p in tr.optim.state}
        snap_s = (tr.grad_scaler._scale.clone(), tr.grad_scaler._growth_tracker.clone())
        snap_r = (torch.cuda.get_rng_state(), tr._gen.get_state(), tr.data_source.g.get_state())

        def three_steps():
            losses, txts = [], []
            for s in (4, 5, 6):
                losses.append(float(tr.train_step(s)))
                txts.append(float(tr.last_text_loss))
            torch.cuda.synchronize()
            return losses, txts, [p.detach().clone() for p in params], tr.optim.param_groups[0]["lr"]

        l0, t0, p0, lr0 = three_steps()
        with torch.no_grad():
            for p, q in zip(params, snap_p):
                p.copy_(q)
                for k, v in snap_o.get(id(p), {}).items():
                    tr.optim.state[p][k].copy_(v)
            tr.grad_scaler._scale.copy_(snap_s[0])
            tr.grad_scaler._growth_tracker.copy_(snap_s[1])
        packing.bump_epoch()
        torch.cuda.set_rng_state(snap_r[0])
        tr._gen.set_state(snap_r[1])
        tr.data_source.g.set_state(snap_r[2])
        tr.scheduler.step(3)
        xi, ci, pi = [a.cuda() for a in model_inputs(3, 2, 16, 16)]
        net(xi, torch.tensor([0.3, 0.7]), ci, pi)[0].sum().backward()
        tr.optim.zero_grad()
        torch.cuda.set_rng_state(snap_r[0])
        tr.capture_graph(4)
        assert tr._graph is not None
        l1, t1, p1, lr1 = three_steps()
    finally:
        engine._WG_OVERLAP = overlap
    worst = max((rel(a, b), float((a - b).abs().max()) / (2e-3 * float(b.abs().max()) + 1e-6)) for a, b in zip(p0, p1))
    print(f"[text_loss graph] eager losses {l0} (text terms {t0})  replayed {l1} (text terms {t1}); parameters: worst rel-L2 {worst[0]:.3e} (bar 1e-3)")
    assert all(math.isfinite(v) for v in l0 + l1 + t0 + t1)
    assert any(v > 0 for v in t0) and any(v > 0 for v in t1), "no step had a text term"
    assert lr0 == lr1 and l0[0] == l1[0] and t0[0] == t1[0] and np.allclose(l0, l1, rtol=1e-3)
    for a, b in zip(p0, p1):
        assert rel(a, b) < 1e-3 and float((a - b).abs().max()) <= 2e-3 * float(b.abs().max()) + 1e-6


# ---------------------------------------------------------------------------------------------- 5: the sampler
def test_sampler_equals_a_plain_loop_over_forward():
    """sample_imgs (which skips the text head: text_head=False), two Euler steps with guidance and a stub text encoder, against the same two steps
    written as a loop over net.forward(...)[0] on the (2B) guidance batch: bit for bit, in parity, fast and mxfp8 precision."""
    class _Cfg:
        latent_channels, shift_factor, scaling_factor = 16, 0.0, 8.0

    class _VAE:
        config, dtype = _Cfg(), torch.float32

        def decode(self, z):
            class D:
                sample = z
            return D

    class _Enc:
        VAE = _VAE()

        def __init__(self, th, tp):
            self.th, self.tp = th, tp

        def text_to_embedding(self, text):
            return self.th.clone(), self.tp.clone()

    _, th, tp = model_inputs(40, 1, 16, 16, text_scale=30.0)
    B, steps, cfg_scale = 2, 2, 3.0
    try:
        for precision in ("parity", "fast", "mxfp8"):
            net = build(precision)
            net.text_encoders = _Enc(th, tp)
            try:
                img = net.sample_imgs(B, steps, ["x"], cfg_scale=cfg_scale, width=128, height=128, sampler="euler", generator=torch.Generator().manual_seed(99))
            finally:
                del net.text_encoders
            xl = torch.randn((B, 16, 16, 16), generator=torch.Generator().manual_seed(99)).cuda()
            cc = torch.cat([th.expand(B, -1, -1), torch.zeros(B, *th.shape[1:])]).contiguous().cuda()
            pp = torch.cat([tp.expand(B, -1), torch.zeros(B, tp.shape[-1])]).contiguous().cuda()
            with torch.no_grad():
                for t_now in torch.linspace(1, 1.0 / steps, steps).tolist():
                    out = net(torch.cat([xl, xl]), torch.full((2 * B,), t_now), cc.clone(), pp.clone())
                    assert isinstance(out, tuple) and out[1].shape == (2 * B, TOKENS, TEXT_DIM) and bool(torch.isfinite(out[1]).all())
                    v = out[0]
                    xl = xl.sub(((1 + cfg_scale) * v[:B] - cfg_scale * v[B:]), alpha=1 / steps)
            net.train()
            ref = (xl / 8.0).clamp(-1, 1).float()
            print(f"[text_loss sampler] {precision}: rel-L2 vs the plain loop = {rel(img, ref):.3e}")
            assert img.shape == (B, 16, 16, 16) and bool(torch.isfinite(img).all())
            assert torch.equal(img, ref), (precision, rel(img, ref))
    finally:
        _net["micro"].set_precision("fast")
