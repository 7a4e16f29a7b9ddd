"""text_loss=True at the ABI, construction, checkpoint, trainer and yardstick level.  No GPU needed.

The entry point mmdit_text_loss lives in a header of its own, include/mmdit_hip_textloss.h, and in the binding's _TEXTLOSS_SIGNATURES table: the
versioned core ABI (58 entry points, MMDIT_ABI_VERSION 10) and the four other side headers do not move.  diff_model accepts text_loss=True with the
reference's state dict (every block a full dual block, out_text_proj after time_scale), round-trips it through defaults and checkpoints, and still
refuses it together with kv_merge_attn; model_trainer accepts text_loss_weight > 0 for such a model only.

Yardstick soundness: a float64 model of the summation order and rounding points the header documents is run over the cases of the GPU sweep
(tests/test_text_loss_gpu.py) and held to the bars the kernel is held to there.
"""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_text_loss_gpu as A  # noqa: E402

NAME = "mmdit_text_loss"
HD128_NAMES = ["mmdit_attn_bwd_hd128", "mmdit_attn_fwd_hd128", "mmdit_qk_norm_rope_bwd_hd128", "mmdit_qk_norm_rope_fwd_hd128"]
ROPE3_NAMES = ["mmdit_qk_norm_rope3_bwd", "mmdit_qk_norm_rope3_fwd"]
QKHALF_NAMES = ["mmdit_attn_bwd_qkhalf", "mmdit_attn_fwd_qkhalf", "mmdit_qk_norm_rope_bwd_qkhalf", "mmdit_qk_norm_rope_fwd_qkhalf"]
MICRO = dict(dim=128, num_heads=2, num_blocks=3)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PROTOTYPE = ["const void* pred", "int pred_dtype", "const void* label", "int label_dtype", "const unsigned char* mask", "int64_t rows", "int cols", "float coef",
             "void* dpred", "int dpred_dtype", "float* partials", "float* loss", "mmdit_stream_t stream"]


def _lib():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib


def _model(text_loss=True, **kw):
    import sd3_amd  # noqa: F401
    from sd3_amd.models.diff_model import diff_model
    kw.setdefault("positional_encoding", "RoPE2d")
    kw.setdefault("MLP_type", "swiglu")
    return diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", device=torch.device("cpu"),
                      text_loss=text_loss, checkpoint_MLP=False, checkpoint_attn=False, **kw)


# ---------------------------------------------------------------------------------------------- ABI
def test_declared_in_the_textloss_header_only():
    L = _lib()
    assert L.declared_textloss_symbols() == [NAME] and set(L._TEXTLOSS_SIGNATURES) == {NAME}
    for table in (L._SIGNATURES, L._EXT_SIGNATURES, L._HD128_SIGNATURES, L._ROPE3_SIGNATURES, L._QKHALF_SIGNATURES):
        assert NAME not in table
    for path in (L.HEADER_PATH, L.HEADER_EXT_PATH, L.HEADER_HD128_PATH, L.HEADER_ROPE3_PATH, L.HEADER_QKHALF_PATH):
        with open(path) as f:
            txt = f.read().lower()
        assert "text_loss" not in txt and "textloss" not in txt, path
    with open(L.HEADER_TEXTLOSS_PATH) as f:
        txt = f.read()
    assert '#include "mmdit_hip.h"' in txt and "model_trainer.py:399-454" in txt and "mmdit_flow_loss" in txt
    defs = dict(re.findall(r"#define (MMDIT_\w+) (\d+)", txt))
    assert (int(defs["MMDIT_TEXT_LOSS_ROWS_PER_WG"]), int(defs["MMDIT_TEXT_LOSS_MAX_PARTIALS"])) == (L.TEXT_LOSS_ROWS_PER_WG, L.TEXT_LOSS_MAX_PARTIALS) == (A.ROWS, A.PARTS)
    assert (int(defs["MMDIT_TEXT_LOSS_LANE_COLS"]), int(defs["MMDIT_TEXT_LOSS_WAVE_COLS"])) == (L.TEXT_LOSS_LANE_COLS, L.TEXT_LOSS_WAVE_COLS) == (A.LANE_COLS, A.WAVE_COLS)
    assert A.WAVE_COLS == 64 * A.LANE_COLS and A.PARTS % 64 == 0


def test_the_other_headers_do_not_move():
    L = _lib()
    assert len(L.declared_symbols()) == 58 and L.ABI_VERSION == 10 and set(L._SIGNATURES) == set(L.declared_symbols())
    with open(L.HEADER_PATH) as f:
        assert re.search(r"#define\s+MMDIT_ABI_VERSION\s+10\b", f.read())
    assert L.declared_ext_symbols() == ["mmdit_attn_fwd_e4m3"] and set(L._EXT_SIGNATURES) == {"mmdit_attn_fwd_e4m3"}
    assert L.declared_hd128_symbols() == HD128_NAMES and set(L._HD128_SIGNATURES) == set(HD128_NAMES)
    assert L.declared_rope3_symbols() == ROPE3_NAMES and set(L._ROPE3_SIGNATURES) == set(ROPE3_NAMES)
    assert L.declared_qkhalf_symbols() == QKHALF_NAMES and set(L._QKHALF_SIGNATURES) == set(QKHALF_NAMES)


def test_signature_equals_the_prototype():
    L = _lib()
    with open(L.HEADER_TEXTLOSS_PATH) as f:
        m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", f.read())
    assert m, "no prototype"
    proto = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert proto == PROTOTYPE

    def ctype(arg):
        ty = arg.rsplit(" ", 1)[0].replace("const ", "")
        if ty.endswith("*") or ty == "mmdit_stream_t":
            return ctypes.c_void_p
        return {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64}[ty]
    argtypes, restype = L._TEXTLOSS_SIGNATURES[NAME]
    assert restype is ctypes.c_int and argtypes == [ctype(a) for a in proto]


def test_bound_and_exported():
    L = _lib()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, NAME)
    fn = getattr(L.lib(), NAME)
    assert fn.argtypes == L._TEXTLOSS_SIGNATURES[NAME][0] and fn.restype is ctypes.c_int
    assert L.lib().mmdit_abi_version() == 10


def test_build_lists_the_source_and_the_header():
    import importlib.util
    L = _lib()
    spec = importlib.util.spec_from_file_location("_mmdit_build_textloss", os.path.join(os.path.dirname(L.LIB_PATH), "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert "text_loss.hip" in B.SOURCES and os.path.samefile(B.HEADER_TEXTLOSS, L.HEADER_TEXTLOSS_PATH)
    with open(os.path.join(B.CSRC, "text_loss.hip")) as f:
        src = f.read()
    assert "mmdit_hip_textloss.h" in src and "asm" not in src and "atomic" not in src.lower()
    # a header every object's content hash covers
    assert B.source_hash("text_loss.hip") != B._sha([os.path.join(B.CSRC, "text_loss.hip")], "")


def test_ops_argument_checks_raise_before_the_library_is_touched(monkeypatch):
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib as L, ops
    monkeypatch.setattr(L, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    pred, label, mask = torch.zeros(6, 16), torch.zeros(6, 16), torch.zeros(6, dtype=torch.bool)
    for args in ((pred, label[:, :8], mask), (pred, label, mask[:-1]), (pred, label, mask.to(torch.uint8)), (pred[:, :12], label[:, :12], mask),
                 (pred.half(), label, mask), (pred, label.double(), mask), (pred.flatten(), label.flatten(), mask), (pred, label, mask)):
        with pytest.raises(RuntimeError):
            ops.text_loss(*args, 1.0)
    with pytest.raises(RuntimeError, match="grad_dtype"):
        ops.text_loss(pred, label, mask, 1.0, grad_dtype=torch.float16)


# ---------------------------------------------------------------------------------------------- construction, state dict, checkpoints
def test_model_constructs():
    """Fails on the parent commit: diff_model raised for text_loss=True."""
    net = _model(**MICRO)
    assert net.defaults["text_loss"] is True and net.text_loss is True
    assert not any(b.last for b in net.blocks) and all(hasattr(b, "MLP_c") and hasattr(b, "norm2_c") and hasattr(b, "scale1_c") and hasattr(b, "scale2_c") for b in net.blocks)
    assert all(hasattr(b.attn, "out_proj_c") for b in net.blocks)
    assert net.out_text_proj.weight.shape == (2304, 128) and net.out_text_proj.bias.shape == (2304,)
    assert list(net._modules)[-2:] == ["out_proj", "out_text_proj"] and list(net._parameters)[-1] == "time_scale"
    assert net._packs.Wtxt.rows == [2304] and net._packs.Wtxt.params[0] is net.out_text_proj.weight
    assert net.blocks[-1]._pmod.rows == [128] * 12
    plain = _model(False, **MICRO)
    assert plain.blocks[-1].last and not hasattr(plain, "out_text_proj") and not hasattr(plain._packs, "Wtxt") and plain.blocks[-1]._pmod.rows == [128] * 8
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):
        net(torch.zeros(1, 16, 8, 8), torch.tensor([0.5]), torch.zeros(1, 154, 2304), torch.zeros(1, 768))


def test_state_dict_equals_the_reference_spec_and_loads_the_rule_weights():
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu_textloss.json")) as f:
        spec = json.load(f)
    with open(os.path.join(GOLD, "state_dict_spec_micro_swiglu.json")) as f:
        spec_plain = json.load(f)
    net = _model(**MICRO)
    assert [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()] == spec["state_dict"]
    assert [n for n, _ in net.named_parameters()] == spec["named_parameters"]
    assert [n for n, p in net.named_parameters() if not p.requires_grad] == spec["no_grad"] and len(spec["no_grad"]) == 3
    assert sum(p.numel() for p in net.parameters()) == spec["num_params"]
    keys, plain_keys = [k[0] for k in spec["state_dict"]], [k[0] for k in spec_plain["state_dict"]]
    extra = [k for k in keys if k not in plain_keys]
    assert len(keys) == len(plain_keys) + 11 and [k for k in keys if k in plain_keys] == plain_keys
    assert extra[-2:] == ["out_text_proj.weight", "out_text_proj.bias"] and all(k.startswith("blocks.2.") for k in extra[:-2])
    sd, rule_extra = A.textloss_state_dict(net, **MICRO)
    assert rule_extra == extra
    net.load_state_dict(sd, strict=True)
    full = A.make_state_dict(0, MLP_type="swiglu", **MICRO)
    four = A.make_state_dict(1, MLP_type="swiglu", dim=128, num_heads=2, num_blocks=4)
    own = net.state_dict()
    assert all(torch.equal(own[k], full[k]) for k in plain_keys) and all(torch.equal(own[k], four[k]) for k in extra[:-2])
    g = torch.Generator().manual_seed(4242)
    assert torch.equal(own["out_text_proj.weight"], torch.randn(2304, 128, generator=g) * 128 ** -0.5) and torch.equal(own["out_text_proj.bias"], 0.02 * torch.randn(2304, generator=g))


def test_defaults_round_trip_and_checkpoint_reload(tmp_path):
    net = _model(**MICRO)
    assert json.loads(json.dumps(net.defaults)) == net.defaults and net.defaults["text_loss"] is True
    rebuilt = type(net)(**{**json.loads(json.dumps(net.defaults)), "device": torch.device("cpu")})
    assert [(k, v.shape) for k, v in rebuilt.state_dict().items()] == [(k, v.shape) for k, v in net.state_dict().items()] and rebuilt.defaults == net.defaults
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())) * 0.01)
    net.saveModel(str(tmp_path))
    with open(os.path.join(str(tmp_path), "model_params.json")) as f:
        assert json.load(f)["text_loss"] is True
    other = _model(False, dim=256, num_heads=2, num_blocks=1).set_precision("parity")      # a differently configured instance, without the option
    assert not other.text_loss
    other.loadModel(str(tmp_path), "model.pkl", "model_params.json")
    assert other.defaults["text_loss"] is True and other.text_loss is True and other.precision == "parity" and not any(b.last for b in other.blocks)
    assert all(m.precision == "parity" for m in other.modules() if hasattr(m, "precision"))
    sd, sd2 = net.state_dict(), other.state_dict()
    assert list(sd.keys()) == list(sd2.keys()) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert other._packs.Wtxt.params[0] is other.out_text_proj.weight
    # and back: a text_loss instance loads a plain checkpoint
    plain = _model(False, **MICRO)
    plain.saveModel(str(tmp_path / "plain"))
    net.loadModel(str(tmp_path / "plain"), "model.pkl", "model_params.json")
    assert net.text_loss is False and net.blocks[-1].last and not hasattr(net, "out_text_proj") and not hasattr(net._packs, "Wtxt")


def test_options_compose_and_kv_merge_stays_refused():
    for kw in (dict(MLP_type="gelu", **MICRO), dict(positional_encoding="RoPE2dV2", **MICRO), dict(qk_half_dim=True, **MICRO), dict(dim=256, num_heads=2, num_blocks=2)):
        net = _model(**kw)
        assert net.text_loss and not net.blocks[-1].last and len(A.textloss_state_dict(net, **{"MLP_type": kw.get("MLP_type", "swiglu"), "dim": kw["dim"], "num_heads": 2,
                                                                                              "num_blocks": kw["num_blocks"]})[1]) == 11
    for prec in ("parity", "fp8", "mxfp8", "fast"):      # the e4m3 modes are accepted: an ordinary dual last block, a bf16 head
        assert _model(**MICRO).set_precision(prec).precision == prec
    with pytest.raises(RuntimeError, match="qk_half_dim"):
        _model(qk_half_dim=True, **MICRO).set_precision("fp8")
    with pytest.raises(RuntimeError) as e:
        _model(kv_merge_attn=True, **MICRO)
    assert "text_loss" in str(e.value) and "kv_merge_attn" in str(e.value)
    assert _model(False, kv_merge_attn=True, **MICRO).kv_merge_attn


# ---------------------------------------------------------------------------------------------- trainer
def _trainer(net, tmp_path, **kw):
    from sd3_amd.model_trainer import model_trainer
    return model_trainer(net, batchSize=2, accumulation_steps=1, totalSteps=10, lr=1e-3, ema_update_freq=1, ema_decay=0.9, warmup_steps=0, use_lr_scheduler=False,
                         device=torch.device("cpu"), saveDir=str(tmp_path), numSaveSteps=100, max_res=128, use_ema=False, **kw)


def test_trainer_refusals_and_the_draw(tmp_path):
    plain, net = _model(False, **MICRO), _model(**MICRO)
    with pytest.raises(RuntimeError, match="text_loss"):
        _trainer(plain, tmp_path, text_loss_weight=0.1)
    with pytest.raises(AssertionError):
        _trainer(net, tmp_path, text_loss_weight=-0.1)
    with pytest.raises(AssertionError):
        _trainer(plain, tmp_path, text_loss_weight=-0.1)
    t0 = _trainer(plain, tmp_path)
    assert not t0.text_loss and t0.text_loss_weight == 0.0 and t0.last_text_loss is None
    # weight 0: the 7-tuple and the RNG stream of a run without the option, on a text_loss model too
    torch.manual_seed(7)
    a = t0._draw()
    torch.manual_seed(7)
    b = _trainer(net, tmp_path, text_loss_weight=0.0)._draw()
    assert len(a) == len(b) == 7 and all(torch.equal(x, y) for x, y in zip(a[3:], b[3:]))
    # weight > 0: the mask is drawn AFTER the null masks from the CPU generator (the reference's order), then ANDed per half
    tr = _trainer(net, tmp_path, text_loss_weight=0.25, null_prob_gemma=0.6, null_prob_bert=0.6)
    assert tr.text_loss and tr.text_loss_weight == 0.25 and tr.last_text_loss.shape == () and tr.last_img_loss.shape == ()
    t1 = _trainer(plain, tmp_path, null_prob_gemma=0.6, null_prob_bert=0.6)
    torch.manual_seed(7)
    a = t1._draw()
    torch.manual_seed(7)
    d = tr._draw()
    assert len(d) == 9 and all(torch.equal(x, y) for x, y in zip(a[3:], d[3:7])) and bool(d[5].any()) and bool(d[6].any())
    torch.manual_seed(7)
    t1._sample_conditioning(2)
    raw = torch.rand(2, 154, dtype=torch.float) < 0.25
    masked, labels, mask, n_gemma, n_bert = d[1], d[7], d[8], d[5], d[6]
    want = torch.cat([raw[:, :77] & n_gemma[:, None], raw[:, 77:] & n_bert[:, None]], dim=1)
    assert mask.dtype == torch.bool and torch.equal(mask, want)
    assert labels.shape == (2, 154, 2304) and torch.equal(masked, labels * ~mask[:, :, None]) and masked.dtype == labels.dtype


def test_train_py_has_the_option():
    with open(os.path.join(os.path.dirname(GOLD), "..", "train.py")) as f:
        src = f.read()
    assert '"--text-loss-weight"' in src and "default=0.0" in src.split('"--text-loss-weight"')[1].split("\n")[0]
    assert "text_loss=(a.text_loss_weight > 0.0)" in src and "text_loss_weight=a.text_loss_weight" in src


def test_fixture_mask_counts():
    gold = np.load(os.path.join(GOLD, "forward_micro_textloss.npz"))
    mask = A.grad_inputs()[5]
    assert np.array_equal(gold["mask"], mask.numpy()) and list(gold["mask_counts"]) == [19, 13] == [int(mask[:, :77].sum()), int(mask[:, 77:].sum())]
    assert os.path.getsize(os.path.join(GOLD, "forward_micro_textloss.npz")) <= os.path.getsize(os.path.join(GOLD, "forward_micro_kvmerge.npz"))
    for rec, n in (("T", 107), ("S", 120)):
        assert len(gold[rec + "_names"]) == len(gold[rec + "_norms"]) == len(gold[rec + "_samples"]) == len(gold[rec + "_bf16_rel"]) == n
    zero = [str(n) for n, v in zip(gold["T_names"], gold["T_norms"]) if v == 0.0]
    assert zero == ["blocks.2.attn.query_proj_x.weight", "blocks.2.attn.q_norm_x.weight"]
    with open(os.path.join(GOLD, "generation_report_textloss.json")) as f:
        rep = json.load(f)
    assert rep["mask_counts"] == [19, 13] and rep["image_only_gradients_vs_grads_micro_max_abs_dev"] == 0.0 and rep["forward"]["v_bit_equal_to_micro_plain"]
    assert abs(rep["forward"]["txt_pred_bf16_rel"] - float(gold["txt_bf16_rel"])) < 1e-12


# ---------------------------------------------------------------------------------------------- yardstick soundness
def rounding_model(pred, label, mask, coef, out_dtype):
    """The header's evaluation with float64 arithmetic rounded to fp32 (to out_dtype for dpred) at the documented points and nowhere else."""
    f32 = lambda t: t.float().double()      # noqa: E731
    rows, cols = pred.shape
    c32 = float(np.float32(coef))
    d = f32(pred.double() - label.double()) * mask[:, None].double()
    dpred = f32(float(np.float32(2.0 * c32)) * d).to(out_dtype)
    groups = -(-rows // A.ROWS)
    grid = min(groups, A.PARTS)
    iters, steps = -(-groups // grid), -(-cols // A.WAVE_COLS)
    D = torch.zeros(iters * grid * A.ROWS, steps * A.WAVE_COLS, dtype=torch.float64)
    D[:rows, :cols] = d
    D = D.view(iters, grid, A.ROWS, steps, 64, A.LANE_COLS)
    s = torch.zeros(grid, A.ROWS, 64, dtype=torch.float64)
    for it in range(iters):            # 1. the serial fma chain of every lane
        for st in range(steps):
            for e in range(A.LANE_COLS):
                x = D[it, :, :, st, :, e]
                s = f32(x * x + s)
    lane = torch.arange(64)

    def butterfly(v):                  # 2. xor-butterfly, offsets 32 .. 1
        for o in (32, 16, 8, 4, 2, 1):
            v = f32(v + v[..., lane ^ o])
        return v
    w = butterfly(s)[..., 0]           # (grid, ROWS)
    part = w[:, 0]
    for k in range(1, A.ROWS):         # 3. wave sums in wave order
        part = f32(part + w[:, k])
    P = torch.zeros(-(-grid // 64) * 64, dtype=torch.float64)
    P[:grid] = part
    t = torch.zeros(64, dtype=torch.float64)
    for row in P.view(-1, 64):         # 4. 64 lanes over the partials, butterfly, * coef
        t = f32(t + row)
    return f32(butterfly(t)[0] * c32), dpred


def test_rounding_model_stays_inside_the_bars():
    """See the module docstring.  One pass over the shapes and masks of the GPU sweep, every pred / label dtype combination, dpred in both dtypes;
    prints the worst ratio per output."""
    torch.set_num_threads(8)
    worst = {"loss": [0.0, ""], "dpred bf16": [0.0, ""], "dpred fp32": [0.0, ""]}
    seen_wrap = False
    for rows, cols in A.SHAPES:
        p32, l32, coef = A.make_case(rows, cols)
        ins = {A.F32: (p32, l32), A.BF16: (p32.to(A.BF16), l32.to(A.BF16))}
        bar = A.loss_bar(rows, cols)
        seen_wrap |= -(-rows // A.ROWS) > A.PARTS
        for kind in A.MASKS:
            mask = A.make_mask(kind, rows)
            for pdt in (A.BF16, A.F32):
                for ldt in (A.BF16, A.F32):
                    pred, label = ins[pdt][0], ins[ldt][1]
                    ref_loss, ref_d = A.reference(pred, label, mask, coef)
                    for odt in (A.BF16, A.F32):
                        loss, d = rounding_model(pred, label, mask, coef, odt)
                        where = f"r{rows}-c{cols}-{kind}-{str(pdt)[6:]}/{str(ldt)[6:]}/{str(odt)[6:]}"
                        if not bool(mask.any()):
                            assert float(loss) == 0.0 and not bool(d.float().abs().any())
                            continue
                        rl = abs(float(loss - ref_loss)) / float(ref_loss) / bar
                        lim = ((A.U if odt == A.BF16 else 0.0) + 4 * A.E32) * ref_d.abs()
                        rd = float(((d.double() - ref_d).abs() / lim.clamp_min(1e-300))[mask].max())
                        assert not bool(d[~mask].float().abs().any())
                        for k, v in (("loss", rl), ("dpred " + ("bf16" if odt == A.BF16 else "fp32"), rd)):
                            if v > worst[k][0]:
                                worst[k] = [v, where]
    print("\n[text_loss rounding model] worst ratio to the bar over %d shapes x %d masks x 8 dtype combinations: " % (len(A.SHAPES), len(A.MASKS))
          + ", ".join(f"{k} {v[0]:.3f} (@ {v[1]})" for k, v in worst.items()))
    assert seen_wrap
    for k, (v, where) in worst.items():
        assert 0.0 < v <= 1.0, (k, v, where)


def test_sweep_covers_the_launch_edges():
    R, P = A.ROWS, A.PARTS
    assert {1, R - 1, R, R + 1, R * P - 1, R * P, R * P + 1} == set(A.ROW_SIZES) and A.COL_SIZES == [8, 16, 2056, 2304]
    assert A.grid_of(R * P) == P == A.grid_of(R * P + 1) and A.grid_of(R * P - 1) == P and A.grid_of(R + 1) == 2
    assert A.serial_length(R * P + 1, 2304) == 2 * A.serial_length(R * P, 2304) == 2 * 5 * 8      # the grid-stride wraps: a second row group per workgroup
    assert 2056 % A.WAVE_COLS and 2056 % 8 == 0 and -(-2056 // A.WAVE_COLS) == 5 and 16 < A.WAVE_COLS
    assert A.MASKS == ["none", "all", "first", "last", "alternating", "seeded25"] and len(A.DTYPES) == 8
    assert A.loss_roundings(1, 2304) == 59 and A.loss_roundings(R * P + 1, 2304) == 102 and A.loss_bar(R * P + 1, 2304) < 1e-5 < R * P * 2304 * A.E32
