"""Opt-in e4m3 attention (csrc/attention_e4m3.hip, mmdit_attn_fwd_e4m3) on the GPU: per-row float64 parity at the kernel's tile edges, ill-scaled
inputs, the MX output form, argument errors, and the model-level opt-in (set_precision(..., attention="e4m3")).

References, float64 on the CPU from the same bf16 inputs:
  A   exact attention.
  E   attention with the operands quantised at the kernel's documented rounding points (header comment of csrc/attention_e4m3.hip):
      pow2(a) = 2^floor(log2(448 / a)) (1 for a = 0); Q and K per row e4m3(row * pow2(amax)); scores from the quantised operands, de-scaled,
      times `scale`; P = e4m3(256 exp(s - FINAL row max)); V per tile of T keys e4m3(V * pow2(amax of the tile)); O = P8 V8 / (256 l),
      l the sum of the unrounded p.  Casts are torch.float8_e4m3fn (round to nearest even) behind a clamp to +-448.
Bar, per output row (one query of one batch and head), K the kernel's output:
      |K - A|inf <= 2 |E - A|inf + 2^-7 |A|inf
  factor 2: the one rounding point E cannot restate -- the online softmax quantises P relative to the RUNNING maximum, not the final one;
  additive term: one bf16 output rounding.  The test prints the worst ratio  |K - A|inf / (2 |E - A|inf + 2^-7 |A|inf)  per case
  (measured values: profiles/attn_e4m3.txt)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 0.125


def _tiles():
    import sd3_amd  # noqa: F401
    from sd3_amd import _lib
    return _lib.ATTN_E4M3_KEY_TILE, _lib.ATTN_E4M3_QUERY_TILE


T, TQ = _tiles()
SHAPES = [(T - 1, 0), (T - 1, T - 1), (T, T // 2), (T + 1, 1), (2 * T + 5, TQ + 3), (410, 256)]       # (S, n_img); B = 1, H = 2
ILL = ["row64", "flat", "vtile1000"]                                                                    # at S = T + 1
B, H = 1, 2


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ---------------------------------------------------------------------------------------------- inputs and references
def make_inputs(S, family="random"):
    """Seeded randn bf16 (Q, K, V), each (B, H, S, 64), on the CPU."""
    g = torch.Generator().manual_seed(7001 * S + 13 * (["random"] + ILL).index(family))
    Q, K, V = (torch.randn(B, H, S, 64, generator=g) for _ in range(3))
    if family == "row64":          # one query row and one key row 64 x larger than the rest
        Q[:, :, 5] *= 64.0
        K[:, :, 7] *= 64.0
    elif family == "flat":         # all keys identical: uniform softmax
        K = K[:, :, :1].expand(B, H, S, 64).contiguous()
    elif family == "vtile1000":    # the first key tile of V 1000 x larger than the second
        V[:, :, :T] *= 1000.0
    return Q.to(torch.bfloat16), K.to(torch.bfloat16), V.to(torch.bfloat16)


def _pow2(amax):
    """2^e with amax * 2^e in (224, 448]: e = floor(log2(448 / amax)), from the exponent and mantissa of amax (exact); 1 for amax = 0."""
    mant, ex = torch.frexp(amax)                                     # amax = mant * 2^ex, 0.5 <= mant < 1
    e = 8 - (ex - 1) - (2.0 * mant > 1.75).to(ex.dtype)
    return torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax))


def _e4m3(x):
    return x.clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn).double()


def ref_exact(Q, K, V):
    Q, K, V = Q.double(), K.double(), V.double()
    return torch.softmax(SCALE * Q @ K.mT, -1) @ V


def ref_e4m3(Q, K, V):
    Q, K, V = Q.double(), K.double(), V.double()
    S = Q.shape[2]
    sq, sk = _pow2(Q.abs().amax(-1, keepdim=True)), _pow2(K.abs().amax(-1, keepdim=True))
    s = (_e4m3(Q * sq) @ _e4m3(K * sk).mT) / (sq * sk.mT) * SCALE
    p = torch.exp(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    P8 = _e4m3(256.0 * p)
    V8 = torch.empty_like(V)
    for t0 in range(0, S, T):
        tile = V[:, :, t0:t0 + T]
        sv = _pow2(tile.abs().amax((-1, -2), keepdim=True))
        V8[:, :, t0:t0 + T] = _e4m3(tile * sv) / sv
    return (P8 @ V8) / (256.0 * l)


def _merge(Ox, Oc):
    parts = [o for o in (Ox, Oc) if o is not None and o.shape[1] > 0]
    m = torch.cat(parts, 1) if len(parts) > 1 else parts[0]
    return m.reshape(m.shape[0], m.shape[1], H, 64).permute(0, 2, 1, 3)


def _row_ratio(Kout, A, E):
    """per row: |K - A|inf / (2 |E - A|inf + 2^-7 |A|inf) -> (B, H, S)"""
    inf = lambda x: x.abs().amax(-1)
    return inf(Kout - A) / (2.0 * inf(E - A) + 2.0 ** -7 * inf(A))


_REFS = {}


def refs(S, family="random"):
    """Inputs and both references of one case, computed once and shared by the tests that need them."""
    if (S, family) not in _REFS:
        Q, K, V = make_inputs(S, family)
        A, E = ref_exact(Q, K, V), ref_e4m3(Q, K, V)
        assert bool(torch.isfinite(E).all()) and bool(torch.isfinite(A).all()), (S, family)
        _REFS[(S, family)] = (Q, K, V, A, E)
    return _REFS[(S, family)]


def _run(ops, Q, K, V, n_img):
    Ox, Oc = ops.attn_fwd_e4m3(Q.cuda(), K.cuda(), V.cuda(), n_img, SCALE)
    S = Q.shape[2]
    assert Ox.shape == (B, n_img, H * 64) and Ox.dtype == torch.bfloat16
    assert (Oc is None) == (n_img == S) and (Oc is None or Oc.shape == (B, S - n_img, H * 64))
    return Ox, Oc, _merge(Ox, Oc).double().cpu()


# ---------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("S,n_img", SHAPES, ids=lambda v: str(v))
def test_rows_within_the_bar(ops, S, n_img):
    Q, K, V, A, E = refs(S)
    _, _, out = _run(ops, Q, K, V, n_img)
    assert bool(torch.isfinite(out).all())
    ratio = _row_ratio(out, A, E)
    agg = float((out - A).norm() / A.norm())
    print(f"[attn e4m3] S={S} n_img={n_img}: worst row ratio {float(ratio.max()):.3f} (row {int(ratio.argmax())}), median {float(ratio.median()):.3f}; "
          f"||K-A||/||A|| = {agg:.3e}, ||E-A||/||A|| = {float((E - A).norm() / A.norm()):.3e}")
    assert float(ratio.max()) <= 1.0, (S, n_img, int(ratio.argmax()), float(ratio.max()))
    if S == 410:     # the e4m3 path ran, not a bf16 fallback: its aggregate error exceeds the bf16 kernel's on the same inputs
        Ox0, Oc0, _ = ops.attn_fwd(Q.cuda(), K.cuda(), V.cuda(), n_img, SCALE, 0)
        agg0 = float((_merge(Ox0, Oc0).double().cpu() - A).norm() / A.norm())
        print(f"[attn e4m3] S={S}: mmdit_attn_fwd mode 0 ||K-A||/||A|| = {agg0:.3e}")
        assert agg > agg0, (agg, agg0)


@pytest.mark.parametrize("family", ILL)
def test_ill_scaled_inputs(ops, family):
    S = T + 1
    Q, K, V, A, E = refs(S, family)
    _, _, out = _run(ops, Q, K, V, 1)
    assert bool(torch.isfinite(out).all())
    ratio = _row_ratio(out, A, E)
    print(f"[attn e4m3] S={S} {family}: worst row ratio {float(ratio.max()):.3f} (row {int(ratio.argmax())})")
    if family == "row64":
        # per-row scales keep every other row inside the bar (and the scaled row itself: asserted with the rest below)
        print(f"[attn e4m3] S={S} {family}: the scaled query row {float(ratio[:, :, 5].max()):.3f}, the other rows {float(ratio[:, :, torch.arange(S) != 5].max()):.3f}")
    if family == "flat":                                         # uniform softmax: the output is the mean of V
        mean = V.double().mean(2, keepdim=True).expand_as(A)
        assert float((A - mean).abs().max()) < 1e-12
        assert float(_row_ratio(out, mean, E).max()) <= 1.0
    assert float(ratio.max()) <= 1.0, (family, int(ratio.argmax()), float(ratio.max()))


@pytest.mark.parametrize("S,n_img", [(T + 1, 1), (410, 256)], ids=lambda v: str(v))
def test_mx_form_is_the_quantised_bf16_form(ops, S, n_img):
    """Codes and E8M0 scale bytes equal mmdit_mxfp8_quantize of the bf16 form's output, bit for bit."""
    Q, K, V, _, _ = refs(S)
    Ox, Oc, _ = _run(ops, Q, K, V, n_img)
    mxx, mxc = ops.attn_fwd_e4m3(Q.cuda(), K.cuda(), V.cuda(), n_img, SCALE, mx=True)
    assert isinstance(mxx, ops.MxAct) and isinstance(mxc, ops.MxAct)
    for mx, o in ((mxx, Ox), (mxc, Oc)):
        rows, D = o.shape[0] * o.shape[1], o.shape[2]
        q_ref, sc_ref = ops.quant_mxfp8(o.reshape(rows, D))
        assert mx.q.shape == (rows, D) and mx.q.dtype == torch.float8_e4m3fn
        assert torch.equal(mx.q.view(torch.uint8), q_ref.view(torch.uint8)), (S, "codes")
        assert torch.equal(ops.mx_scales_to_rows(mx.sc, rows, D), ops.mx_scales_to_rows(sc_ref, rows, D)), (S, "scales")


def test_argument_errors(ops):
    """S = 0, n_img > S and a NULL output return the library's error status; the outputs are not touched."""
    from sd3_amd import _lib
    S = T
    Q = torch.randn(B, H, S, 64, device="cuda").to(torch.bfloat16)
    Ox = torch.full((B, S, H * 64), 7.0, dtype=torch.bfloat16, device="cuda")
    Oc = torch.full((B, S, H * 64), 7.0, dtype=torch.bfloat16, device="cuda")
    fn, st = _lib.lib().mmdit_attn_fwd_e4m3, torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert fn(p(Q), p(Q), p(Q), B, H, 0, 0, SCALE, p(Ox), p(Oc), None, None, st) == _lib.ERR_SHAPE
    assert fn(p(Q), p(Q), p(Q), B, H, S, S + 1, SCALE, p(Ox), p(Oc), None, None, st) == _lib.ERR_SHAPE
    assert fn(p(Q), p(Q), p(Q), B, H, S, -1, SCALE, p(Ox), p(Oc), None, None, st) == _lib.ERR_SHAPE
    assert fn(p(Q), p(Q), p(Q), B, H, S, S // 2, SCALE, None, p(Oc), None, None, st) == _lib.ERR_ARG
    assert fn(p(Q), p(Q), p(Q), B, H, S, S // 2, SCALE, p(Ox), None, None, None, st) == _lib.ERR_ARG
    assert fn(p(Q), p(Q), p(Q), B, H, S, S // 2, SCALE, p(Ox), p(Oc), p(Ox), None, st) == _lib.ERR_ARG     # MX form without the text stream's scales
    assert fn(None, p(Q), p(Q), B, H, S, S // 2, SCALE, p(Ox), p(Oc), None, None, st) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((Ox == 7.0).all()) and bool((Oc == 7.0).all())
    with pytest.raises(RuntimeError, match="mmdit_attn_fwd_e4m3"):
        ops.attn_fwd_e4m3(Q, Q, Q, S + 1, SCALE)


# ---------------------------------------------------------------------------------------------- model level
CONFIGS = {"micro": (dict(dim=128, num_heads=2, num_blocks=3), 16, 16), "xs": (dict(dim=256, num_heads=4, num_blocks=2), 64, 64)}
_nets = {}


def _net(cname):
    from oracle.weights import make_state_dict
    from sd3_amd.models.diff_model import diff_model
    if cname not in _nets:
        cfg = CONFIGS[cname][0]
        net = diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu",
                         device=torch.device("cuda:0"), positional_encoding="RoPE2d", checkpoint_MLP=False, checkpoint_attn=False, **cfg)
        net.load_state_dict(make_state_dict(0, **cfg), strict=True)
        _nets[cname] = net
    return _nets[cname]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("cname", list(CONFIGS))
def test_model_forward_with_e4m3_attention(ops, cname):
    """"fp8" / "mxfp8" with attention="e4m3": finite, and as close to the bf16 fast forward as the project asks of its fp8 mode
    (test_fp8_inference_mode: 1e-4 < rel-L2 < 8e-2); set_precision("mxfp8") afterwards is the pre-feature mxfp8 forward bit for bit."""
    from oracle.weights import make_inputs as model_inputs
    from sd3_amd import engine
    _, h, w = CONFIGS[cname]
    net = _net(cname)
    x, c, cp = model_inputs(21, 2, h, w, text_scale=30.0)
    t = torch.tensor([0.2, 0.9])
    fwd = lambda: net(x.cuda(), t, c.clone().cuda(), cp.clone().cuda())
    try:
        with torch.no_grad():
            net.set_precision("fast")
            v_fast = fwd()
            net.set_precision("mxfp8")
            v_mx_before = fwd()
            for prec in ("fp8", "mxfp8"):
                net.set_precision(prec)
                r_bf16 = _rel(fwd(), v_fast)
                net.set_precision(prec, attention="e4m3")
                assert engine.FP8.attn_e4m3 == (prec == "fp8") and engine.MXFP8.attn_e4m3 == (prec == "mxfp8")
                v = fwd()
                r = _rel(v, v_fast)
                print(f"[attn e4m3] {cname} {prec}: forward rel-L2 vs bf16 fast mode: e4m3 attention {r:.3e}, bf16 attention {r_bf16:.3e}")
                assert bool(torch.isfinite(v).all()) and 1e-4 < r < 8e-2, (cname, prec, r)
                assert not torch.equal(v, v_fast)
            net.set_precision("mxfp8")
            assert torch.equal(fwd(), v_mx_before)
    finally:
        net.set_precision("fast")


def test_sampler_runs_with_e4m3_attention(ops):
    """4-step Euler sample_imgs on the micro model in "mxfp8" + e4m3 attention, stand-in text encoder / VAE objects."""
    from oracle.weights import make_inputs as model_inputs

    class _Cfg:
        latent_channels, shift_factor, scaling_factor = 16, 0.1159, 0.3611

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

    net = _net("micro")
    _, th, tp = model_inputs(40, 1, 16, 16, text_scale=30.0)
    net.text_encoders = _Enc(th, tp)
    try:
        net.set_precision("mxfp8", attention="e4m3")
        img = net.sample_imgs(2, 4, ["x"], cfg_scale=3.0, width=128, height=128, sampler="euler", generator=torch.Generator().manual_seed(99))
        assert img.shape == (2, 16, 16, 16) and bool(torch.isfinite(img).all())
    finally:
        del net.text_encoders
        net.train()
        net.set_precision("fast")
