"""fp8 / mxfp8 inference at odd head counts on the GPU: the zero-padding e4m3 quantisers (csrc/fp8_pad.hip, include/mmdit_hip_fp8pad.h) through the
C ABI with the test's own buffers, the unchanged e4m3 GEMM kernels on padded operands, and the model path (engine._to_fp8).

With dim = 64 * heads an odd head count gives K = dim = 64 (mod 128); the e4m3 GEMM kernels need K % 128 == 0.  The quantisers write both operands
into rows padded with zero codes to K_pad = the next multiple of 128 and the GEMM runs on K_pad: a zero code times anything is zero.

Kernel tests: every output buffer is pre-filled with 0xFF (an e4m3fn NaN code, the E8M0 NaN scale) before every call; the padded quantisers are held
bit for bit to the plain ones on the same x (columns [0, K), the first K / 32 scales per row, dequantisation scale / state), the pad to 0x00 and the
all-zero-block scale code, and once to a torch restatement.  The GEMM on padded operands is held to the float64 product of the DEQUANTISED operands
with the per-element / per-row / per-column yardstick of tests/test_gemm_edges_gpu.py (its ratios() and bars, c = (K_pad + 8) 2^-23).
Model tests: every QKV / out-projection / MLP launch of a dim = 192 and a dim = 1216 model takes e4m3 operands with K % 128 == 0 (fails on the
parent commit: three of the four sites stayed bf16), the forward stays inside the windows the project holds its fp8 modes to, nothing changes where
nothing is padded, the sampler equals a loop over forward, the padded weight caches follow the pack generation."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROWS = (1, 127, 128, 129, 300)      # a partial 128-row scale group, exactly one, one row past it, two groups and a partial third
K_PADDED = (64, 192, 1216)          # the pad is the second half of the only tile / of the second tile / of the tenth
K_PLAIN = (128, 256)                # no padding: the plain entry points' outputs byte for byte
FF = 0xFF


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def _L():
    from sd3_amd import _lib
    return _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(t):
    L = _L()
    return L.BF16 if t.dtype == torch.bfloat16 else L.F32


def _x(rows, K, dtype, seed, ld_extra=0):
    """Operand (rows, K) with block magnitudes 2^-6 .. 2^6 and one all-zero 32-block, as a view with leading dimension K + ld_extra into a NaN tensor."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, K), generator=g)
    x = (x.view(rows, K // 32, 32) * torch.exp2(torch.randint(-6, 7, (rows, K // 32, 1), generator=g).float())).view(rows, K)
    x[0, :32] = 0.0
    big = torch.full((rows, K + ld_extra), float("nan"), dtype=dtype, device="cuda")
    big[:, :K] = x.to(dtype).cuda()
    return big[:, :K]


def _ff(*shape):
    return torch.full(shape, FF, dtype=torch.uint8, device="cuda")


def _k_pad(K):
    return (K + 127) // 128 * 128


def _amax(x):
    """mmdit_fp8_amax over the elements of x (a contiguous copy: the entry point takes an element count)."""
    L = _L()
    a = torch.zeros(1, dtype=torch.float32, device="cuda")
    xc = x.contiguous()
    assert L.lib().mmdit_fp8_amax(_p(xc), _dt(xc), xc.numel(), _p(a), _st()) == 0
    return a


_zero_code = []


def zero_block_code():
    """The scale byte the plain MX quantiser gives an all-zero block (2^-127)."""
    if not _zero_code:
        L = _L()
        z = torch.zeros((1, 64), dtype=torch.bfloat16, device="cuda")
        q, sc = _ff(1, 64), _ff(_mx_bytes(1, 64))
        assert L.lib().mmdit_mxfp8_quantize(_p(z), L.BF16, 1, 64, 64, _p(q), _p(sc), _st()) == 0
        by = _scale_rows(sc, 1, 64)
        assert int(by[0, 0]) == int(by[0, 1]) == 0 and int(q.max()) == 0
        _zero_code.append(int(by[0, 0]))
    return _zero_code[0]


def _mx_bytes(rows, K):
    return (K // 64) * ((rows + 127) // 128 * 128) * 2 + 512


def _scale_rows(sc, rows, K):
    """(rows, K / 32) view of the scale bytes: the layout of mmdit_gemm_args.scale_mode 1 restated from the core header (per 64-wide K half the rows in
    groups of 128, inside a group the byte of (row, half-block h) at (row & 31) * 8 + h * 4 + ((row >> 5) & 3))."""
    rp = (rows + 127) // 128 * 128
    return sc[:(K // 64) * rp * 2].view(K // 64, rp // 128, 32, 2, 4).permute(1, 4, 2, 0, 3).reshape(rp, K // 32)[:rows]


def _check_codes(q, q_plain, rows, K, what):
    Kp = _k_pad(K)
    assert q.shape == (rows, Kp)
    assert torch.equal(q[:, :K], q_plain.view(rows, K)), (what, "codes of [0, K)")
    assert int(q[:, K:].to(torch.int32).abs().sum()) == 0, (what, "pad bytes are not 0x00")


# ---------------------------------------------------------------------------------------------- 1: padded quantisers against the plain ones
def _quantiser_case(rows, K, dtype, ld_extra=0):
    L = _L()
    lib = L.lib()
    Kp = _k_pad(K)
    x = _x(rows, K, dtype, 1000 * rows + K, ld_extra)
    xc = x.contiguous()
    ldx = x.stride(0)
    what = (rows, K, str(dtype), ld_extra)
    # per-tensor, two passes
    amax = _amax(x)
    q0, s0 = _ff(rows * K), torch.full((1,), float("nan"), device="cuda")
    assert lib.mmdit_fp8_quantize(_p(xc), _dt(x), rows * K, _p(amax), _p(q0), _p(s0), _st()) == 0
    q1, s1 = _ff(rows, Kp), torch.full((1,), float("nan"), device="cuda")
    assert lib.mmdit_fp8_quantize_pad(_p(x), _dt(x), rows, K, ldx, _p(amax), _p(q1), _p(s1), _st()) == 0
    _check_codes(q1, q0, rows, K, what + ("per-tensor",))
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and float(s1) > 0
    # delayed scaling: three calls on three different activations, so that every slot of the amax ring is read, written and cleared with padding
    st0, st1 = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    st0[:1], st1[:1] = amax, amax
    for phase, gain in enumerate((1.0, 1.3, 0.4)):
        xp = (x.float() * gain).to(dtype)      # (dense: leading dimension K)
        margin = 1.0 if phase == 0 else 1.5
        q0, q1 = _ff(rows * K), _ff(rows, Kp)
        assert lib.mmdit_fp8_quantize_delayed(_p(xp), _dt(xp), rows * K, _p(st0), phase, margin, _p(q0), _st()) == 0
        assert lib.mmdit_fp8_quantize_delayed_pad(_p(xp), _dt(xp), rows, K, K, _p(st1), phase, margin, _p(q1), _st()) == 0
        _check_codes(q1, q0, rows, K, what + ("delayed", phase))
        assert torch.equal(st0.view(torch.int32), st1.view(torch.int32)), (what, "state", phase, st0.tolist(), st1.tolist())
        assert float(st1[(phase + 1) % 3]) == float(xp.float().abs().max()) and float(st1[(phase + 2) % 3]) == 0.0
    # MX
    q0, sc0 = _ff(rows, K), _ff(_mx_bytes(rows, K))
    assert lib.mmdit_mxfp8_quantize(_p(x), _dt(x), rows, K, ldx, _p(q0), _p(sc0), _st()) == 0
    q1, sc1 = _ff(rows, Kp), _ff(_mx_bytes(rows, Kp))
    assert lib.mmdit_mxfp8_quantize_pad(_p(x), _dt(x), rows, K, ldx, _p(q1), _p(sc1), _st()) == 0
    _check_codes(q1, q0, rows, K, what + ("mx",))
    by = _scale_rows(sc1, rows, Kp)
    assert torch.equal(by[:, :K // 32], _scale_rows(sc0, rows, K)), (what, "scales of [0, K)")
    assert bool((by[:, K // 32:] == zero_block_code()).all()), (what, "pad-block scales")
    assert int((by == FF).sum()) == 0, (what, "an unwritten scale byte of a real row")
    # ... and nothing else was written: the bytes of the rows between rows and rows_pad128 and the 512 spare bytes keep the fill
    idx = _scale_rows(torch.arange(sc1.numel(), device="cuda"), rows, Kp).reshape(-1)
    other = torch.ones(sc1.numel(), dtype=torch.bool, device="cuda")
    other[idx] = False
    assert bool((sc1[other] == FF).all()), (what, "scale bytes outside the real rows were written")
    if Kp == K:      # no padding: the plain entry points' outputs byte for byte
        assert torch.equal(q1, q0) and torch.equal(sc1, sc0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", K_PADDED + K_PLAIN)
def test_padded_quantisers_equal_the_plain_ones(ops, K, dtype):
    for rows in ROWS:
        _quantiser_case(rows, K, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_padded_quantisers_with_a_wider_leading_dimension(ops, dtype):
    """ldx > K: the operand is a view into a NaN tensor (a read past column K would reach the amax and the codes)."""
    _quantiser_case(129, 192, dtype, ld_extra=64)
    _quantiser_case(300, 64, dtype, ld_extra=8)


def test_ops_wrappers_pad_on_request_only(ops):
    x = _x(129, 192, torch.bfloat16, 5).contiguous()
    for fn in (ops.quant_fp8, ops.quant_mxfp8):
        (q, s), (qp, sp) = fn(x), fn(x, pad=True)
        assert q.shape == (129, 192) and qp.shape == (129, 256) and qp.dtype == torch.float8_e4m3fn
        assert torch.equal(qp.view(torch.uint8)[:, :192], q.view(torch.uint8)) and int(qp.view(torch.uint8)[:, 192:].max()) == 0
    assert torch.equal(ops.quant_fp8(x)[1], ops.quant_fp8(x, pad=True)[1]) and ops.quant_mxfp8(x, pad=True)[1].numel() == ops.mx_scale_bytes(129, 256)
    a, b = ops.Fp8Site(), ops.Fp8Site()      # two sites in step: the same state and codes, padded or not
    for k in range(4):
        (q, s), (qp, sp) = a.quantise(x * (1 + k)), b.quantise(x * (1 + k), pad=True)
        assert q.shape == (129, 192) and qp.shape == (129, 256) and torch.equal(a.state, b.state) and torch.equal(s, sp) and a.phase == b.phase == k + 1
        assert torch.equal(qp.view(torch.uint8)[:, :192], q.view(torch.uint8)) and int(qp.view(torch.uint8)[:, 192:].max()) == 0
    y = _x(129, 256, torch.bfloat16, 6).contiguous()
    for fn in (ops.quant_fp8, ops.quant_mxfp8, ops.Fp8Site().quantise):
        assert fn(y, pad=True)[0].shape == (129, 256)
    assert ops.quant_fp8(x.view(3, 43, 192), pad=True)[0].shape == (3, 43, 192)      # (not 2-D: today's path)


# ---------------------------------------------------------------------------------------------- 2: an independent restatement in torch
def test_padded_quantisers_equal_a_torch_restatement(ops):
    """(rows, K) = (129, 192).  Per-tensor: scale = amax / 448, codes = e4m3fn(saturate(x * (448 / amax))) in fp32 (the kernel multiplies by the
    reciprocal scale).  MX (core header): per 32-block the smallest 2^e with amax / 2^e <= 448 -- e = floor(log2 amax) - 8, one more when the mantissa
    of amax exceeds 1.75, 2^-127 for an all-zero block --, codes = e4m3fn(saturate(x / 2^e)).  The pad: zero codes, scale byte 0."""
    L = _L()
    lib = L.lib()
    rows, K, Kp = 129, 192, 256
    x = _x(rows, K, torch.bfloat16, 77).contiguous()
    xf = x.float().cpu()
    a = xf.abs().max()
    want = torch.zeros((rows, Kp), dtype=torch.uint8)
    want[:, :K] = (xf * (torch.tensor(448.0) / a)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    amax = _amax(x)
    q, s = _ff(rows, Kp), torch.zeros(1, device="cuda")
    assert lib.mmdit_fp8_quantize_pad(_p(x), L.BF16, rows, K, K, _p(amax), _p(q), _p(s), _st()) == 0
    assert float(amax) == float(a) and float(s) == float(a / 448.0)
    bad = int((q.cpu() != want).sum())
    print(f"[fp8 pad] per-tensor codes differing from the torch restatement: {bad} of {rows * Kp}")
    assert bad == 0
    xb = xf.view(rows, K // 32, 32)
    am = xb.abs().amax(-1, keepdim=True)
    mant, ex = torch.frexp(am)                          # am = mant 2^ex, mant in [0.5, 1)
    e = torch.where(am > 0, ex - 1 - 8, torch.full_like(ex, -127))
    e = torch.where(2 * mant > 1.75, e + 1, e).clamp(-127, 127)
    want[:, :K] = (xb / torch.exp2(e.double()).float()).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).view(rows, K)
    want_sc = torch.zeros((rows, Kp // 32), dtype=torch.uint8)
    want_sc[:, :K // 32] = (e + 127).to(torch.uint8).view(rows, K // 32)
    q, sc = _ff(rows, Kp), _ff(_mx_bytes(rows, Kp))
    assert lib.mmdit_mxfp8_quantize_pad(_p(x), L.BF16, rows, K, K, _p(q), _p(sc), _st()) == 0
    assert torch.equal(q.cpu(), want) and torch.equal(_scale_rows(sc, rows, Kp).cpu(), want_sc)
    assert int(want_sc[0, 0]) == 0      # (the all-zero block of the operand)


# ---------------------------------------------------------------------------------------------- 3: the e4m3 GEMMs on padded operands
_gemm_ref = {}


def _gemm_operands(ops, M, N, K, mx):
    """Padded operands of one problem, their float64 dequantised values and the float64 product: computed once per (shape, mode)."""
    key = (M, N, K, mx)
    if key not in _gemm_ref:
        A, B = _x(M, K, torch.bfloat16, 31 * M + K).contiguous(), (_x(N, K, torch.bfloat16, 17 * N + K) * 0.05).to(torch.bfloat16).contiguous()
        if mx:
            (qa, sa), (qb, sb) = ops.quant_mxfp8(A, pad=True), ops.quant_mxfp8(B, pad=True)
            Kp = qa.shape[1]
            deq = lambda q, s, r: (q.float().double().view(r, Kp // 32, 32) * torch.exp2(_scale_rows(s, r, Kp).double() - 127.0).unsqueeze(-1)).view(r, Kp)      # noqa: E731
            A64, B64 = deq(qa, sa, M), deq(qb, sb, N)
        else:
            (qa, sa), (qb, sb) = ops.quant_fp8(A, pad=True), ops.quant_fp8(B, pad=True)
            A64, B64 = qa.float().double() * sa.double(), qb.float().double() * sb.double()
        assert qa.shape == (M, _k_pad(K)) and qb.shape == (N, _k_pad(K))
        assert float((A64[:, :K] - A.double()).norm() / A.double().norm()) < 4e-2      # (the operands are the quantised model operands, not noise)
        _gemm_ref[key] = (qa, sa, qb, sb, A64 @ B64.T, A64.abs() @ B64.abs().T)
    return _gemm_ref[key]


@pytest.mark.parametrize("mx", [0, 1], ids=["per-tensor", "mx"])
@pytest.mark.parametrize("M,N,K", [(130, 192, 192), (257, 1216, 1216), (64, 3648, 1216)])
def test_e4m3_gemm_on_padded_operands(ops, M, N, K, mx):
    """Both scale modes, fp32 and bf16 output, against the float64 product of the dequantised operands: the yardstick of test_gemm_edges_gpu.py with
    K_pad terms -- y = c |A| |B|^T (+ 2^-8 |ref| for a bf16 output), c = (K_pad + 8) 2^-23, for MX max(c, 2 kappa); bars 2.0 per element, 1.0 per
    row and per column, and the rounding-bias bar.  Then the pad columns of a COPY of A are overwritten with the code of 448 (and, MX, its pad-block
    scales with 2^0) while B's pad stays zero: the result must not move by a bit -- the kernels do read the pad, and a zero in either operand
    suffices."""
    import test_gemm_edges_gpu as G
    qa, sa, qb, sb, ref, absP = _gemm_operands(ops, M, N, K, mx)
    Kp = qa.shape[1]
    c = (Kp + 8) * G.E23
    det = (max(c, 2 * G.MX_KAPPA) if mx else c) * absP
    qa2, sa2 = qa.clone(), sa.clone()
    qa2.view(torch.uint8)[:, K:] = 0x7E      # e4m3fn 448
    if mx:
        by = torch.full((M, Kp // 32), 127, dtype=torch.uint8, device="cuda")
        by[:, :K // 32] = _scale_rows(sa, M, Kp)[:, :K // 32]
        sa2 = G.mx_pack(by, FF, FF)
        assert torch.equal(_scale_rows(sa2, M, Kp)[:, :K // 32], _scale_rows(sa, M, Kp)[:, :K // 32])
    assert float(qa2[:, K:].float().min()) == 448.0
    for out_dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        out = ops.gemm(qa, qb, out_dtype=out_dtype, scale_a=sa, scale_b=sb, scale_mode=mx)
        assert out.shape == (M, N) and bool(torch.isfinite(out).all())
        rnd = G.U * ref.abs() if out_dtype == torch.bfloat16 else torch.zeros_like(ref)
        r = G.ratios(out, ref, det, rnd)
        print(f"[fp8 pad gemm] {M}x{N}x{K} (K_pad {Kp}) {'mx' if mx else 'per-tensor'} -> {name}: worst ratio per element {r['el']:.3f}, row {r['row']:.3f}, "
              f"column {r['col']:.3f}, bias {r['bias']}")
        assert G.verdict(r) == [], (M, N, K, mx, name, r)
        out2 = ops.gemm(qa2, qb, out_dtype=out_dtype, scale_a=sa2, scale_b=sb, scale_mode=mx)
        assert torch.equal(out2, out), (M, N, K, mx, name, "448 in A's pad against B's zero pad moved the result")


# ---------------------------------------------------------------------------------------------- 4: argument checks
def test_argument_errors_write_nothing(ops):
    L = _L()
    lib = L.lib()
    rows, K = 5, 192
    x = torch.ones((rows, K), dtype=torch.bfloat16, device="cuda")
    amax = torch.ones(1, device="cuda")
    q, sc, s = _ff(rows, 256), _ff(_mx_bytes(rows, 256)), torch.full((4,), 7.0, device="cuda")
    X, Q, SC, S, AM, st = _p(x), _p(q), _p(sc), _p(s), _p(amax), _st()
    pt, dl, mx = lib.mmdit_fp8_quantize_pad, lib.mmdit_fp8_quantize_delayed_pad, lib.mmdit_mxfp8_quantize_pad
    # a NULL operand
    assert pt(None, L.BF16, rows, K, K, AM, Q, S, st) == pt(X, L.BF16, rows, K, K, None, Q, S, st) == L.ERR_ARG
    assert pt(X, L.BF16, rows, K, K, AM, None, S, st) == pt(X, L.BF16, rows, K, K, AM, Q, None, st) == L.ERR_ARG
    assert dl(None, L.BF16, rows, K, K, S, 0, 1.0, Q, st) == dl(X, L.BF16, rows, K, K, None, 0, 1.0, Q, st) == dl(X, L.BF16, rows, K, K, S, 0, 1.0, None, st) == L.ERR_ARG
    assert mx(None, L.BF16, rows, K, K, Q, SC, st) == mx(X, L.BF16, rows, K, K, None, SC, st) == mx(X, L.BF16, rows, K, K, Q, None, st) == L.ERR_ARG
    for bad_rows in (0, -3):
        assert pt(X, L.BF16, bad_rows, K, K, AM, Q, S, st) == dl(X, L.BF16, bad_rows, K, K, S, 0, 1.0, Q, st) == mx(X, L.BF16, bad_rows, K, K, Q, SC, st) == L.ERR_ARG
    # K off the 64-wide half tile (and K <= 0)
    for bad_K in (96, 32, 200, 0, -64):
        assert pt(X, L.BF16, rows, bad_K, 256, AM, Q, S, st) == dl(X, L.BF16, rows, bad_K, 256, S, 0, 1.0, Q, st) == mx(X, L.BF16, rows, bad_K, 256, Q, SC, st) == L.ERR_SHAPE
    # the leading dimension, the delayed form's phase and margin, the dtype
    assert pt(X, L.BF16, rows, K, 128, AM, Q, S, st) == mx(X, L.BF16, rows, K, 196, Q, SC, st) == L.ERR_ARG
    assert dl(X, L.BF16, rows, K, K, S, -1, 1.0, Q, st) == dl(X, L.BF16, rows, K, K, S, 0, 0.5, Q, st) == L.ERR_ARG
    assert pt(X, L.FP8, rows, K, K, AM, Q, S, st) == dl(X, L.FP8, rows, K, K, S, 0, 1.0, Q, st) == mx(X, L.FP8, rows, K, K, Q, SC, st) == L.ERR_DTYPE
    torch.cuda.synchronize()
    assert bool((q == FF).all()) and bool((sc == FF).all()) and bool((s == 7.0).all()) and float(amax) == 1.0


# ---------------------------------------------------------------------------------------------- model level
CONFIGS = {"h3": (dict(dim=192, num_heads=3, num_blocks=2), 16, 16), "h19": (dict(dim=1216, num_heads=19, num_blocks=2), 16, 16),
           "xs": (dict(dim=256, num_heads=4, num_blocks=2), 64, 64)}
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


def _inputs(cname):
    from oracle.weights import make_inputs
    _, h, w = CONFIGS[cname]
    x, c, cp = make_inputs(21, 2, h, w, text_scale=30.0)
    return x.cuda(), torch.tensor([0.2, 0.9]), c.cuda(), cp.cuda()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _forward(net, cname):
    x, t, c, cp = _inputs(cname)
    with torch.no_grad():
        return net(x, t, c.clone(), cp.clone())


def _record(monkeypatch, ops, net, cname):
    """One no_grad forward with every GEMM launch recorded: a list of launches, each a list of (A, B) per problem (the fused QKV launch of the bf16
    route counts when it runs: a refused one is followed by the grouped launch of the same problems)."""
    launches = []
    grouped, fused = ops.gemm_grouped, ops.gemm_qkv_norm_rope

    def rec_grouped(problems):
        launches.append([(p["A"], p["B"]) for p in problems])
        return grouped(problems)

    def rec_fused(problems, *a, **kw):
        out = fused(problems, *a, **kw)
        if out is not None:
            launches.append([(p["A"], p["B"]) for p in problems])
        return out

    with monkeypatch.context() as mp:
        mp.setattr(ops, "gemm_grouped", rec_grouped)
        mp.setattr(ops, "gemm_qkv_norm_rope", rec_fused)
        out = _forward(net, cname)
    return launches, out


@pytest.mark.parametrize("prec", ["fp8", "mxfp8"])
@pytest.mark.parametrize("cname", ["h3", "h19"])
def test_every_site_is_e4m3(ops, monkeypatch, cname, prec):
    """Fails on the parent commit: at dim = 192 / 1216 the QKV, out-projection and MLP-up launches (K = dim) stayed bf16, only MLP down was e4m3.
    The launches of the bf16 "fast" forward and of the e4m3 forward are the same sequence of weights; the ones that changed are exactly the four
    sites of every block, every problem of them with float8_e4m3fn A and B and A.shape[1] % 128 == 0."""
    from sd3_amd import engine
    net = _net(cname)
    d, nb = CONFIGS[cname][0]["dim"], CONFIGS[cname][0]["num_blocks"]
    try:
        net.set_precision("fast")
        fast, _ = _record(monkeypatch, ops, net, cname)
        net.set_precision(prec)
        low, out = _record(monkeypatch, ops, net, cname)
        cache = engine.MXFP8._q if prec == "mxfp8" else engine.FP8._q
        origin = {id(ent[1]): ent[0] for ent in cache.values()}      # e4m3 weight copy -> the bf16 weight it was made from
        assert bool(torch.isfinite(out).all())
        assert len(low) == len(fast)
        sites = []
        for lf, ll in zip(fast, low):
            assert len(lf) == len(ll)
            e4 = [B.dtype == torch.float8_e4m3fn for _, B in ll]
            assert all(e4) or not any(e4)
            for (Af, Bf), (Al, Bl) in zip(lf, ll):
                if e4[0]:
                    assert origin[id(Bl)].data_ptr() == Bf.data_ptr() and Bf.dtype == torch.bfloat16             # the same weight, quantised
                    assert Al.dtype == torch.float8_e4m3fn and Al.shape[1] % 128 == 0 and Al.shape[1] == Bl.shape[1] == ops.fp8_k_pad(Bf.shape[1])
                    assert Al.shape[0] == Af.shape[0] and Bl.shape[0] == Bf.shape[0]
                else:
                    assert Bl.data_ptr() == Bf.data_ptr() and Bl.dtype == Bf.dtype and Al.dtype == Af.dtype and Al.shape == Af.shape      # untouched
            if e4[0]:
                sites.append((lf[0][1].shape[1], len(ll)))
        # per block: QKV, out-projection, MLP up (K = d) and MLP down (K = 4 d); two streams, the last block's text stream ends after attention
        want = []
        for b in range(nb):
            streams = 1 if b == nb - 1 else 2
            want += [(d, 2), (d, streams), (d, streams), (4 * d, streams)]
        assert sites == want, (sites, want)
    finally:
        net.set_precision("fast")


@pytest.mark.parametrize("cname", ["h3", "h19"])
def test_forward_distance_from_the_bf16_forward(ops, cname):
    """Seed 21, text_scale 30, t = [0.2, 0.9] (test_model_gpu.py::test_fp8_inference_mode).  "fp8": finite and 1e-4 < rel-L2 < 8e-2 (that test's
    bar); "mxfp8": not further from bf16 than 1.1 x the per-tensor mode and inside the mode's window 1e-4 .. 1.5e-1 (tests/test_configs_l_gpu.py);
    attention="e4m3": 1e-4 < rel-L2 < 8e-2 in both (tests/test_attn_e4m3_gpu.py).  Grad mode stays refused, "fast" afterwards is the first bf16
    output bit for bit."""
    net = _net(cname)
    try:
        net.set_precision("fast")
        v_fast = _forward(net, cname)
        r = {}
        for prec in ("fp8", "mxfp8"):
            for attention in ("bf16", "e4m3"):
                net.set_precision(prec, attention=attention)
                v = _forward(net, cname)
                assert bool(torch.isfinite(v).all()), (prec, attention)
                r[prec, attention] = _rel(v, v_fast)
                print(f"[fp8 pad] {cname} {prec} attention={attention}: forward rel-L2 vs the bf16 fast forward = {r[prec, attention]:.3e}")
            x, t, c, cp = _inputs(cname)
            with pytest.raises(RuntimeError):
                net(x, t, c.clone(), cp.clone())        # grad mode on: refused
        assert 1e-4 < r["fp8", "bf16"] < 8e-2
        assert 1e-4 < r["mxfp8", "bf16"] < 1.5e-1 and r["mxfp8", "bf16"] < 1.1 * r["fp8", "bf16"]
        assert 1e-4 < r["fp8", "e4m3"] < 8e-2 and 1e-4 < r["mxfp8", "e4m3"] < 8e-2
        net.set_precision("fast")
        assert torch.equal(_forward(net, cname), v_fast)
    finally:
        net.set_precision("fast")


@pytest.mark.parametrize("prec", ["fp8", "mxfp8"])
def test_nothing_changes_where_nothing_is_padded(ops, monkeypatch, prec):
    """dim = 256: every operand handed to the GEMM has the activation's own shape, and "mxfp8" still takes the fused producer route (the
    activations reach engine._to_fp8 as MxAct, no quantise pass)."""
    from sd3_amd import engine
    net = _net("xs")
    seen = []
    to_fp8 = engine._to_fp8

    def rec(m, p):
        q = to_fp8(m, p)
        seen.append((p["A"], p["B"], q["A"], q["B"]))
        return q

    try:
        net.set_precision(prec)
        with monkeypatch.context() as mp:
            mp.setattr(engine, "_to_fp8", rec)
            out = _forward(net, "xs")
        assert bool(torch.isfinite(out).all()) and len(seen) == 8 * 2 - 3      # four sites x two streams x two blocks, the last block's text stream short
        for A, B, qa, qb in seen:
            assert qa.dtype == qb.dtype == torch.float8_e4m3fn and tuple(qa.shape) == tuple(A.shape) and tuple(qb.shape) == tuple(B.shape)
            assert isinstance(A, ops.MxAct) == (prec == "mxfp8")
    finally:
        net.set_precision("fast")


def test_sampler_equals_a_plain_loop_over_forward(ops):
    """sample_imgs at dim = 192 in "fp8", two Euler steps with guidance and a stub text encoder, against the same two steps written as a loop over
    net.forward on the (2B) guidance batch: the same kernels on the same values, the delayed-scaling sites in the same phase sequence (now
    quantising into padded buffers), bit for bit."""
    from oracle.weights import make_inputs

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

    _, th, tp = make_inputs(40, 1, 16, 16, text_scale=30.0)
    B, steps, cfg_scale = 2, 2, 3.0
    net = _net("h3")
    try:
        net.set_precision("fp8")      # (fresh delayed-scaling sites)
        net.text_encoders = _Enc(th, tp)
        try:
            img = net.sample_imgs(B, steps, ["x"], cfg_scale=cfg_scale, width=128, height=128, sampler="euler", generator=torch.Generator().manual_seed(99))
        finally:
            del net.text_encoders
        net.set_precision("fp8")      # (fresh sites again: the loop walks the same phases)
        xl = torch.randn((B, 16, 16, 16), generator=torch.Generator().manual_seed(99)).cuda()
        cc = torch.cat([th.expand(B, -1, -1), torch.zeros(B, *th.shape[1:])]).contiguous().cuda()
        pp = torch.cat([tp.expand(B, -1), torch.zeros(B, tp.shape[-1])]).contiguous().cuda()
        with torch.no_grad():
            for t_now in torch.linspace(1, 1.0 / steps, steps).tolist():
                v = net(torch.cat([xl, xl]), torch.full((2 * B,), t_now), cc.clone(), pp.clone())
                xl = xl.sub(((1 + cfg_scale) * v[:B] - cfg_scale * v[B:]), alpha=1 / steps)
        ref = (xl / 8.0).clamp(-1, 1).float()
        print(f"[fp8 pad sampler] fp8 at dim 192: rel-L2 vs the plain loop = {_rel(img, ref):.3e}")
        assert img.shape == (B, 16, 16, 16) and bool(torch.isfinite(img).all())
        assert torch.equal(img.cpu(), ref.cpu()), _rel(img, ref)
    finally:
        net.train()
        net.set_precision("fast")


def test_padded_weight_caches_follow_replays(ops):
    """tests/test_graph_gpu.py::test_fp8_weight_caches_follow_replays at dim = 192: the captured AdamW rewrites the bf16 weight copies at every
    replay; the padded e4m3 copies (keyed on id(B) and the pack generation) must notice.  capture -> replay -> mxfp8 forward -> replay -> again,
    each equal to a fresh model's with the same parameters."""
    import test_graph_gpu as G
    from oracle.weights import make_inputs
    from sd3_amd.models.diff_model import diff_model
    cfg = CONFIGS["h3"][0]
    G.CONFIGS.setdefault("h3", cfg)
    _, _, _, _, tr = G.graph_vs_eager("h3", 4, 128, n_steps=1, pattern="each")
    net = tr.model
    x, c, cp = [a.cuda() for a in make_inputs(11, 2, 16, 16, text_scale=30.0)]
    t = torch.tensor([0.4, 0.6])
    outs = []
    for k in range(2):
        tr.train_step(20 + k)                       # replay
        net.eval()
        if k == 0:
            net.set_precision("mxfp8")      # (clears the quantised-weight caches)
        else:
            net.precision = "mxfp8"          # (does not: the caches must notice the replay by themselves)
        with torch.no_grad():
            v = net(x, t, c.clone(), cp.clone())
        fresh = diff_model(inCh=16, class_dim=768, patch_size=2, hidden_scale=4.0, attn_type="softmax_flash", MLP_type="swiglu",
                           device=torch.device("cuda:0"), positional_encoding="RoPE2d", **cfg)
        fresh.load_state_dict(net.state_dict())
        fresh.set_precision("mxfp8")
        fresh.eval()
        with torch.no_grad():
            vf = fresh(x, t, c.clone(), cp.clone())
        outs.append((v.clone(), vf.clone()))
        net.precision = "fast"
        net.train()
    for k, (v, vf) in enumerate(outs):
        assert torch.equal(v, vf), f"mxfp8 forward after replay {k} used stale padded weights (rel {_rel(v, vf):.3e})"
    assert not torch.equal(outs[0][0], outs[1][0])      # (the replay in between did change the weights)
    net.set_precision("fast")
