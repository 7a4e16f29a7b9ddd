"""Head width 128: tile-edge sweep of the attention kernels (csrc/attention_hd128.hip) and of the QK-RMSNorm / RoPE kernels
(the HD = 128 instantiations of csrc/rowops.hip) with per-row and per-element float64 parity through ops.* and the C ABI (include/mmdit_hip_hd128.h).

Attention.  Reference and yardstick are those of test_attention_edges_gpu.py, restated for a 128-wide head (SCALE = 128 ** -0.5):
plain float64 torch attention of the bf16-rounded operands; with u = 2^-8, componentwise,

  yO = u (|O| + P |V|)                      yV = u (|dV| + P^T |dO|)
  dbar = rowsum(|dO| * (P |V|)),  A = P * (|dP| + |delta| + dbar)
  yQ = u (|dQ| + scale A |K|)               yK = u (|dK| + scale A^T |Q|)

and for every row and every element  ||out_row - ref_row|| <= 1.0 ||y_row||,  |out - ref| <= 2.0 y,  |lse - ref| <= 1e-4 max(1, |ref|).
The bars follow from the rounding points (P, dS, O and the outputs in bf16, delta from the rounded O), which are those of the 64-wide
kernels; tests/test_hd128_abi.py runs a float64 model of exactly those rounding points over the cases below and holds IT to the same bars.
Mode 1 is compared with the oracle's restatement of the reference's CPU branch under the 3e-3 whole-tensor bar of the 64-wide sweep.

Shapes are built from the kernels' tile edges: the 32-query wave, the MMDIT_ATTN_HD128_KEY_TILE = 32 key tile and the
MMDIT_ATTN_HD128_QUERY_TILE = 128 workgroup; S on, one before and one past each edge; 1, 2, 3 key tiles (the double buffer wraps at the
third), 4, 5 and 9; n_img = S (no text, Oc = None), 1, on an edge and inside a wave; batch * heads a multiple of 8 (the XCD-interleaved
branch of map_block with 1, 2 and 3 query tiles) and not.  "random" and "lastkey" run on every shape, the five edge families where S is one
past an edge.

QK-norm / RoPE.  The yardstick construction of test_rowops_edges_gpu.py (math_qk / yard_qk) for a 128-wide row: the sum over a head vector
is 8 serial adds per lane, 4 butterfly steps and the scaling, depth 13.  Bars: per element 2.0, per row and per column 1.0.

Worst measured ratios: profiles/hd128_parity.txt.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 128
U = 2.0 ** -8          # bf16 unit roundoff (round to nearest)
u = 2.0 ** -24         # fp32
SCALE = 128 ** -0.5
ROW_BAR, ELEM_BAR = 1.0, 2.0
KT, QT = 32, 128       # MMDIT_ATTN_HD128_KEY_TILE, MMDIT_ATTN_HD128_QUERY_TILE (test_hd128_abi.py checks them against the header)


@pytest.fixture(scope="module")
def ops():
    import sd3_amd  # noqa: F401
    from sd3_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ---------------------------------------------------------------------------------------------- shapes
# (S, n_img, batch, heads); batch * heads no multiple of 8: the plain branch of map_block
_PLAIN = [
    (1, 1, 1, 1),          # one key, one query
    (31, 31, 2, 3),        # one short of a wave / key tile, no text (Oc = None)
    (32, 32, 1, 1),        # exactly one wave and one key tile
    (33, 32, 2, 3),        # 2 key tiles, the second holds ONE valid key; split on the wave edge; the second wave has one valid query
    (33, 1, 1, 1),         # split at row 1
    (63, 40, 2, 3),        # one short of two tiles; split inside a wave
    (64, 64, 1, 1),        # 2 full key tiles, no text
    (65, 64, 2, 3),        # 3 key tiles: the double buffer wraps (tile 2 lands in buffer 0); one-key tail
    (65, 33, 1, 1),
    (95, 64, 2, 3),        # 3 tiles, 31-key ragged tile
    (96, 96, 1, 1),        # 3 full tiles
    (97, 96, 2, 3),        # 4 tiles, one-key tail; the fourth wave has one valid query
    (127, 100, 1, 1),      # one short of a workgroup
    (128, 128, 2, 3),      # exactly one workgroup, 4 tiles, no ragged tile
    (128, 1, 1, 1),
    (129, 128, 2, 3),      # 5 tiles; a second workgroup with a single valid query (waves 1..3 inactive); split on the workgroup edge
    (129, 1, 1, 1),
    (160, 128, 2, 3),      # second workgroup = exactly one wave
    (257, 256, 1, 1),      # 9 tiles, a third workgroup with a single valid query
]
# batch * heads = 8 or 16: the XCD-interleaved branch, ntile = 1, 2 and 3
_SWIZZLED = [(1, 1, 2, 4), (33, 32, 1, 16), (96, 40, 2, 4), (128, 128, 1, 16), (129, 128, 2, 4), (129, 1, 1, 16), (257, 200, 2, 4)]
# the families beyond "random" and "lastkey" run where S is one past an edge
_EDGE = [(33, 32, 2, 3), (33, 1, 1, 1), (65, 64, 2, 3), (97, 96, 2, 3), (129, 128, 2, 4), (129, 1, 1, 16), (257, 256, 1, 1)]
_EDGE_FAMILIES = ["ragged0", "late", "early", "large", "flat"]
FAMILIES = ["random", "lastkey"] + _EDGE_FAMILIES

# "lastkey" needs a second key to share the softmax with: S = 1 runs "random" only
CASES = [(shape, "random") for shape in _PLAIN + _SWIZZLED] + [(shape, "lastkey") for shape in _PLAIN + _SWIZZLED if shape[0] > 1] + \
        [(shape, fam) for fam in _EDGE_FAMILIES for shape in _EDGE]


def _case_id(case):
    (S, n_img, Bt, H), fam = case
    return f"S{S}-img{n_img}-b{Bt}h{H}-{fam}"


# ---------------------------------------------------------------------------------------------- input families
def _orth(x, d):
    """x without its component along the sign vector d (|d|^2 = 128)."""
    return x - (x @ d)[..., None] * d / float(HD)


def _bf(x):
    return x.to(torch.bfloat16)


def _growth(S):
    """Key gain that rises inside a tile and jumps at every tile edge: a tile with a single valid key still raises the running maximum."""
    j = torch.arange(S, dtype=torch.float64)
    return 1.0 + 0.5 * torch.floor(j / KT) + 0.25 * (j % KT) / KT


def _tile_max(s):
    """Row maximum per key tile: (..., S, nkv)."""
    S = s.shape[-1]
    return torch.stack([s[..., t * KT:min((t + 1) * KT, S)].amax(-1) for t in range((S + KT - 1) // KT)], -1)


def make_inputs(shape, family):
    """Seeded bf16 (Q, K, V, dO), each (batch, heads, S, 128), on the CPU: the families of test_attention_edges_gpu.py at width 128.  Every
    family asserts its own precondition in float64 on the ROUNDED operands."""
    S, n_img, Bt, H = shape
    g = torch.Generator().manual_seed(100003 * S + 1009 * n_img + 17 * Bt * H + FAMILIES.index(family))
    n = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)      # noqa: E731
    full = (Bt, H, S, HD)
    d = torch.randint(0, 2, (HD,), generator=g).double() * 2 - 1
    Q, K = n(*full), n(*full)
    score = lambda Qb, Kb: SCALE * Qb.double() @ Kb.double().mT      # noqa: E731
    if family == "random":
        Q, K = _bf(Q), _bf(K)
    elif family in ("lastkey", "ragged0"):
        # key kd = b d, every query has the same component 0.5 d: the score of kd is the same for all queries; b puts it at the median (over
        # queries) logsumexp of the other keys, i.e. a median softmax weight of 1/2 -- P, dS round everywhere and a second copy of key kd
        # (a clamped padding row that gets counted) moves its weight from p to 2p / (1 + p)
        nkv = (S + KT - 1) // KT
        kd = S - 1 if family == "lastkey" else KT * (nkv - 1)
        assert family == "lastkey" or S % KT, "ragged0 needs a ragged tile"
        Q = _bf(_orth(Q, d) + 0.5 * d)
        K = _bf(K)
        others = score(Q, K)
        others[..., kd] = -math.inf
        b = float(torch.logsumexp(others, -1).median() / (SCALE * (Q.double() @ d).median()))
        K[..., kd, :] = _bf(b * d)
        w = torch.softmax(score(Q, K), -1)[..., kd]
        shared = ((w > 0.2) & (w < 0.8)).double().mean()
        assert shared >= 0.5, f"{family}: key {kd} holds 0.2..0.8 of the softmax for only {float(shared):.2f} of the queries"
    elif family in ("late", "early"):
        # scores c gain(key) + small noise: the gain carries the ordering, the noise keeps P from being a function of the key alone
        gain = _growth(S) if family == "late" else _growth(S).flip(0)
        Q = _bf(0.5 * d + 0.5 * _orth(Q, d))
        K = _bf(0.5 * gain[:, None] * d + 0.1 * _orth(K, d))
        tm = _tile_max(score(Q, K))
        if family == "late":      # every tile raises the running maximum: the rescale runs with alpha < 1 in every iteration
            rising = (tm[..., 1:] > tm[..., :-1]).all(-1).double().mean()
            assert rising >= 0.9, f"late: the per-tile row maximum rises through all tiles for only {float(rising):.2f} of the rows"
        else:                     # the maximum of every query lies in tile 0
            assert bool((tm[..., 1:] <= tm[..., :1]).all()), "early: a later tile exceeds tile 0"
    elif family == "large":
        # common component kappa d on both sides: scale q.k = 85 + noise; the common 85 cancels in the softmax, the rest does not
        kappa = math.sqrt(85.0 / (SCALE * HD))
        Q, K = _bf(kappa * d + 0.5 * Q), _bf(kappa * d + 0.5 * K)
        s = score(Q, K)
        assert 60.0 <= float(s.abs().max()) <= 100.0, f"large: max |scale q.k| = {float(s.abs().max()):.1f}"
        assert bool(torch.exp(s.float()).isinf().any()), "large: exp(score) does not overflow fp32 without the shift"
    elif family == "flat":
        Q, K = _bf(Q), _bf(K[:, :, :1].expand(full).contiguous())
        s = score(Q, K)
        assert float((torch.softmax(s, -1) - 1.0 / S).abs().max()) < 1e-14
        assert float((torch.logsumexp(s, -1) - (s[..., 0] + math.log(S))).abs().max()) < 1e-12
    else:
        raise KeyError(family)
    return Q, K, _bf(n(*full)), _bf(n(*full))


# ---------------------------------------------------------------------------------------------- float64 reference + yardstick
def _ref_fwd(Q, K, V):
    s = SCALE * Q @ K.mT
    P = torch.softmax(s, -1)
    O = P @ V
    return dict(P=P, O=O, lse=torch.logsumexp(s, -1), PV=P @ V.abs(), yO=U * (O.abs() + P @ V.abs()))


def _ref_bwd(Q, K, V, dO, fwd):
    P, O = fwd["P"], fwd["O"]
    dP = dO @ V.mT
    delta = (dO * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ, dK, dV = SCALE * dS @ K, SCALE * dS.mT @ Q, P.mT @ dO
    dbar = (dO.abs() * fwd["PV"]).sum(-1, keepdim=True)
    A = P * (dP.abs() + delta.abs() + dbar)
    return dict(dQ=dQ, dK=dK, dV=dV, yQ=U * (dQ.abs() + SCALE * A @ K.abs()), yK=U * (dK.abs() + SCALE * A.mT @ Q.abs()), yV=U * (dV.abs() + P.mT @ dO.abs()))


def _ratios(out, ref, y):
    """(worst per-row ratio, worst per-element ratio, flat index of the worst row).  y = 0 (a text query under dOc = None) demands out == ref."""
    diff = (out.double() - ref).abs()
    row = diff.norm(dim=-1) / y.norm(dim=-1).clamp_min(1e-300)
    el = diff / y.clamp_min(1e-300)
    return float(row.max()), float(el.max()), int(row.argmax())


def _split(x, n_img):
    """(batch, heads, S, 128) -> head-merged per-stream (batch, n_img, heads * 128), (batch, S - n_img, heads * 128) or None."""
    Bt, H, S, _ = x.shape
    m = x.permute(0, 2, 1, 3).reshape(Bt, S, H * HD)
    return m[:, :n_img].contiguous(), (m[:, n_img:].contiguous() if S > n_img else None)


def _merge(Ox, Oc, H):
    m = torch.cat([Ox, Oc], 1) if Oc is not None else Ox
    return m.reshape(m.shape[0], m.shape[1], H, HD).permute(0, 2, 1, 3)


WORST = {}             # kernel family -> output -> (per-row, case id), (per-element, case id)


def _record(kernel, name, row, el, cid):
    w = WORST.setdefault(kernel, {}).setdefault(name, [(-1.0, ""), (-1.0, "")])
    if row > w[0][0]:
        w[0] = (row, cid)
    if el > w[1][0]:
        w[1] = (el, cid)


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\n[hd128 sweep] worst ratio to the yardstick per kernel family (bars: per row / column 1.0, per element 2.0)")
    for kernel, outs in WORST.items():
        for name, (r, e) in outs.items():
            print(f"  {kernel:<24} {name:<10} per-row {r[0]:.3f} @ {r[1]:<34} per-element {e[0]:.3f} @ {e[1]}")


class _Case:
    """One (shape, family): operands, the float64 reference and the kernel's own forward outputs, built once and shared by every entry point."""

    def __init__(self, ops, shape, family):
        self.shape, self.family, self.id = shape, family, _case_id((shape, family))
        self.S, self.n_img, self.Bt, self.H = shape
        self.Q, self.K, self.V, self.dO = (t.cuda() for t in make_inputs(shape, family))
        self.d64 = [t.double() for t in (self.Q, self.K, self.V)]
        self.fwd = _ref_fwd(*self.d64)
        self.Ox, self.Oc, self.lse = ops.attn_fwd(self.Q, self.K, self.V, self.n_img, SCALE, 0)
        self._bwd = {}

    def dO_streams(self, last):
        dOx, dOc = _split(self.dO, self.n_img)
        return dOx, (None if last else dOc)

    def bwd(self, last):
        if last not in self._bwd:
            dO = self.dO.double().clone()
            if last:
                dO[:, :, self.n_img:] = 0.0           # no gradient reaches the text rows of the last block's output
            self._bwd[last] = _ref_bwd(*self.d64, dO, self.fwd)
        return self._bwd[last]


@pytest.fixture(scope="module", params=CASES, ids=_case_id)
def case(request, ops):
    return _Case(ops, *request.param)


# ---------------------------------------------------------------------------------------------- attention forward
def test_fwd_flash(case):
    """attn_fwd mode 0 at width 128: O per row and per element within the yardstick, finite, lse to fp32 accuracy."""
    out = _merge(case.Ox, case.Oc, case.H)
    assert (case.Oc is None) == (case.S == case.n_img)
    assert case.Ox.shape == (case.Bt, case.n_img, case.H * HD) and case.lse.shape == (case.Bt, case.H, case.S)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(case.lse).all())
    row, el, at = _ratios(out, case.fwd["O"], case.fwd["yO"])
    lse_ref = case.fwd["lse"]
    lse_err = float(((case.lse.double() - lse_ref).abs() / lse_ref.abs().clamp_min(1.0)).max())
    print(f"[hd128 attn fwd flash] {case.id}: O per-row {row:.3f} (row {at}) per-element {el:.3f}; lse {lse_err:.2e}")
    _record("attn_fwd_hd128 mode 0", "O", row, el, case.id)
    assert row <= ROW_BAR, (case.id, "row", at, row)
    assert el <= ELEM_BAR, (case.id, el)
    assert lse_err <= 1e-4, (case.id, lse_err)


@pytest.mark.parametrize("shape", _PLAIN + _SWIZZLED, ids=lambda s: "S%d-img%d-b%dh%d" % s)
def test_fwd_oracle_mode(ops, shape):
    """attn_fwd mode 1 rounds where the reference's CPU branch rounds (scores, P and O in bf16): whole-tensor comparison against the oracle's
    restatement of that branch under the 3e-3 bar of test_attention_edges_gpu.py, at every shape of the sweep."""
    from oracle.mmdit_oracle import attention_core
    S, n_img, Bt, H = shape
    Q, K, V, _ = make_inputs(shape, "random")
    Ox, Oc, lse = ops.attn_fwd(Q.cuda(), K.cuda(), V.cuda(), n_img, SCALE, 1)
    ref = attention_core(Q.float(), K.float(), V.float(), SCALE, "oracle_bf16").double()
    out = _merge(Ox, Oc, H).double().cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    r = float((out - ref).norm() / ref.norm())
    rows = ((out - ref).norm(dim=-1) / ref.norm(dim=-1)).max()
    print(f"[hd128 attn fwd oracle mode] S={S} img={n_img} b{Bt}h{H}: rel-L2 {r:.2e}, worst row {float(rows):.2e}")
    w = WORST.setdefault("attn_fwd_hd128 mode 1", {}).setdefault("O rel-L2", [(-1.0, ""), (-1.0, "")])
    if r > w[0][0]:
        w[0] = w[1] = (r, "S%d-img%d-b%dh%d-random" % shape)
    assert r < 3e-3, (shape, r)


# ---------------------------------------------------------------------------------------------- attention backward
@pytest.mark.parametrize("last", [False, True], ids=["dOc", "last"])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_bwd(case, ops, out_dtype, last):
    """attn_bwd at width 128 fed the kernel's own forward outputs, as the trainer feeds it: bf16 and fp32 outputs, with a text output
    gradient and without (the last block)."""
    dOx, dOc = case.dO_streams(last)
    dQ, dK, dV = ops.attn_bwd(case.Q, case.K, case.V, case.Ox, case.Oc, dOx, dOc, case.lse, case.n_img, SCALE, out_dtype)
    ref = case.bwd(last)
    kernel = "attn_bwd_hd128 -> " + ("bf16" if out_dtype == torch.bfloat16 else "fp32")
    res = {}
    for name, out, y in (("dQ", dQ, "yQ"), ("dK", dK, "yK"), ("dV", dV, "yV")):
        assert out.dtype == out_dtype and out.shape == case.Q.shape and bool(torch.isfinite(out).all()), (case.id, name)
        res[name] = _ratios(out, ref[name], ref[y])
        _record(kernel, name, res[name][0], res[name][1], case.id + ("-last" if last else ""))
    print(f"[{kernel}] {case.id}{' last' if last else ''}: " + ", ".join(f"{k} per-row {v[0]:.3f} (row {v[2]}) per-element {v[1]:.3f}" for k, v in res.items()))
    for name, (row, el, at) in res.items():
        assert row <= ROW_BAR, (case.id, name, "row", at, row)
        assert el <= ELEM_BAR, (case.id, name, el)


# ---------------------------------------------------------------------------------------------- status codes and the python dispatch
def test_status_codes_nothing_launched(ops):
    """Bad arguments come back as MMDIT_ERR_ARG / MMDIT_ERR_SHAPE / MMDIT_ERR_DTYPE and nothing is launched: the outputs keep their contents."""
    from sd3_amd import _lib
    L = _lib.lib()
    S, Bt, H = 40, 1, 2
    Q, K, V, dO = (t.cuda() for t in make_inputs((S, 33, Bt, H), "random"))
    Ox, Oc = torch.full((Bt, 33, H * HD), 7.0, dtype=torch.bfloat16, device="cuda"), torch.full((Bt, 7, H * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((Bt, H, S), 7.0, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    fwd = lambda **kw: L.mmdit_attn_fwd_hd128(*[kw.get(k, v) for k, v in (("Q", p(Q)), ("K", p(K)), ("V", p(V)), ("batch", Bt), ("heads", H), ("S", S), ("n_img", 33),      # noqa: E731
                                                                         ("scale", SCALE), ("mode", 0), ("Ox", p(Ox)), ("Oc", p(Oc)), ("lse", p(lse)), ("stream", None))])
    assert fwd(Q=None) == _lib.ERR_ARG and fwd(lse=None) == _lib.ERR_ARG and fwd(batch=0) == _lib.ERR_ARG and fwd(heads=-1) == _lib.ERR_ARG
    assert fwd(mode=2) == _lib.ERR_ARG and fwd(Oc=None) == _lib.ERR_ARG          # (a text stream without its output)
    assert fwd(S=0) == _lib.ERR_SHAPE and fwd(n_img=0) == _lib.ERR_SHAPE and fwd(n_img=S + 1) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((Ox == 7).all()) and bool((Oc == 7).all()) and bool((lse == 7).all())
    assert fwd() == 0
    dOx, dOc = _split(dO, 33)
    delta = torch.full((Bt, H, S), 7.0, device="cuda")
    dQ, dK, dV = (torch.full(Q.shape, 7.0, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    bwd = lambda **kw: L.mmdit_attn_bwd_hd128(*[kw.get(k, v) for k, v in (("Q", p(Q)), ("K", p(K)), ("V", p(V)), ("Ox", p(Ox)), ("Oc", p(Oc)), ("dOx", p(dOx)), ("dOc", p(dOc)),      # noqa: E731
                                                                         ("lse", p(lse)), ("delta", p(delta)), ("batch", Bt), ("heads", H), ("S", S), ("n_img", 33), ("scale", SCALE),
                                                                         ("dQ", p(dQ)), ("dK", p(dK)), ("dV", p(dV)), ("dt", _lib.BF16), ("stream", None))])
    assert bwd(dt=2) == _lib.ERR_DTYPE and bwd(dt=-1) == _lib.ERR_DTYPE
    assert bwd(dQ=None) == _lib.ERR_ARG and bwd(delta=None) == _lib.ERR_ARG and bwd(Oc=None) == _lib.ERR_ARG
    assert bwd(S=0) == _lib.ERR_SHAPE and bwd(n_img=S + 1) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (dQ, dK, dV, delta))
    assert bwd() == 0 and bwd(dOc=None) == 0      # (dOc may be NULL: the last block)
    # QK-norm / RoPE
    qkv = torch.randn(4, 3 * H * HD, device="cuda").to(torch.bfloat16)
    w = torch.ones(HD, device="cuda")
    Qo = torch.full((1, H, 4, HD), 7.0, dtype=torch.bfloat16, device="cuda")
    Ko, Vo = Qo.clone(), Qo.clone()
    pr = (_lib.QkProblem * 1)()
    pr[0].qkv, pr[0].wq, pr[0].wk, pr[0].tokens, pr[0].tok0 = p(qkv), p(w), p(w), 4, 0
    qf = lambda **kw: L.mmdit_qk_norm_rope_fwd_hd128(*[kw.get(k, v) for k, v in (("probs", pr), ("count", 1), ("dt", _lib.BF16), ("batch", 1), ("heads", H), ("s", 4),      # noqa: E731
                                                                                ("Q", p(Qo)), ("K", p(Ko)), ("V", p(Vo)), ("stream", None))])
    assert qf(count=3) == _lib.ERR_ARG and qf(Q=None) == _lib.ERR_ARG and qf(s=3) == _lib.ERR_ARG      # (token range outside the joint length)
    assert qf(dt=2) == _lib.ERR_DTYPE and qf(heads=_lib.QK_HD128_MAX_HEADS + 1) == _lib.ERR_SHAPE
    pr[0].rope_cos = p(w)                                                                                # cos without sin
    assert qf() == _lib.ERR_ARG
    pr[0].rope_cos = None
    qb = lambda **kw: L.mmdit_qk_norm_rope_bwd_hd128(*[kw.get(k, v) for k, v in (("probs", pr), ("count", 1), ("dQ", p(Qo)), ("dK", p(Ko)), ("dV", p(Vo)), ("dq", _lib.BF16),      # noqa: E731
                                                                                ("ti", _lib.BF16), ("to", _lib.BF16), ("batch", 1), ("heads", H), ("s", 4), ("stream", None))])
    assert qb() == _lib.ERR_ARG                                                                          # dqkv / dwq / dwk missing
    dqkv, dw = torch.full(qkv.shape, 7.0, dtype=torch.bfloat16, device="cuda"), torch.full((2, HD), 7.0, device="cuda")
    pr[0].dqkv, pr[0].dwq, pr[0].dwk = p(dqkv), p(dw[0]), p(dw[1])
    assert qb(dq=_lib.F32) == _lib.ERR_DTYPE and qb(dV=None) == _lib.ERR_ARG and qb(heads=_lib.QK_HD128_MAX_HEADS + 1) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (Qo, Ko, Vo, dqkv, dw))
    assert qf() == 0 and qb() == 0
    torch.cuda.synchronize()


def test_python_dispatch_refusals(ops):
    """ops.* at width 128: s_kv raises, the fused backward stays off, a width that is neither 64 nor 128 raises."""
    Q = torch.zeros((1, 2, 64, HD), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.attn_fwd(Q, Q[:, :, :32].contiguous(), Q[:, :, :32].contiguous(), 32, SCALE, 0, s_kv=32)
    assert not ops.attn_bwd_qk_ok(Q, 32, torch.zeros((32, 3 * 2 * HD), dtype=torch.bfloat16, device="cuda"))
    Q96 = torch.zeros((1, 2, 64, 96), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.attn_fwd(Q96, Q96, Q96, 32, 96 ** -0.5, 0)
    with pytest.raises(RuntimeError):      # 64-wide norm weights with a 128-wide Q
        ops.qk_norm_rope_fwd(torch.zeros((64, 3 * 2 * HD), dtype=torch.bfloat16, device="cuda"), torch.ones(64, device="cuda"), torch.ones(64, device="cuda"), None, None,
                             1, 64, 2, 64, 0, Q, Q.clone(), Q.clone())


# ---------------------------------------------------------------------------------------------- QK-RMSNorm + RoPE at width 128
RMS_EPS = float(torch.finfo(torch.float32).eps)
QK_DEPTH = 13          # 8 serial adds per lane, 4 butterfly steps over the 16 lanes of a head vector, the scaling by 1 / 128
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
QK_COMBOS = ((BF, BF, BF), (F32, F32, F32), (BF, F32, F32))      # (dQ / dK / dV, saved qkv, dqkv)
RL_MIN_ROWS, MAX_HEADS = 2048, 21      # MMDIT_QK_HD128_RL_MIN_ROWS, MMDIT_QK_HD128_MAX_HEADS

# (batch, heads, ((tokens, rope), ...) in launch order, dtype combo, (tokens in front of, behind the streams))
QK_CASES = [
    (1, 1, ((1, True),), 0, (5, 2)),                       # one row; tok0 = 5
    (2, 3, ((24, True), (10, False)), 0, (0, 0)),          # the block's pair: image with RoPE, text without; grid = tokens (same token per workgroup)
    (2, 3, ((10, False), (24, True)), 2, (0, 4)),          # text first
    (2, 2, ((24, True),), 1, (3, 0)),                      # fp32 everywhere, tok0 = 3
    (3, MAX_HEADS, ((6, True), (5, False)), 0, (0, 0)),    # the most heads a row's workgroup holds (1008 threads)
    (1, 1, ((1100, True),), 0, (7, 0)),                    # more tokens than workgroups: the factors are loaded per row (general path), rows off the grid
    (16, 2, ((135, True), (135, False)), 2, (0, 0)),       # 2160 rows per problem: 10 rows per workgroup; 540 lanes = 4 tokens sets, rows = 4 x lanes (on)
    (17, 2, ((128, True),), 0, (0, 0)),                    # 2176 rows, 10 per workgroup, 640 lanes: 3.4 passes (off)
    (9, 3, ((256, True),), 0, (0, 0)),                     # 2304 rows, 7 per workgroup, no multiple of 256 lanes fits: general path at rl > 1
    (700, 1, ((3, False),), 1, (2, 3)),                    # 2100 rows, 21 per workgroup (1008 threads), no RoPE
    # the two shapes at which the launch policy of width 64 runs one lane per token and this width's does not (qk_grid in csrc/rowops.hip):
    (3, 2, ((1000, True),), 0, (0, 0)),                    # 3000 rows, 10 per workgroup; 768 lanes < 1000 tokens <= 2048, a multiple of 10: 76 workgroups, factors per row
    (1, 2, ((600, True),), 2, (0, 0)),                     # 600 rows, one per workgroup; 512 lanes < 600 tokens <= 1024: 512 workgroups, factors per row
]


def _qk_id(c):
    return f"b{c[0]}h{c[1]}-" + "+".join(f"{t}{'r' if r else ''}" for t, r in c[2]) + f"-c{c[3]}-pad{c[4][0]}.{c[4][1]}"


def data_qk(c):
    Bt, H, streams, combo, pad = c
    tg, ti, to = QK_COMBOS[combo]
    S = pad[0] + sum(t for t, _ in streams) + pad[1]
    g = torch.Generator().manual_seed(977 * Bt + 31 * H + S + combo)
    rn = lambda *sh: torch.randn(*sh, generator=g)      # noqa: E731
    dQ, dK, dV = (rn(Bt, H, S, HD).to(tg) for _ in range(3))
    ts, tok0 = [], pad[0]
    for T, rope in streams:
        ts.append(dict(B=Bt, H=H, T=T, S=S, tok0=tok0, qkv=(0.5 + 2 * rn(Bt * T, 3 * H * HD)).to(ti), wq=1.0 + 0.3 * rn(HD), wk=1.0 + 0.3 * rn(HD), dQ=dQ, dK=dK, dV=dV,
                       cos=2 * torch.rand(T, HD, generator=g) - 1 if rope else None, sin=2 * torch.rand(T, HD, generator=g) - 1 if rope else None,
                       dwq0=rn(HD), dwk0=rn(HD)))
        tok0 += T
    return ts


def _qk_split(z):
    return z[..., 0::2], z[..., 1::2]


def _qk_join(e, o):
    return torch.stack([e, o], -1).flatten(-2)


def _qk_tables(t, dt):
    if t["cos"] is None:
        return None
    c0, c1 = _qk_split(t["cos"].to(dt)[None, :, None, :])
    s0, s1 = _qk_split(t["sin"].to(dt)[None, :, None, :])
    return c0, c1, s0, s1


def math_qk(t, dt):
    """Closed forms of the forward and the backward of one stream in dtype dt (math_qk of test_rowops_edges_gpu.py at width 128)."""
    B, H, T, tok0 = t["B"], t["H"], t["T"], t["tok0"]
    x = t["qkv"].to(dt).view(B, T, 3, H, HD)
    tab = _qk_tables(t, dt)
    heads = lambda z: z.permute(0, 2, 1, 3).reshape(-1, HD)      # noqa: E731  (B, T, H, 128) -> rows of (B, H, T)
    o, aux, parts = {}, {}, []
    for part, name in ((0, "q"), (1, "k")):
        xp, w = x[:, :, part], t["w" + name].to(dt)
        q = (xp * xp).mean(-1, keepdim=True)
        r = (q + RMS_EPS).rsqrt()
        xn = xp * r
        n = xn * w
        if tab is not None:
            c0, c1, s0, s1 = tab
            a, b = _qk_split(n)
            fwd = _qk_join(a * c0 - b * s0, b * c1 + a * s1)
        else:
            fwd = n
        o[name.upper()] = heads(fwd)
        dz = t["d" + name.upper()].to(dt)[:, :, tok0:tok0 + T].permute(0, 2, 1, 3)
        if tab is not None:
            da, db = _qk_split(dz)
            dzr = _qk_join(da * c0 + db * s1, db * c1 - da * s0)
        else:
            dzr = dz
        dzw = dzr * w
        dot = (dzw * xn).mean(-1, keepdim=True)
        parts.append(r * (dzw - xn * dot))
        o["dw" + name] = (t[f"dw{name}0"].to(dt) + (dzr * xn).sum((0, 1, 2)))[None]
        aux[name] = dict(xp=xp, q=q, r=r, xn=xn, n=n, dz=dz, dzr=dzr, dzw=dzw, dot=dot)
    o["V"] = heads(x[:, :, 2])
    parts.append(t["dV"].to(dt)[:, :, tok0:tok0 + T].permute(0, 2, 1, 3))
    o["dqkv"] = torch.stack(parts, 2).reshape(B * T, 3 * H * HD)
    return o, aux


def yard_qk(combo, t, ref, aux):
    """yard_qk of test_rowops_edges_gpu.py with the sum depth of a 128-wide row: name -> (deterministic part, output rounding part)."""
    tg, ti, to = QK_COMBOS[combo]
    B, H, T = t["B"], t["H"], t["T"]
    tab = _qk_tables(t, F64)
    heads = lambda z: z.permute(0, 2, 1, 3).reshape(-1, HD)      # noqa: E731
    z = torch.zeros_like
    mk = lambda v: v.mean(-1, keepdim=True)      # noqa: E731
    y, parts = {}, []
    for name in ("q", "k"):
        a = aux[name]
        w = t["w" + name].double().abs()
        xp, q, r, xn, n = a["xp"].abs(), a["q"], a["r"], a["xn"].abs(), a["n"].abs()
        dr = r * (0.5 * (QK_DEPTH + 1) * u * q / (q + RMS_EPS) + 2 * u)
        e_xn = xp * dr + u * xn
        e_n = w * e_xn + u * n
        dz, dzr, dzw, dot = a["dz"].abs(), a["dzr"].abs(), a["dzw"].abs(), a["dot"].abs()
        if tab is not None:
            c0, c1, s0, s1 = (v.abs() for v in tab)
            na, nb = _qk_split(n)
            ea, eb = _qk_split(e_n)
            e_f = _qk_join(c0 * ea + s0 * eb + 2 * u * (na * c0 + nb * s0), c1 * eb + s1 * ea + 2 * u * (nb * c1 + na * s1))
            da, db = _qk_split(dz)
            e_dz = _qk_join(2 * u * (da * c0 + db * s1), 2 * u * (db * c1 + da * s0))
        else:
            e_f, e_dz = e_n, z(dz)
        y[name.upper()] = (heads(e_f), U * ref[name.upper()].abs())
        e_dzw = w * e_dz + u * dzw
        ddot = QK_DEPTH * u * mk(dzw * xn) + mk(e_dzw * xn + dzw * e_xn)
        core = (a["dzw"] - a["xn"] * a["dot"]).abs()
        parts.append(r * (e_dzw + e_xn * dot + xn * ddot + 2 * u * (dzw + xn * dot)) + dr * core + u * r * core)
        terms = dzr * xn
        y["dw" + name] = (((e_dz * xn + dzr * e_xn + u * terms).sum((0, 1, 2)) + (B * T * H + 2) * u * (terms.sum((0, 1, 2)) + t[f"dw{name}0"].double().abs()))[None],
                          z(ref["dw" + name]))
    v = ref["V"].abs()
    y["V"] = (z(v), U * v if ti == F32 else z(v))
    parts.append(z(parts[0]))
    det = torch.stack(parts, 2).reshape(B * T, 3 * H * HD)
    y["dqkv"] = (det, U * ref["dqkv"].abs() if to == BF else z(det))
    if to == BF:      # (the dV third of a bf16 dqkv is an exact copy)
        y["dqkv"][1].view(B, T, 3, H, HD)[:, :, 2] = 0
    return y


def qk_ratios(out, ref, det, rnd):
    """Worst ratio to y = det + rnd per element, per row and per column (ratios of test_gemm_edges_gpu.py).  y = 0 demands out == ref."""
    diff = out.double().cpu() - ref
    y = det + rnd
    tiny = 1e-300
    return (float((diff.abs() / y.clamp_min(tiny)).max()), float((diff.norm(dim=1) / y.norm(dim=1).clamp_min(tiny)).max()),
            float((diff.norm(dim=0) / y.norm(dim=0).clamp_min(tiny)).max()))


@pytest.mark.parametrize("c", QK_CASES, ids=_qk_id)
def test_qk_norm_rope_hd128(ops, c):
    """qk_norm_rope_fwd / _bwd (plain and pair forms) at width 128 against float64: Q, K, V of every stream, dqkv, and dwq / dwk ADDED to their
    initial contents; the token rows of Q / K / V outside the streams keep their contents."""
    Bt, H, streams, combo, pad = c
    tg, ti, to = QK_COMBOS[combo]
    ts = data_qk(c)
    S = ts[0]["S"]
    Q, K, V = (torch.full((Bt, H, S, HD), 3.0, dtype=BF, device="cuda") for _ in range(3))
    cu = lambda v: None if v is None else v.cuda()      # noqa: E731
    dev = [dict(qkv=t["qkv"].cuda(), wq=t["wq"].cuda(), wk=t["wk"].cuda(), cos=cu(t["cos"]), sin=cu(t["sin"]), dwq=t["dwq0"].cuda(), dwk=t["dwk0"].cuda()) for t in ts]
    fw = [(d["qkv"], d["wq"], d["wk"], d["cos"], d["sin"], t["T"], t["tok0"]) for d, t in zip(dev, ts)]
    dQ, dK, dV = (ts[0][k].cuda() for k in ("dQ", "dK", "dV"))
    if len(ts) == 2:
        ops.qk_norm_rope_fwd_pair(fw[0], fw[1], Bt, H, S, Q, K, V)
        dqkv = ops.qk_norm_rope_bwd_pair(dQ, dK, dV, fw[0] + (dev[0]["dwq"], dev[0]["dwk"]), fw[1] + (dev[1]["dwq"], dev[1]["dwk"]), Bt, H, S, to)
    else:
        d, t = dev[0], ts[0]
        ops.qk_norm_rope_fwd(d["qkv"], d["wq"], d["wk"], d["cos"], d["sin"], Bt, t["T"], H, S, t["tok0"], Q, K, V)
        dqkv = [ops.qk_norm_rope_bwd(dQ, dK, dV, d["qkv"], d["wq"], d["wk"], d["cos"], d["sin"], Bt, t["T"], H, S, t["tok0"], d["dwq"], d["dwk"], to)]
    torch.cuda.synchronize()
    cid = _qk_id(c)
    for i, (t, d) in enumerate(zip(ts, dev)):
        ref, aux = math_qk(t, F64)
        y = yard_qk(combo, t, ref, aux)
        win = lambda X: X[:, :, t["tok0"]:t["tok0"] + t["T"]].reshape(-1, HD)      # noqa: E731
        outs = dict(Q=win(Q), K=win(K), V=win(V), dqkv=dqkv[i], dwq=d["dwq"][None], dwk=d["dwk"][None])
        assert dqkv[i].dtype == to and dqkv[i].shape == t["qkv"].shape
        for name, out in outs.items():
            assert bool(torch.isfinite(out).all()), (cid, i, name)
            el, row, col = qk_ratios(out, ref[name], *y[name])
            print(f"[hd128 qk] {cid} stream {i} {name}: per-element {el:.3f} per-row {row:.3f} per-column {col:.3f}")
            _record("qk_norm_rope_hd128 " + ("fwd" if name in "QKV" else "bwd"), name, max(row, col), el, cid)
            assert el <= ELEM_BAR and row <= ROW_BAR and col <= ROW_BAR, (cid, i, name, el, row, col)
    used = torch.zeros(S, dtype=torch.bool)
    for t in ts:
        used[t["tok0"]:t["tok0"] + t["T"]] = True
    for X in (Q, K, V):
        assert bool((X[:, :, ~used.cuda()] == 3.0).all()), (cid, "a token row outside the streams was written")
