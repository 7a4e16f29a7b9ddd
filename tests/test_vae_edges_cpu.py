"""What tests/test_vae_edges_gpu.py relies on, checked without a GPU: that every path of the restated launch arithmetic is present in the case list,
and the comparator on these kernels -- a float32 torch model of each kernel passes the bars (one case per kernel), and each damage the sweep exists to
catch fails them on the element, row or column it touches: GroupNorm eps 1e-5, a straddling channel normalised with the thread's first group, the last
row of a statistics chunk left out, SiLU skipped on the second pixel in flight, a softmax sum without its last column, a non-zero padding column,
im2col mode 2 without the -1, a changed border byte of a padded output."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # (the sweep's tables, references and comparator live in the GPU module next to this file)
import test_gemm_edges_gpu as G  # noqa: E402
import test_vae_edges_gpu as V  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32


def test_launch_arithmetic_restatement():
    assert V.grid_cap(0) == 1 and V.grid_cap(256) == 1 and V.grid_cap(257) == 2 and V.grid_cap(65535 * 256) == 65535 and V.grid_cap(1 << 30) == 65535
    assert not V.past_cap(65535 * 256) and V.past_cap(65535 * 256 + 1)
    assert 1024 * 1024 * (128 // 8) == 65536 * 256                                   # a 1024^2 decode with C = 128 sits on the cap
    assert V.gn_rpb(128, 3) == 128 and V.gn_rpb(262144, 1) == 128 and V.gn_rpb(262145, 1) == 256 and V.gn_rpb(1 << 20, 16) == 8192
    assert V.gn_rpb(1, 4096) == 128                                                  # (rpb < HW stops the doubling)
    assert [V.gn_nty(C) for C in (8, 24, 96, 128, 512, 2048)] == [256, 85, 21, 16, 4, 1]
    assert V.gn_depth(2048, 32, 257, 3) == 128 + 64 + 3 + 2 and V.gn_depth(128, 32, 129, 1) == 8 + 64 + 2 + 2


def test_every_named_path_is_in_the_case_list():
    ids = [c.id for c in V.CASES]
    assert len(ids) == len(set(ids))
    have = set().union(*(c.paths() for c in V.CASES))
    want = {f"{k}:past_cap" for k in ("nchw_to_nhwc", "nhwc_to_nchw", "im2col", "pad_cast")}
    want |= {"nchw_to_nhwc:f32", "nchw_to_nhwc:bf16", "nchw_to_nhwc:padTrue", "nchw_to_nhwc:padFalse", "nchw_to_nhwc:affine0", "nchw_to_nhwc:affine1",
             "nchw_to_nhwc:partial_groupTrue", "nhwc_to_nchw:ld>CTrue", "nhwc_to_nchw:ld>CFalse", "nhwc_to_nchw:clamp0", "nhwc_to_nchw:clamp1",
             "im2col:mode0", "im2col:mode1", "im2col:mode2", "im2col:H1", "im2col:W1", "pad_cast:f32", "pad_cast:bf16", "pad_cast:up0", "pad_cast:up1"}
    want |= {"groupnorm:" + s for s in ("f32", "bf16", "silu0", "silu1", "pad0", "pad1", "random", "offset", "smallvar", "poison", "rpb_doubles", "idle_threads",
                                        "thread_spans_groups", "cpg<8", "straddle", "cpg1", "one_group", "G64", "nty1", "fewer_rows_than_nty",
                                        "rows_in_flight_beyond_end", "second_stats_chunk", "second_apply_chunk", "apply_chunk_edge127", "apply_chunk_edge0",
                                        "apply_chunk_edge1", "second_pixel_in_flight_absent")}
    want |= {f"softmax:rows%4={i}" for i in range(4)} | {"softmax:cols<64", "softmax:cols=64", "softmax:cols>64", "softmax:ld-cols>=8True", "softmax:ld-cols>=8False",
                                                          "softmax:no_padding", "softmax:one_lane_second_trip", "softmax:random", "softmax:saturating",
                                                          "softmax:scale1True", "softmax:scale1False"}
    assert want <= have, sorted(want - have)
    # the past-the-cap cases stay just past it (about 270 MB each), the rpb doubling is the issue's shape, every GroupNorm option meets both straddling shapes
    for c in V.CASES:
        if c.exact_only:
            assert V.past_cap(c.work()) and c.work() < 65535 * 256 + (1 << 15), c.id
    assert any(c.kind == "groupnorm" and (c.B, c.HW, c.C) == (1, 262145, 8) for c in V.CASES)
    for C, Gn in ((128, 32), (96, 8)):
        assert {(c.dt, c.silu, c.pad) for c in V.CASES if c.kind == "groupnorm" and (c.C, c.Gn) == (C, Gn)} == {(d, s, p) for d in ("f32", "bf16") for s in (0, 1) for p in (0, 1)}
    gn = {(c.C, c.Gn) for c in V.CASES if c.kind == "groupnorm"}
    assert gn >= {(128, 32), (512, 32), (32, 32), (64, 32), (96, 8), (24, 1), (512, 64), (2048, 32)}
    assert {c.HW for c in V.CASES if c.kind == "groupnorm"} >= {1, 3, 127, 128, 129, 257} and {c.B for c in V.CASES if c.kind == "groupnorm"} >= {1, 3}


# ---------------------------------------------------------------------------------------------- float32 models of the kernels (vae.hip, line by line)
def im2col_model(x, mode, no_minus_one=False):
    B, H, W, C = x.shape
    Ho, Wo = V.im2col_out(mode, H, W)
    yo, xo = torch.arange(Ho)[:, None].expand(Ho, Wo), torch.arange(Wo)[None, :].expand(Ho, Wo)
    taps = []
    for kh in range(3):
        for kw in range(3):
            if mode == 1:
                yi, xi = 2 * yo + kh, 2 * xo + kw
                ok = (yi < H) & (xi < W)
            elif mode == 2:
                yu, xu = yo + kh - (0 if no_minus_one else 1), xo + kw - 1
                ok = (yu >= 0) & (xu >= 0) & (yu < Ho) & (xu < Wo)
                yi, xi = yu >> 1, xu >> 1
            else:
                yi, xi = yo + kh - 1, xo + kw - 1
                ok = (yi >= 0) & (xi >= 0) & (yi < H) & (xi < W)
            v = x[:, yi.clamp(0, H - 1), xi.clamp(0, W - 1)]
            taps.append(torch.where(ok[None, :, :, None], v, torch.zeros_like(v)))
    return torch.stack(taps, 3).reshape(B * Ho * Wo, 9 * C)


def gn_model(c, t, eps=None, damage=None):
    B, HW, C, Gn = c.B, c.HW, c.C, c.Gn
    cpg, nty = C // Gn, V.gn_nty(C)
    x = t["x"].float().view(B, HW, C)
    ch = torch.arange(C)
    true_g = ch // cpg
    counted = torch.ones(B, HW, 1)
    if damage == "lost_row":
        counted[1, 127] = 0.0                                                        # the last row of image 1's first statistics chunk
    s1 = torch.zeros(B, Gn).index_add_(1, true_g, (x * counted).sum(1))
    s2 = torch.zeros(B, Gn).index_add_(1, true_g, (x * x * counted).sum(1))
    inv_n = torch.tensor(1.0 / (float(HW) * float(cpg)), dtype=F32)
    m = s1 * inv_n
    var = (s2 * inv_n - m * m).clamp_min(0.0)
    g = (ch // 8 * 8) // cpg if damage == "first_group" else true_g
    sc = torch.rsqrt(var + torch.tensor(t["eps"] if eps is None else eps, dtype=F32))[:, g] * t["gamma"].float()
    of = t["beta"].float() - m[:, g] * sc
    o = torch.addcmul(of[:, None, :], x, sc[:, None, :])
    y = o * torch.sigmoid(o) if c.silu else o
    if damage == "silu_skip":
        second = ((torch.arange(HW) % V.PPB) // nty) % 2 == 1                        # q = p + nty of every pair in flight
        y[:, second] = o[:, second]
    return y.reshape(B * HW, C).to(BF)


def softmax_model(c, t, damage=None):
    x = t["x"][:, :c.cols].float() * torch.tensor(t["scale"], dtype=F32)
    e = torch.exp(x - x.amax(1, keepdim=True))
    s = e.sum(1, keepdim=True)
    if damage == "lost_col":
        s[2] = e[2, :-1].sum()
    out = torch.zeros(c.rows, c.ld, dtype=BF)
    out[:, :c.cols] = (e * (1.0 / s)).to(BF)
    if damage == "pad_nonzero":
        out[1, c.cols] = 2.0 ** -130
    return out


def model(c, t):
    k, x = c.kind, t["x"]
    if k == "nchw_to_nhwc":
        out = torch.zeros(c.B, c.HW, c.Cp, dtype=BF)
        out[:, :, :c.C] = ((x.float() + torch.tensor(t["shift"], dtype=F32)) * torch.tensor(t["scale"], dtype=F32)).transpose(1, 2).to(BF)
        return out.view(-1, c.Cp)
    if k == "nhwc_to_nchw":
        return torch.minimum(torch.maximum(x[:, :c.C], torch.tensor(t["lo"])), torch.tensor(t["hi"])).view(c.B, c.HW, c.C).transpose(1, 2).reshape(c.B * c.C, c.HW)
    if k == "im2col":
        return im2col_model(x, c.mode)
    if k == "pad_cast":
        Ho, Wo = c.H << c.up, c.W << c.up
        return x.to(BF).view(c.B, c.H, c.W, c.C)[:, torch.arange(Ho) >> c.up][:, :, torch.arange(Wo) >> c.up].reshape(-1, c.C)
    if k == "groupnorm":
        return gn_model(c, t)
    return softmax_model(c, t)


_MODEL_CASES = [V.Case("nchw_to_nhwc", dt="f32", C=9, Cp=16, HW=77, B=3, aff=1), V.Case("nchw_to_nhwc", dt="bf16", C=3, Cp=64, HW=15, B=3, aff=0),
                V.Case("nhwc_to_nchw", C=3, ld=8, HW=77, B=3, clamp=1), V.Case("im2col", mode=0, H=5, W=6, C=24, B=3), V.Case("im2col", mode=1, H=6, W=2, C=8, B=3),
                V.Case("im2col", mode=2, H=3, W=2, C=8, B=3), V.Case("pad_cast", dt="f32", up=1, H=3, W=6, C=24, B=3),
                V.Case("groupnorm", C=96, Gn=8, HW=129, B=3, dt="f32", silu=1, pad=0), V.Case("groupnorm", "offset", C=128, Gn=32, HW=257, B=3, dt="bf16", silu=0, pad=0),
                V.Case("groupnorm", "smallvar", C=128, Gn=32, HW=129, B=3, dt="f32", silu=1, pad=0), V.Case("groupnorm", C=2048, Gn=32, HW=3, B=1, dt="bf16", silu=1, pad=0),
                V.Case("softmax", rows=5, cols=63, ld=64, scale=1.0), V.Case("softmax", rows=37, cols=129, ld=137, scale=512 ** -0.5),
                V.Case("softmax", "saturating", rows=3, cols=100, ld=104, scale=512 ** -0.5)]


@pytest.mark.parametrize("c", _MODEL_CASES, ids=lambda c: c.id)
def test_float32_model_of_the_kernel_passes_the_bars(c):
    t = V.build(c, "cpu")
    ref, det, rnd = V.reference(c, t)
    out = model(c, t)
    r = G.ratios(out, ref, det, rnd)
    print(f"[vae comparator] {c.id}: fp32 model elem {r['el']:.3f} row {r['row']:.3f} col {r['col']:.3f} bias {r['bias']}")
    assert G.verdict(r) == [] and V.check(c, t, out, ref, det, rnd) == [], (r, V.check(c, t, out, ref, det, rnd))


def _rows(out, ref, det, rnd):
    return (out.double() - ref).norm(dim=1) / (det + rnd).norm(dim=1).clamp_min(G.TINY)


def _cols(out, ref, det, rnd):
    return (out.double() - ref).norm(dim=0) / (det + rnd).norm(dim=0).clamp_min(G.TINY)


def _distinct_groups(c, t, g):
    """The twin's own inputs for the GroupNorm damages: every group at its own level and spread, |gamma| >= 0.5 (iid groups have nearly equal
    statistics, and a tiny gamma hides a wrong mean)."""
    cpg = c.C // c.Gn
    x = t["x"].float().view(c.B, c.HW, c.Gn, cpg)
    x = x * (1 + 0.25 * torch.arange(c.Gn).view(1, 1, c.Gn, 1)) + 3.0 * torch.arange(c.Gn).view(1, 1, c.Gn, 1)
    t["x"] = x.reshape(c.B * c.HW, c.C).to(V.DT[c.dt])
    s = torch.randn(c.C, generator=g)
    t["gamma"] = torch.sign(s) * (0.5 + s.abs())
    return t


def test_groupnorm_damages_fail_where_they_touch():
    g = torch.Generator().manual_seed(9)
    # eps = 1e-5 instead of 1e-6 on the small-variance family: every element outside the constant group moves by half its size
    c = V.Case("groupnorm", "smallvar", C=128, Gn=32, HW=129, B=3, dt="f32", silu=0, pad=0)
    t = V.build(c, "cpu")
    ref = V.reference(c, t)
    assert G.verdict(G.ratios(gn_model(c, t), *ref)) == []
    r = G.ratios(gn_model(c, t, eps=1e-5), *ref)
    rows = _rows(gn_model(c, t, eps=1e-5), *ref)
    print(f"[vae comparator] groupnorm eps 1e-5 on smallvar: elem {r['el']:.1f} row {r['row']:.1f} (every row >= {float(rows.min()):.1f})")
    assert {"el", "row", "col"} <= set(G.verdict(r)) and float(rows.min()) > G.ROW_BAR
    # the group of a straddling channel taken as the thread's first group: cpg = 12, so channels 12 .. 15, 36 .. 39, 60 .. 63, 84 .. 87 get the group before
    c = V.Case("groupnorm", C=96, Gn=8, HW=129, B=2, dt="f32", silu=0, pad=0)
    t = _distinct_groups(c, V.build(c, "cpu"), g)
    ref = V.reference(c, t)
    assert G.verdict(G.ratios(gn_model(c, t), *ref)) == []
    cols = _cols(gn_model(c, t, damage="first_group"), *ref)
    hit = torch.zeros(96, dtype=torch.bool)
    hit[[ch for ch in range(96) if (ch // 8 * 8) // 12 != ch // 12]] = True
    assert hit.nonzero().view(-1).tolist() == [12, 13, 14, 15, 36, 37, 38, 39, 60, 61, 62, 63, 84, 85, 86, 87]
    print(f"[vae comparator] groupnorm first-group damage: damaged columns >= {float(cols[hit].min()):.1f}, others <= {float(cols[~hit].max()):.3f}")
    assert float(cols[hit].min()) > G.ROW_BAR and float(cols[~hit].max()) <= G.ROW_BAR
    # the last row of a statistics chunk (row 127 of image 1) left out of the sums: every row of image 1 fails, images 0 and 2 pass
    c = V.Case("groupnorm", C=128, Gn=32, HW=129, B=3, dt="bf16", silu=1, pad=0)
    t = V.build(c, "cpu")
    t["x"].view(3, 129, 128)[1, 127] = 10.0
    t = _distinct_groups(c, t, g)
    ref = V.reference(c, t)
    assert G.verdict(G.ratios(gn_model(c, t), *ref)) == []
    rows = _rows(gn_model(c, t, damage="lost_row"), *ref).view(3, 129)
    print(f"[vae comparator] groupnorm lost statistics row: image 1 rows >= {float(rows[1].min()):.1f}, images 0 / 2 <= {float(rows[[0, 2]].max()):.3f}")
    assert float(rows[1].min()) > G.ROW_BAR and float(rows[[0, 2]].max()) <= G.ROW_BAR
    # SiLU skipped on the second pixel in flight (nty = 16: pixels 16 .. 31, 48 .. 63, ... of every 128-pixel chunk)
    out = gn_model(c, t, damage="silu_skip")
    rows = _rows(out, *ref).view(3, 129)
    second = ((torch.arange(129) % 128) // 16) % 2 == 1
    print(f"[vae comparator] groupnorm SiLU skipped: second pixels >= {float(rows[:, second].min()):.1f}, first pixels <= {float(rows[:, ~second].max()):.3f}")
    assert int(second.sum()) == 64 and float(rows[:, second].min()) > G.ROW_BAR and float(rows[:, ~second].max()) <= G.ROW_BAR


def test_softmax_damages_fail_where_they_touch():
    c = V.Case("softmax", rows=5, cols=63, ld=64, scale=1.0)
    t = V.build(c, "cpu")
    t["x"][2, 62] = float(t["x"][2, :63].max())          # the last column carries weight in row 2
    ref = V.reference(c, t)
    assert G.verdict(G.ratios(softmax_model(c, t), *ref)) == [] and V.check(c, t, softmax_model(c, t), *ref) == []
    rows = _rows(softmax_model(c, t, "lost_col"), *ref)
    print(f"[vae comparator] softmax without its last column in row 2: rows {[round(float(v), 2) for v in rows]}")
    assert float(rows[2]) > G.ROW_BAR and float(rows[[0, 1, 3, 4]].max()) <= G.ROW_BAR
    out = softmax_model(c, t, "pad_nonzero")
    r = G.ratios(out, *ref)
    assert "el" in G.verdict(r) and r["at"][:2] == (1, 63) and V.check(c, t, out, *ref) == ["a padding column is not zero"]


def test_im2col_without_the_minus_one_is_not_bit_identical_and_a_changed_border_byte_is_reported():
    c = V.Case("im2col", mode=2, H=3, W=2, C=8, B=3)
    t = V.build(c, "cpu")
    ref, det, rnd = V.reference(c, t)
    assert int((V.bits(im2col_model(t["x"], 2)) != V.bits(ref.to(BF))).sum()) == 0
    out = im2col_model(t["x"], 2, no_minus_one=True)
    r = G.ratios(out, ref, det, rnd)
    wrong = (V.bits(out) != V.bits(ref.to(BF))).view(3, 6, 4, 9, 8)
    assert {"el", "row", "col"} <= set(G.verdict(r)) and bool(wrong.any(-1).any(-1).all())          # every output row has a wrong tap
    for shape, dtype, pad in (((3, 5, 8, 24), BF, True), ((7, 16), BF, False), ((6, 77), F32, False)):
        o = V.Win(shape, dtype, "cpu", pad)
        o.win.zero_()                                                    # writes inside the window are not reported
        assert o.touched() == 0
        spots = [o.big[:o.g][-1:], o.big[o.g + o.n:][:1]] + ([o.t[1, 0, 3, 5:6], o.t[2, 4, 7, :1], o.t[0, 2, 0, 23:], o.t[0, 3, 7, :1]] if pad else [])
        for s in spots:
            keep = s.clone()
            s.view(torch.uint8)[0] ^= 1
            assert o.touched() == 1
            s.copy_(keep)
        assert o.touched() == 0
