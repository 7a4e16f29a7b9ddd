"""Joint image+text attention: mirror of the reference's src/blocks/Attention.py for the trained
configuration (dual stream, attn_type softmax / softmax_flash, RoPE2d or RoPE2dV2, non-causal; ctor 16-114,
forward 118-135, 174-194, 220-239, 258-293, 410-425).  Experimental attention types of the reference
(cosine, cosine3, cosine4, cosine_norm, relu, silu, exp, both, 1-D RoPE) are out of scope and
raise.  positional_encoding="RoPE2dV2" (rotary_embedding_2d_v2.RoPE2D: channel triples rotated by a row and a column angle) runs on the unfused
route: plain QKV GEMM, mmdit_qk_norm_rope3_fwd / _bwd (include/mmdit_hip_rope3.h), attention; no kv_merge_attn, no fp8 / mxfp8.  kv_merge_attn (243-251) is implemented: the keys / values of adjacent token pairs of each stream are
averaged (mmdit_qk_norm_rope_fwd_merge) and S queries attend to S / 2 keys (mmdit_attn_fwd_kv).
Head width dim / num_heads: 64 (every fused and e4m3 form) or 128 (the plain kernels of include/mmdit_hip_hd128.h; no kv_merge_attn).
qk_half_dim (33-67): queries and keys are projected to dim / 2 -- with dim = 64 * num_heads a head has 32-wide queries / keys (RMSNorm(32),
RotaryEmbedding(16)) and 64-wide values at scale 64 ** -0.5 -- and the block runs on the unfused route: plain QKV GEMM with N = 2 * dim,
mmdit_qk_norm_rope_fwd_qkhalf / _bwd_qkhalf, mmdit_attn_fwd_qkhalf / _bwd_qkhalf (include/mmdit_hip_qkhalf.h); RoPE2d and head width 64 only, no
kv_merge_attn, no fp8 / mxfp8.
attn_type="cosine2" (69-86, 153-162, 330-339): queries and keys are L2-normalised over the head vector (F.normalize, eps 1e-12) -- no q_norm_* /
k_norm_* modules, no scale --, the image stream's are rotated as for softmax, and the weights are (q . k + 1) / sum: evaluated in linear time as
(q KV + vsum) / (q . ksum + S) through the per-(batch, head) state KV = sum_j k_j (x) v_j.  The block runs on the unfused route: plain QKV GEMM,
mmdit_qk_l2norm_rope_fwd / _bwd, mmdit_attn_cos2_fwd / _bwd (include/mmdit_hip_cos2.h); Q / K / V / O are bf16 in "fast" and fp32 in "parity"
precision.  RoPE2d and head width 64 only, no kv_merge_attn, no qk_half_dim, no fp8 / mxfp8."""
from types import SimpleNamespace as NS

import torch
from torch import nn

from .. import _lib, engine, ops
from ..packing import Pack
from .rotary_embedding import RotaryEmbedding
from .rotary_embedding_2d_v2 import RoPE2D

F32, BF16 = torch.float32, torch.bfloat16


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, orig_shape, x, c, *params):
        m = mod._mode()
        w = mod.weights(m)
        B, N, d = x.shape
        Mt, H, S, dev = c.shape[1], mod.num_heads, x.shape[1] + c.shape[1], x.device
        rope = mod.rotary_emb.tables(orig_shape[-2] // 2, orig_shape[-1] // 2, dev)
        xa, ca = m.act(x.reshape(B * N, d).contiguous()), m.act(c.reshape(B * Mt, d).contiguous())
        qkv_x = ops.gemm(xa, w.Wqkv_x, out_dtype=m.T, precision=m.prec)
        qkv_c = ops.gemm(ca, w.Wqkv_c, out_dtype=m.T, precision=m.prec)
        Q = torch.empty((B, H, S, mod.head_dim_qk), dtype=m.T if mod.cos2 else BF16, device=dev)
        if mod.cos2:      # (Q / K / V / O in the activation dtype: bf16 "fast", fp32 "parity"; lse is den)
            K, V = torch.empty_like(Q), torch.empty_like(Q)
            ops.qk_l2norm_rope_fwd_pair((qkv_x, rope[0], rope[1], N, 0), (qkv_c, None, None, Mt, N), B, H, S, Q, K, V)
            Ox, Oc, lse = ops.attn_cos2_fwd(Q, K, V, N)
        elif mod.qk_half_dim:
            K, V = torch.empty_like(Q), torch.empty((B, H, S, mod.head_dim), dtype=BF16, device=dev)
            ops.qk_norm_rope_fwd_qkhalf(qkv_x, w.wq_x, w.wk_x, rope[0], rope[1], B, N, H, S, 0, Q, K, V)
            ops.qk_norm_rope_fwd_qkhalf(qkv_c, w.wq_c, w.wk_c, None, None, B, Mt, H, S, N, Q, K, V)
            Ox, Oc, lse = ops.attn_fwd_qkhalf(Q, K, V, N, mod.scale, m.attn_mode)
        elif mod.rope3:
            K, V = torch.empty_like(Q), torch.empty_like(Q)
            ops.qk_norm_rope3_fwd(qkv_x, w.wq_x, w.wk_x, rope[0], rope[1], B, N, H, S, 0, Q, K, V)
            ops.qk_norm_rope3_fwd(qkv_c, w.wq_c, w.wk_c, None, None, B, Mt, H, S, N, Q, K, V)
            Ox, Oc, lse = ops.attn_fwd(Q, K, V, N, mod.scale, m.attn_mode)
        elif mod.kv_merge_attn:
            mod._check_even(N, Mt)
            K, V = torch.empty((B, H, S // 2, 64), dtype=BF16, device=dev), torch.empty((B, H, S // 2, 64), dtype=BF16, device=dev)
            ops.qk_norm_rope_fwd_merge_pair((qkv_x, w.wq_x, w.wk_x, rope[0], rope[1], N, 0), (qkv_c, w.wq_c, w.wk_c, None, None, Mt, N), B, H, S, Q, K, V)
            Ox, Oc, lse = ops.attn_fwd(Q, K, V, N, mod.scale, m.attn_mode, s_kv=S // 2)
        else:
            K, V = torch.empty_like(Q), torch.empty_like(Q)
            ops.qk_norm_rope_fwd(qkv_x, w.wq_x, w.wk_x, rope[0], rope[1], B, N, H, S, 0, Q, K, V)
            ops.qk_norm_rope_fwd(qkv_c, w.wq_c, w.wk_c, None, None, B, Mt, H, S, N, Q, K, V)
            Ox, Oc, lse = ops.attn_fwd(Q, K, V, N, mod.scale, m.attn_mode)
        Oxa = m.act(Ox.view(B * N, d))
        out_x = ops.gemm(Oxa, w.Wo_x, out_dtype=F32, precision=m.prec).view(B, N, d)
        if mod.last:
            Oca, out_c = None, (Oc.clone() if Oc.dtype == F32 else ops.cast(Oc, F32))   # raw head-merged attention output (Attention.py:425)
        else:
            Oca = m.act(Oc.view(B * Mt, d))
            out_c = ops.gemm(Oca, w.Wo_c, out_dtype=F32, precision=m.prec).view(B, Mt, d)
        ctx.mod, ctx.m, ctx.rope, ctx.dims = mod, m, rope, (B, N, Mt, H, d)
        ctx.save_for_backward(xa, ca, qkv_x, qkv_c, Q, K, V, Ox, Oc, lse, Oxa, Oca)
        return out_x, out_c

    @staticmethod
    def backward(ctx, dox, doc):
        xa, ca, qkv_x, qkv_c, Q, K, V, Ox, Oc, lse, Oxa, Oca = ctx.saved_tensors
        mod, m, rope = ctx.mod, ctx.m, ctx.rope
        B, N, Mt, H, d = ctx.dims
        S, dev = N + Mt, xa.device
        w = mod.weights(m)
        gout = {}
        dax = m.act(dox.reshape(B * N, d).contiguous())
        oT = m.T if mod.cos2 else BF16      # (dtype of the attention output and of its gradient)
        dOx = ops.gemm(dax, w.Wo_x, b_kmajor=True, out_dtype=oT, precision=m.prec)
        mod._po_x.split_grad(ops.gemm(dax, Oxa, a_kmajor=True, b_kmajor=True, out_dtype=F32, precision=m.prec), gout)
        if mod.last:
            dOc = None if doc is None else m.act(doc.reshape(B, Mt, d).float().contiguous()) if mod.cos2 else ops.cast(doc.reshape(B, Mt, d).float().contiguous(), BF16)
        else:
            dac = m.act(doc.reshape(B * Mt, d).contiguous())
            dOc = ops.gemm(dac, w.Wo_c, b_kmajor=True, out_dtype=oT, precision=m.prec)
            mod._po_c.split_grad(ops.gemm(dac, Oca, a_kmajor=True, b_kmajor=True, out_dtype=F32, precision=m.prec), gout)
        gq_x, gk_x, gq_c, gk_c = [None] * 4 if mod.cos2 else [torch.zeros(mod.head_dim_qk, dtype=F32, device=dev) for _ in range(4)]      # (cosine2: no norm weights)
        if mod.cos2:
            dQ, dK, dV = ops.attn_cos2_bwd(Q, K, V, Ox, Oc, dOx, dOc, lse, N, m.T)
            dqkv_x, dqkv_c = ops.qk_l2norm_rope_bwd_pair(dQ, dK, dV, (qkv_x, rope[0], rope[1], N, 0), (qkv_c, None, None, Mt, N), B, H, S, m.T)
        elif mod.qk_half_dim:
            dQ, dK, dV = ops.attn_bwd_qkhalf(Q, K, V, Ox, Oc, dOx, dOc, lse, N, mod.scale, m.T)
            dqkv_x = ops.qk_norm_rope_bwd_qkhalf(dQ, dK, dV, qkv_x, w.wq_x, w.wk_x, rope[0], rope[1], B, N, H, S, 0, gq_x, gk_x, m.T)
            dqkv_c = ops.qk_norm_rope_bwd_qkhalf(dQ, dK, dV, qkv_c, w.wq_c, w.wk_c, None, None, B, Mt, H, S, N, gq_c, gk_c, m.T)
        elif mod.rope3:
            dQ, dK, dV = ops.attn_bwd(Q, K, V, Ox, Oc, dOx, dOc, lse, N, mod.scale, m.T)
            dqkv_x = ops.qk_norm_rope3_bwd(dQ, dK, dV, qkv_x, w.wq_x, w.wk_x, rope[0], rope[1], B, N, H, S, 0, gq_x, gk_x, m.T)
            dqkv_c = ops.qk_norm_rope3_bwd(dQ, dK, dV, qkv_c, w.wq_c, w.wk_c, None, None, B, Mt, H, S, N, gq_c, gk_c, m.T)
        elif mod.kv_merge_attn:
            dQ, dK, dV = ops.attn_bwd(Q, K, V, Ox, Oc, dOx, dOc, lse, N, mod.scale, m.T, s_kv=S // 2)
            dqkv_x, dqkv_c = ops.qk_norm_rope_bwd_merge_pair(dQ, dK, dV, (qkv_x, w.wq_x, w.wk_x, rope[0], rope[1], N, 0, gq_x, gk_x),
                                                             (qkv_c, w.wq_c, w.wk_c, None, None, Mt, N, gq_c, gk_c), B, H, S, m.T)
        else:
            dQ, dK, dV = ops.attn_bwd(Q, K, V, Ox, Oc, dOx, dOc, lse, N, mod.scale, m.T)
            dqkv_x = ops.qk_norm_rope_bwd(dQ, dK, dV, qkv_x, w.wq_x, w.wk_x, rope[0], rope[1], B, N, H, S, 0, gq_x, gk_x, m.T)
            dqkv_c = ops.qk_norm_rope_bwd(dQ, dK, dV, qkv_c, w.wq_c, w.wk_c, None, None, B, Mt, H, S, N, gq_c, gk_c, m.T)
        dx = ops.gemm(dqkv_x, w.Wqkv_x, b_kmajor=True, out_dtype=F32, precision=m.prec).view(B, N, d)
        dc = ops.gemm(dqkv_c, w.Wqkv_c, b_kmajor=True, out_dtype=F32, precision=m.prec).view(B, Mt, d)
        mod._pqkv_x.split_grad(ops.gemm(dqkv_x, xa, a_kmajor=True, b_kmajor=True, out_dtype=F32, precision=m.prec), gout)
        mod._pqkv_c.split_grad(ops.gemm(dqkv_c, ca, a_kmajor=True, b_kmajor=True, out_dtype=F32, precision=m.prec), gout)
        if not mod.cos2:
            gout[id(mod.q_norm_x.weight)], gout[id(mod.k_norm_x.weight)] = gq_x, gk_x
            gout[id(mod.q_norm_c.weight)], gout[id(mod.k_norm_c.weight)] = gq_c, gk_c
        return (None, None, dx, dc) + tuple(gout.get(id(p)) for p in mod._param_list())


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, attn_type="cosine", causal=False, emb_dim=None, positional_encoding="absolute", RoPE_Scale=1,
                 kv_merge_attn=False, qk_half_dim=False, layer_idx=None, dual=False, last=False):
        super().__init__()
        if attn_type not in ("softmax", "softmax_flash", "cosine2"):
            raise RuntimeError(f"attn_type must be 'softmax', 'softmax_flash' or 'cosine2' on the HIP path, but got {attn_type}")
        if not dual or causal or emb_dim is not None:
            raise RuntimeError("Attention: only the dual-stream, non-causal configuration of the trained model is implemented")
        if positional_encoding not in ("RoPE2d", "RoPE2dV2"):
            raise RuntimeError("Attention: only positional_encoding='RoPE2d' and 'RoPE2dV2' are implemented")
        if dim % num_heads or dim // num_heads not in _lib.HEAD_DIMS:
            raise RuntimeError(f"Attention: head_dim = dim / num_heads must be 64 (the reference's dim = 64*num_heads convention, train.py:37-39) or 128, "
                               f"the widths the attention kernels are built for, but got dim={dim}, num_heads={num_heads}")
        if kv_merge_attn and dim // num_heads != 64:
            raise RuntimeError("Attention: kv_merge_attn is built for head_dim 64 only (the pair-averaging kernels mmdit_qk_norm_rope_*_merge / mmdit_attn_*_kv are 64 wide)")
        if kv_merge_attn and positional_encoding == "RoPE2dV2":
            raise RuntimeError("Attention: kv_merge_attn is not built for positional_encoding='RoPE2dV2' (the pair-averaging kernels "
                               "mmdit_qk_norm_rope_*_merge rotate channel pairs; mmdit_qk_norm_rope3_* has no merging form)")
        if qk_half_dim and kv_merge_attn:
            raise RuntimeError("Attention: qk_half_dim is not built with kv_merge_attn (the pair-averaging kernels mmdit_qk_norm_rope_*_merge / mmdit_attn_*_kv "
                               "take 64-wide queries and keys; mmdit_qk_norm_rope_*_qkhalf has no merging form)")
        if qk_half_dim and positional_encoding == "RoPE2dV2":
            raise RuntimeError("Attention: qk_half_dim is not built for positional_encoding='RoPE2dV2' (mmdit_qk_norm_rope3_* rotates channel triples of 64- "
                               "or 128-wide heads; mmdit_qk_norm_rope_*_qkhalf rotates pairs)")
        if qk_half_dim and dim // num_heads != 64:
            raise RuntimeError(f"Attention: qk_half_dim is built for dim = 64 * num_heads only (32-wide queries / keys, 64-wide values: "
                               f"include/mmdit_hip_qkhalf.h), but got dim={dim}, num_heads={num_heads}")
        self.cos2 = attn_type == "cosine2"
        if self.cos2 and kv_merge_attn:
            raise RuntimeError("Attention: attn_type='cosine2' is not built with kv_merge_attn (mmdit_attn_cos2_* sums over every key: there is no "
                               "pair-averaging form of mmdit_qk_l2norm_rope_*)")
        if self.cos2 and qk_half_dim:
            raise RuntimeError("Attention: attn_type='cosine2' is not built with qk_half_dim (mmdit_attn_cos2_* keeps a 64 x 64 state: queries, keys and "
                               "values are 64 wide)")
        if self.cos2 and positional_encoding == "RoPE2dV2":
            raise RuntimeError("Attention: attn_type='cosine2' is not built for positional_encoding='RoPE2dV2' (mmdit_qk_l2norm_rope_* rotates channel "
                               "pairs; mmdit_qk_norm_rope3_* applies the RMSNorm that cosine2 does not have)")
        if self.cos2 and dim // num_heads != 64:
            raise RuntimeError(f"Attention: attn_type='cosine2' is built for dim = 64 * num_heads only (the 64 x 64 state of include/mmdit_hip_cos2.h), "
                               f"but got dim={dim}, num_heads={num_heads}")
        self.rope3 = positional_encoding == "RoPE2dV2"
        self.qk_half_dim = bool(qk_half_dim)
        dim_qk = dim // 2 if qk_half_dim else dim      # (Attention.py:33)
        self.positional_encoding, self.kv_merge_attn, self.RoPE_Scale = positional_encoding, kv_merge_attn, RoPE_Scale
        self.layer_idx, self.dual, self.last = layer_idx, dual, last
        self.query_proj_x = nn.Linear(dim, dim_qk, bias=False)
        self.key_proj_x = nn.Linear(dim, dim_qk, bias=False)
        self.value_proj_x = nn.Linear(dim, dim, bias=False)
        self.out_proj_x = nn.Linear(dim, dim, bias=False)
        self.query_proj_c = nn.Linear(dim, dim_qk, bias=False)
        self.key_proj_c = nn.Linear(dim, dim_qk, bias=False)
        self.value_proj_c = nn.Linear(dim, dim, bias=False)
        if not self.last:
            self.out_proj_c = nn.Linear(dim, dim, bias=False)
        self.dim, self.num_heads = dim, num_heads
        self.head_dim_qk, self.head_dim = dim_qk // num_heads, dim // num_heads
        if not self.cos2:      # (cosine2: F.normalize instead of the RMSNorms, no scale -- Attention.py:69-86)
            self.scale = self.head_dim ** -0.5
            self.q_norm_x = nn.RMSNorm(self.head_dim_qk)
            self.k_norm_x = nn.RMSNorm(self.head_dim_qk)
            self.q_norm_c = nn.RMSNorm(self.head_dim_qk)
            self.k_norm_c = nn.RMSNorm(self.head_dim_qk)
        self.attn_type = attn_type   # both softmax names run the same HIP flash kernel
        self.causal = causal
        if self.rope3:
            self.rotary_emb = RoPE2D(self.head_dim_qk, interpolate_factor=1 / RoPE_Scale)
        else:
            self.rotary_emb = RotaryEmbedding(self.head_dim_qk // 2, use_xpos=False, interpolate_factor=1 / RoPE_Scale)
        self._pqkv_x = Pack([self.query_proj_x.weight, self.key_proj_x.weight, self.value_proj_x.weight])
        self._pqkv_c = Pack([self.query_proj_c.weight, self.key_proj_c.weight, self.value_proj_c.weight])
        self._po_x = Pack([self.out_proj_x.weight])
        self._po_c = None if self.last else Pack([self.out_proj_c.weight])
        self.precision = "fast"

    def _mode(self):
        return engine.FAST if self.precision == "fast" else engine.PARITY

    @staticmethod
    def _check_even(n_img, n_txt):
        # (the reference asserts the same, Attention.py:246-247)
        assert n_img % 2 == 0, "Merge attention requires an even number of keys"
        assert n_txt % 2 == 0, "Merge attention requires an even number of keys"

    def _param_list(self):
        return [p for p in self.parameters() if p.requires_grad]

    def weights(self, m):
        if self.cos2:      # (no norm weights)
            return NS(Wqkv_x=self._pqkv_x.get(m), Wqkv_c=self._pqkv_c.get(m), Wo_x=self._po_x.get(m), Wo_c=None if self.last else self._po_c.get(m),
                      kv_merge=False, hd=self.head_dim, rope3=False, qk_half=False, cos2=True)
        return NS(Wqkv_x=self._pqkv_x.get(m), Wqkv_c=self._pqkv_c.get(m), Wo_x=self._po_x.get(m),
                  Wo_c=None if self.last else self._po_c.get(m),
                  wq_x=self.q_norm_x.weight.detach(), wk_x=self.k_norm_x.weight.detach(),
                  wq_c=self.q_norm_c.weight.detach(), wk_c=self.k_norm_c.weight.detach(), kv_merge=bool(self.kv_merge_attn), hd=self.head_dim, rope3=self.rope3,
                  qk_half=self.qk_half_dim)

    def scatter_grads(self, g, out: dict):
        self._pqkv_x.split_grad(g.Wqkv_x, out)
        self._pqkv_c.split_grad(g.Wqkv_c, out)
        self._po_x.split_grad(g.Wo_x, out)
        if not self.last:
            self._po_c.split_grad(g.Wo_c, out)
        if self.cos2:
            return
        out[id(self.q_norm_x.weight)], out[id(self.k_norm_x.weight)] = g.wq_x, g.wk_x
        out[id(self.q_norm_c.weight)], out[id(self.k_norm_c.weight)] = g.wq_c, g.wk_c

    def forward(self, x, c=None, orig_shape=None):
        assert c is not None, "Dual attention requires context tensor c"
        return _AttentionFn.apply(self, tuple(orig_shape), x, c, *self._param_list())
