// What the per-head QK RMSNorm + RoPE + head-split row kernels share: the pair kernels at head width 64 and 128 and the kv_merge kernels
// (rowops.hip), the rotary-triple kernels (rowops_rope3.hip): one kernel-side problem struct and its selection in a list launch, one lane-group
// sum, one problem-list validator.
#pragma once
#include "common.h"
#include <float.h>

constexpr float RMS_EPS = FLT_EPSILON;    // nn.RMSNorm(eps=None) on fp32 input: finfo(float32).eps

// sum over the G = 8 or 16 lanes of a head vector (HD / 8 lanes of 8 elements: a G-aligned lane group of one wave)
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
  if constexpr (G == 16) v += __shfl_xor(v, 8, 64);
  return v;
}

namespace {      // (as in the sources that include this: the kernel symbols, which spell their parameter types, stay internal to their object)
// a list of one or two problems (workgroups [0, g0) = problem 0): the image and the text rows of a block write the same Q / K / V, different token ranges
struct QkProb {
  const void* qkv; const float* wq; const float* wk; const float* rcos; const float* rsin; int rows, tokens, tok0;
  const void* dQ; const void* dK; const void* dV; void* dqkv; float* dwq; float* dwk;      // (backward only)
};
}  // namespace

// dtype combinations of the backward kernels (dQ / dK / dV, saved qkv, dqkv): 0 all bf16, 1 all fp32, 2 bf16 gradients of an fp32 projection
static inline int qk_bwd_combo(int dq_dtype, int qkv_dtype, int dqkv_dtype) {
  return (dq_dtype == MMDIT_BF16 && qkv_dtype == MMDIT_BF16 && dqkv_dtype == MMDIT_BF16) ? 0
       : (dq_dtype == MMDIT_F32 && qkv_dtype == MMDIT_F32 && dqkv_dtype == MMDIT_F32)    ? 1
       : (dq_dtype == MMDIT_BF16 && qkv_dtype == MMDIT_F32 && dqkv_dtype == MMDIT_F32)   ? 2 : -1;
}

// Every QK-norm + RoPE launcher validates its problem list here, once, and gets the kernel-side problems back.
// head_dim: 64 or 128, else MMDIT_ERR_SHAPE.  heads_max: the most heads the launch's workgroup of one row (one pair) holds, 0 = no cap; more
// heads return heads_err (MMDIT_ERR_ARG from the entry points of the core header, MMDIT_ERR_SHAPE from the 128-wide ones: what their headers say).
// merge: kv_merge_attn averages adjacent token pairs, and a pair never straddles two streams or two samples -- an odd tokens, tok0 or s_total
// is MMDIT_ERR_SHAPE.  bwd: dQ / dK / dV and the per-problem gradient pointers are required.  A token range outside [0, s_total] (the sum in
// 64 bits) is MMDIT_ERR_ARG; batch * tokens rows beyond INT_MAX are MMDIT_ERR_SHAPE (the kernels index rows with int).
static inline int qk_list(const mmdit_qk_problem* probs, int count, int batch, int heads, int head_dim, int s_total, int heads_max, int heads_err,
                          bool merge, bool bwd, const void* dQ, const void* dK, const void* dV, QkProb (&q)[2]) {
  MMDIT_CHECK_ARG(probs && count >= 1 && count <= 2 && batch > 0 && heads > 0 && s_total > 0 && (!bwd || (dQ && dK && dV)));
  if (head_dim != 64 && head_dim != 128) return MMDIT_ERR_SHAPE;
  if (heads_max && heads > heads_max) return heads_err;
  for (int i = 0; i < count; i++) {
    const mmdit_qk_problem* p = probs + i;
    MMDIT_CHECK_ARG(p->qkv && p->wq && p->wk && p->tokens > 0 && p->tok0 >= 0 && p->tok0 + (int64_t)p->tokens <= s_total && (p->rope_cos == nullptr) == (p->rope_sin == nullptr));
    MMDIT_CHECK_ARG(!bwd || (p->dqkv && p->dwq && p->dwk));
    if ((int64_t)batch * p->tokens > 0x7fffffff) return MMDIT_ERR_SHAPE;
    if (merge && ((p->tokens | p->tok0 | s_total) & 1)) return MMDIT_ERR_SHAPE;
    q[i] = QkProb{p->qkv, p->wq, p->wk, p->rope_cos, p->rope_sin, batch * p->tokens, p->tokens, p->tok0, dQ, dK, dV,
                  bwd ? p->dqkv : nullptr, bwd ? p->dwq : nullptr, bwd ? p->dwk : nullptr};
  }
  return 0;
}

// The first statement of a list kernel (QkProb p0, QkProb p1, int g0): declares the problem `p` of this workgroup (workgroup-uniform), the index
// `bid` of the workgroup among those of ITS problem and their number `nwg`.  (A macro: as inline functions the same three expressions reach the
// scheduler in another order, and either the forward or the backward kernels come out with another instruction stream.)
#define QK_SELECT(p, bid, nwg)                                                                        \
  const bool first = (int)blockIdx.x < g0;                                                            \
  const QkProb& p = first ? p0 : p1;                                                                  \
  const int bid = first ? (int)blockIdx.x : (int)blockIdx.x - g0, nwg = first ? g0 : (int)gridDim.x - g0
