/* Head width 128: entry points of libmmdit_hip.so beside the versioned core ABI of mmdit_hip.h (MMDIT_ABI_VERSION and the core symbol
 * list do not change when an entry point is added here).  Same conventions as the core header and mmdit_hip_ext.h: plain device pointers
 * + sizes, nothing allocated, nothing synchronised, launches only on the given stream; 0 on success, MMDIT_ERR_* (< 0) for invalid
 * arguments -- in which case nothing is launched -- or a positive hipError_t from the launch.
 *
 * The reference's Attention takes any dim / num_heads (Attention.py:16-67); the core header's kernels are built for 64.  These four are
 * the unfused route of a block at 128: QK-norm / RoPE / head split, attention forward, attention backward, QK-norm / RoPE backward.
 * The fused and e4m3 forms (mmdit_gemm_qkv_norm_rope, mmdit_attn_bwd_qk, mmdit_attn_fwd_mx, mmdit_attn_fwd_e4m3, the kv_merge launches)
 * exist at width 64 only.  The kernels are plain (one register-staged double buffer, no LDS-DMA ring) and not tuned.
 */
#ifndef MMDIT_HIP_HD128_H
#define MMDIT_HIP_HD128_H

#include "mmdit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tile edges of the attention kernels: rows of a streamed LDS tile (keys in the forward and dQ kernels, queries in the dK/dV kernel) and
 * stationary rows per workgroup (4 waves of 32 queries; keys in the dK/dV kernel): the shapes their tests are built around. */
#define MMDIT_ATTN_HD128_KEY_TILE 32
#define MMDIT_ATTN_HD128_QUERY_TILE 128
/* QK-norm / RoPE: a qkv row is one workgroup of 48 * heads threads, so heads <= 21; the backward packs 1024 / (48 * heads) rows into a
 * workgroup once every problem of the list has this many rows (the launch policy of the 64-wide entry points, whose row has 24 * heads threads:
 * the two widths are one kernel source and one policy). */
#define MMDIT_QK_HD128_MAX_HEADS 21
#define MMDIT_QK_HD128_RL_MIN_ROWS 2048

/* Joint softmax attention core, non-causal, head_dim 128, bf16 operands, fp32 accumulate: mmdit_attn_fwd of the core header at width 128.
 * Replaces flash_attn_func (Attention.py:293) and its CPU twin (Attention.py:277-284).
 * Q, K, V: bf16 (batch, heads, S, 128).  Ox (batch, n_img, heads * 128), Oc (batch, S - n_img, heads * 128) bf16 (Oc may be NULL when
 * n_img == S), lse fp32 (batch, heads, S).
 * mode 0: flash (fp32 scores, online softmax in the log2 domain, unnormalised P rounded to bf16, O rounded to bf16) -- the rounding points
 * of mmdit_attn_fwd mode 0.  mode 1: the rounding points of the reference's CPU branch (scores -> bf16, * scale -> bf16, softmax -> bf16,
 * P V -> bf16; two passes) -- those of mmdit_attn_fwd mode 1.
 * S < 1, n_img < 1 or n_img > S: MMDIT_ERR_SHAPE.  A NULL operand, batch <= 0, heads <= 0 or another mode: MMDIT_ERR_ARG. */
int mmdit_attn_fwd_hd128(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img,
                         float scale, int mode, void* Ox, void* Oc, float* lse, mmdit_stream_t stream);

/* Backward of the above (autograd of Attention.py:266-293): mmdit_attn_bwd of the core header at width 128.  dOx / dOc bf16 (dOc may be
 * NULL = zeros), delta fp32 workspace (batch, heads, S) -- rowsum(dO * O) of the rounded O, produced by the dQ pass and consumed by the
 * dK/dV pass --, dQ, dK, dV (batch, heads, S, 128) written (not accumulated) in dq_dtype.  P and dS are rounded to bf16 for their matrix
 * products, as at width 64.  dq_dtype other than MMDIT_BF16 / MMDIT_F32: MMDIT_ERR_DTYPE; shapes and pointers as in the forward. */
int mmdit_attn_bwd_hd128(const void* Q, const void* K, const void* V, const void* Ox, const void* Oc,
                         const void* dOx, const void* dOc, const float* lse, float* delta,
                         int batch, int heads, int S, int n_img, float scale,
                         void* dQ, void* dK, void* dV, int dq_dtype, mmdit_stream_t stream);

/* Per-head QK RMSNorm + axial 2-D RoPE + head split into the joint [image;text] buffers at head_dim 128: mmdit_qk_norm_rope_fwd of the
 * core header at width 128.  Attention.py:130-135 (q/k_norm_*), 178-194 + rotary_embedding.py:36-76,269-288 (RoPE2d), 259-261 (cat).
 * qkv: (batch * tokens, 3 * heads * 128) rows of one stream = [q | k | v]; wq / wk: fp32 (128); rope_cos / rope_sin: fp32 (tokens, 128)
 * tables or NULL; writes bf16 Q, K, V (batch, heads, s_total, 128) at token offset tok0.  A list of count = 1 or 2 problems in one launch.
 * heads > MMDIT_QK_HD128_MAX_HEADS: MMDIT_ERR_SHAPE; qkv_dtype other than MMDIT_BF16 / MMDIT_F32: MMDIT_ERR_DTYPE; a NULL operand, a bad
 * count, s_total <= 0 or a token range outside [0, s_total]: MMDIT_ERR_ARG; batch * tokens > INT_MAX: MMDIT_ERR_SHAPE. */
int mmdit_qk_norm_rope_fwd_hd128(const mmdit_qk_problem* probs, int count, int qkv_dtype, int batch, int heads, int s_total,
                                 void* Q, void* K, void* V, mmdit_stream_t stream);

/* Backward of the above (Attention.py:130-135, 178-194 under autograd): mmdit_qk_norm_rope_bwd of the core header at width 128.  dqkv from
 * dQ, dK, dV (batch, heads, s_total, 128; dtype dq_dtype); dwq / dwk (128 floats each) are ADDED to (atomics).  dtype combinations
 * (dq, qkv, dqkv): all bf16, all fp32, or bf16 gradients of an fp32 projection (else MMDIT_ERR_DTYPE); other checks as in the forward. */
int mmdit_qk_norm_rope_bwd_hd128(const mmdit_qk_problem* probs, int count, const void* dQ, const void* dK, const void* dV, int dq_dtype,
                                 int qkv_dtype, int dqkv_dtype, int batch, int heads, int s_total, mmdit_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MMDIT_HIP_HD128_H */
