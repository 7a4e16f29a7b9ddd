/* RoPE2dV2 (positional_encoding="RoPE2dV2"): entry points of libmmdit_hip.so beside the versioned core ABI of mmdit_hip.h
 * (MMDIT_ABI_VERSION and the core symbol list do not change when an entry point is added here).  Same conventions as the core header,
 * mmdit_hip_ext.h and mmdit_hip_hd128.h: plain device pointers + sizes, nothing allocated, nothing synchronised, launches only on the
 * given stream; 0 on success, MMDIT_ERR_* (< 0) for invalid arguments -- in which case nothing is launched -- or a positive hipError_t
 * from the launch.
 *
 * The reference's second 2-D rotary encoding (rotary_embedding_2d_v2.py, Attention.py:105-107, 220-239) rotates channel TRIPLES of a
 * normalised image query / key by two angles -- one from the token's row, one from its column on the patch grid -- and writes the three
 * rotated components as three concatenated groups.  With T = head_dim / 3 (integer division), z the per-head RMSNorm output and
 * (a, b, d) = (z[3j], z[3j+1], z[3j+2]), j < T:
 *     out[j]      = a cos(th_j) - b sin(th_j) cos(al_j) + d sin(th_j) sin(al_j)
 *     out[T + j]  = a sin(th_j) + b cos(th_j) cos(al_j) - d cos(th_j) sin(al_j)
 *     out[2T + j] =               b sin(al_j)           + d cos(al_j)
 *     out[k]      = z[k]  for k >= 3T          (channel 63 at width 64; channels 126, 127 at width 128)
 * An orthogonal map (a rotation, then a de-interleaving permutation), so the backward is its transpose.  The pair kernels of the core
 * header cannot express it through their tables; these two are the unfused route of a block with this encoding, at head width 64 or 128:
 * plain grouped QKV GEMM, then this row kernel, then mmdit_attn_fwd / mmdit_attn_fwd_hd128.
 *
 * The kernels have ONE layout for every row and head count (a head vector is head_dim / 8 lanes of 8 elements; the (row, q|k|v, head)
 * vectors of a problem are dealt to the workgroups in a grid-stride loop), so there is no switch constant and no cap on heads.
 */
#ifndef MMDIT_HIP_ROPE3_H
#define MMDIT_HIP_ROPE3_H

#include "mmdit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-head QK RMSNorm + RoPE2dV2 + head split into the joint [image;text] buffers: the role of mmdit_qk_norm_rope_fwd.
 * qkv: (batch * tokens, 3 * heads * head_dim) rows of one stream = [q | k | v], bf16 or fp32 (qkv_dtype); wq / wk: fp32 (head_dim);
 * rope_cos / rope_sin of mmdit_qk_problem: fp32 (tokens, 2T) tables, rope_cos = [cos th_0 .. cos th_{T-1} | cos al_0 .. cos al_{T-1}],
 * rope_sin the same with sines -- or both NULL: no rotation and no permutation (the text stream: the norm only, natural channel order).
 * Writes bf16 Q, K, V (batch, heads, s_total, head_dim) at token offset tok0; V is the rounded copy of the v columns.  Everything is fp32
 * from the loaded row; Q / K are rounded to bf16 once.  A list of count = 1 or 2 problems in one launch; any heads >= 1.
 * head_dim other than 64 / 128: MMDIT_ERR_SHAPE; qkv_dtype other than MMDIT_BF16 / MMDIT_F32: MMDIT_ERR_DTYPE; a NULL operand, a bad
 * count, only one of the two tables, or a token range outside [0, s_total]: MMDIT_ERR_ARG. */
int mmdit_qk_norm_rope3_fwd(const mmdit_qk_problem* probs, int count, int qkv_dtype, int batch, int heads, int head_dim,
                            int s_total, void* Q, void* K, void* V, mmdit_stream_t stream);

/* Backward of the above: the role of mmdit_qk_norm_rope_bwd.  dqkv of every problem from dQ, dK, dV (batch, heads, s_total, head_dim;
 * dtype dq_dtype): the transposed rotation (da = g0 cos th + g1 sin th, db = -g0 sin th cos al + g1 cos th cos al + g2 sin al,
 * dd = g0 sin th sin al - g1 cos th sin al + g2 cos al with (g0, g1, g2) = (dOut[j], dOut[T+j], dOut[2T+j])), then the RMSNorm backward;
 * dwq / dwk (head_dim floats each) are ADDED to (atomics).  dtype combinations (dq, qkv, dqkv): all bf16, all fp32, or bf16 gradients of
 * an fp32 projection (else MMDIT_ERR_DTYPE); other checks as in the forward. */
int mmdit_qk_norm_rope3_bwd(const mmdit_qk_problem* probs, int count, const void* dQ, const void* dK, const void* dV, int dq_dtype,
                            int qkv_dtype, int dqkv_dtype, int batch, int heads, int head_dim, int s_total, mmdit_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MMDIT_HIP_ROPE3_H */
