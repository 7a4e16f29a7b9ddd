/* attn_type="cosine2" (diff_model(..., attn_type="cosine2")): entry points of libmmdit_hip.so beside the versioned core ABI of mmdit_hip.h
 * (MMDIT_ABI_VERSION and the core symbol list do not change when an entry point is added here).  Same conventions as the core header,
 * mmdit_hip_ext.h, mmdit_hip_hd128.h, mmdit_hip_rope3.h, mmdit_hip_qkhalf.h and mmdit_hip_textloss.h: plain device pointers + sizes, nothing
 * allocated, nothing synchronised, launches only on the given stream; 0 on success, MMDIT_ERR_* (< 0) for invalid arguments -- in which case
 * nothing is launched and nothing is written -- or a positive hipError_t from the launch.
 *
 * The reference's cosine2 attention (Attention.py:153-162, 330-339) L2-normalises queries and keys over the head vector (F.normalize, eps
 * 1e-12; no RMSNorm, no norm weights), rotates the image stream's as for softmax, and attends with the weights (q_i . k_j + 1) / sum_j:
 *     prod = q @ k.mT + 1;   out = (prod / prod.sum(-1)) @ v
 * which is, exactly,
 *     out_i = (q_i . KV + vsum) / (q_i . ksum + S),   KV = sum_j k_j (x) v_j (64 x 64), ksum = sum_j k_j, vsum = sum_j v_j  per (batch, head)
 * -- linear in the sequence length S.  Head width 64 only.  Every sum is fp32 (fp32 FMA kernels: the state never meets a bf16 rounding); the
 * only roundings below fp32 are the stored bf16 Q / K / V / O and gradients of the bf16 form.  No atomics anywhere: the token reduction is cut
 * into chunks of MMDIT_ATTN_COS2_TOKEN_CHUNK tokens whose partial states go to the caller's workspace and are summed in chunk order, so two
 * launches on the same operands are bit-equal.  Plain kernels, not tuned.
 */
#ifndef MMDIT_HIP_COS2_H
#define MMDIT_HIP_COS2_H

#include "mmdit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Head width of these entry points. */
#define MMDIT_COS2_HEAD_DIM 64
/* Tokens per partial state of the reduction over tokens (one workgroup, one slot of the workspace), and tokens per workgroup of the row
 * passes: the shapes their tests are built around. */
#define MMDIT_ATTN_COS2_TOKEN_CHUNK 128
#define MMDIT_ATTN_COS2_ROW_TILE 64

/* Per-head L2 normalisation x / max(||x||_2, 1e-12) + axial 2-D RoPE + head split into the joint [image;text] buffers: the role of
 * mmdit_qk_norm_rope_fwd at head width 64.  qkv: (batch * tokens, 3 * heads * 64) rows of one stream = [q | k | v], bf16 or fp32 (qkv_dtype);
 * the wq / wk / dwq / dwk members of mmdit_qk_problem are ignored and may be NULL; rope_cos / rope_sin: fp32 (tokens, 64) tables, or both
 * NULL (the text stream: the normalisation only).  Writes Q, K, V (batch, heads, s_total, 64) in out_dtype (bf16 or fp32) at token offset
 * tok0; V is the (rounded) copy of the raw v columns.  A list of count = 1 or 2 problems in one launch; any heads >= 1.
 * A NULL operand, a bad count, only one of the two tables, or a token range outside [0, s_total]: MMDIT_ERR_ARG; batch * tokens beyond
 * INT_MAX: MMDIT_ERR_SHAPE; qkv_dtype / out_dtype other than MMDIT_BF16 / MMDIT_F32: MMDIT_ERR_DTYPE. */
int mmdit_qk_l2norm_rope_fwd(const mmdit_qk_problem* probs, int count, int qkv_dtype, int out_dtype, int batch, int heads, int s_total,
                             void* Q, void* K, void* V, mmdit_stream_t stream);

/* Backward of the above: the transposed rotation, then dx = (dz - z (z . dz)) / max(||x||, 1e-12) with z the normalised vector; the v
 * columns pass through.  dqkv of every problem (the row layout of qkv) from dQ, dK, dV (batch, heads, s_total, 64), dtype dq_dtype.  No
 * weight gradient, so no atomics.  dtype combinations (dq, qkv, dqkv): all bf16, all fp32, or bf16 gradients of an fp32 projection (else
 * MMDIT_ERR_DTYPE); other checks as in the forward. */
int mmdit_qk_l2norm_rope_bwd(const mmdit_qk_problem* probs, int count, const void* dQ, const void* dK, const void* dV, int dq_dtype,
                             int qkv_dtype, int dqkv_dtype, int batch, int heads, int s_total, mmdit_stream_t stream);

/* Bytes of the workspace `ws` of the two launches below (the backward's need, which is twice the forward's): per (batch, head) two final
 * states and two partial states per chunk of MMDIT_ATTN_COS2_TOKEN_CHUNK tokens.  0 for batch, heads or S < 1.  Host function, no launch. */
long long mmdit_attn_cos2_ws_bytes(int batch, int heads, int S);

/* Joint cosine2 attention, non-causal.  Q, K, V: (batch, heads, S, 64) in qkv_dtype (bf16 or fp32), as the row kernel above leaves them.
 * Ox (batch, n_img, heads * 64), Oc (batch, S - n_img, heads * 64) in o_dtype, head-merged and split by stream exactly as mmdit_attn_fwd
 * writes them (Ox may be NULL when n_img == 0, Oc when n_img == S); den fp32 (batch, heads, S) = q_i . ksum + S, kept for the backward.
 * Two stages: the reduction over tokens (partial states per chunk -> ws, summed in chunk order), then a pass over the query rows.
 * dtype pairs (qkv, o): both bf16 or both fp32 (else MMDIT_ERR_DTYPE).  A NULL operand, batch <= 0 or heads <= 0: MMDIT_ERR_ARG;
 * S <= 0, n_img outside [0, S] or more than INT_MAX chunks / row tiles: MMDIT_ERR_SHAPE. */
int mmdit_attn_cos2_fwd(const void* Q, const void* K, const void* V, int qkv_dtype, int batch, int heads, int S, int n_img,
                        void* Ox, void* Oc, int o_dtype, float* den, void* ws, mmdit_stream_t stream);

/* Backward of the above.  With g = dO (dOx / dOc in o_dtype; dOc may be NULL = zeros, the last block), o = the stored O and den as written
 * by the forward:  dn_i = g_i / den_i,  dd_i = -(g_i . o_i) / den_i,  dq_i = KV dn_i + dd_i ksum,  dKV = sum_i q_i (x) dn_i,
 * dvsum = sum_i dn_i,  dksum = sum_i dd_i q_i,  dk_j = dKV v_j + dksum,  dv_j = k_j^T dKV + dvsum.  The same two kernel shapes as the
 * forward (the state {KV, ksum} is formed again).  dQ, dK, dV (batch, heads, S, 64) are written (not accumulated) in dq_dtype.
 * dtype triples (qkv, o, dq): all bf16, bf16 operands with fp32 gradients, or all fp32 (else MMDIT_ERR_DTYPE); other checks as in the forward. */
int mmdit_attn_cos2_bwd(const void* Q, const void* K, const void* V, int qkv_dtype, const void* Ox, const void* Oc,
                        const void* dOx, const void* dOc, int o_dtype, const float* den, int batch, int heads, int S, int n_img,
                        void* dQ, void* dK, void* dV, int dq_dtype, void* ws, mmdit_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MMDIT_HIP_COS2_H */
