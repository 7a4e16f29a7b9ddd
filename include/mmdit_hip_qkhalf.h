/* qk_half_dim (diff_model(..., qk_half_dim=True)): entry points of libmmdit_hip.so beside the versioned core ABI of mmdit_hip.h
 * (MMDIT_ABI_VERSION and the core symbol list do not change when an entry point is added here).  Same conventions as the core header,
 * mmdit_hip_ext.h, mmdit_hip_hd128.h and mmdit_hip_rope3.h: plain device pointers + sizes, nothing allocated, nothing synchronised,
 * launches only on the given stream; 0 on success, MMDIT_ERR_* (< 0) for invalid arguments -- in which case nothing is launched -- or a
 * positive hipError_t from the launch.
 *
 * With qk_half_dim the reference projects queries and keys to dim / 2 (Attention.py:33-67): with dim = 64 * num_heads a head has 32-wide
 * queries and keys -- normalised (RMSNorm(32)) and rotated (RotaryEmbedding(16): a (tokens, 32) table) at that width -- and 64-wide values,
 * and attends at scale = 64 ** -0.5 (the VALUE width).  A row of the QKV projection is therefore [q heads*32 | k heads*32 | v heads*64]
 * (2 * dim columns), which none of the other kernel families can express; these four are the unfused route of such a block: plain grouped
 * QKV GEMM with N = 2 * dim, then the row kernel, then the attention.  No kv_merge_attn, RoPE2dV2, e4m3 or fused forms.  The kernels are
 * plain (one register-staged double buffer, no LDS-DMA ring; one path for every row and head count) and not tuned.
 */
#ifndef MMDIT_HIP_QKHALF_H
#define MMDIT_HIP_QKHALF_H

#include "mmdit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Head widths of these entry points: queries / keys and values. */
#define MMDIT_QKHALF_QK_DIM 32
#define MMDIT_QKHALF_V_DIM 64
/* Tile edges of the attention kernels: rows of a streamed LDS tile (keys in the forward and dQ kernels, queries in the dK/dV kernel) and
 * stationary rows per workgroup (4 waves of 32 queries; keys in the dK/dV kernel): the shapes their tests are built around. */
#define MMDIT_ATTN_QKHALF_KEY_TILE 32
#define MMDIT_ATTN_QKHALF_QUERY_TILE 128

/* Joint softmax attention core, non-causal, bf16 operands, fp32 accumulate: mmdit_attn_fwd of the core header with 32-wide queries / keys.
 * Q, K: bf16 (batch, heads, S, 32); V: bf16 (batch, heads, S, 64).  Ox (batch, n_img, heads * 64), Oc (batch, S - n_img, heads * 64) bf16
 * (Oc may be NULL when n_img == S), lse fp32 (batch, heads, S).
 * mode 0: flash (fp32 scores, online softmax in the log2 domain, unnormalised P rounded to bf16, O rounded to bf16) -- the rounding points
 * of mmdit_attn_fwd mode 0.  mode 1: the rounding points of the reference's CPU branch (scores -> bf16, * scale -> bf16, softmax -> bf16,
 * P V -> bf16; two passes) -- those of mmdit_attn_fwd mode 1.
 * S < 1, n_img < 1 or n_img > S: MMDIT_ERR_SHAPE.  A NULL operand, batch <= 0, heads <= 0 or another mode: MMDIT_ERR_ARG. */
int mmdit_attn_fwd_qkhalf(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img,
                          float scale, int mode, void* Ox, void* Oc, float* lse, mmdit_stream_t stream);

/* Backward of the above: mmdit_attn_bwd of the core header with 32-wide queries / keys.  dOx / dOc bf16 (dOc may be NULL = zeros), delta
 * fp32 workspace (batch, heads, S) -- rowsum(dO * O) of the rounded O, produced by the dQ pass and consumed by the dK/dV pass --, dQ, dK
 * (batch, heads, S, 32) and dV (batch, heads, S, 64) written (not accumulated) in dq_dtype.  P and dS are rounded to bf16 for their matrix
 * products, as at width 64.  dq_dtype other than MMDIT_BF16 / MMDIT_F32: MMDIT_ERR_DTYPE; shapes and pointers as in the forward. */
int mmdit_attn_bwd_qkhalf(const void* Q, const void* K, const void* V, const void* Ox, const void* Oc,
                          const void* dOx, const void* dOc, const float* lse, float* delta,
                          int batch, int heads, int S, int n_img, float scale,
                          void* dQ, void* dK, void* dV, int dq_dtype, mmdit_stream_t stream);

/* Per-head QK RMSNorm (eps = FLT_EPSILON) + axial 2-D RoPE + head split into the joint [image;text] buffers: the role of
 * mmdit_qk_norm_rope_fwd.  qkv: (batch * tokens, heads * 32 | heads * 32 | heads * 64) rows of one stream = [q | k | v], bf16 or fp32
 * (qkv_dtype); wq / wk: fp32 (32); rope_cos / rope_sin of mmdit_qk_problem: fp32 (tokens, 32) tables, or both NULL (the text stream: the
 * norm only).  Writes bf16 Q, K (batch, heads, s_total, 32) and V (batch, heads, s_total, 64) at token offset tok0; V is the rounded copy
 * of the raw v columns.  A list of count = 1 or 2 problems in one launch; any heads >= 1 (a head vector is 4 lanes (q / k) or 8 lanes (v)
 * of 8 elements, dealt to the workgroups in a grid-stride loop).
 * qk_dim other than 32 or v_dim other than 64: MMDIT_ERR_SHAPE; qkv_dtype other than MMDIT_BF16 / MMDIT_F32: MMDIT_ERR_DTYPE; a NULL
 * operand, a bad count, only one of the two tables, or a token range outside [0, s_total]: MMDIT_ERR_ARG. */
int mmdit_qk_norm_rope_fwd_qkhalf(const mmdit_qk_problem* probs, int count, int qkv_dtype, int batch, int heads, int qk_dim, int v_dim,
                                  int s_total, void* Q, void* K, void* V, mmdit_stream_t stream);

/* Backward of the above: the role of mmdit_qk_norm_rope_bwd.  dqkv of every problem (the row layout of qkv) from dQ, dK (batch, heads,
 * s_total, 32) and dV (batch, heads, s_total, 64), dtype dq_dtype; dwq / dwk (32 floats each) are ADDED to (atomics).  dtype combinations
 * (dq, qkv, dqkv): all bf16, all fp32, or bf16 gradients of an fp32 projection (else MMDIT_ERR_DTYPE); other checks as in the forward. */
int mmdit_qk_norm_rope_bwd_qkhalf(const mmdit_qk_problem* probs, int count, const void* dQ, const void* dK, const void* dV, int dq_dtype,
                                  int qkv_dtype, int dqkv_dtype, int batch, int heads, int qk_dim, int v_dim, int s_total,
                                  mmdit_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MMDIT_HIP_QKHALF_H */
