/* Extension entry points of libmmdit_hip.so: opt-in kernels that are not part of the versioned core ABI of mmdit_hip.h
 * (MMDIT_ABI_VERSION and the core symbol list do not change when an entry point is added here).  Same conventions as the core
 * header: plain device pointers + sizes, nothing allocated, nothing synchronised, launches only on the given stream; 0 on success,
 * MMDIT_ERR_* (< 0) for invalid arguments -- in which case nothing is launched -- or a positive hipError_t from the launch.
 */
#ifndef MMDIT_HIP_EXT_H
#define MMDIT_HIP_EXT_H

#include "mmdit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tile edges of the e4m3 attention kernel (keys per LDS tile, queries per workgroup): the shapes its tests are built around. */
#define MMDIT_ATTN_E4M3_KEY_TILE 64
#define MMDIT_ATTN_E4M3_QUERY_TILE 128

/* Joint [image;text] softmax attention forward with e4m3 operands on both matrix products (reference: Attention.py:266-293, the
 * flash-attention call of the joint sequence; inference only: no lse, no backward).  Opt-in for the "fp8" / "mxfp8" precision modes.
 *   Q, K, V: bf16 (batch, heads, S, 64), as the QKV epilogue writes them; S >= 1, 0 <= n_img <= S (else MMDIT_ERR_SHAPE).
 *   Quantisation happens inside the launch on the tiles as they are loaded (no state, no extra pass).  With pow2(a) the power of two
 *   that maps a into (224, 448] (1 for a = 0), every conversion round-to-nearest-even and saturating at +-448:
 *     Q, K   one scale per row: e4m3(row * pow2(amax |row|));
 *     scores fp32 accumulator / (pow2_q pow2_k) * scale, keys past S masked to -inf; online softmax in fp32 with the unrounded p;
 *     P      e4m3(256 p), p relative to the running row maximum; the factor 256 leaves with the final 1 / l;
 *     V      one scale per tile of MMDIT_ATTN_E4M3_KEY_TILE keys (of one batch and head; rows past S count as zero):
 *            e4m3(V * pow2(amax |tile|)), removed in fp32 when the tile's partial product joins the output accumulator;
 *     O      bf16(o / l).
 *   scales_x == NULL: bf16 outputs Ox (batch, n_img, heads * 64), Oc (batch, S - n_img, heads * 64).
 *   scales_x != NULL: Ox / Oc are e4m3 codes of the same geometry and scales_x / scales_c their E8M0 block scales in the layout of
 *     mmdit_gemm_args.scale_mode 1 (K = heads * 64), bit-identical to the bf16 outputs followed by the core header's MX quantise pass.
 *   The pointers of a stream without tokens (n_img == 0: Ox, scales_x unless it selects the MX form; n_img == S: Oc, scales_c) may
 *   be NULL; any other NULL pointer, batch <= 0 or heads <= 0 is MMDIT_ERR_ARG. */
int mmdit_attn_fwd_e4m3(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale,
                        void* Ox, void* Oc, void* scales_x, void* scales_c, mmdit_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MMDIT_HIP_EXT_H */
