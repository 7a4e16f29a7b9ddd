/* MX-emitting producers on zero-padded rows ("mxfp8" inference at widths off the 128-wide K tile): entry points of libmmdit_hip.so beside the
 * versioned core ABI of mmdit_hip.h (MMDIT_ABI_VERSION and the core symbol list do not change when an entry point is added here).  Same
 * conventions as the core header, mmdit_hip_ext.h and mmdit_hip_fp8pad.h: plain device pointers + sizes, nothing allocated, nothing
 * synchronised, launches only on the given stream; 0 on success, MMDIT_ERR_* (< 0) for invalid arguments -- in which case nothing is
 * launched and nothing is written -- or a positive hipError_t from the launch.
 *
 * The MX producers of the core header and of mmdit_hip_ext.h (mmdit_ln_modulate_fwd_mx, mmdit_attn_fwd_mx, mmdit_attn_fwd_e4m3 with MX
 * outputs) write the e4m3 codes of a (rows, d) activation into rows of d bytes and the E8M0 block scales of a (rows, d) operand.  The e4m3
 * GEMM kernels need K % 128 == 0, and dim = 64 * heads with an odd head count gives d = 64 (mod 128).  The producers below write what
 * mmdit_hip_fp8pad.h defines for such an operand, so that the GEMM takes their output as it takes mmdit_mxfp8_quantize_pad's:
 *     K_pad = (d + 127) / 128 * 128
 *   - q[rows][K_pad]: columns [0, d) hold exactly the bytes the unpadded producer writes, columns [d, K_pad) the zero code 0x00;
 *   - the scales are laid out as those of a (rows, K_pad) operand ((K_pad / 64) * rows_pad128 * 2 + 512 bytes): the d / 32 scales of the
 *     blocks inside [0, d) are the unpadded producer's bytes in the same places (the place of a scale byte does not depend on the row
 *     width), the scales of the pad blocks are 0x00 (2^-127, the code of an all-zero block);
 *   - pad codes (16-byte vector stores) and pad scales are written on EVERY call: the caller's buffers may be uninitialised (an unwritten
 *     e4m3fn byte can be a NaN code, an unwritten E8M0 byte the NaN scale 0xFF);
 *   - scale bytes of the rows between rows and rows_pad128 are not written, as with the unpadded producers.
 * Together: bit-identical to the bf16 producer followed by mmdit_mxfp8_quantize_pad.  When d % 128 == 0 there is no pad and the outputs
 * equal the unpadded producers' byte for byte (the same kernels run).  The device code is the unpadded kernels' own (a template flag).
 *
 * Common argument checks: d (heads * 64) not a positive multiple of 64, or rows * K_pad / 16 beyond INT_MAX: MMDIT_ERR_SHAPE; a NULL
 * operand, output or scale pointer: MMDIT_ERR_ARG; dtypes as for the unpadded forms.
 */
#ifndef MMDIT_HIP_MXPAD_H
#define MMDIT_HIP_MXPAD_H

#include "mmdit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* adaLN with MX output over a list of count = 1 or 2 problems of the same width in ONE launch (the image and the text stream of a block):
 * mmdit_ln_modulate_fwd's problem list with out = the code rows q[rows][K_pad] of a problem and scales_e8m0_<i> the scale buffer of
 * problem i (scales_e8m0_1 is ignored when count == 1).  acc != NULL in all problems or in none: the pending gated residual update
 * (bf16 acc, acc_dtype = MMDIT_BF16; x_out is written), as in mmdit_ln_modulate_fwd_mx.  x_out, mean and rstd are the unpadded kernel's. */
int mmdit_ln_modulate_fwd_mx_pad(const mmdit_ln_fwd_problem* probs, int count, int d, int acc_dtype, void* scales_e8m0_0, void* scales_e8m0_1,
                                 mmdit_stream_t stream);

/* mmdit_attn_fwd_mx with the head-merged outputs Ox / Oc as e4m3 (B, tokens, K_pad), d = heads * 64.  The pad of a token and its two scale
 * bytes belong to no head: the workgroups of the last head write them for their own query rows (one writer, no atomics, one launch). */
int mmdit_attn_fwd_mx_pad(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale,
                          void* Ox_fp8, void* Oc_fp8, void* scales_x, void* scales_c, mmdit_stream_t stream);

/* The MX-output form of mmdit_attn_fwd_e4m3, the attention with e4m3 operands on both matrix products, with the outputs padded the same way; scales_x (and
 * scales_c unless n_img == S) must be given, n_img >= 1. */
int mmdit_attn_fwd_e4m3_mx_pad(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale,
                               void* Ox_fp8, void* Oc_fp8, void* scales_x, void* scales_c, mmdit_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MMDIT_HIP_MXPAD_H */
