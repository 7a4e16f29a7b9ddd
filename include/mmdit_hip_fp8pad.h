/* Zero-padded e4m3 quantisers (fp8 / mxfp8 inference at widths off the 128-wide K tile): entry points of libmmdit_hip.so beside the versioned
 * core ABI of mmdit_hip.h (MMDIT_ABI_VERSION and the core symbol list do not change when an entry point is added here).  Same conventions as
 * the core header, mmdit_hip_ext.h and mmdit_hip_cos2.h: plain device pointers + sizes, nothing allocated, nothing synchronised, launches only
 * on the given stream; 0 on success, MMDIT_ERR_* (< 0) for invalid arguments -- in which case nothing is launched and nothing is written -- or
 * a positive hipError_t from the launch.
 *
 * The e4m3 GEMM kernels need K % 128 == 0 (mmdit_gemm_args).  With dim = 64 * heads every odd head count gives K = dim = 64 (mod 128): the
 * QKV, out-projection and MLP-up operands of such a model.  These quantisers write the codes of a row-major operand x[rows][K] into rows of
 *     K_pad = (K + 127) / 128 * 128
 * bytes: columns [0, K) hold exactly the bytes the plain quantiser of the core header writes for the same x, columns [K, K_pad) the zero
 * code 0x00.  Both operands of a GEMM are padded that way and the GEMM runs unchanged with K = lda = ldb = K_pad: a zero code times anything
 * is zero, the product is exact.  The pad (64 bytes per row when K % 128 == 64, none when K % 128 == 0) is written by the kernel on EVERY
 * call, with ordinary 16-byte vector stores: the caller's buffers may be uninitialised (an unwritten e4m3fn byte can be a NaN code, 0x7F /
 * 0xFF, and an unwritten E8M0 byte the NaN scale 0xFF -- one of them poisons a whole output row of the GEMM).  When K % 128 == 0 the outputs
 * equal the plain entry points' byte for byte.  The arithmetic is the plain quantisers' own (one device header, csrc/fp8_quant.h).  Non-finite
 * inputs leave as the core header says next to mmdit_mxfp8_quantize.
 *
 * Common argument checks: a NULL pointer, rows <= 0, ldx < K or ldx % 8 != 0 (16-byte row loads): MMDIT_ERR_ARG; K <= 0, K % 64 != 0 or
 * rows * K_pad / 16 beyond INT_MAX: MMDIT_ERR_SHAPE; x_dtype other than MMDIT_BF16 / MMDIT_F32: MMDIT_ERR_DTYPE.
 */
#ifndef MMDIT_HIP_FP8PAD_H
#define MMDIT_HIP_FP8PAD_H

#include "mmdit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-tensor form, the second pass of the two-pass quantiser: amax[0] = max|x| over the same rows * K elements, collected by the core
 * header's amax pass (row by row when ldx > K).  q[rows][K_pad] = round_to_e4m3(x * 448 / amax) with zero pad, scale[0] = amax / 448
 * (the dequantisation scale of mmdit_gemm_args.scale_*, scale_mode 0).  Used for the cached weight copies. */
int mmdit_fp8_quantize_pad(const void* x, int x_dtype, int rows, int K, int64_t ldx, const float* amax, void* q_fp8, float* scale,
                           mmdit_stream_t stream);

/* Delayed scaling, one pass: the core header's delayed quantiser on the same 4-float state {amax ring [3], dequantisation scale (output)}
 * -- quantise with margin * state[phase % 3], maximise this call's amax (over the rows * K elements of x: the pad adds nothing) into
 * state[(phase + 1) % 3], clear state[(phase + 2) % 3] -- writing q[rows][K_pad] with zero pad.  phase < 0 or margin < 1: MMDIT_ERR_ARG. */
int mmdit_fp8_quantize_delayed_pad(const void* x, int x_dtype, int rows, int K, int64_t ldx, float* state, int phase, float margin, void* q_fp8,
                                   mmdit_stream_t stream);

/* MX (OCP microscaling) form, one pass, no state: q[rows][K_pad] and the E8M0 block scales in the scale_mode 1 layout of a (rows, K_pad)
 * operand ((K_pad / 64) * rows_pad128 * 2 + 512 bytes, rows_pad128 = rows rounded up to 128).  The K / 32 scales of the blocks inside
 * [0, K) are the core MX quantiser's (their place in the layout does not depend on the row width); the scales of the pad blocks are the
 * code of an all-zero block, 0x00 = 2^-127, also written on every call.  Scale bytes of the rows between rows and rows_pad128 are not
 * written (the GEMM reads them for output rows it never stores, as with the core quantiser). */
int mmdit_mxfp8_quantize_pad(const void* x, int x_dtype, int rows, int K, int64_t ldx, void* q_fp8, void* scales_e8m0, mmdit_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MMDIT_HIP_FP8PAD_H */
