/* text_loss (diff_model(..., text_loss=True), model_trainer(text_loss_weight > 0)): entry point of libmmdit_hip.so beside the versioned core
 * ABI of mmdit_hip.h (MMDIT_ABI_VERSION and the core symbol list do not change when an entry point is added here).  Same conventions as the
 * core header and its siblings (mmdit_hip_ext.h, _hd128.h, _rope3.h, _qkhalf.h): plain device pointers + sizes, nothing allocated, nothing
 * synchronised, launches only on the given stream; 0 on success, MMDIT_ERR_* (< 0) for invalid arguments -- in which case nothing is
 * launched -- or a positive hipError_t from the launch.
 *
 * With text_loss the reference predicts the text embedding back from the final text stream (out_text_proj, diff_model.py:215-217, 344-346)
 * and the trainer adds a masked reconstruction term (model_trainer.py:399-454):
 *     text_loss_weight * (MSE(txt_pred, labels) * mask[:, :, None]).mean()
 * over (batch, 154, 2304) with a per-TOKEN mask that is true for few tokens (25 % of the tokens of null-conditioned samples).  The kernel below
 * is that term and its gradient with the token = row structure made explicit: rows the mask excludes are never read.
 */
#ifndef MMDIT_HIP_TEXTLOSS_H
#define MMDIT_HIP_TEXTLOSS_H

#include "mmdit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Launch shape of mmdit_text_loss (the shapes its tests are built around): a workgroup is MMDIT_TEXT_LOSS_ROWS_PER_WG waves of 64 lanes and
 * takes that many consecutive rows at a time, one row per wave; at most MMDIT_TEXT_LOSS_MAX_PARTIALS workgroups are launched, and with more
 * row groups than that a workgroup goes on to the group MAX_PARTIALS further (grid-stride).  A lane covers MMDIT_TEXT_LOSS_LANE_COLS
 * consecutive columns per step and the wave MMDIT_TEXT_LOSS_WAVE_COLS = 64 * LANE_COLS. */
#define MMDIT_TEXT_LOSS_ROWS_PER_WG 4
#define MMDIT_TEXT_LOSS_MAX_PARTIALS 256
#define MMDIT_TEXT_LOSS_LANE_COLS 8
#define MMDIT_TEXT_LOSS_WAVE_COLS 512

/* Masked squared-error loss over rows and its gradient.
 * pred, label: (rows, cols) row-major, each bf16 or fp32 (pred_dtype / label_dtype); mask: one byte per row, 0 or 1 (the storage of a
 * torch.bool); coef: the caller's weight / (element count * accumulation steps).
 *   loss[0]    = coef * sum_{r : mask[r]} sum_c (pred[r,c] - label[r,c])^2
 *   dpred[r,c] = 2 * coef * (pred[r,c] - label[r,c])  for rows with mask[r] != 0,  exactly +0 for the others
 * dpred: (rows, cols) in dpred_dtype (bf16 or fp32); EVERY row is written (no memset needed); NULL: forward only (dpred_dtype is then not
 * looked at).  Rows with mask[r] == 0 are never loaded (a wave-uniform branch): their pred / label may hold anything, NaN included.
 *
 * Evaluation (what the tests' bounds are derived from).  Per element: d = fl32(pred - label) from the loaded values widened to fp32 (one
 * rounding; exact for two bf16 values of nearby exponent), gradient fl_out(fl32((2 * coef) * d)) with 2 * coef formed exactly on the host.
 * Summation order of the loss, innermost first:
 *   1. serial, per lane: ONE fp32 accumulator s over everything the lane visits, s = fma(d, d, s) (one rounding per element): its row groups
 *      in grid-stride order, in a row its column steps c0 = 8 * lane, + 512, ... in ascending order, in a step the 8 elements in ascending
 *      order.  Serial length <= ceil(ceil(rows / ROWS_PER_WG) / grid) * ceil(cols / WAVE_COLS) * LANE_COLS with grid = min(ceil(rows /
 *      ROWS_PER_WG), MAX_PARTIALS) workgroups;
 *   2. tree, per wave: xor-butterfly over the 64 lanes, offsets 32, 16, 8, 4, 2, 1 (6 levels);
 *   3. the ROWS_PER_WG wave sums of a workgroup in wave order, ((w0 + w1) + w2) + w3, written to partials[workgroup];
 *   4. partials, second launch of one wave: lane l adds partials[l], partials[l + 64], ... in ascending order (<= MAX_PARTIALS / 64 = 4
 *      terms, starting from 0), the same 6-level butterfly, then one multiplication by coef.
 * Every term is >= 0, so the relative error of the sum is bounded by (number of roundings a term passes through) * 2^-24 to first order.
 * No atomics, no zero-initialised workspace, the same bits in every run: see mmdit_flow_loss in mmdit_hip.h for why that matters under
 * hipGraph replay.  partials: MMDIT_TEXT_LOSS_MAX_PARTIALS floats of workspace (every launched workgroup writes its slot, the rest is not read).
 *
 * 16-byte loads and stores: cols % 8 == 0 and 16-byte aligned pred / label / dpred.
 * rows < 1, cols < 8 or cols % 8 != 0: MMDIT_ERR_SHAPE.  A dtype other than MMDIT_BF16 / MMDIT_F32: MMDIT_ERR_DTYPE.  A NULL pred, label,
 * mask, partials or loss, or a misaligned pointer: MMDIT_ERR_ARG. */
int mmdit_text_loss(const void* pred, int pred_dtype, const void* label, int label_dtype, const unsigned char* mask,
                    int64_t rows, int cols, float coef, void* dpred, int dpred_dtype,
                    float* partials, float* loss, mmdit_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MMDIT_HIP_TEXTLOSS_H */
