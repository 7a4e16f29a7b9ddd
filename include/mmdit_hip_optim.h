/* Optimizer entry points of libmmdit_hip.so outside the versioned core ABI of mmdit_hip.h (MMDIT_ABI_VERSION and the core symbol list do not
 * change when an entry point is added here).  Same conventions as the core header and its siblings: plain device pointers + sizes, nothing
 * allocated, nothing synchronised, launches only on the given stream; 0 on success, MMDIT_ERR_* (< 0) for invalid arguments -- in which case
 * nothing is launched -- or a positive hipError_t from the launch.
 */
#ifndef MMDIT_HIP_OPTIM_H
#define MMDIT_HIP_OPTIM_H

#include "mmdit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mmdit_adamw_step_dlr with one step counter PER TENSOR: step_counts is a DEVICE array of fp32 counters, step_counts[i] the number of steps
 * tensors[i] has taken so far (the index is the row of the tensor table, i.e. the value stored in chunk_tensor[c], also when chunk_tensor /
 * chunk_off point into the middle of the chunk map).  The bias corrections of chunk c use t = step_counts[chunk_tensor[c]] + 1.
 * torch's fused AdamW keeps `step` per parameter and skips parameters whose .grad is None, so the counters of one param group differ as
 * soon as a parameter receives its first gradient late or misses a step (torch/optim/adamw.py, _fused_adamw: `state_steps`); the
 * reference trainer zeroes gradients to None after every step (model_trainer.py:503).  Everything else as mmdit_adamw_step_dlr. */
int mmdit_adamw_step_dlr_pt(const mmdit_adamw_tensor* tensors, const int* chunk_tensor, const int64_t* chunk_off, int n_chunks, const float* coef_found,
                            const float* step_counts, const double* lr_dev, double beta1, double beta2, double eps, double weight_decay, mmdit_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MMDIT_HIP_OPTIM_H */
