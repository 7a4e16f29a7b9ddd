// Masked text-reconstruction loss and its gradient (include/mmdit_hip_textloss.h).  A plain streaming kernel: one wave per row, a
// wave-uniform branch on the row's mask byte, 16-byte loads and stores, one fp32 accumulator per lane; the reduction is the two-launch,
// fixed-order scheme of mmdit_flow_loss (rowops.hip).
#include "common.h"
#include "../../include/mmdit_hip_textloss.h"

namespace {
constexpr int TL_ROWS = MMDIT_TEXT_LOSS_ROWS_PER_WG;
constexpr int TL_LANE = MMDIT_TEXT_LOSS_LANE_COLS;
constexpr int TL_WAVE = MMDIT_TEXT_LOSS_WAVE_COLS;
static_assert(TL_LANE == 8 && TL_WAVE == 64 * TL_LANE, "a lane moves 8 elements (ld8 / st8), a wave 64 lanes of them");
static_assert(MMDIT_TEXT_LOSS_MAX_PARTIALS % 64 == 0, "the final wave reads the partials 64 at a time");

template <typename TP, typename TL, typename TO>
__global__ __launch_bounds__(64 * TL_ROWS) void text_loss_partial_kernel(const TP* __restrict__ pred, const TL* __restrict__ label, const unsigned char* __restrict__ mask,
                                                                         int64_t rows, int cols, float coef2, TO* __restrict__ dpred, float* __restrict__ partials) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t groups = (rows + TL_ROWS - 1) / TL_ROWS;
  float s = 0.f;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t r = g * TL_ROWS + wave;
    if (r >= rows) continue;      // (the last group may be short; wave-uniform)
    const int on = __builtin_amdgcn_readfirstlane((int)mask[r]);      // one byte per row: the same address in every lane
    const int64_t base = r * (int64_t)cols;
    if (on) {
      for (int c = lane * TL_LANE; c < cols; c += TL_WAVE) {
        float a[8], b[8], o[8];
        ld8(pred + base + c, a);
        ld8(label + base + c, b);
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const float d = a[e] - b[e];
          s = __builtin_fmaf(d, d, s);
          o[e] = coef2 * d;
        }
        if (dpred) st8(dpred + base + c, o);
      }
    } else if (dpred) {      // excluded row: nothing is loaded, the gradient row is +0
      const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      // (not for the loop vectoriser: it rewrites this loop into 4-byte stores, four times the store instructions for the same bytes)
#pragma clang loop vectorize(disable) interleave(disable)
      for (int c = lane * TL_LANE; c < cols; c += TL_WAVE) st8(dpred + base + c, z);
    }
  }
  __shared__ float sm[TL_ROWS];
  s = wave_sum(s);
  if (lane == 0) sm[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = sm[0];
#pragma unroll
    for (int w = 1; w < TL_ROWS; w++) t += sm[w];
    partials[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(64) void text_loss_final_kernel(const float* __restrict__ partials, int count, float coef, float* __restrict__ loss) {
  float s = 0.f;
  for (int i = threadIdx.x; i < count; i += 64) s += partials[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) loss[0] = s * coef;
}

template <typename TP, typename TL>
void launch_out(const void* pred, const void* label, const unsigned char* mask, int64_t rows, int cols, float coef2, void* dpred, int dpred_dtype,
                float* partials, int grid, hipStream_t s) {
  if (dpred != nullptr && dpred_dtype == MMDIT_BF16)
    hipLaunchKernelGGL((text_loss_partial_kernel<TP, TL, bf16_t>), dim3(grid), dim3(64 * TL_ROWS), 0, s, (const TP*)pred, (const TL*)label, mask, rows, cols, coef2, (bf16_t*)dpred, partials);
  else      // (a forward-only launch takes the fp32 instantiation with a NULL output)
    hipLaunchKernelGGL((text_loss_partial_kernel<TP, TL, float>), dim3(grid), dim3(64 * TL_ROWS), 0, s, (const TP*)pred, (const TL*)label, mask, rows, cols, coef2, (float*)dpred, partials);
}
}  // namespace

extern "C" int mmdit_text_loss(const void* pred, int pred_dtype, const void* label, int label_dtype, const unsigned char* mask,
                               int64_t rows, int cols, float coef, void* dpred, int dpred_dtype,
                               float* partials, float* loss, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(pred && label && mask && partials && loss);
  MMDIT_CHECK_ARG((((uintptr_t)pred | (uintptr_t)label | (uintptr_t)dpred) & 15) == 0);
  const bool pd = pred_dtype == MMDIT_BF16 || pred_dtype == MMDIT_F32, ld = label_dtype == MMDIT_BF16 || label_dtype == MMDIT_F32;
  if (!pd || !ld || (dpred != nullptr && dpred_dtype != MMDIT_BF16 && dpred_dtype != MMDIT_F32)) return MMDIT_ERR_DTYPE;
  if (rows < 1 || cols < 8 || cols % 8 != 0) return MMDIT_ERR_SHAPE;
  const int64_t groups = (rows + TL_ROWS - 1) / TL_ROWS;
  const int grid = (int)(groups < MMDIT_TEXT_LOSS_MAX_PARTIALS ? groups : MMDIT_TEXT_LOSS_MAX_PARTIALS);
  hipStream_t s = (hipStream_t)stream;
  const float coef2 = 2.f * coef;
  if (pred_dtype == MMDIT_BF16 && label_dtype == MMDIT_BF16) launch_out<bf16_t, bf16_t>(pred, label, mask, rows, cols, coef2, dpred, dpred_dtype, partials, grid, s);
  else if (pred_dtype == MMDIT_BF16) launch_out<bf16_t, float>(pred, label, mask, rows, cols, coef2, dpred, dpred_dtype, partials, grid, s);
  else if (label_dtype == MMDIT_BF16) launch_out<float, bf16_t>(pred, label, mask, rows, cols, coef2, dpred, dpred_dtype, partials, grid, s);
  else launch_out<float, float>(pred, label, mask, rows, cols, coef2, dpred, dpred_dtype, partials, grid, s);
  hipLaunchKernelGGL(text_loss_final_kernel, dim3(1), dim3(64), 0, s, (const float*)partials, grid, coef, loss);
  return mmdit_launch_status();
}
