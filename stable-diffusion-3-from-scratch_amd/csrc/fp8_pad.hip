// Zero-padded e4m3 quantisers (include/mmdit_hip_fp8pad.h): the per-tensor, delayed-scaling and MX quantisers of rowops.hip writing rows of
// K_pad = K rounded up to the 128-wide K tile of the e4m3 GEMM kernels, the columns [K, K_pad) as zero codes.  The arithmetic is shared with
// the plain quantisers (fp8_quant.h); only the indexing differs: the output has its own row pitch.  HBM-bound row kernels: 16-byte stores.
#include "fp8_quant.h"
#include "../../include/mmdit_hip_fp8pad.h"

namespace {

// One thread per 16 output bytes (a "piece"): ppr = K_pad / 16 pieces per row, piece i of the launch = (row i / ppr, piece c = i % ppr).
// K % 64 == 0 puts every piece wholly inside [0, K) -- 16 values in, quantised -- or wholly inside the pad -- a zero store.  total =
// rows * ppr < 2^31 (host check), so the 32-bit grid stride cannot wrap.
// DELAYED: the state protocol of fp8_quant_delayed_kernel (rowops.hip); otherwise amax in, scale out as fp8_quant_kernel.
template <typename TI, bool DELAYED>
__global__ __launch_bounds__(256) void fp8_quant_pad_kernel(const TI* __restrict__ x, unsigned K, int64_t ldx, unsigned ppr, unsigned total,
                                                            const float* __restrict__ amax, float* __restrict__ state, int phase, float margin,
                                                            uint4* __restrict__ q, float* __restrict__ scale) {
  __shared__ float sm[4];
  float dq;
  const float s = DELAYED ? fp8_range(state[phase % 3] * margin, dq) : fp8_range(amax[0], dq);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (DELAYED) { state[3] = dq; state[(phase + 2) % 3] = 0.f; }
    else scale[0] = dq;
  }
  float m = 0.f;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const unsigned row = i / ppr, c = i - row * ppr;
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    if (c * 16 < K) {
      const TI* src = x + (int64_t)row * ldx + c * 16;
      float v0[8], v1[8];
      ld8(src, v0);
      ld8(src + 8, v1);
      if (DELAYED) m = fp8_amax8(fp8_amax8(m, v0), v1);
      const uint2 lo = fp8_pack8(v0, s), hi = fp8_pack8(v1, s);
      o = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
    q[i] = o;
  }
  if (DELAYED) fp8_wg_amax(m, state + (phase + 1) % 3, sm);
}

// MX: one thread per 32-block of the padded row (fp8_quant.h: the pad blocks are quantised from zeros).
template <typename TI>
__global__ __launch_bounds__(256) void mxfp8_quant_pad_kernel(const TI* __restrict__ x, int rows, int K, int Kq, int64_t ldx, uint4* __restrict__ q,
                                                              unsigned char* __restrict__ sc) {
  mx_quant_block((int64_t)blockIdx.x * 256 + threadIdx.x, x, rows, K, Kq, ldx, q, sc);
}

// shared argument checks; *pieces = rows * K_pad / 16
int pad_checks(const void* x, int x_dtype, int rows, int K, int64_t ldx, const void* q, int* k_pad, int64_t* pieces) {
  MMDIT_CHECK_ARG(x && q && rows > 0);
  if (K <= 0 || K % 64 != 0 || K > (1 << 30)) return MMDIT_ERR_SHAPE;
  MMDIT_CHECK_ARG(ldx >= K && ldx % 8 == 0);
  if (x_dtype != MMDIT_F32 && x_dtype != MMDIT_BF16) return MMDIT_ERR_DTYPE;
  *k_pad = (K + 127) / 128 * 128;
  *pieces = (int64_t)rows * (*k_pad / 16);
  if (*pieces > 0x7fffffffll) return MMDIT_ERR_SHAPE;
  return 0;
}

template <bool DELAYED>
int launch_pad(const void* x, int x_dtype, int K, int64_t ldx, int k_pad, int64_t pieces, const float* amax, float* state, int phase, float margin,
               void* q, float* scale, mmdit_stream_t stream) {
  const int64_t g0 = (pieces + 255) / 256;
  const int64_t cap = DELAYED ? 1024 : 4096;      // (DELAYED: one atomic per workgroup on one address -- the plain delayed quantiser's cap)
  const dim3 grid((unsigned)(g0 > cap ? cap : g0));
  hipStream_t s = (hipStream_t)stream;
  if (x_dtype == MMDIT_F32)
    hipLaunchKernelGGL((fp8_quant_pad_kernel<float, DELAYED>), grid, dim3(256), 0, s, (const float*)x, (unsigned)K, ldx, (unsigned)(k_pad / 16), (unsigned)pieces,
                       amax, state, phase, margin, (uint4*)q, scale);
  else
    hipLaunchKernelGGL((fp8_quant_pad_kernel<bf16_t, DELAYED>), grid, dim3(256), 0, s, (const bf16_t*)x, (unsigned)K, ldx, (unsigned)(k_pad / 16), (unsigned)pieces,
                       amax, state, phase, margin, (uint4*)q, scale);
  return mmdit_launch_status();
}
}  // namespace

extern "C" int mmdit_fp8_quantize_pad(const void* x, int x_dtype, int rows, int K, int64_t ldx, const float* amax, void* q_fp8, float* scale,
                                      mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(amax && scale);
  int k_pad;
  int64_t pieces;
  const int rc = pad_checks(x, x_dtype, rows, K, ldx, q_fp8, &k_pad, &pieces);
  if (rc) return rc;
  return launch_pad<false>(x, x_dtype, K, ldx, k_pad, pieces, amax, nullptr, 0, 1.f, q_fp8, scale, stream);
}

extern "C" int mmdit_fp8_quantize_delayed_pad(const void* x, int x_dtype, int rows, int K, int64_t ldx, float* state, int phase, float margin, void* q_fp8,
                                              mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(state && phase >= 0 && margin >= 1.f);
  int k_pad;
  int64_t pieces;
  const int rc = pad_checks(x, x_dtype, rows, K, ldx, q_fp8, &k_pad, &pieces);
  if (rc) return rc;
  return launch_pad<true>(x, x_dtype, K, ldx, k_pad, pieces, nullptr, state, phase, margin, q_fp8, nullptr, stream);
}

extern "C" int mmdit_mxfp8_quantize_pad(const void* x, int x_dtype, int rows, int K, int64_t ldx, void* q_fp8, void* scales_e8m0, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(scales_e8m0);
  int k_pad;
  int64_t pieces;
  const int rc = pad_checks(x, x_dtype, rows, K, ldx, q_fp8, &k_pad, &pieces);
  if (rc) return rc;
  const int64_t nblk = pieces / 2;      // 32-blocks of the padded operand
  const dim3 grid((unsigned)((nblk + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  if (x_dtype == MMDIT_F32)
    hipLaunchKernelGGL((mxfp8_quant_pad_kernel<float>), grid, dim3(256), 0, s, (const float*)x, rows, K, k_pad, ldx, (uint4*)q_fp8, (unsigned char*)scales_e8m0);
  else
    hipLaunchKernelGGL((mxfp8_quant_pad_kernel<bf16_t>), grid, dim3(256), 0, s, (const bf16_t*)x, rows, K, k_pad, ldx, (uint4*)q_fp8, (unsigned char*)scales_e8m0);
  return mmdit_launch_status();
}
