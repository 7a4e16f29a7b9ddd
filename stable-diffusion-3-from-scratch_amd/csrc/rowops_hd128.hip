// Per-head QK RMSNorm + axial RoPE + head split at head width 128 (mmdit_qk_norm_rope_fwd_hd128 / _bwd_hd128, include/mmdit_hip_hd128.h;
// reference: Attention.py:130-135, 178-194, 259-261 and their autograd).  The arithmetic and the accumulation scheme of
// qk_norm_rope_fwd_body / qk_norm_rope_bwd_body in rowops.hip with 16 lanes x 8 elements per head vector instead of 8 x 8:
// a qkv row is 48 * heads threads (thread = (part q/k/v, head, 8-element chunk)), two rows in flight per workgroup and iteration, the
// norm-weight gradients summed per thread over its rows, over the heads with LDS atomics, and added with 256 global atomics per workgroup.
// Plain kernels, not tuned.
#include "common.h"
#include "../../include/mmdit_hip_hd128.h"

namespace {

constexpr int HD = 128;
constexpr int CH = HD / 8;                  // 8-element chunks (= lanes) per head vector
constexpr int ROW_T = 3 * CH;               // threads per head of a qkv row
constexpr float RMS_EPS = 1.1920929e-07f;   // nn.RMSNorm(eps=None) on fp32 input: finfo(float32).eps (= RMS_EPS of rowops.hip)

// sum over the 16 lanes of a head vector (a 16-aligned lane group: the threads of a row are a multiple of 16)
__device__ __forceinline__ float group16_sum(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
  return v;
}

// a list of one or two problems (workgroups [0, g0) = problem 0): the image and the text rows of a block write the same Q / K / V, different token ranges
struct QkProb {
  const void* qkv; const float* wq; const float* wk; const float* rcos; const float* rsin; int rows, tokens, tok0;
  const void* dQ; const void* dK; const void* dV; void* dqkv; float* dwq; float* dwk;      // (backward only)
};

// (bid, rstride) = this workgroup's index and the number of workgroups of ITS problem
template <typename TI>
__device__ __forceinline__ void qk_fwd_body(int bid, int rstride, const TI* __restrict__ qkv, const float* __restrict__ wq, const float* __restrict__ wk,
                                            const float* __restrict__ rcos, const float* __restrict__ rsin,
                                            int rows, int tokens, int heads, int s_total, int tok0,
                                            bf16_t* __restrict__ Q, bf16_t* __restrict__ K, bf16_t* __restrict__ V) {
  const int hc = threadIdx.x % (CH * heads), part = threadIdx.x / (CH * heads), head = hc / CH, chunk = hc % CH;
  bf16_t* obase = part == 0 ? Q : part == 1 ? K : V;
  float w[8];
#pragma unroll
  for (int e = 0; e < 8; e++) w[e] = 0.f;
  if (part < 2) ld8((part == 0 ? wq : wk) + chunk * 8, w);
  // grid a multiple of the tokens per sample: every row of this workgroup is the same token, its RoPE factors are loaded once
  const bool same_token = rcos && rstride % tokens == 0;
  float cs[2][8], sn[2][8];
  if (same_token && part < 2) {
    const int n = bid % tokens;
    ld8(rcos + (int64_t)n * HD + chunk * 8, cs[0]);
    ld8(rsin + (int64_t)n * HD + chunk * 8, sn[0]);
#pragma unroll
    for (int e = 0; e < 8; e++) { cs[1][e] = cs[0][e]; sn[1][e] = sn[0][e]; }
  }
  for (int row0 = bid; row0 < rows; row0 += 2 * rstride) {
    float x[2][8];
    // both rows' loads are issued unconditionally (a row past the end re-reads the last row and is dropped below)
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int row = min(row0 + k * rstride, rows - 1);
      ld8(qkv + (((int64_t)row * 3 + part) * heads + head) * HD + chunk * 8, x[k]);
    }
    if (part < 2 && rcos && !same_token) {
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const int n = min(row0 + k * rstride, rows - 1) % tokens;
        ld8(rcos + (int64_t)n * HD + chunk * 8, cs[k]);
        ld8(rsin + (int64_t)n * HD + chunk * 8, sn[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int row = row0 + k * rstride;
      if (row >= rows) break;
      const int n = row % tokens, b = row / tokens;
      if (part < 2) {
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) ss += x[k][e] * x[k][e];
        const float rinv = rsqrtf(group16_sum(ss) * (1.f / HD) + RMS_EPS);
#pragma unroll
        for (int e = 0; e < 8; e++) x[k][e] = x[k][e] * rinv * w[e];
        if (rcos) {
#pragma unroll
          for (int p = 0; p < 4; p++) {
            const float a = x[k][2 * p], bb = x[k][2 * p + 1];
            x[k][2 * p] = a * cs[k][2 * p] - bb * sn[k][2 * p];
            x[k][2 * p + 1] = bb * cs[k][2 * p + 1] + a * sn[k][2 * p + 1];
          }
        }
      }
      st8(obase + (((int64_t)b * heads + head) * s_total + tok0 + n) * HD + chunk * 8, x[k]);
    }
  }
}
template <typename TI>
__global__ __launch_bounds__(1024) void qk_fwd_hd128_kernel(QkProb p0, QkProb p1, int g0, int heads, int s_total,
                                                            bf16_t* __restrict__ Q, bf16_t* __restrict__ K, bf16_t* __restrict__ V) {
  const bool first = (int)blockIdx.x < g0;     // (workgroup-uniform)
  const QkProb& p = first ? p0 : p1;
  qk_fwd_body<TI>(first ? (int)blockIdx.x : (int)blockIdx.x - g0, first ? g0 : (int)gridDim.x - g0, (const TI*)p.qkv, p.wq, p.wk, p.rcos, p.rsin,
                  p.rows, p.tokens, heads, s_total, p.tok0, Q, K, V);
}

// Backward: a workgroup is RL row lanes of 48 * heads threads; the RL rows of an iteration share ONE set of 256 global atomics at the end.
template <typename TG, typename TI, typename TO>
__device__ __forceinline__ void qk_bwd_body(int bid, int rstride, const TG* __restrict__ dQ, const TG* __restrict__ dK, const TG* __restrict__ dV,
                                            const TI* __restrict__ qkv, const float* __restrict__ wq, const float* __restrict__ wk,
                                            const float* __restrict__ rcos, const float* __restrict__ rsin,
                                            int rows, int tokens, int heads, int s_total, int tok0,
                                            TO* __restrict__ dqkv, float* __restrict__ dwq, float* __restrict__ dwk) {
  __shared__ float sdw[2][HD];
  for (int i = threadIdx.x; i < 2 * HD; i += blockDim.x) sdw[i / HD][i % HD] = 0.f;
  __syncthreads();
  const int per_row = ROW_T * heads, rlane = threadIdx.x / per_row, t = threadIdx.x - rlane * per_row;
  { const int RL = blockDim.x / per_row; bid = bid * RL + rlane; rstride *= RL; }
  const int hc = t % (CH * heads), part = t / (CH * heads), head = hc / CH, chunk = hc % CH;
  const TG* gbase = part == 0 ? dQ : part == 1 ? dK : dV;
  float w[8], aw[8];
#pragma unroll
  for (int e = 0; e < 8; e++) { w[e] = 0.f; aw[e] = 0.f; }
  if (part < 2) ld8((part == 0 ? wq : wk) + chunk * 8, w);
  const bool same_token = rcos && rstride % tokens == 0;
  // ONE copy of the factors (the kernel sits at the 128-VGPR cap of a 1024-thread workgroup): loaded here when every row of this lane is
  // the same token, else per row right before its use
  float cs[8], sn[8];
  if (same_token && part < 2) {
    const int n = bid % tokens;
    ld8(rcos + (int64_t)n * HD + chunk * 8, cs);
    ld8(rsin + (int64_t)n * HD + chunk * 8, sn);
  }
  for (int row0 = bid; row0 < rows; row0 += 2 * rstride) {
    float dz[2][8], x[2][8];
    // loads of both rows issued back to back, unconditionally (a row past the end re-reads the last row and is dropped below)
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int row = min(row0 + k * rstride, rows - 1);
      const int n = row % tokens, b = row / tokens;
      ld8_nt(gbase + (((int64_t)b * heads + head) * s_total + tok0 + n) * HD + chunk * 8, dz[k]);      // (single use; the saved qkv below: last use)
    }
    if (part < 2) {
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const int row = min(row0 + k * rstride, rows - 1);
        ld8_nt(qkv + (((int64_t)row * 3 + part) * heads + head) * HD + chunk * 8, x[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int row = row0 + k * rstride;
      if (row >= rows) break;
      if (part < 2) {
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) ss += x[k][e] * x[k][e];
        const float rinv = rsqrtf(group16_sum(ss) * (1.f / HD) + RMS_EPS);
        if (rcos) {
          if (!same_token) {
            ld8(rcos + (int64_t)(row % tokens) * HD + chunk * 8, cs);
            ld8(rsin + (int64_t)(row % tokens) * HD + chunk * 8, sn);
          }
#pragma unroll
          for (int p = 0; p < 4; p++) {
            const float da = dz[k][2 * p], db = dz[k][2 * p + 1];
            dz[k][2 * p] = da * cs[2 * p] + db * sn[2 * p + 1];
            dz[k][2 * p + 1] = db * cs[2 * p + 1] - da * sn[2 * p];
          }
        }
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const float xh = x[k][e] * rinv;
          aw[e] += dz[k][e] * xh;
          dz[k][e] *= w[e];                 // d(xhat)
          dot += dz[k][e] * xh;
          x[k][e] = xh;
        }
        dot = group16_sum(dot) * (1.f / HD);
#pragma unroll
        for (int e = 0; e < 8; e++) dz[k][e] = rinv * (dz[k][e] - x[k][e] * dot);
      }
      st8(dqkv + (((int64_t)row * 3 + part) * heads + head) * HD + chunk * 8, dz[k]);
    }
  }
  // weight gradients: sum over rows (done) and heads: LDS atomics per (part, column), then 256 global atomics per workgroup
  if (part < 2) {
#pragma unroll
    for (int e = 0; e < 8; e++) atomicAdd(&sdw[part][chunk * 8 + e], aw[e]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * HD; i += blockDim.x) atomicAdd((i < HD ? dwq : dwk) + i % HD, sdw[i / HD][i % HD]);
}
template <typename TG, typename TI, typename TO>
__global__ __launch_bounds__(1024) void qk_bwd_hd128_kernel(QkProb p0, QkProb p1, int g0, int heads, int s_total) {
  const bool first = (int)blockIdx.x < g0;     // (workgroup-uniform)
  const QkProb& p = first ? p0 : p1;
  qk_bwd_body<TG, TI, TO>(first ? (int)blockIdx.x : (int)blockIdx.x - g0, first ? g0 : (int)gridDim.x - g0, (const TG*)p.dQ, (const TG*)p.dK, (const TG*)p.dV,
                          (const TI*)p.qkv, p.wq, p.wk, p.rcos, p.rsin, p.rows, p.tokens, heads, s_total, p.tok0, (TO*)p.dqkv, p.dwq, p.dwk);
}

// validates the problem list (as qk_list of rowops.hip) and returns the kernel-side problems
static inline int qk_list(const mmdit_qk_problem* probs, int count, int batch, int heads, int s_total, bool bwd, const void* dQ, const void* dK, const void* dV, QkProb (&q)[2]) {
  MMDIT_CHECK_ARG(probs && count >= 1 && count <= 2 && batch > 0 && heads > 0 && s_total > 0 && (!bwd || (dQ && dK && dV)));
  if (heads > MMDIT_QK_HD128_MAX_HEADS) return MMDIT_ERR_SHAPE;      // a row is one workgroup of 48 * heads <= 1024 threads
  for (int i = 0; i < count; i++) {
    const mmdit_qk_problem* p = probs + i;
    MMDIT_CHECK_ARG(p->qkv && p->wq && p->wk && p->tokens > 0 && p->tok0 >= 0 && p->tok0 + (int64_t)p->tokens <= s_total && (p->rope_cos == nullptr) == (p->rope_sin == nullptr));
    MMDIT_CHECK_ARG(!bwd || (p->dqkv && p->dwq && p->dwk));
    if ((int64_t)batch * p->tokens > 0x7fffffff) return MMDIT_ERR_SHAPE;
    q[i] = QkProb{p->qkv, p->wq, p->wk, p->rope_cos, p->rope_sin, batch * p->tokens, p->tokens, p->tok0, dQ, dK, dV,
                  bwd ? p->dqkv : nullptr, bwd ? p->dwq : nullptr, bwd ? p->dwk : nullptr};
  }
  return 0;
}
// workgroups of one problem: up to `lanes_max` rows in flight, RL per workgroup; with RoPE a multiple of the tokens per sample when one fits
// (every row of a lane is then the same token and the factors are loaded once)
static inline int qk_grid(const QkProb& p, int lanes_max, int rl) {
  int lanes = p.rows < lanes_max ? p.rows : lanes_max;
  if (p.rcos && p.tokens <= lanes) {
    int k = lanes / p.tokens;
    while (k > 1 && (k * p.tokens) % rl) k--;
    if ((k * p.tokens) % rl == 0) return k * p.tokens / rl;
  }
  return lanes / rl > 0 ? lanes / rl : 1;
}

}  // namespace

extern "C" int mmdit_qk_norm_rope_fwd_hd128(const mmdit_qk_problem* probs, int count, int qkv_dtype, int batch, int heads, int s_total,
                                            void* Q, void* K, void* V, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V);
  QkProb q[2] = {};
  if (int e = qk_list(probs, count, batch, heads, s_total, false, nullptr, nullptr, nullptr, q)) return e;
  if (qkv_dtype != MMDIT_BF16 && qkv_dtype != MMDIT_F32) return MMDIT_ERR_DTYPE;
  int g[2] = {0, 0};
  for (int i = 0; i < count; i++) g[i] = qk_grid(q[i], 1024, 1);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g[0] + g[1]), block(ROW_T * heads);
  if (qkv_dtype == MMDIT_BF16) hipLaunchKernelGGL((qk_fwd_hd128_kernel<bf16_t>), grid, block, 0, s, q[0], q[1], g[0], heads, s_total, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)V);
  else hipLaunchKernelGGL((qk_fwd_hd128_kernel<float>), grid, block, 0, s, q[0], q[1], g[0], heads, s_total, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)V);
  return mmdit_launch_status();
}

extern "C" int mmdit_qk_norm_rope_bwd_hd128(const mmdit_qk_problem* probs, int count, const void* dQ, const void* dK, const void* dV, int dq_dtype,
                                            int qkv_dtype, int dqkv_dtype, int batch, int heads, int s_total, mmdit_stream_t stream) {
  QkProb q[2] = {};
  if (int e = qk_list(probs, count, batch, heads, s_total, true, dQ, dK, dV, q)) return e;
  // dtype combinations (dQ / dK / dV, saved qkv, dqkv): all bf16, all fp32, bf16 gradients of an fp32 projection -- those of mmdit_qk_norm_rope_bwd
  const int combo = (dq_dtype == MMDIT_BF16 && qkv_dtype == MMDIT_BF16 && dqkv_dtype == MMDIT_BF16) ? 0
                  : (dq_dtype == MMDIT_F32 && qkv_dtype == MMDIT_F32 && dqkv_dtype == MMDIT_F32)    ? 1
                  : (dq_dtype == MMDIT_BF16 && qkv_dtype == MMDIT_F32 && dqkv_dtype == MMDIT_F32)   ? 2 : -1;
  if (combo < 0) return MMDIT_ERR_DTYPE;
  // row lanes per workgroup: as many as fit 1024 threads once every problem has MMDIT_QK_HD128_RL_MIN_ROWS rows (one block shape per launch)
  const int min_rows = count == 2 && q[1].rows < q[0].rows ? q[1].rows : q[0].rows;
  const int rl = min_rows >= MMDIT_QK_HD128_RL_MIN_ROWS ? 1024 / (ROW_T * heads) : 1;
  int g[2] = {0, 0};
  for (int i = 0; i < count; i++) g[i] = qk_grid(q[i], rl > 1 ? 768 : 512, rl);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g[0] + g[1]), block(ROW_T * heads * rl);
#define QKL(TG, TI, TO) hipLaunchKernelGGL((qk_bwd_hd128_kernel<TG, TI, TO>), grid, block, 0, s, q[0], q[1], g[0], heads, s_total)
  if (combo == 0) QKL(bf16_t, bf16_t, bf16_t);
  else if (combo == 1) QKL(float, float, float);
  else QKL(bf16_t, float, float);
#undef QKL
  return mmdit_launch_status();
}
