// Per-head QK RMSNorm + axial RoPE2d + head split with 32-wide queries / keys and 64-wide values (qk_half_dim: mmdit_qk_norm_rope_fwd_qkhalf /
// _bwd_qkhalf, include/mmdit_hip_qkhalf.h; reference: Attention.py:33-67, 130-135, 178-194, 259-261 and their autograd).
// A qkv row is [q heads*32 | k heads*32 | v heads*64] = 16 * heads chunks of 8 elements, and a head vector is 4 consecutive chunks (q / k)
// or 8 (v): the work item is one chunk = one lane, its index IS the index of the chunk in the qkv buffer, a q / k vector is a 4-aligned
// lane group of one wave.  As in rowops_rope3.hip the chunks of a problem are dealt to 256-thread workgroups in a grid-stride loop, so any row
// and head count takes the same path.  The rotation pairs channels (2p, 2p + 1), which sit in one chunk: no LDS in the forward.
// The arithmetic (sum of squares, rsqrt, the two norm products, the rotation, the norm backward and the weight-gradient accumulation) is that
// of qk_norm_rope_fwd_body / qk_norm_rope_bwd_body in rowops.hip at width 32; the problem list and its validation are those kernels'
// (qk_rows.h).  Plain kernels, not tuned.
#include "qk_rows.h"
#include "../../include/mmdit_hip_qkhalf.h"

namespace {

constexpr int WG = 256;                             // threads per workgroup = chunks per iteration
constexpr int DQK = MMDIT_QKHALF_QK_DIM, DV = MMDIT_QKHALF_V_DIM;
constexpr int GQ = DQK / 8, GV = DV / 8;            // lanes of a q / k vector and of a v vector
static_assert(GQ == 4 && GV == 8, "the lane-group sum and the chunk decoding below");

// sum over the 4 lanes of a q / k vector (a 4-aligned lane group of one wave)
__device__ __forceinline__ float sum4(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

// where chunk `r` of a row sits: part 0 q / 1 k / 2 v, its head and its piece of the head vector
struct Where { int part, head, piece; };
__device__ __forceinline__ Where decode(int r, int heads) {
  if (r < 2 * GQ * heads) {
    const int part = r >= GQ * heads, hc = r - part * GQ * heads;
    return {part, hc / GQ, hc % GQ};
  }
  const int hc = r - 2 * GQ * heads;
  return {2, hc / GV, hc % GV};
}

// (bid, nwg) = this workgroup's index and the number of workgroups of ITS problem
template <typename TI>
__device__ __forceinline__ void qkh_fwd_body(int bid, int nwg, const TI* __restrict__ qkv, const float* __restrict__ wq, const float* __restrict__ wk,
                                             const float* __restrict__ rcos, const float* __restrict__ rsin,
                                             int rows, int tokens, int heads, int s_total, int tok0,
                                             bf16_t* __restrict__ Q, bf16_t* __restrict__ K, bf16_t* __restrict__ V) {
  const int per_row = (2 * GQ + GV) * heads;
  const int64_t total = (int64_t)rows * per_row;      // (a multiple of 4: a lane group is live or past the end as a whole)
  // every boundary of a row is a multiple of 4 chunks and so is WG: the piece a thread holds of a q / k vector never changes
  float wqv[8], wkv[8];
  ld8(wq + (threadIdx.x & (GQ - 1)) * 8, wqv);
  ld8(wk + (threadIdx.x & (GQ - 1)) * 8, wkv);
  for (int64_t base = (int64_t)bid * WG; base < total; base += (int64_t)nwg * WG) {
    const bool live = base + threadIdx.x < total;
    const int64_t item = live ? base + threadIdx.x : (int64_t)(threadIdx.x & (GQ - 1));      // a lane past the end re-reads the first vector and stores nothing
    const int row = (int)(item / per_row);
    const Where w = decode((int)(item - (int64_t)row * per_row), heads);
    const int n = row % tokens, b = row / tokens;
    float x[8];
    ld8(qkv + item * 8, x);
    if (w.part < 2) {
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) ss += x[e] * x[e];
      const float rinv = rsqrtf(sum4(ss) * (1.f / DQK) + RMS_EPS);
#pragma unroll
      for (int e = 0; e < 8; e++) x[e] = x[e] * rinv * (w.part == 0 ? wqv[e] : wkv[e]);
      if (rcos) {
        float cs[8], sn[8];
        ld8(rcos + (int64_t)n * DQK + w.piece * 8, cs);
        ld8(rsin + (int64_t)n * DQK + w.piece * 8, sn);
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const float a = x[2 * p], bb = x[2 * p + 1];
          x[2 * p] = a * cs[2 * p] - bb * sn[2 * p];
          x[2 * p + 1] = bb * cs[2 * p + 1] + a * sn[2 * p + 1];
        }
      }
    }
    if (live) {
      const int64_t tok = ((int64_t)b * heads + w.head) * s_total + tok0 + n;
      if (w.part == 2) st8(V + tok * DV + w.piece * 8, x);
      else st8((w.part == 0 ? Q : K) + tok * DQK + w.piece * 8, x);
    }
  }
}
template <typename TI>
__global__ __launch_bounds__(WG) void qkh_fwd_kernel(QkProb p0, QkProb p1, int g0, int heads, int s_total,
                                                     bf16_t* __restrict__ Q, bf16_t* __restrict__ K, bf16_t* __restrict__ V) {
  QK_SELECT(p, bid, nwg);
  qkh_fwd_body<TI>(bid, nwg, (const TI*)p.qkv, p.wq, p.wk, p.rcos, p.rsin, p.rows, p.tokens, heads, s_total, p.tok0, Q, K, V);
}

// Backward: the norm-weight gradients are summed per thread over its items (a thread keeps its piece, its part changes: one accumulator
// each for q and k), over the threads with LDS atomics, and added with 2 * 32 global atomics per workgroup.
template <typename TG, typename TI, typename TO>
__device__ __forceinline__ void qkh_bwd_body(int bid, int nwg, const TG* __restrict__ dQ, const TG* __restrict__ dK, const TG* __restrict__ dV,
                                             const TI* __restrict__ qkv, const float* __restrict__ wq, const float* __restrict__ wk,
                                             const float* __restrict__ rcos, const float* __restrict__ rsin,
                                             int rows, int tokens, int heads, int s_total, int tok0,
                                             TO* __restrict__ dqkv, float* __restrict__ dwq, float* __restrict__ dwk) {
  __shared__ float sdw[2][DQK];
  for (int i = threadIdx.x; i < 2 * DQK; i += WG) sdw[i / DQK][i % DQK] = 0.f;
  __syncthreads();
  const int per_row = (2 * GQ + GV) * heads;
  const int64_t total = (int64_t)rows * per_row;
  const int pq = threadIdx.x & (GQ - 1);      // (the piece of every q / k vector this thread meets: see the forward)
  float wqv[8], wkv[8], awq[8], awk[8];
  ld8(wq + pq * 8, wqv);
  ld8(wk + pq * 8, wkv);
#pragma unroll
  for (int e = 0; e < 8; e++) { awq[e] = 0.f; awk[e] = 0.f; }
  for (int64_t base = (int64_t)bid * WG; base < total; base += (int64_t)nwg * WG) {      // (as in the forward)
    const bool live = base + threadIdx.x < total;
    const int64_t item = live ? base + threadIdx.x : (int64_t)(threadIdx.x & (GQ - 1));
    const int row = (int)(item / per_row);
    const Where w = decode((int)(item - (int64_t)row * per_row), heads);
    const int n = row % tokens, b = row / tokens;
    const int64_t tok = ((int64_t)b * heads + w.head) * s_total + tok0 + n;
    float dz[8];
    if (w.part == 2) ld8_nt(dV + tok * DV + w.piece * 8, dz);      // (single use; the saved qkv below: last use)
    else ld8_nt((w.part == 0 ? dQ : dK) + tok * DQK + w.piece * 8, dz);
    if (w.part < 2) {
      float x[8];
      ld8_nt(qkv + item * 8, x);
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) ss += x[e] * x[e];
      const float rinv = rsqrtf(sum4(ss) * (1.f / DQK) + RMS_EPS);
      if (rcos) {
        float cs[8], sn[8];
        ld8(rcos + (int64_t)n * DQK + w.piece * 8, cs);
        ld8(rsin + (int64_t)n * DQK + w.piece * 8, sn);
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const float da = dz[2 * p], db = dz[2 * p + 1];
          dz[2 * p] = da * cs[2 * p] + db * sn[2 * p + 1];
          dz[2 * p + 1] = db * cs[2 * p + 1] - da * sn[2 * p];
        }
      }
      const float keep = live ? 1.f : 0.f;      // (a lane past the end repeats the first vector: it must not be counted twice)
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const float xh = x[e] * rinv, t = dz[e] * xh * keep;
        awq[e] += w.part == 0 ? t : 0.f;
        awk[e] += w.part == 1 ? t : 0.f;
        dz[e] *= w.part == 0 ? wqv[e] : wkv[e];                 // d(xhat)
        dot += dz[e] * xh;
        x[e] = xh;
      }
      dot = sum4(dot) * (1.f / DQK);
#pragma unroll
      for (int e = 0; e < 8; e++) dz[e] = rinv * (dz[e] - x[e] * dot);
    }
    if (live) st8(dqkv + item * 8, dz);
  }
#pragma unroll
  for (int e = 0; e < 8; e++) {
    atomicAdd(&sdw[0][pq * 8 + e], awq[e]);
    atomicAdd(&sdw[1][pq * 8 + e], awk[e]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * DQK; i += WG) atomicAdd((i < DQK ? dwq : dwk) + i % DQK, sdw[i / DQK][i % DQK]);
}
template <typename TG, typename TI, typename TO>
__global__ __launch_bounds__(WG) void qkh_bwd_kernel(QkProb p0, QkProb p1, int g0, int heads, int s_total) {
  QK_SELECT(p, bid, nwg);
  qkh_bwd_body<TG, TI, TO>(bid, nwg, (const TG*)p.dQ, (const TG*)p.dK, (const TG*)p.dV, (const TI*)p.qkv, p.wq, p.wk, p.rcos, p.rsin,
                           p.rows, p.tokens, heads, s_total, p.tok0, (TO*)p.dqkv, p.dwq, p.dwk);
}

// workgroups of one problem: one per WG chunks, at most `wg_max` (the grid-stride loop takes the rest)
static inline int qkh_grid(const QkProb& p, int heads, int wg_max) {
  const int64_t need = ((int64_t)p.rows * (2 * GQ + GV) * heads + WG - 1) / WG;
  return (int)(need < wg_max ? need : wg_max);
}

// the widths these kernels are built for; the shared validator knows the value width (64) as a head width
static inline int qkh_list(const mmdit_qk_problem* probs, int count, int batch, int heads, int qk_dim, int v_dim, int s_total, bool bwd,
                           const void* dQ, const void* dK, const void* dV, QkProb (&q)[2]) {
  if (qk_dim != DQK || v_dim != DV) return MMDIT_ERR_SHAPE;
  return qk_list(probs, count, batch, heads, DV, s_total, 0, 0, false, bwd, dQ, dK, dV, q);
}

}  // namespace

extern "C" int mmdit_qk_norm_rope_fwd_qkhalf(const mmdit_qk_problem* probs, int count, int qkv_dtype, int batch, int heads, int qk_dim, int v_dim,
                                             int s_total, void* Q, void* K, void* V, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V);
  QkProb q[2] = {};
  if (int e = qkh_list(probs, count, batch, heads, qk_dim, v_dim, s_total, false, nullptr, nullptr, nullptr, q)) return e;
  if (qkv_dtype != MMDIT_BF16 && qkv_dtype != MMDIT_F32) return MMDIT_ERR_DTYPE;
  int g[2] = {0, 0};
  for (int i = 0; i < count; i++) g[i] = qkh_grid(q[i], heads, 2048);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g[0] + g[1]), block(WG);
#define QKL(TI) hipLaunchKernelGGL((qkh_fwd_kernel<TI>), grid, block, 0, s, q[0], q[1], g[0], heads, s_total, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)V)
  if (qkv_dtype == MMDIT_BF16) QKL(bf16_t);
  else QKL(float);
#undef QKL
  return mmdit_launch_status();
}

extern "C" int mmdit_qk_norm_rope_bwd_qkhalf(const mmdit_qk_problem* probs, int count, const void* dQ, const void* dK, const void* dV, int dq_dtype,
                                             int qkv_dtype, int dqkv_dtype, int batch, int heads, int qk_dim, int v_dim, int s_total,
                                             mmdit_stream_t stream) {
  QkProb q[2] = {};
  if (int e = qkh_list(probs, count, batch, heads, qk_dim, v_dim, s_total, true, dQ, dK, dV, q)) return e;
  const int combo = qk_bwd_combo(dq_dtype, qkv_dtype, dqkv_dtype);
  if (combo < 0) return MMDIT_ERR_DTYPE;
  int g[2] = {0, 0};
  for (int i = 0; i < count; i++) g[i] = qkh_grid(q[i], heads, 512);      // (2 * 32 global atomics per workgroup)
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g[0] + g[1]), block(WG);
#define QKL(TG, TI, TO) hipLaunchKernelGGL((qkh_bwd_kernel<TG, TI, TO>), grid, block, 0, s, q[0], q[1], g[0], heads, s_total)
  if (combo == 0) QKL(bf16_t, bf16_t, bf16_t);
  else if (combo == 1) QKL(float, float, float);
  else QKL(bf16_t, float, float);
#undef QKL
  return mmdit_launch_status();
}
