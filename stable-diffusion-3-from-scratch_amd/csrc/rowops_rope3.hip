// Per-head QK RMSNorm + RoPE2dV2 + head split (mmdit_qk_norm_rope3_fwd / _bwd, include/mmdit_hip_rope3.h; reference:
// rotary_embedding_2d_v2.py, Attention.py:130-135, 220-239, 259-261 and their autograd) at head width 64 and 128.
// The work item is one head vector (row, part q/k/v, head) = HD / 8 lanes x 8 elements: its index IS the index of the vector in the qkv
// buffer, so the items of a problem are dealt to the workgroups in a grid-stride loop and any row and head count takes the same path.
// The rotation reads channel triples (3j, 3j+1, 3j+2) and writes channels j, T+j, 2T+j (T = HD / 3), neither of which follows the
// 8-element chunk a lane loads and stores with one 16-byte access.  So a head vector goes through LDS once: the lanes write their chunk
// (the normalised z in the forward, the incoming gradient in the backward), and every lane gathers the (up to) three values each of ITS
// eight output channels needs -- global reads and writes stay aligned 16-byte vectors in both directions.
// The arithmetic around the rotation (sum of squares, rsqrt, the two norm products, the norm backward and the weight-gradient
// accumulation) is that of qk_norm_rope_fwd_body / qk_norm_rope_bwd_body in rowops.hip; the problem list, its validation and the lane-group sum are
// those kernels' (qk_rows.h).  Plain kernels, not tuned.
#include "qk_rows.h"
#include "../../include/mmdit_hip_rope3.h"

namespace {

constexpr int WG = 256;                     // threads per workgroup: WG / (HD / 8) head vectors per iteration
// (bid, nwg) = this workgroup's index and the number of workgroups of ITS problem
template <typename TI, int HD>
__device__ __forceinline__ void qk3_fwd_body(int bid, int nwg, const TI* __restrict__ qkv, const float* __restrict__ wq, const float* __restrict__ wk,
                                             const float* __restrict__ rcos, const float* __restrict__ rsin,
                                             int rows, int tokens, int heads, int s_total, int tok0,
                                             bf16_t* __restrict__ Q, bf16_t* __restrict__ K, bf16_t* __restrict__ V) {
  constexpr int G = HD / 8, IPW = WG / G, T = HD / 3;
  __shared__ float sz[IPW][HD];
  const int slot = threadIdx.x / G, chunk = threadIdx.x % G;
  float wqv[8], wkv[8];
  ld8(wq + chunk * 8, wqv);
  ld8(wk + chunk * 8, wkv);
  const int64_t total = (int64_t)rows * 3 * heads;
  // `base` is workgroup-uniform: every thread runs the same number of iterations (the barriers below); a slot past the end re-reads the
  // last head vector and stores nothing
  for (int64_t base = (int64_t)bid * IPW; base < total; base += (int64_t)nwg * IPW) {
    const bool live = base + slot < total;
    const int64_t item = live ? base + slot : total - 1;
    const int head = (int)(item % heads), part = (int)((item / heads) % 3), row = (int)(item / (3 * (int64_t)heads));
    const int n = row % tokens, b = row / tokens;
    float x[8], o[8];
    ld8(qkv + item * HD + chunk * 8, x);
    if (part < 2) {
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) ss += x[e] * x[e];
      const float rinv = rsqrtf(group_sum<G>(ss) * (1.f / HD) + RMS_EPS);
#pragma unroll
      for (int e = 0; e < 8; e++) x[e] = x[e] * rinv * (part == 0 ? wqv[e] : wkv[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = x[e];
    if (rcos) {      // (workgroup-uniform)
      if (part < 2) {
#pragma unroll
        for (int e = 0; e < 8; e++) sz[slot][chunk * 8 + e] = x[e];
      }
      __syncthreads();
      if (part < 2) {
        const float* cs = rcos + (int64_t)n * (2 * T);
        const float* sn = rsin + (int64_t)n * (2 * T);
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int k = chunk * 8 + e;
          if (k < 3 * T) {      // (channels >= 3T pass through)
            const int grp = k / T, j = k - grp * T;
            const float a = sz[slot][3 * j], bb = sz[slot][3 * j + 1], d = sz[slot][3 * j + 2];
            const float ca = cs[T + j], sa = sn[T + j];
            if (grp == 2) {
              o[e] = bb * sa + d * ca;
            } else {
              const float ct = cs[j], st = sn[j];
              o[e] = grp == 0 ? a * ct - bb * st * ca + d * st * sa : a * st + bb * ct * ca - d * ct * sa;
            }
          }
        }
      }
      __syncthreads();      // (the next iteration overwrites sz)
    }
    if (live) {
      bf16_t* obase = part == 0 ? Q : part == 1 ? K : V;
      st8(obase + (((int64_t)b * heads + head) * s_total + tok0 + n) * HD + chunk * 8, o);
    }
  }
}
template <typename TI, int HD>
__global__ __launch_bounds__(WG) void qk3_fwd_kernel(QkProb p0, QkProb p1, int g0, int heads, int s_total,
                                                     bf16_t* __restrict__ Q, bf16_t* __restrict__ K, bf16_t* __restrict__ V) {
  QK_SELECT(p, bid, nwg);
  qk3_fwd_body<TI, HD>(bid, nwg, (const TI*)p.qkv, p.wq, p.wk, p.rcos, p.rsin, p.rows, p.tokens, heads, s_total, p.tok0, Q, K, V);
}

// Backward: the incoming gradient of a head vector goes through LDS (channel 3j + r needs dOut[j], dOut[T+j], dOut[2T+j]); the norm-weight
// gradients are summed per thread over its items (a thread keeps its chunk, its part changes: one accumulator each for q and k), over the
// threads with LDS atomics, and added with 2 * HD global atomics per workgroup.
template <typename TG, typename TI, typename TO, int HD>
__device__ __forceinline__ void qk3_bwd_body(int bid, int nwg, const TG* __restrict__ dQ, const TG* __restrict__ dK, const TG* __restrict__ dV,
                                             const TI* __restrict__ qkv, const float* __restrict__ wq, const float* __restrict__ wk,
                                             const float* __restrict__ rcos, const float* __restrict__ rsin,
                                             int rows, int tokens, int heads, int s_total, int tok0,
                                             TO* __restrict__ dqkv, float* __restrict__ dwq, float* __restrict__ dwk) {
  constexpr int G = HD / 8, IPW = WG / G, T = HD / 3;
  __shared__ float sg[IPW][HD];
  __shared__ float sdw[2][HD];
  for (int i = threadIdx.x; i < 2 * HD; i += WG) sdw[i / HD][i % HD] = 0.f;
  __syncthreads();
  const int slot = threadIdx.x / G, chunk = threadIdx.x % G;
  float wqv[8], wkv[8], awq[8], awk[8];
  ld8(wq + chunk * 8, wqv);
  ld8(wk + chunk * 8, wkv);
#pragma unroll
  for (int e = 0; e < 8; e++) { awq[e] = 0.f; awk[e] = 0.f; }
  const int64_t total = (int64_t)rows * 3 * heads;
  for (int64_t base = (int64_t)bid * IPW; base < total; base += (int64_t)nwg * IPW) {      // (as in the forward)
    const bool live = base + slot < total;
    const int64_t item = live ? base + slot : total - 1;
    const int head = (int)(item % heads), part = (int)((item / heads) % 3), row = (int)(item / (3 * (int64_t)heads));
    const int n = row % tokens, b = row / tokens;
    const TG* gbase = part == 0 ? dQ : part == 1 ? dK : dV;
    float g[8], dz[8], x[8];
    ld8_nt(gbase + (((int64_t)b * heads + head) * s_total + tok0 + n) * HD + chunk * 8, g);      // (single use; the saved qkv below: last use)
#pragma unroll
    for (int e = 0; e < 8; e++) { dz[e] = g[e]; x[e] = 0.f; }
    if (part < 2) ld8_nt(qkv + item * HD + chunk * 8, x);
    if (rcos) {      // (workgroup-uniform)
      if (part < 2) {
#pragma unroll
        for (int e = 0; e < 8; e++) sg[slot][chunk * 8 + e] = g[e];
      }
      __syncthreads();
      if (part < 2) {
        const float* cs = rcos + (int64_t)n * (2 * T);
        const float* sn = rsin + (int64_t)n * (2 * T);
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const int k = chunk * 8 + e;
          if (k < 3 * T) {
            const int j = k / 3, r = k - 3 * j;
            const float g0 = sg[slot][j], g1 = sg[slot][T + j], g2 = sg[slot][2 * T + j];
            const float ct = cs[j], st = sn[j], ca = cs[T + j], sa = sn[T + j];
            dz[e] = r == 0 ? g0 * ct + g1 * st : r == 1 ? g1 * ct * ca - g0 * st * ca + g2 * sa : g0 * st * sa - g1 * ct * sa + g2 * ca;
          }
        }
      }
      __syncthreads();
    }
    if (part < 2) {
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) ss += x[e] * x[e];
      const float rinv = rsqrtf(group_sum<G>(ss) * (1.f / HD) + RMS_EPS);
      const float keep = live ? 1.f : 0.f;      // (a slot past the end repeats the last item: it must not be counted twice)
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const float xh = x[e] * rinv, t = dz[e] * xh * keep;
        awq[e] += part == 0 ? t : 0.f;
        awk[e] += part == 1 ? t : 0.f;
        dz[e] *= part == 0 ? wqv[e] : wkv[e];                 // d(xhat)
        dot += dz[e] * xh;
        x[e] = xh;
      }
      dot = group_sum<G>(dot) * (1.f / HD);
#pragma unroll
      for (int e = 0; e < 8; e++) dz[e] = rinv * (dz[e] - x[e] * dot);
    }
    if (live) st8(dqkv + item * HD + chunk * 8, dz);
  }
#pragma unroll
  for (int e = 0; e < 8; e++) {
    atomicAdd(&sdw[0][chunk * 8 + e], awq[e]);
    atomicAdd(&sdw[1][chunk * 8 + e], awk[e]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * HD; i += WG) atomicAdd((i < HD ? dwq : dwk) + i % HD, sdw[i / HD][i % HD]);
}
template <typename TG, typename TI, typename TO, int HD>
__global__ __launch_bounds__(WG) void qk3_bwd_kernel(QkProb p0, QkProb p1, int g0, int heads, int s_total) {
  QK_SELECT(p, bid, nwg);
  qk3_bwd_body<TG, TI, TO, HD>(bid, nwg, (const TG*)p.dQ, (const TG*)p.dK, (const TG*)p.dV, (const TI*)p.qkv, p.wq, p.wk, p.rcos, p.rsin,
                               p.rows, p.tokens, heads, s_total, p.tok0, (TO*)p.dqkv, p.dwq, p.dwk);
}

// workgroups of one problem: one per WG / (HD / 8) head vectors, at most `wg_max` (the grid-stride loop takes the rest)
static inline int qk3_grid(const QkProb& p, int heads, int head_dim, int wg_max) {
  const int64_t ipw = WG / (head_dim / 8), need = ((int64_t)p.rows * 3 * heads + ipw - 1) / ipw;
  return (int)(need < wg_max ? need : wg_max);
}

}  // namespace

extern "C" int mmdit_qk_norm_rope3_fwd(const mmdit_qk_problem* probs, int count, int qkv_dtype, int batch, int heads, int head_dim,
                                       int s_total, void* Q, void* K, void* V, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V);
  QkProb q[2] = {};
  if (int e = qk_list(probs, count, batch, heads, head_dim, s_total, 0, 0, false, false, nullptr, nullptr, nullptr, q)) return e;
  if (qkv_dtype != MMDIT_BF16 && qkv_dtype != MMDIT_F32) return MMDIT_ERR_DTYPE;
  int g[2] = {0, 0};
  for (int i = 0; i < count; i++) g[i] = qk3_grid(q[i], heads, head_dim, 2048);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g[0] + g[1]), block(WG);
#define QKL(TI, HD) hipLaunchKernelGGL((qk3_fwd_kernel<TI, HD>), grid, block, 0, s, q[0], q[1], g[0], heads, s_total, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)V)
  if (qkv_dtype == MMDIT_BF16) { if (head_dim == 64) QKL(bf16_t, 64); else QKL(bf16_t, 128); }
  else { if (head_dim == 64) QKL(float, 64); else QKL(float, 128); }
#undef QKL
  return mmdit_launch_status();
}

extern "C" int mmdit_qk_norm_rope3_bwd(const mmdit_qk_problem* probs, int count, const void* dQ, const void* dK, const void* dV, int dq_dtype,
                                       int qkv_dtype, int dqkv_dtype, int batch, int heads, int head_dim, int s_total, mmdit_stream_t stream) {
  QkProb q[2] = {};
  if (int e = qk_list(probs, count, batch, heads, head_dim, s_total, 0, 0, false, true, dQ, dK, dV, q)) return e;
  const int combo = qk_bwd_combo(dq_dtype, qkv_dtype, dqkv_dtype);
  if (combo < 0) return MMDIT_ERR_DTYPE;
  int g[2] = {0, 0};
  for (int i = 0; i < count; i++) g[i] = qk3_grid(q[i], heads, head_dim, 512);      // (2 * head_dim global atomics per workgroup)
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g[0] + g[1]), block(WG);
#define QKL(TG, TI, TO, HD) hipLaunchKernelGGL((qk3_bwd_kernel<TG, TI, TO, HD>), grid, block, 0, s, q[0], q[1], g[0], heads, s_total)
#define QKH(TG, TI, TO) do { if (head_dim == 64) QKL(TG, TI, TO, 64); else QKL(TG, TI, TO, 128); } while (0)
  if (combo == 0) QKH(bf16_t, bf16_t, bf16_t);
  else if (combo == 1) QKH(float, float, float);
  else QKH(bf16_t, float, float);
#undef QKH
#undef QKL
  return mmdit_launch_status();
}
