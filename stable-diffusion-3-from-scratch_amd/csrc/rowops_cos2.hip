// Per-head L2 normalisation + axial RoPE2d + head split at head width 64 (attn_type="cosine2": mmdit_qk_l2norm_rope_fwd / _bwd,
// include/mmdit_hip_cos2.h; reference: Attention.py:153-162 (F.normalize over the head vector, eps 1e-12), 178-194 and their autograd).
// A qkv row is [q heads*64 | k heads*64 | v heads*64] = 24 * heads chunks of 8 elements, and a head vector is 8 consecutive chunks: the work
// item is one chunk = one lane, its index IS the index of the chunk in the qkv buffer, a head vector is an 8-aligned lane group of one wave.
// As in rowops_qkhalf.hip the chunks of a problem are dealt to 256-thread workgroups in a grid-stride loop, so any row and head count takes
// the same path.  The rotation pairs channels (2p, 2p + 1), which sit in one chunk: no LDS.  There are no norm weights, so the backward has
// no weight gradient and no atomics.  The problem struct and its selection in a list launch are those of the other row kernels (qk_rows.h);
// the validator is this file's own (the norm-weight pointers of a problem may be NULL here).  Plain kernels, not tuned.
#include "qk_rows.h"
#include "../../include/mmdit_hip_cos2.h"

namespace {

constexpr int WG = 256;                        // threads per workgroup = chunks per iteration
constexpr int HD = MMDIT_COS2_HEAD_DIM;
constexpr int G = HD / 8;                      // lanes of a head vector
static_assert(G == 8, "group_sum<8> and the chunk decoding below");
constexpr float L2_EPS = 1e-12f;               // F.normalize(eps=1e-12): x / max(||x||, eps)

// (bid, nwg) = this workgroup's index and the number of workgroups of ITS problem
template <typename TI, typename TO>
__device__ __forceinline__ void l2_fwd_body(int bid, int nwg, const TI* __restrict__ qkv, const float* __restrict__ rcos, const float* __restrict__ rsin,
                                            int rows, int tokens, int heads, int s_total, int tok0,
                                            TO* __restrict__ Q, TO* __restrict__ K, TO* __restrict__ V) {
  const int per_part = G * heads, per_row = 3 * per_part;
  const int64_t total = (int64_t)rows * per_row;      // (a multiple of 8: a lane group is live or past the end as a whole)
  for (int64_t base = (int64_t)bid * WG; base < total; base += (int64_t)nwg * WG) {
    const bool live = base + threadIdx.x < total;
    const int64_t item = live ? base + threadIdx.x : (int64_t)(threadIdx.x & (G - 1));      // a lane past the end re-reads the first vector and stores nothing
    const int row = (int)(item / per_row), r = (int)(item - (int64_t)row * per_row);
    const int part = r / per_part, head = (r - part * per_part) / G, piece = r & (G - 1);
    const int n = row % tokens, b = row / tokens;
    float x[8];
    ld8(qkv + item * 8, x);
    if (part < 2) {
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) ss += x[e] * x[e];
      const float nrm = fmaxf(sqrtf(group_sum<G>(ss)), L2_EPS);
#pragma unroll
      for (int e = 0; e < 8; e++) x[e] = x[e] / nrm;
      if (rcos) {
        float cs[8], sn[8];
        ld8(rcos + (int64_t)n * HD + piece * 8, cs);
        ld8(rsin + (int64_t)n * HD + piece * 8, sn);
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const float a = x[2 * p], bb = x[2 * p + 1];
          x[2 * p] = a * cs[2 * p] - bb * sn[2 * p];
          x[2 * p + 1] = bb * cs[2 * p + 1] + a * sn[2 * p + 1];
        }
      }
    }
    if (live) {
      const int64_t tok = ((int64_t)b * heads + head) * s_total + tok0 + n;
      st8((part == 0 ? Q : part == 1 ? K : V) + tok * HD + piece * 8, x);
    }
  }
}
template <typename TI, typename TO>
__global__ __launch_bounds__(WG) void l2_fwd_kernel(QkProb p0, QkProb p1, int g0, int heads, int s_total,
                                                    TO* __restrict__ Q, TO* __restrict__ K, TO* __restrict__ V) {
  QK_SELECT(p, bid, nwg);
  l2_fwd_body<TI, TO>(bid, nwg, (const TI*)p.qkv, p.rcos, p.rsin, p.rows, p.tokens, heads, s_total, p.tok0, Q, K, V);
}

// Backward: dz -> transposed rotation -> dx = (dz - z (z . dz)) / max(||x||, eps), z = x / max(||x||, eps) (a row of zeros: dz / eps)
template <typename TG, typename TI, typename TO>
__device__ __forceinline__ void l2_bwd_body(int bid, int nwg, const TG* __restrict__ dQ, const TG* __restrict__ dK, const TG* __restrict__ dV,
                                            const TI* __restrict__ qkv, const float* __restrict__ rcos, const float* __restrict__ rsin,
                                            int rows, int tokens, int heads, int s_total, int tok0, TO* __restrict__ dqkv) {
  const int per_part = G * heads, per_row = 3 * per_part;
  const int64_t total = (int64_t)rows * per_row;
  for (int64_t base = (int64_t)bid * WG; base < total; base += (int64_t)nwg * WG) {      // (as in the forward)
    const bool live = base + threadIdx.x < total;
    const int64_t item = live ? base + threadIdx.x : (int64_t)(threadIdx.x & (G - 1));
    const int row = (int)(item / per_row), r = (int)(item - (int64_t)row * per_row);
    const int part = r / per_part, head = (r - part * per_part) / G, piece = r & (G - 1);
    const int n = row % tokens, b = row / tokens;
    const int64_t tok = ((int64_t)b * heads + head) * s_total + tok0 + n;
    float dz[8];
    ld8_nt((part == 0 ? dQ : part == 1 ? dK : dV) + tok * HD + piece * 8, dz);      // (single use; the saved qkv below: last use)
    if (part < 2) {
      float x[8];
      ld8_nt(qkv + item * 8, x);
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) ss += x[e] * x[e];
      const float nrm = fmaxf(sqrtf(group_sum<G>(ss)), L2_EPS);
      if (rcos) {
        float cs[8], sn[8];
        ld8(rcos + (int64_t)n * HD + piece * 8, cs);
        ld8(rsin + (int64_t)n * HD + piece * 8, sn);
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const float da = dz[2 * p], db = dz[2 * p + 1];
          dz[2 * p] = da * cs[2 * p] + db * sn[2 * p + 1];
          dz[2 * p + 1] = db * cs[2 * p + 1] - da * sn[2 * p];
        }
      }
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) { x[e] = x[e] / nrm; dot += dz[e] * x[e]; }
      dot = group_sum<G>(dot);
#pragma unroll
      for (int e = 0; e < 8; e++) dz[e] = (dz[e] - x[e] * dot) / nrm;
    }
    if (live) st8(dqkv + item * 8, dz);
  }
}
template <typename TG, typename TI, typename TO>
__global__ __launch_bounds__(WG) void l2_bwd_kernel(QkProb p0, QkProb p1, int g0, int heads, int s_total) {
  QK_SELECT(p, bid, nwg);
  l2_bwd_body<TG, TI, TO>(bid, nwg, (const TG*)p.dQ, (const TG*)p.dK, (const TG*)p.dV, (const TI*)p.qkv, p.rcos, p.rsin,
                          p.rows, p.tokens, heads, s_total, p.tok0, (TO*)p.dqkv);
}

// workgroups of one problem: one per WG chunks, at most `wg_max` (the grid-stride loop takes the rest)
static inline int l2_grid(const QkProb& p, int heads, int wg_max) {
  const int64_t need = ((int64_t)p.rows * 3 * G * heads + WG - 1) / WG;
  return (int)(need < wg_max ? need : wg_max);
}

// qk_list of qk_rows.h without the norm weights: wq / wk / dwq / dwk are ignored and may be NULL
static inline int l2_list(const mmdit_qk_problem* probs, int count, int batch, int heads, int s_total, bool bwd,
                          const void* dQ, const void* dK, const void* dV, QkProb (&q)[2]) {
  MMDIT_CHECK_ARG(probs && count >= 1 && count <= 2 && batch > 0 && heads > 0 && s_total > 0 && (!bwd || (dQ && dK && dV)));
  for (int i = 0; i < count; i++) {
    const mmdit_qk_problem* p = probs + i;
    MMDIT_CHECK_ARG(p->qkv && p->tokens > 0 && p->tok0 >= 0 && p->tok0 + (int64_t)p->tokens <= s_total && (p->rope_cos == nullptr) == (p->rope_sin == nullptr));
    MMDIT_CHECK_ARG(!bwd || p->dqkv);
    if ((int64_t)batch * p->tokens > 0x7fffffff) return MMDIT_ERR_SHAPE;
    q[i] = QkProb{p->qkv, nullptr, nullptr, p->rope_cos, p->rope_sin, batch * p->tokens, p->tokens, p->tok0, dQ, dK, dV,
                  bwd ? p->dqkv : nullptr, nullptr, nullptr};
  }
  return 0;
}

}  // namespace

extern "C" int mmdit_qk_l2norm_rope_fwd(const mmdit_qk_problem* probs, int count, int qkv_dtype, int out_dtype, int batch, int heads, int s_total,
                                        void* Q, void* K, void* V, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V);
  QkProb q[2] = {};
  if (int e = l2_list(probs, count, batch, heads, s_total, false, nullptr, nullptr, nullptr, q)) return e;
  if ((qkv_dtype != MMDIT_BF16 && qkv_dtype != MMDIT_F32) || (out_dtype != MMDIT_BF16 && out_dtype != MMDIT_F32)) return MMDIT_ERR_DTYPE;
  int g[2] = {0, 0};
  for (int i = 0; i < count; i++) g[i] = l2_grid(q[i], heads, 2048);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g[0] + g[1]), block(WG);
#define QKL(TI, TO) hipLaunchKernelGGL((l2_fwd_kernel<TI, TO>), grid, block, 0, s, q[0], q[1], g[0], heads, s_total, (TO*)Q, (TO*)K, (TO*)V)
  if (qkv_dtype == MMDIT_BF16 && out_dtype == MMDIT_BF16) QKL(bf16_t, bf16_t);
  else if (qkv_dtype == MMDIT_BF16) QKL(bf16_t, float);
  else if (out_dtype == MMDIT_BF16) QKL(float, bf16_t);
  else QKL(float, float);
#undef QKL
  return mmdit_launch_status();
}

extern "C" int mmdit_qk_l2norm_rope_bwd(const mmdit_qk_problem* probs, int count, const void* dQ, const void* dK, const void* dV, int dq_dtype,
                                        int qkv_dtype, int dqkv_dtype, int batch, int heads, int s_total, mmdit_stream_t stream) {
  QkProb q[2] = {};
  if (int e = l2_list(probs, count, batch, heads, s_total, true, dQ, dK, dV, q)) return e;
  const int combo = qk_bwd_combo(dq_dtype, qkv_dtype, dqkv_dtype);
  if (combo < 0) return MMDIT_ERR_DTYPE;
  int g[2] = {0, 0};
  for (int i = 0; i < count; i++) g[i] = l2_grid(q[i], heads, 2048);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(g[0] + g[1]), block(WG);
#define QKL(TG, TI, TO) hipLaunchKernelGGL((l2_bwd_kernel<TG, TI, TO>), grid, block, 0, s, q[0], q[1], g[0], heads, s_total)
  if (combo == 0) QKL(bf16_t, bf16_t, bf16_t);
  else if (combo == 1) QKL(float, float, float);
  else QKL(bf16_t, float, float);
#undef QKL
  return mmdit_launch_status();
}
