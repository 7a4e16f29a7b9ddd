// Linear-time cosine2 attention at head width 64 (attn_type="cosine2": mmdit_attn_cos2_fwd / _bwd, include/mmdit_hip_cos2.h; reference:
// Attention.py:330-339).  With unit-norm q, k:   out_i = sum_j (q_i . k_j + 1) v_j / sum_j (q_i . k_j + 1) = (q_i KV + vsum) / (q_i . ksum + S),
// KV = sum_j k_j (x) v_j, ksum = sum_j k_j, vsum = sum_j v_j per (batch, head): a STATE of 64 * 64 + 64 + 64 floats.  Two kernel shapes:
//   reduce : outer products A_j (x) B_j (+ sum_j w_j A_j, sum_j B_j) over the tokens of one chunk (MMDIT_ATTN_COS2_TOKEN_CHUNK) -> one partial
//            state in the workspace; a second stage sums the partial states of a (batch, head) in chunk order (and keeps the transpose).
//   rows   : out_i = x_i M + vec (+ w_i vec2), a 64 x 64 state applied to the rows of one tile (MMDIT_ATTN_COS2_ROW_TILE).
// Forward: reduce(A = k, B = v, w = 1), rows(x = q, M = KV, vec = vsum; divided by den_i = q_i . ksum + S, which is kept).
// Backward (g = dO, o = the stored O):  dn_i = g_i / den_i, dd_i = -(g_i . o_i) / den_i;  reduce(k, v, 1) again and reduce(A = q, B = dn, w = dd)
// = {dKV, dksum, dvsum};  rows: dq = dn KV^T + dd ksum,  dk = v dKV^T + dksum,  dv = k dKV + dvsum.
// Arithmetic: every operand is widened to fp32 on load, every product and sum is an fp32 FMA in a fixed order (token order inside a chunk,
// chunk order across chunks, channel order in the row pass) -- no atomics, no bf16 MFMA, the state is never rounded below fp32; the only
// roundings below fp32 are those of the stored outputs.  Plain kernels, not tuned.
#include "common.h"
#include "qk_rows.h"
#include "../../include/mmdit_hip_cos2.h"

namespace {

constexpr int HD = MMDIT_COS2_HEAD_DIM;
constexpr int CHUNK = MMDIT_ATTN_COS2_TOKEN_CHUNK, RT = MMDIT_ATTN_COS2_ROW_TILE;
constexpr int SUB = 32;                              // tokens staged in LDS at a time by the reduction (256 threads x one 8-element piece)
constexpr int WG = 256;
constexpr int STATE = HD * HD + 2 * HD;              // a partial state: M (64 x 64, row = A's channel) | sum w A | sum B
constexpr int FSTATE = 2 * HD * HD + 2 * HD;         // a final state: M | M^T | sum w A | sum B
static_assert(HD == 64 && CHUNK % SUB == 0 && RT * 4 == WG && SUB * 8 == WG, "thread maps below");

// the row of token i of (batch b, head h) in a head-merged, stream-split O / dO: nullptr when the stream's pointer is
template <typename T>
__device__ __forceinline__ const T* o_row(const T* X, const T* C, int b, int h, int heads, int i, int S, int n_img) {
  if (i < n_img) return X ? X + (((int64_t)b * n_img + i) * heads + h) * HD : nullptr;
  return C ? C + (((int64_t)b * (S - n_img) + (i - n_img)) * heads + h) * HD : nullptr;
}

// MODE 0: A = K, B = V, w = 1.  MODE 1: A = Q, B = dn = g / den, w = dd = -(g . o) / den.
// grid: x = bh * nchunks + chunk.  Thread (ty, tx) = (tid / 16, tid % 16) owns the 4 x 4 block (4 ty .., 4 tx ..) of M.
template <typename TQ, typename TO, int MODE>
__global__ __launch_bounds__(WG) void cos2_reduce_kernel(const TQ* __restrict__ A, const TQ* __restrict__ B, const TO* __restrict__ Ox, const TO* __restrict__ Oc,
                                                         const TO* __restrict__ dOx, const TO* __restrict__ dOc, const float* __restrict__ den,
                                                         int heads, int S, int n_img, int nchunks, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float As[SUB][HD];
  __shared__ __attribute__((aligned(16))) float Bs[SUB][HD];
  __shared__ float Ws[SUB];
  const int bh = blockIdx.x / nchunks, chunk = blockIdx.x - bh * nchunks;
  const int b = bh / heads, h = bh - b * heads;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, jj = tid >> 3, piece = tid & 7;
  float acc[4][4], asum[4], bsum[4];
#pragma unroll
  for (int a = 0; a < 4; a++) {
    asum[a] = 0.f; bsum[a] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; c++) acc[a][c] = 0.f;
  }
  for (int sub = 0; sub < CHUNK / SUB; sub++) {
    const int i = chunk * CHUNK + sub * SUB + jj;      // the token this thread stages one piece of
    const bool valid = i < S;
    float av[8], bv[8], w = 1.f;
#pragma unroll
    for (int e = 0; e < 8; e++) { av[e] = 0.f; bv[e] = 0.f; }
    if (valid) ld8(A + ((int64_t)bh * S + i) * HD + piece * 8, av);
    if constexpr (MODE == 0) {
      if (valid) ld8(B + ((int64_t)bh * S + i) * HD + piece * 8, bv);
    } else {
      float ov[8];
#pragma unroll
      for (int e = 0; e < 8; e++) ov[e] = 0.f;
      const TO* gr = valid ? o_row(dOx, dOc, b, h, heads, i, S, n_img) : nullptr;      // (nullptr: dOc == NULL, the gradient is zero)
      if (gr) {
        ld8(gr + piece * 8, bv);
        ld8(o_row(Ox, Oc, b, h, heads, i, S, n_img) + piece * 8, ov);
      }
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) dot += bv[e] * ov[e];
      dot = group_sum<8>(dot);                         // (the 8 pieces of a token are an 8-aligned lane group; every lane takes part)
      const float d = valid ? den[(int64_t)bh * S + i] : 1.f;
      w = -dot / d;
#pragma unroll
      for (int e = 0; e < 8; e++) bv[e] = bv[e] / d;
    }
    __syncthreads();                                   // (the previous sub-tile has been consumed)
    *(float4*)&As[jj][piece * 8] = make_float4(av[0], av[1], av[2], av[3]);
    *(float4*)&As[jj][piece * 8 + 4] = make_float4(av[4], av[5], av[6], av[7]);
    *(float4*)&Bs[jj][piece * 8] = make_float4(bv[0], bv[1], bv[2], bv[3]);
    *(float4*)&Bs[jj][piece * 8 + 4] = make_float4(bv[4], bv[5], bv[6], bv[7]);
    if (piece == 0) Ws[jj] = w;
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < SUB; j++) {                    // (rows past S are zeros)
      const float4 a4 = *(const float4*)&As[j][ty * 4], b4 = *(const float4*)&Bs[j][tx * 4];
      const float aa[4] = {a4.x, a4.y, a4.z, a4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
      const float wj = Ws[j];
#pragma unroll
      for (int a = 0; a < 4; a++) {
        asum[a] = __builtin_fmaf(aa[a], wj, asum[a]);
        bsum[a] += bb[a];
#pragma unroll
        for (int c = 0; c < 4; c++) acc[a][c] = __builtin_fmaf(aa[a], bb[c], acc[a][c]);
      }
    }
  }
  float* out = part + (int64_t)blockIdx.x * STATE;
#pragma unroll
  for (int a = 0; a < 4; a++) *(float4*)(out + (ty * 4 + a) * HD + tx * 4) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
  if (tx == 0) *(float4*)(out + HD * HD + ty * 4) = make_float4(asum[0], asum[1], asum[2], asum[3]);
  if (ty == 0) *(float4*)(out + HD * HD + HD + tx * 4) = make_float4(bsum[0], bsum[1], bsum[2], bsum[3]);
}

// Second stage: the partial states of one (batch, head) summed in chunk order.  grid: (ceil(STATE / WG), bh).
__global__ __launch_bounds__(WG) void cos2_sum_kernel(const float* __restrict__ part, int nchunks, float* __restrict__ fin) {
  const int e = blockIdx.x * WG + threadIdx.x;
  if (e >= STATE) return;
  const float* p = part + (int64_t)blockIdx.y * nchunks * STATE + e;
  float s = 0.f;
  for (int c = 0; c < nchunks; c++) s += p[(int64_t)c * STATE];
  float* f = fin + (int64_t)blockIdx.y * FSTATE;
  if (e < HD * HD) {
    f[e] = s;
    f[HD * HD + (e & (HD - 1)) * HD + (e >> 6)] = s;      // M^T
  } else {
    f[HD * HD + e] = s;
  }
}

// Row pass.  WHICH 0: o = (q KV + vsum) / den, den = q . ksum + S (written).  1: dq = dn KV^T + dd ksum.  2: dk = v dKV^T + dksum.  3: dv = k dKV + dvsum.
// fs = the final state {KV, ksum, vsum} of this (batch, head), fd = {dKV, dksum, dvsum}.  Thread (tok, cg) = (tid / 4, tid % 4) forms 16 outputs of one row.
template <typename TQ, typename TO, typename TG, int WHICH>
__device__ __forceinline__ void cos2_rows_body(int bh, int tile, const TQ* __restrict__ Q, const TQ* __restrict__ K, const TQ* __restrict__ V,
                                               const TO* Ox, const TO* Oc, const TO* dOx, const TO* dOc, float* den, const float* __restrict__ fs,
                                               const float* __restrict__ fd, int heads, int S, int n_img, TO* Oxw, TO* Ocw, TG* __restrict__ dout,
                                               float (&Ms)[HD][HD], float (&xs)[RT][HD + 1], float (&vec)[2][HD], float (&wt)[RT]) {
  const int tid = threadIdx.x, b = bh / heads, h = bh - b * heads;
  // the matrix with the input channel as its row: KV, KV^T (stored at + HD*HD), dKV^T, dKV
  const float* M = WHICH == 0 ? fs : WHICH == 1 ? fs + HD * HD : WHICH == 2 ? fd + HD * HD : fd;
  for (int idx = tid * 4; idx < HD * HD; idx += WG * 4) *(float4*)(&Ms[0][0] + idx) = *(const float4*)(M + idx);
  if (tid < HD) {
    const float* tail = (WHICH < 2 ? fs : fd) + 2 * HD * HD;      // sum w A | sum B
    vec[0][tid] = WHICH == 0 ? tail[HD + tid] : WHICH == 1 ? 0.f : WHICH == 2 ? tail[tid] : tail[HD + tid];      // vsum | 0 | dksum | dvsum
    vec[1][tid] = tail[tid];                                                                                  // ksum (WHICH 0: den; WHICH 1: dd ksum)
  }
#pragma unroll
  for (int it = 0; it < RT * 8 / WG; it++) {
    const int jj = it * (WG / 8) + (tid >> 3), piece = tid & 7, i = tile * RT + jj;
    const bool valid = i < S;
    float x[8], w = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) x[e] = 0.f;
    if constexpr (WHICH == 1) {
      float ov[8];
#pragma unroll
      for (int e = 0; e < 8; e++) ov[e] = 0.f;
      const TO* gr = valid ? o_row(dOx, dOc, b, h, heads, i, S, n_img) : nullptr;
      if (gr) {
        ld8(gr + piece * 8, x);
        ld8(o_row(Ox, Oc, b, h, heads, i, S, n_img) + piece * 8, ov);
      }
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) dot += x[e] * ov[e];
      dot = group_sum<8>(dot);
      const float d = valid ? den[(int64_t)bh * S + i] : 1.f;
      w = -dot / d;
#pragma unroll
      for (int e = 0; e < 8; e++) x[e] = x[e] / d;
    } else {
      const TQ* src = WHICH == 0 ? Q : WHICH == 2 ? V : K;
      if (valid) ld8(src + ((int64_t)bh * S + i) * HD + piece * 8, x);
    }
#pragma unroll
    for (int e = 0; e < 8; e++) xs[jj][piece * 8 + e] = x[e];
    if (piece == 0) wt[jj] = w;
  }
  __syncthreads();
  const int tok = tid >> 2, cg = tid & 3, i = tile * RT + tok;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; c++) acc[c] = 0.f;
  float dotk = 0.f;
#pragma unroll 4
  for (int d = 0; d < HD; d++) {
    const float xd = xs[tok][d];
    if constexpr (WHICH == 0) dotk = __builtin_fmaf(xd, vec[1][d], dotk);
#pragma unroll
    for (int c4 = 0; c4 < 4; c4++) {
      const float4 m = *(const float4*)&Ms[d][cg * 16 + c4 * 4];
      acc[c4 * 4 + 0] = __builtin_fmaf(xd, m.x, acc[c4 * 4 + 0]);
      acc[c4 * 4 + 1] = __builtin_fmaf(xd, m.y, acc[c4 * 4 + 1]);
      acc[c4 * 4 + 2] = __builtin_fmaf(xd, m.z, acc[c4 * 4 + 2]);
      acc[c4 * 4 + 3] = __builtin_fmaf(xd, m.w, acc[c4 * 4 + 3]);
    }
  }
  if (i >= S) return;
  float o[2][8];
  if constexpr (WHICH == 0) {
    const float dn = dotk + (float)S;
#pragma unroll
    for (int c = 0; c < 16; c++) o[c >> 3][c & 7] = (acc[c] + vec[0][cg * 16 + c]) / dn;
    if (cg == 0) den[(int64_t)bh * S + i] = dn;
    TO* orow = i < n_img ? Oxw + (((int64_t)b * n_img + i) * heads + h) * HD : Ocw + (((int64_t)b * (S - n_img) + (i - n_img)) * heads + h) * HD;
    st8(orow + cg * 16, o[0]);
    st8(orow + cg * 16 + 8, o[1]);
  } else {
    const float w = wt[tok];
#pragma unroll
    for (int c = 0; c < 16; c++) o[c >> 3][c & 7] = WHICH == 1 ? __builtin_fmaf(w, vec[1][cg * 16 + c], acc[c]) : acc[c] + vec[0][cg * 16 + c];
    TG* orow = dout + ((int64_t)bh * S + i) * HD + cg * 16;
    st8(orow, o[0]);
    st8(orow + 8, o[1]);
  }
}

// grid: x = bh * ntiles + tile.
template <typename TQ, typename TO>
__global__ __launch_bounds__(WG) void cos2_fwd_rows_kernel(const TQ* __restrict__ Q, const float* __restrict__ fin, int heads, int S, int n_img, int ntiles,
                                                           TO* __restrict__ Ox, TO* __restrict__ Oc, float* __restrict__ den) {
  __shared__ __attribute__((aligned(16))) float Ms[HD][HD];
  __shared__ float xs[RT][HD + 1];
  __shared__ float vec[2][HD];
  __shared__ float wt[RT];
  const int bh = blockIdx.x / ntiles, tile = blockIdx.x - bh * ntiles;
  cos2_rows_body<TQ, TO, float, 0>(bh, tile, Q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, den, fin + (int64_t)bh * FSTATE, nullptr,
                                   heads, S, n_img, Ox, Oc, nullptr, Ms, xs, vec, wt);
}

// grid: x = bh * ntiles + tile, y = 0 dq | 1 dk | 2 dv.  fin: the final states {KV ..} of every (batch, head), then the final states {dKV ..}.
template <typename TQ, typename TO, typename TG>
__global__ __launch_bounds__(WG) void cos2_bwd_rows_kernel(const TQ* __restrict__ Q, const TQ* __restrict__ K, const TQ* __restrict__ V,
                                                           const TO* __restrict__ Ox, const TO* __restrict__ Oc, const TO* __restrict__ dOx,
                                                           const TO* __restrict__ dOc, const float* __restrict__ den, const float* __restrict__ fin,
                                                           int nbh, int heads, int S, int n_img, int ntiles,
                                                           TG* __restrict__ dQ, TG* __restrict__ dK, TG* __restrict__ dV) {
  __shared__ __attribute__((aligned(16))) float Ms[HD][HD];
  __shared__ float xs[RT][HD + 1];
  __shared__ float vec[2][HD];
  __shared__ float wt[RT];
  const int bh = blockIdx.x / ntiles, tile = blockIdx.x - bh * ntiles;
  const float* fs = fin + (int64_t)bh * FSTATE;
  const float* fd = fin + ((int64_t)nbh + bh) * FSTATE;
  float* dn = const_cast<float*>(den);      // (read only in these instantiations)
  if (blockIdx.y == 0)
    cos2_rows_body<TQ, TO, TG, 1>(bh, tile, Q, K, V, Ox, Oc, dOx, dOc, dn, fs, fd, heads, S, n_img, nullptr, nullptr, dQ, Ms, xs, vec, wt);
  else if (blockIdx.y == 1)
    cos2_rows_body<TQ, TO, TG, 2>(bh, tile, Q, K, V, Ox, Oc, dOx, dOc, dn, fs, fd, heads, S, n_img, nullptr, nullptr, dK, Ms, xs, vec, wt);
  else
    cos2_rows_body<TQ, TO, TG, 3>(bh, tile, Q, K, V, Ox, Oc, dOx, dOc, dn, fs, fd, heads, S, n_img, nullptr, nullptr, dV, Ms, xs, vec, wt);
}

struct Cos2Dims { int nbh, nchunks, ntiles; };
// shapes shared by both launches; the workgroup index of a launch is an int
static inline int cos2_dims(int batch, int heads, int S, int n_img, Cos2Dims& d) {
  MMDIT_CHECK_ARG(batch > 0 && heads > 0);
  if (S <= 0 || n_img < 0 || n_img > S) return MMDIT_ERR_SHAPE;
  const int64_t nbh = (int64_t)batch * heads, nchunks = ((int64_t)S + CHUNK - 1) / CHUNK, ntiles = ((int64_t)S + RT - 1) / RT;
  if (2 * nbh > 65535 || nbh * ntiles > 0x7fffffff) return MMDIT_ERR_SHAPE;      // (2 * nbh: the y extent of the backward's summing grid)
  d = Cos2Dims{(int)nbh, (int)nchunks, (int)ntiles};
  return 0;
}
// workspace: [2 * nbh final states][2 * nbh * nchunks partial states]
static inline float* cos2_partials(void* ws, const Cos2Dims& d) { return (float*)ws + (int64_t)2 * d.nbh * FSTATE; }

}  // namespace

extern "C" long long mmdit_attn_cos2_ws_bytes(int batch, int heads, int S) {
  if (batch < 1 || heads < 1 || S < 1) return 0;
  const long long nbh = (long long)batch * heads, nchunks = ((long long)S + CHUNK - 1) / CHUNK;
  return 2 * nbh * (FSTATE + nchunks * STATE) * (long long)sizeof(float);
}

extern "C" int mmdit_attn_cos2_fwd(const void* Q, const void* K, const void* V, int qkv_dtype, int batch, int heads, int S, int n_img,
                                   void* Ox, void* Oc, int o_dtype, float* den, void* ws, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && den && ws);
  Cos2Dims d;
  if (int e = cos2_dims(batch, heads, S, n_img, d)) return e;
  MMDIT_CHECK_ARG((Ox || n_img == 0) && (Oc || n_img == S));
  if (!((qkv_dtype == MMDIT_BF16 && o_dtype == MMDIT_BF16) || (qkv_dtype == MMDIT_F32 && o_dtype == MMDIT_F32))) return MMDIT_ERR_DTYPE;
  hipStream_t s = (hipStream_t)stream;
  float* fin = (float*)ws;
  float* part = cos2_partials(ws, d);
  const dim3 block(WG), g1(d.nbh * d.nchunks), g2((STATE + WG - 1) / WG, d.nbh), g3(d.nbh * d.ntiles);
#define COS2(TQ, TO)                                                                                                                                   \
  hipLaunchKernelGGL((cos2_reduce_kernel<TQ, TO, 0>), g1, block, 0, s, (const TQ*)K, (const TQ*)V, (const TO*)nullptr, (const TO*)nullptr,         \
                     (const TO*)nullptr, (const TO*)nullptr, (const float*)nullptr, heads, S, n_img, d.nchunks, part);                              \
  hipLaunchKernelGGL(cos2_sum_kernel, g2, block, 0, s, (const float*)part, d.nchunks, fin);                                                           \
  hipLaunchKernelGGL((cos2_fwd_rows_kernel<TQ, TO>), g3, block, 0, s, (const TQ*)Q, (const float*)fin, heads, S, n_img, d.ntiles, (TO*)Ox, (TO*)Oc, den)
  if (qkv_dtype == MMDIT_BF16) { COS2(bf16_t, bf16_t); }
  else { COS2(float, float); }
#undef COS2
  return mmdit_launch_status();
}

extern "C" int mmdit_attn_cos2_bwd(const void* Q, const void* K, const void* V, int qkv_dtype, const void* Ox, const void* Oc,
                                   const void* dOx, const void* dOc, int o_dtype, const float* den, int batch, int heads, int S, int n_img,
                                   void* dQ, void* dK, void* dV, int dq_dtype, void* ws, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && den && ws && dQ && dK && dV);
  Cos2Dims d;
  if (int e = cos2_dims(batch, heads, S, n_img, d)) return e;
  MMDIT_CHECK_ARG(((Ox && dOx) || n_img == 0) && (Oc || n_img == S || !dOc));      // (dOc may be NULL = zeros: Oc is then not read)
  const int combo = (qkv_dtype == MMDIT_BF16 && o_dtype == MMDIT_BF16 && dq_dtype == MMDIT_BF16) ? 0
                  : (qkv_dtype == MMDIT_BF16 && o_dtype == MMDIT_BF16 && dq_dtype == MMDIT_F32)  ? 1
                  : (qkv_dtype == MMDIT_F32 && o_dtype == MMDIT_F32 && dq_dtype == MMDIT_F32)    ? 2 : -1;
  if (combo < 0) return MMDIT_ERR_DTYPE;
  hipStream_t s = (hipStream_t)stream;
  float* fin = (float*)ws;
  float* part = cos2_partials(ws, d);
  float* part_d = part + (int64_t)d.nbh * d.nchunks * STATE;
  const dim3 block(WG), g1(d.nbh * d.nchunks), g2((STATE + WG - 1) / WG, 2 * d.nbh), g3(d.nbh * d.ntiles, 3);
#define COS2(TQ, TO, TG)                                                                                                                               \
  hipLaunchKernelGGL((cos2_reduce_kernel<TQ, TO, 0>), g1, block, 0, s, (const TQ*)K, (const TQ*)V, (const TO*)nullptr, (const TO*)nullptr,         \
                     (const TO*)nullptr, (const TO*)nullptr, (const float*)nullptr, heads, S, n_img, d.nchunks, part);                              \
  hipLaunchKernelGGL((cos2_reduce_kernel<TQ, TO, 1>), g1, block, 0, s, (const TQ*)Q, (const TQ*)nullptr, (const TO*)Ox, (const TO*)Oc,             \
                     (const TO*)dOx, (const TO*)dOc, den, heads, S, n_img, d.nchunks, part_d);                                                      \
  hipLaunchKernelGGL(cos2_sum_kernel, g2, block, 0, s, (const float*)part, d.nchunks, fin);                                                           \
  hipLaunchKernelGGL((cos2_bwd_rows_kernel<TQ, TO, TG>), g3, block, 0, s, (const TQ*)Q, (const TQ*)K, (const TQ*)V, (const TO*)Ox, (const TO*)Oc,  \
                     (const TO*)dOx, (const TO*)dOc, den, (const float*)fin, d.nbh, heads, S, n_img, d.ntiles, (TG*)dQ, (TG*)dK, (TG*)dV)
  if (combo == 0) { COS2(bf16_t, bf16_t, bf16_t); }
  else if (combo == 1) { COS2(bf16_t, bf16_t, float); }
  else { COS2(float, float, float); }
#undef COS2
  return mmdit_launch_status();
}
