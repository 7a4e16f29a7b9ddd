// Joint [image;text] softmax attention for gfx950 with 32-wide queries / keys and 64-wide values (qk_half_dim: mmdit_attn_fwd_qkhalf /
// mmdit_attn_bwd_qkhalf, include/mmdit_hip_qkhalf.h; reference call sites Attention.py:33-67, 266-293 and its autograd).  bf16 MFMA operands,
// fp32 accumulate.
//
// Orientation and rounding points are those of attention.hip and attention_hd128.hip: S^T = K Q^T and O^T = V^T P^T with
// v_mfma_f32_32x32x16_bf16, so a query's softmax statistics live in one lane pair (l, l + 32) and the score accumulators are already the
// B operand of the second product.
//   forward mode 0: raw fp32 scores, online softmax in the log2 domain (v_exp_f32), unnormalised P rounded to bf16 for P V, O rounded to bf16
//   forward mode 1: the reference's CPU branch (Attention.py:277-284): bf16(bf16(q k) * scale), softmax in fp32 over two passes, P rounded
//                   to bf16, O rounded to bf16
//   backward:       P = exp2(s * scale * log2e - lse * log2e) and dS = P (dP - delta) rounded to bf16 for their MFMAs, delta = rowsum(dO * O)
//                   from the ROUNDED O (written by the dQ kernel, read by the dK/dV kernel)
//
// Plain kernels built as attention_hd128.hip is, not tuned: 4 waves = 128 queries (keys, in the dK/dV kernel) per workgroup,
// 32-row tiles of the streamed operands, register-staged double buffer (global -> VGPR -> LDS, one barrier per tile), padded row pitch, no
// LDS-DMA ring, no fused epilogue.  The score product has two K-steps (32 / 16), the dP product four (64 / 16); the P V / dV side has two
// 32-column blocks, dQ / dK one.  A streamed tile is exactly one 32-row MFMA block, so a fully padded 32-key block never exists: the last
// tile is the only ragged one.
#include "common.h"
#include "../../include/mmdit_hip_qkhalf.h"

namespace {

constexpr int DQK = MMDIT_QKHALF_QK_DIM;            // width of a query / key head
constexpr int DV = MMDIT_QKHALF_V_DIM;              // width of a value head
constexpr int KT = MMDIT_ATTN_QKHALF_KEY_TILE;      // rows of a streamed LDS tile
constexpr int NW = 4;                               // waves per workgroup
constexpr int QT = MMDIT_ATTN_QKHALF_QUERY_TILE;    // stationary rows per workgroup
constexpr int NT = NW * 64;
constexpr int PITCH_QK = 2 * DQK + 16;              // tile row pitch in bytes: 16-byte aligned rows for ds_read_b128, off the bank period
constexpr int PITCH_V = 2 * DV + 16;
constexpr int TILE_QK = KT * PITCH_QK, TILE_V = KT * PITCH_V;
constexpr int KS_QK = DQK / 16, KS_V = DV / 16;     // MFMA K-steps over a query / key row and over a value row
constexpr int DB_V = DV / 32;                       // 32-column blocks of the value width (the query / key width is one block)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
static_assert(DQK == 32 && DV == 64 && KT == 32 && QT == 32 * NW && NT == 256, "thread -> tile element maps below");

__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// B-operand fragment from 8 consecutive accumulator registers (fp32 -> bf16), regs [h8 * 8, h8 * 8 + 8)
__device__ __forceinline__ bf16x8 pack_frag(const f32x16& p, int h8) {
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] = pack_bf2(p[h8 * 8 + 2 * i], p[h8 * 8 + 2 * i + 1]);
  return __builtin_bit_cast(bf16x8, w);
}
// A-operand fragment of X^T, X a row-major [32][width] LDS tile of row pitch PITCH: lane owns column cb * 32 + (lane & 31); its 8 k-slots are
// the tile rows 16 h8 + 4 (lane >> 5) + {0..3} and + 8 + {0..3} -- the row order pack_frag produces from an accumulator whose rows are the
// tile rows
template <int PITCH>
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int h8, int cb, int lane) {
  const int row = 16 * h8 + 4 * (lane >> 5) + ((lane & 15) >> 2);
  const int col = cb * 32 + 16 * ((lane >> 4) & 1) + (lane & 3) * 4;
  const char* p = tile + row * PITCH + col * 2;
  const s16x4 lo = lds_tr16(p), hi = lds_tr16(p + 8 * PITCH);
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}
// A-operand fragment of the tile itself: lane owns row lane & 31, k = ks * 16 + (lane >> 5) * 8 .. + 7
template <int PITCH>
__device__ __forceinline__ bf16x8 row_frag(const char* tile, int ks, int lane) {
  return *LDS_PTR(const bf16x8, tile + (lane & 31) * PITCH + (ks * 16 + (lane >> 5) * 8) * 2);
}

// One 16-byte chunk per thread.  A [32][32] bf16 tile is 128 chunks (threads 0..127: row tid >> 2, piece tid & 3), a [32][64] tile 256
// (row tid >> 3, piece tid & 7).  Rows past the end are zero: no load leaves the operand.
__device__ __forceinline__ u32x4 g2r_qk(const bf16_t* g, int row0, int nrows, int tid) {
  const int row = row0 + (tid >> 2);
  return tid < 128 && row < nrows ? *(const u32x4*)(g + (int64_t)row * DQK + (tid & 3) * 8) : (u32x4){0, 0, 0, 0};
}
__device__ __forceinline__ void r2s_qk(const u32x4& c, char* tile, int tid) {
  if (tid < 128) *LDS_PTR(u32x4, tile + (tid >> 2) * PITCH_QK + (tid & 3) * 16) = c;
}
__device__ __forceinline__ u32x4 g2r_v(const bf16_t* g, int row0, int nrows, int tid) {
  const int row = row0 + (tid >> 3);
  return row < nrows ? *(const u32x4*)(g + (int64_t)row * DV + (tid & 7) * 8) : (u32x4){0, 0, 0, 0};
}
__device__ __forceinline__ void r2s_v(const u32x4& c, char* tile, int tid) {
  *LDS_PTR(u32x4, tile + (tid >> 3) * PITCH_V + (tid & 7) * 16) = c;
}

// the 64-wide head slice of token s (joint index) in the stream-split (batch, tokens, heads * 64) tensors; NULL for a missing text tensor
__device__ __forceinline__ const bf16_t* tok_ptr(const bf16_t* x_img, const bf16_t* x_txt, int64_t b, int s, int n_img, int n_txt, int D, int h) {
  if (s < n_img) return x_img + ((b * n_img + s) * (int64_t)D + h * DV);
  return x_txt ? x_txt + ((b * n_txt + (s - n_img)) * (int64_t)D + h * DV) : nullptr;
}

// 1-D grid -> (tile, batch * head): all tiles of one (batch, head) on one XCD (see map_block of attention.hip; locality only)
__device__ __forceinline__ void map_block(int ntile, int BH, int& tile, int& bh) {
  const int id = blockIdx.x;
  if (BH % 8 == 0) {
    const int xcd = id & 7, j = id >> 3;
    tile = j % ntile;
    bh = (j / ntile) * 8 + xcd;
  } else {
    tile = id % ntile;
    bh = id / ntile;
  }
}

__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; r++) a[r] = 0.f;
}

// ------------------------------------------------------------------------------------------------
// forward.  ORACLE = mode 1.
// ------------------------------------------------------------------------------------------------
template <bool ORACLE>
__global__ __launch_bounds__(NT) void attn_fwd_qkhalf_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                             int BH, int H, int S, int n_img, float scale,
                                                             bf16_t* __restrict__ Ox, bf16_t* __restrict__ Oc, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE_QK + 2 * TILE_V];
  auto kt = [&](int i) { return smem + i * TILE_QK; };
  auto vt = [&](int i) { return smem + 2 * TILE_QK + i * TILE_V; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int qtile, bh;
  map_block((S + QT - 1) / QT, BH, qtile, bh);
  const int h = bh % H;
  const int64_t b = bh / H;
  const bf16_t* Qb = Q + (int64_t)bh * S * DQK;
  const bf16_t* Kb = K + (int64_t)bh * S * DQK;
  const bf16_t* Vb = V + (int64_t)bh * S * DV;
  const int q = qtile * QT + wave * 32 + (lane & 31);
  const int qc = min(q, S - 1);                        // ragged query tile: clamped loads, guarded stores
  const bool active = qtile * QT + wave * 32 < S;      // wave-uniform: a wave whose 32 queries are all padding only helps with the tile copies

  bf16x8 qf[KS_QK];
#pragma unroll
  for (int ks = 0; ks < KS_QK; ks++) qf[ks] = *(const bf16x8*)(Qb + (int64_t)qc * DQK + ks * 16 + (lane >> 5) * 8);

  f32x16 o[DB_V];
#pragma unroll
  for (int db = 0; db < DB_V; db++) zero16(o[db]);
  float m = -INFINITY, l = 0.f;
  const int nkv = (S + KT - 1) / KT;
  u32x4 sk, sv;

  // scores of tile j (masked keys = -inf).  fast: raw; oracle: natural domain, bf16-rounded twice
  auto scores = [&](int j, const char* ktile, f32x16& s) {
    zero16(s);
#pragma unroll
    for (int ks = 0; ks < KS_QK; ks++) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<PITCH_QK>(ktile, ks, lane), qf[ks], s, 0, 0, 0);
    if (ORACLE) {
#pragma unroll
      for (int r = 0; r < 16; r++) s[r] = bf2f(f2bf(bf2f(f2bf(s[r])) * scale));   // Attention.py:277: bf16 matmul, then bf16 * scale
    }
    if ((j + 1) * KT > S) {   // only the last (ragged) tile has keys to mask: wave-uniform branch
#pragma unroll
      for (int r = 0; r < 16; r++)
        if (j * KT + acc_row(r, lane) >= S) s[r] = -INFINITY;
    }
  };
  auto tile_max = [&](const f32x16& s) {
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[r]);
    return fmaxf(mx, __shfl_xor(mx, 32, 64));
  };
  auto pv = [&](const f32x16& p, const char* vtile) {
#pragma unroll
    for (int h8 = 0; h8 < 2; h8++) {
      const bf16x8 pf = pack_frag(p, h8);
#pragma unroll
      for (int db = 0; db < DB_V; db++) o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<PITCH_V>(vtile, h8, db, lane), pf, o[db], 0, 0, 0);
    }
  };

  for (int pass = 0; pass < (ORACLE ? 2 : 1); pass++) {
    sk = g2r_qk(Kb, 0, S, tid);
    sv = g2r_v(Vb, 0, S, tid);
    __syncthreads();   // previous pass done with the buffers
    r2s_qk(sk, kt(0), tid);
    r2s_v(sv, vt(0), tid);
    __syncthreads();
    for (int j = 0; j < nkv; j++) {
      const int cur = j & 1;
      if (j + 1 < nkv) {
        sk = g2r_qk(Kb, (j + 1) * KT, S, tid);
        sv = g2r_v(Vb, (j + 1) * KT, S, tid);
      }
      if (active) {
        f32x16 s;
        scores(j, kt(cur), s);
        if (!ORACLE) {
          // raw scores; m is tracked in the scaled log2 domain: p = exp2(s * c - m) as one fma + v_exp_f32
          const float c = scale * LOG2E;
          const float mn = fmaxf(m, tile_max(s) * c);
          const float alpha = fast_exp2(m - mn);
          float rs = 0.f;
#pragma unroll
          for (int r = 0; r < 16; r++) { const float p = fast_exp2(fmaf(s[r], c, -mn)); s[r] = p; rs += p; }
          rs += __shfl_xor(rs, 32, 64);
          l = l * alpha + rs; m = mn;
#pragma unroll
          for (int db = 0; db < DB_V; db++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[db][r] *= alpha;
          pv(s, vt(cur));
        } else if (pass == 0) {
          const float mn = fmaxf(m, tile_max(s));
          float rs = 0.f;
#pragma unroll
          for (int r = 0; r < 16; r++) rs += expf(s[r] - mn);
          rs += __shfl_xor(rs, 32, 64);
          l = l * expf(m - mn) + rs; m = mn;
        } else {
#pragma unroll
          for (int r = 0; r < 16; r++) s[r] = expf(s[r] - m) / l;   // softmax output, rounded to bf16 by pack_frag
          pv(s, vt(cur));
        }
      }
      if (j + 1 < nkv) {
        r2s_qk(sk, kt(cur ^ 1), tid);
        r2s_v(sv, vt(cur ^ 1), tid);
        __syncthreads();
      }
    }
  }

  if (q < S) {
    const float inv = ORACLE ? 1.f : 1.f / l;
    const int n_txt = S - n_img, D = H * DV;
    bf16_t* dst = q < n_img ? Ox + ((b * n_img + q) * (int64_t)D + h * DV) : Oc + ((b * n_txt + (q - n_img)) * (int64_t)D + h * DV);
#pragma unroll
    for (int db = 0; db < DB_V; db++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float v4[4] = {o[db][g * 4] * inv, o[db][g * 4 + 1] * inv, o[db][g * 4 + 2] * inv, o[db][g * 4 + 3] * inv};
        st4(dst + db * 32 + 8 * g + 4 * (lane >> 5), v4);
      }
    if (lane < 32) lse[(int64_t)bh * S + q] = ORACLE ? m + logf(l) : m * LN2 + logf(l);
  }
}

// ------------------------------------------------------------------------------------------------
// backward dQ: query-stationary, loops over K / V tiles.  dQ^T[d][q] += K^T[d][key] dS^T[key][q], d < 32.  Writes delta[q] =
// sum_d dO[q,d] O[q,d] from the query's own rows (each lane holds half of the 64 features of its query) for the dK/dV kernel that follows on
// the same stream.
// ------------------------------------------------------------------------------------------------
template <typename TG>
__global__ __launch_bounds__(NT) void attn_bwd_dq_qkhalf_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                                const bf16_t* __restrict__ Ox, const bf16_t* __restrict__ Oc,
                                                                const bf16_t* __restrict__ dOx, const bf16_t* __restrict__ dOc,
                                                                const float* __restrict__ lse, float* __restrict__ delta,
                                                                int BH, int H, int S, int n_img, float scale, TG* __restrict__ dQ) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE_QK + 2 * TILE_V];
  auto kt = [&](int i) { return smem + i * TILE_QK; };
  auto vt = [&](int i) { return smem + 2 * TILE_QK + i * TILE_V; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int qtile, bh;
  map_block((S + QT - 1) / QT, BH, qtile, bh);
  const int h = bh % H;
  const int64_t b = bh / H;
  const bf16_t* Qb = Q + (int64_t)bh * S * DQK;
  const bf16_t* Kb = K + (int64_t)bh * S * DQK;
  const bf16_t* Vb = V + (int64_t)bh * S * DV;
  const int q = qtile * QT + wave * 32 + (lane & 31);
  const int qc = min(q, S - 1);
  const bool active = qtile * QT + wave * 32 < S;
  const bf16_t* dop = tok_ptr(dOx, dOc, b, qc, n_img, S - n_img, H * DV, h);

  bf16x8 qf[KS_QK], dof[KS_V];
#pragma unroll
  for (int ks = 0; ks < KS_QK; ks++) qf[ks] = *(const bf16x8*)(Qb + (int64_t)qc * DQK + ks * 16 + (lane >> 5) * 8);
#pragma unroll
  for (int ks = 0; ks < KS_V; ks++) {
    const u32x4 z = {0, 0, 0, 0};
    dof[ks] = dop ? *(const bf16x8*)(dop + ks * 16 + (lane >> 5) * 8) : __builtin_bit_cast(bf16x8, z);
  }
  float dq_delta = 0.f;
  {
    const bf16_t* op = tok_ptr(Ox, Oc, b, qc, n_img, S - n_img, H * DV, h);
    if (dop && op) {
#pragma unroll
      for (int ks = 0; ks < KS_V; ks++) {
        const u32x4 o4 = *(const u32x4*)(op + ks * 16 + (lane >> 5) * 8), d4 = __builtin_bit_cast(u32x4, dof[ks]);
#pragma unroll
        for (int e = 0; e < 4; e++)
          dq_delta += __builtin_bit_cast(float, o4[e] << 16) * __builtin_bit_cast(float, d4[e] << 16) +
                      __builtin_bit_cast(float, o4[e] & 0xffff0000u) * __builtin_bit_cast(float, d4[e] & 0xffff0000u);
      }
    }
    dq_delta += __shfl_xor(dq_delta, 32, 64);
    if (lane < 32 && q < S) delta[(int64_t)bh * S + q] = dq_delta;
  }
  const float lq = lse[(int64_t)bh * S + qc] * LOG2E;
  f32x16 acc;
  zero16(acc);

  const int nkv = (S + KT - 1) / KT;
  u32x4 sk = g2r_qk(Kb, 0, S, tid), sv = g2r_v(Vb, 0, S, tid);
  r2s_qk(sk, kt(0), tid);
  r2s_v(sv, vt(0), tid);
  __syncthreads();
  for (int j = 0; j < nkv; j++) {
    const int cur = j & 1;
    if (j + 1 < nkv) {
      sk = g2r_qk(Kb, (j + 1) * KT, S, tid);
      sv = g2r_v(Vb, (j + 1) * KT, S, tid);
    }
    if (active) {
      const char* ktile = kt(cur);
      const char* vtile = vt(cur);
      f32x16 s, dp;
      zero16(s);
      zero16(dp);
#pragma unroll
      for (int ks = 0; ks < KS_QK; ks++) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<PITCH_QK>(ktile, ks, lane), qf[ks], s, 0, 0, 0);
#pragma unroll
      for (int ks = 0; ks < KS_V; ks++) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<PITCH_V>(vtile, ks, lane), dof[ks], dp, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float p = fast_exp2(fmaf(s[r], scale * LOG2E, -lq));
        s[r] = p * (dp[r] - dq_delta);
      }
      if ((j + 1) * KT > S) {   // padding keys exist in the last tile only: a wave-uniform branch
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (j * KT + acc_row(r, lane) >= S) s[r] = 0.f;
      }
#pragma unroll
      for (int h8 = 0; h8 < 2; h8++) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<PITCH_QK>(ktile, h8, 0, lane), pack_frag(s, h8), acc, 0, 0, 0);
    }
    if (j + 1 < nkv) {
      r2s_qk(sk, kt(cur ^ 1), tid);
      r2s_v(sv, vt(cur ^ 1), tid);
      __syncthreads();
    }
  }
  if (q < S) {
    TG* dst = dQ + ((int64_t)bh * S + q) * DQK;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float v4[4] = {acc[g * 4] * scale, acc[g * 4 + 1] * scale, acc[g * 4 + 2] * scale, acc[g * 4 + 3] * scale};
      st4(dst + 8 * g + 4 * (lane >> 5), v4);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward dK/dV: key-stationary (each wave owns 32 keys), loops over Q / dO tiles of 32 queries.
//   S[q][key] = Q K^T, dP[q][key] = dO V^T  (lane owns key l & 31, rows = queries)
//   dV^T[d][key] += dO^T[d][q] P[q][key] (d < 64),  dK^T[d][key] += Q^T[d][q] dS[q][key] (d < 32)
// ------------------------------------------------------------------------------------------------
template <typename TG>
__global__ __launch_bounds__(NT) void attn_bwd_dkv_qkhalf_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                                 const bf16_t* __restrict__ dOx, const bf16_t* __restrict__ dOc,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 int BH, int H, int S, int n_img, float scale, TG* __restrict__ dK, TG* __restrict__ dV) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE_QK + 2 * TILE_V];
  __shared__ __attribute__((aligned(16))) float stat[2][2][KT];      // [buffer][lse * log2e | delta][query of the tile]
  auto qt = [&](int i) { return smem + i * TILE_QK; };
  auto dot = [&](int i) { return smem + 2 * TILE_QK + i * TILE_V; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int ktile, bh;
  map_block((S + QT - 1) / QT, BH, ktile, bh);
  const int h = bh % H;
  const int64_t b = bh / H;
  const bf16_t* Qb = Q + (int64_t)bh * S * DQK;
  const bf16_t* Kb = K + (int64_t)bh * S * DQK;
  const bf16_t* Vb = V + (int64_t)bh * S * DV;
  const int key = ktile * QT + wave * 32 + (lane & 31);
  const bool active = ktile * QT + wave * 32 < S;      // wave-uniform: a wave whose 32 keys are all padding only helps with the tile copies
  const int keyc = min(key, S - 1);                    // a padding key works on the clamped last key; its dK / dV column is never stored
  const int n_txt = S - n_img, D = H * DV;

  bf16x8 kf[KS_QK], vf[KS_V];
#pragma unroll
  for (int ks = 0; ks < KS_QK; ks++) kf[ks] = *(const bf16x8*)(Kb + (int64_t)keyc * DQK + ks * 16 + (lane >> 5) * 8);
#pragma unroll
  for (int ks = 0; ks < KS_V; ks++) vf[ks] = *(const bf16x8*)(Vb + (int64_t)keyc * DV + ks * 16 + (lane >> 5) * 8);
  f32x16 dk, dv[DB_V];
  zero16(dk);
#pragma unroll
  for (int db = 0; db < DB_V; db++) zero16(dv[db]);

  const int nq = (S + KT - 1) / KT;
  u32x4 sq, sd;
  float lv = 0.f, dl = 0.f;
  auto request = [&](int jq) {
    sq = g2r_qk(Qb, jq * KT, S, tid);
    {
      const int s = jq * KT + (tid >> 3);
      const bf16_t* p = s < S ? tok_ptr(dOx, dOc, b, s, n_img, n_txt, D, h) : nullptr;
      sd = p ? *(const u32x4*)(p + (tid & 7) * 8) : (u32x4){0, 0, 0, 0};
    }
    lv = 0.f, dl = 0.f;
    if (tid < KT && jq * KT + tid < S) { lv = lse[(int64_t)bh * S + jq * KT + tid]; dl = delta[(int64_t)bh * S + jq * KT + tid]; }
  };
  auto park = [&](int buf) {
    r2s_qk(sq, qt(buf), tid);
    r2s_v(sd, dot(buf), tid);
    if (tid < KT) { stat[buf][0][tid] = lv * LOG2E; stat[buf][1][tid] = dl; }
  };
  request(0);
  park(0);
  __syncthreads();
  for (int jq = 0; jq < nq; jq++) {
    const int cur = jq & 1;
    if (jq + 1 < nq) request(jq + 1);
    if (active) {
      const char* qtile = qt(cur);
      const char* dotile = dot(cur);
      f32x16 s, dp;
      zero16(s);
      zero16(dp);
#pragma unroll
      for (int ks = 0; ks < KS_QK; ks++) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<PITCH_QK>(qtile, ks, lane), kf[ks], s, 0, 0, 0);
#pragma unroll
      for (int ks = 0; ks < KS_V; ks++) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<PITCH_V>(dotile, ks, lane), vf[ks], dp, 0, 0, 0);
      f32x16 ds;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int r0 = 8 * g + 4 * (lane >> 5);
        const f32x4 l4 = *LDS_PTR(const f32x4, &stat[cur][0][r0]);
        const f32x4 d4 = *LDS_PTR(const f32x4, &stat[cur][1][r0]);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int r = g * 4 + e;
          const float p = fast_exp2(fmaf(s[r], scale * LOG2E, -l4[e]));
          s[r] = p;
          ds[r] = p * (dp[r] - d4[e]);
        }
      }
      // padding QUERIES exist in the last Q / dO tile only (their rows are zero-filled, lse = delta = 0): masked so that P and dS are zero there
      if ((jq + 1) * KT > S) {
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (jq * KT + acc_row(r, lane) >= S) { s[r] = 0.f; ds[r] = 0.f; }
      }
#pragma unroll
      for (int h8 = 0; h8 < 2; h8++) {
        const bf16x8 pf = pack_frag(s, h8), dsf = pack_frag(ds, h8);
#pragma unroll
        for (int db = 0; db < DB_V; db++) dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<PITCH_V>(dotile, h8, db, lane), pf, dv[db], 0, 0, 0);
        dk = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<PITCH_QK>(qtile, h8, 0, lane), dsf, dk, 0, 0, 0);
      }
    }
    if (jq + 1 < nq) {
      park(cur ^ 1);
      __syncthreads();
    }
  }
  if (key < S) {
    TG* pk = dK + ((int64_t)bh * S + key) * DQK;
    TG* pv = dV + ((int64_t)bh * S + key) * DV;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float k4[4] = {dk[g * 4] * scale, dk[g * 4 + 1] * scale, dk[g * 4 + 2] * scale, dk[g * 4 + 3] * scale};
      st4(pk + 8 * g + 4 * (lane >> 5), k4);
    }
#pragma unroll
    for (int db = 0; db < DB_V; db++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float v4[4] = {dv[db][g * 4], dv[db][g * 4 + 1], dv[db][g * 4 + 2], dv[db][g * 4 + 3]};
        st4(pv + db * 32 + 8 * g + 4 * (lane >> 5), v4);
      }
  }
}

// number of workgroups of a launch, or 0 when it does not fit the 1-D grid
static inline int64_t grid_of(int batch, int heads, int S) {
  const int64_t blocks = (int64_t)((S + QT - 1) / QT) * batch * heads;
  return blocks > 0x7fffffff || (int64_t)batch * heads > 0x7fffffff ? 0 : blocks;
}

}  // namespace

extern "C" int mmdit_attn_fwd_qkhalf(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale, int mode,
                                     void* Ox, void* Oc, float* lse, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && Ox && lse && batch > 0 && heads > 0 && (mode == 0 || mode == 1));
  if (S < 1 || n_img < 1 || n_img > S) return MMDIT_ERR_SHAPE;
  MMDIT_CHECK_ARG(Oc || n_img == S);
  const int64_t blocks = grid_of(batch, heads, S);
  if (!blocks) return MMDIT_ERR_SHAPE;
#define MMDIT_FWDQH(ORACLE) hipLaunchKernelGGL((attn_fwd_qkhalf_kernel<ORACLE>), dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)Q, (const bf16_t*)K, \
                                               (const bf16_t*)V, batch * heads, heads, S, n_img, scale, (bf16_t*)Ox, (bf16_t*)Oc, lse)
  if (mode == 1) MMDIT_FWDQH(true);
  else MMDIT_FWDQH(false);
#undef MMDIT_FWDQH
  return mmdit_launch_status();
}

extern "C" int mmdit_attn_bwd_qkhalf(const void* Q, const void* K, const void* V, const void* Ox, const void* Oc, const void* dOx, const void* dOc,
                                     const float* lse, float* delta, int batch, int heads, int S, int n_img, float scale,
                                     void* dQ, void* dK, void* dV, int dq_dtype, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && Ox && dOx && lse && delta && dQ && dK && dV && batch > 0 && heads > 0);
  if (S < 1 || n_img < 1 || n_img > S) return MMDIT_ERR_SHAPE;
  MMDIT_CHECK_ARG(Oc || n_img == S);
  if (dq_dtype != MMDIT_BF16 && dq_dtype != MMDIT_F32) return MMDIT_ERR_DTYPE;
  const int64_t blocks = grid_of(batch, heads, S);
  if (!blocks) return MMDIT_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  // (delta = rowsum(dO * O) is produced by the dQ kernel, which runs first)
#define MMDIT_BWDQH(TG)                                                                                                                                             \
  do {                                                                                                                                                              \
    hipLaunchKernelGGL((attn_bwd_dq_qkhalf_kernel<TG>), dim3((unsigned)blocks), dim3(NT), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V,              \
                       (const bf16_t*)Ox, (const bf16_t*)Oc, (const bf16_t*)dOx, (const bf16_t*)dOc, lse, delta, batch * heads, heads, S, n_img, scale, (TG*)dQ);  \
    hipLaunchKernelGGL((attn_bwd_dkv_qkhalf_kernel<TG>), dim3((unsigned)blocks), dim3(NT), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V,             \
                       (const bf16_t*)dOx, (const bf16_t*)dOc, lse, delta, batch * heads, heads, S, n_img, scale, (TG*)dK, (TG*)dV);                                \
  } while (0)
  if (dq_dtype == MMDIT_BF16) MMDIT_BWDQH(bf16_t);
  else MMDIT_BWDQH(float);
#undef MMDIT_BWDQH
  return mmdit_launch_status();
}
