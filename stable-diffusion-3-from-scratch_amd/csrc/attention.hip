// Joint [image;text] softmax attention for gfx950, head_dim 64, bf16 MFMA operands, fp32 accumulate.
//
// All matmuls are issued "transposed" so that the softmax row statistic of a query lives in ONE lane:
//   S^T = K Q^T  (v_mfma_f32_32x32x16_bf16: lane owns query l&31, 16 keys per accumulator)
//   O^T = V^T P^T: the accumulator registers of S^T are already the B operand of this MFMA (the
//   key order inside a 16-key slab is a fixed permutation which the V^T operand reproduces by
//   addressing), V^T fragments come from a row-major [key][d] LDS tile via ds_read_b64_tr_b16.
// Forward: one wave = 32 queries, KV tiles of 64 keys double-buffered through LDS.
// Backward: two kernels (dQ: query-stationary; dK/dV: key-stationary) so nothing is atomically reduced.
#include <type_traits>
#include "common.h"
#include "../../include/mmdit_hip_mxpad.h"

namespace {

constexpr int HD = 64;
constexpr int KT = 64;          // keys (or queries) per LDS tile
constexpr int P144 = 144;       // row pitch for ds_read_b128 fragments (conflict-free)
constexpr int P192 = 192;       // row pitch for ds_read_b64_tr_b16 fragments (conflict-free)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// B-operand fragment from 8 consecutive accumulator registers (fp32 -> bf16), regs [h8*8, h8*8+8)
__device__ __forceinline__ bf16x8 pack_frag(const f32x16& p, int h8) {
  u32x4 w;
#pragma unroll
  for (int i = 0; i < 4; i++) w[i] = pack_bf2(p[h8 * 8 + 2 * i], p[h8 * 8 + 2 * i + 1]);
  return __builtin_bit_cast(bf16x8, w);
}

// A-operand fragment of X^T where X is a row-major [row][64] LDS tile (pitch bytes): lane owns column
// cb*32 + (lane&31); its 8 k-slots are rows  rb + 16*h8 + 4*(lane>>5) + {0..3}  and  + 8 + {0..3}
// (the row order produced by pack_frag on an accumulator whose rows are these tile rows).
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int pitch, int rb, int h8, int cb, int lane) {
  const int row = rb + 16 * h8 + 4 * (lane >> 5) + ((lane & 15) >> 2);
  const int col = cb * 32 + 16 * ((lane >> 4) & 1) + (lane & 3) * 4;
  const char* p = tile + row * pitch + col * 2;
  s16x4 lo = lds_tr16(p), hi = lds_tr16(p + 8 * pitch);
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// A-operand fragment of a row-major [row][64] LDS tile: lane owns row rb + (lane&31), k = ks*16 + (lane>>5)*8 ..+7
__device__ __forceinline__ bf16x8 row_frag(const char* tile, int pitch, int rb, int ks, int lane) {
  return *LDS_PTR(const bf16x8, tile + (rb + (lane & 31)) * pitch + (ks * 16 + (lane >> 5) * 8) * 2);
}

// copy a [64 rows][64] bf16 tile global -> LDS (512 16-byte chunks), rows >= nvalid zero-filled.  NT threads (any multiple of 64).
template <int NT> constexpr int tile_chunks() { return (512 + NT - 1) / NT; }
template <int NT>
__device__ __forceinline__ void tile_g2r(u32x4 (&st)[tile_chunks<NT>()], const bf16_t* g, int row0, int nrows_total, int tid) {
#pragma unroll
  for (int i = 0; i < tile_chunks<NT>(); i++) {
    const int c = tid + i * NT, row = c >> 3, kc = c & 7;
    st[i] = (c < 512 && row0 + row < nrows_total) ? *(const u32x4*)(g + (int64_t)(row0 + row) * HD + kc * 8) : (u32x4){0, 0, 0, 0};
  }
}
template <int NT>
__device__ __forceinline__ void tile_r2s(const u32x4 (&st)[tile_chunks<NT>()], char* tile, int pitch, int tid) {
#pragma unroll
  for (int i = 0; i < tile_chunks<NT>(); i++) {
    const int c = tid + i * NT, row = c >> 3, kc = c & 7;
    if (512 % NT == 0 || c < 512) *LDS_PTR(u32x4, tile + row * pitch + kc * 16) = st[i];
  }
}

// Unpadded [64 rows][128 B] tile that is read BOTH ways (ds_read_b128 row fragments and ds_read_b64_tr_b16 transposed fragments,
// e.g. K in the dQ kernel, Q / dO in the dK/dV kernel): no single row pitch is conflict-free for both (144 B: 2-way conflicts on the
// transposed reads, PMC: 21-23 % of the LDS cycles of the backward kernels; 192 B: 4-way on the row reads), an XOR swizzle is:
// 16-byte piece p of row r lives at slot p ^ sw2(r), sw2(r) = ((r >> 1) & 7) ^ (((r >> 1) & 1) << 2).
__device__ __forceinline__ int sw2(int r) { return ((r >> 1) & 7) ^ (((r >> 1) & 1) << 2); }
template <int NT>
__device__ __forceinline__ void tile_r2s_sw(const u32x4 (&st)[tile_chunks<NT>()], char* tile, int tid) {
#pragma unroll
  for (int i = 0; i < tile_chunks<NT>(); i++) {
    const int c = tid + i * NT, row = c >> 3, kc = c & 7;
    if (512 % NT == 0 || c < 512) *LDS_PTR(u32x4, tile + row * 128 + ((kc ^ sw2(row)) << 4)) = st[i];
  }
}
__device__ __forceinline__ bf16x8 row_frag_d(const char* tile, int rb, int ks, int lane) {
  const int r = rb + (lane & 31);
  return *LDS_PTR(const bf16x8, tile + r * 128 + (((ks * 2 + (lane >> 5)) ^ sw2(r)) << 4));
}
__device__ __forceinline__ bf16x8 tr_frag_d(const char* tile, int rb, int h8, int cb, int lane) {
  const int row = rb + 16 * h8 + 4 * (lane >> 5) + ((lane & 15) >> 2);
  const int cbyte = (cb * 32 + 16 * ((lane >> 4) & 1) + (lane & 3) * 4) * 2;
  const char* p0 = tile + row * 128 + ((((cbyte >> 4) ^ sw2(row)) << 4) | (cbyte & 15));
  const char* p1 = tile + (row + 8) * 128 + ((((cbyte >> 4) ^ sw2(row + 8)) << 4) | (cbyte & 15));
  s16x4 lo = lds_tr16(p0), hi = lds_tr16(p1);
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// pointer to the 64-wide head slice of token s (joint index) in the stream-split (B, L, H*64) tensors
__device__ __forceinline__ const bf16_t* tok_ptr(const bf16_t* x_img, const bf16_t* x_txt, int64_t b, int s, int n_img, int n_txt, int D, int h) {
  if (s < n_img) return x_img + ((b * n_img + s) * (int64_t)D + h * HD);
  return x_txt ? x_txt + ((b * n_txt + (s - n_img)) * (int64_t)D + h * HD) : nullptr;
}

// 1-D grid -> (tile, batch*head).  Workgroup b is observed to run on XCD b % 8 (private L2 each): all tiles of one
// (batch, head) are placed on ONE XCD so that its K/V (or Q/dO) is fetched from HBM once instead of once per XCD
// (measured: 577 MiB fetched per forward launch against 120 MB of Q,K,V before this mapping).  Locality only.
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

// ------------------------------------------------------------------------------------------------
// Backward of the per-head QK RMSNorm (+ axial RoPE on image tokens) fused into the epilogues of the attention backward kernels
// (mmdit_attn_bwd_qk): the dQ / dK rows a wave holds in its accumulators go straight to the gradient of the raw QKV projection, the
// stand-alone mmdit_qk_norm_rope_bwd pass (and the dQ / dK / dV round trip through HBM) disappears.  Same arithmetic as
// qk_norm_rope_bwd_body in rowops.hip (reference: Attention.py:130-135, 178-194 under autograd), on the accumulator layout:
// lane = row (l & 31), its 32 features f(db, g, e) = 32 db + 8 g + 4 (l >> 5) + e; the other 32 live in lane l ^ 32.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float partner32(float x, int lane);   // (defined with the forward kernels below)
constexpr float QK_RMS_EPS = 1.1920929e-07f;     // nn.RMSNorm(eps=None) on fp32 input: finfo(float32).eps (= RMS_EPS of rowops.hip)

struct QkFuse {
  const bf16_t* qkv_x; const bf16_t* qkv_c;      // saved raw projections, row-major (rows, 3 * H * 64): [q | k | v] per row
  const float* wq_x; const float* wk_x; const float* wq_c; const float* wk_c;   // norm weights (64)
  const float* rcos; const float* rsin;          // RoPE factors (n_img, 64)
  bf16_t* dqkv_x; bf16_t* dqkv_c;                // outputs, same geometry as qkv_x / qkv_c
  float* dw;                                     // (256) norm-weight gradients [wq_x | wk_x | wq_c | wk_c], accumulated (one atomic add per workgroup and feature)
};

// The epilogue goes through the LDS: a wave parks its 32 x 64 fp32 accumulator tile row-major (stride QK_ROW_F floats: b128 writes of
// the accumulator layout and b128 reads of the row layout are both conflict-free), then 8 lanes own one row (8 features = one 16-byte
// piece of the bf16 row each), 8 rows per pass, 4 passes.  Every global access is then a full 128-byte row segment per 8 lanes
// (the first version worked on the accumulator layout directly: 8-byte pieces of 32 different rows per instruction, 56 such
// instructions per wave -- the texture addresser made the fused form SLOWER than the two-pass one, 401 vs 336 us at MMDIT-B).
constexpr int QK_ROW_F = 68;
constexpr int QK_WAVE_BYTES = 32 * QK_ROW_F * 4;          // 8704 B per wave
template <int NW> constexpr int qk_lds_bytes() { return NW * QK_WAVE_BYTES + 128 * 4; }     // tiles + [image | text][64] weight-gradient sums

__device__ __forceinline__ void acc_to_lds(const f32x16 (&acc)[2], float* tile, int lane) {
  float* p = tile + (lane & 31) * QK_ROW_F + 4 * (lane >> 5);
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int g = 0; g < 4; g++)
      *LDS_PTR(f32x4, p + db * 32 + 8 * g) = (f32x4){acc[db][g * 4], acc[db][g * 4 + 1], acc[db][g * 4 + 2], acc[db][g * 4 + 3]};
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void lds_row8(const float* tile, int r, int c, float (&v)[8]) {
  const f32x4 a = *LDS_PTR(const f32x4, tile + r * QK_ROW_F + 8 * c), b = *LDS_PTR(const f32x4, tile + r * QK_ROW_F + 8 * c + 4);
#pragma unroll
  for (int e = 0; e < 4; e++) { v[e] = a[e]; v[4 + e] = b[e]; }
}
// tile: the wave's parked accumulators = gradient w.r.t. the normalised (and rotated) rows, to be multiplied by `mul`.  x0 / o0: raw
// features / output slot of the wave's row 0 (this head, this part), `pitch` elements between rows; nvalid rows of the 32 exist.
// cs0 / sn0: RoPE factors of row 0's token (image rows; rows are consecutive tokens), nullptr for text rows.  Adds this wave's
// norm-weight gradient into sdw[64] (LDS atomics from 8 lanes).
// the raw rows qk_bwd_tile needs (4 passes x 16 bytes per lane), requested ahead of it
__device__ __forceinline__ void qk_bwd_rows(u32x4 (&xr)[4], int lane, int nvalid, const bf16_t* x0, int64_t pitch) {
  const int c = lane & 7, rsub = lane >> 3;
#pragma unroll
  for (int it = 0; it < 4; it++) xr[it] = __builtin_nontemporal_load((const u32x4*)(x0 + min(it * 8 + rsub, nvalid - 1) * pitch + 8 * c));
}
__device__ __forceinline__ void qk_bwd_tile(const float* tile, float mul, int lane, int nvalid, const bf16_t* x0, bf16_t* o0, int64_t pitch,
                                            const float* w, const float* cs0, const float* sn0, float* sdw, const u32x4* xpre = nullptr) {
  const int c = lane & 7, rsub = lane >> 3;
  float w8[8], dw[8];
  ld8(w + 8 * c, w8);
#pragma unroll
  for (int e = 0; e < 8; e++) dw[e] = 0.f;
  // the four passes' raw rows are requested up front (16 registers as packed bf16): their latency overlaps the first pass
  u32x4 xr[4];
  if (xpre) {      // (compile-time at every call site: the caller requested the rows earlier -- qk_bwd_rows -- so that their latency lies under its barriers)
#pragma unroll
    for (int it = 0; it < 4; it++) xr[it] = xpre[it];
  } else {
#pragma unroll
    for (int it = 0; it < 4; it++) xr[it] = __builtin_nontemporal_load((const u32x4*)(x0 + min(it * 8 + rsub, nvalid - 1) * pitch + 8 * c));   // (last use of the saved projection)
  }
  // Round 6 (profiles/r06_epilogue_waits.txt).  Loads and stores of a wave retire through ONE in-order counter: a pass that requests its RoPE factors
  // behind the previous pass's store waits for that store, and the compiler's count is exact only in straight-line code.  FULL (all 32 rows exist:
  // every wave but the last one or two of a sequence) is therefore a compile-time variant without a conditional store, in which the factors of pass
  // p + 1 are requested into the SAME registers right after pass p's last use of them and BEFORE its store: pass p + 1 then waits with vmcnt(1).
  // Text rows (no rotation) read the norm weights -- 64 valid floats -- and ignore them, so that the load is unconditional too.
  const bool rope = cs0 != nullptr;
  const float* tc = rope ? cs0 : w;
  const float* ts = rope ? sn0 : w;
  auto body = [&](auto full_t) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_t)::value;
    float c8[8], s8[8];
    auto request = [&](int it) __attribute__((always_inline)) {
      const int rq = rope ? (FULL ? it * 8 + rsub : min(it * 8 + rsub, nvalid - 1)) : 0;
      ld8(tc + rq * 64 + 8 * c, c8);
      ld8(ts + rq * 64 + 8 * c, s8);
    };
    request(0);
#pragma unroll
    for (int it = 0; it < 4; it++) {
      const int r = it * 8 + rsub;
      const bool valid = FULL || r < nvalid;
      float dz[8], x[8];
#pragma unroll
      for (int e = 0; e < 4; e++) { x[2 * e] = __builtin_bit_cast(float, xr[it][e] << 16); x[2 * e + 1] = __builtin_bit_cast(float, xr[it][e] & 0xffff0000u); }
      lds_row8(tile, r, c, dz);
#pragma unroll
      for (int e = 0; e < 8; e++) dz[e] *= mul;
      if (rope) {   // transpose of the rotation: pairs (2p, 2p+1)
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const float da = dz[2 * p], dbv = dz[2 * p + 1];
          dz[2 * p] = da * c8[2 * p] + dbv * s8[2 * p + 1];
          dz[2 * p + 1] = dbv * c8[2 * p + 1] - da * s8[2 * p];
        }
      }
      if (it + 1 < 4) request(it + 1);      // (the factors of this pass are dead: same registers; before this pass's store)
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) ss += x[e] * x[e];
      const float rinv = rsqrtf(sum8(ss) * (1.f / 64.f) + QK_RMS_EPS);
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        x[e] *= rinv;                                      // xhat
        dw[e] += valid ? dz[e] * x[e] : 0.f;               // d(norm weight)
        dz[e] *= w8[e];                                    // d(xhat)
        dot += dz[e] * x[e];
      }
      dot = sum8(dot) * (1.f / 64.f);
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; e++) o[e] = rinv * (dz[e] - x[e] * dot);
      if (valid) st8(o0 + r * pitch + 8 * c, o);
    }
  };
  if (nvalid >= 32) body(std::integral_constant<bool, true>{});
  else body(std::integral_constant<bool, false>{});
  // the wave's 32 rows: lanes with equal c hold partial sums for features 8c .. 8c+7 (lane bits 5:3 = row lane)
#pragma unroll
  for (int e = 0; e < 8; e++) {
    float v = dw[e];
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < 8) atomicAdd(&sdw[8 * c + e], v);
  }
}
// dV rows: no arithmetic, the LDS round trip only makes the stores whole 128-byte rows
__device__ __forceinline__ void rows_from_tile(const float* tile, int lane, int nvalid, bf16_t* o0, int64_t pitch) {
  const int c = lane & 7, rsub = lane >> 3;
#pragma unroll
  for (int it = 0; it < 4; it++) {
    const int r = it * 8 + rsub;
    float v[8];
    lds_row8(tile, r, c, v);
    if (r < nvalid) st8(o0 + r * pitch + 8 * c, v);
  }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// KVL (mmdit_attn_fwd_kv / mmdit_attn_bwd_kv, Attention.py:243-251): K and V have s_kv rows of their own (pair-averaged keys: s_kv = S / 2); every
// key-side bound below is Skv, every query-side one S.  KVL = false: Skv IS S at compile time -- the instantiations of the other entry points.
template <int NW, bool ORACLE, bool KVL = false>
__global__ __launch_bounds__(NW * 64) void attn_fwd_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                            int BH, int H, int S, int n_img, float scale,
                                                            bf16_t* __restrict__ Ox, bf16_t* __restrict__ Oc, float* __restrict__ lse, int s_kv = 0) {
  const int Skv = KVL ? s_kv : S;
  constexpr int NT = NW * 64;
  __shared__ __attribute__((aligned(16))) char smem[2 * KT * P144 + 2 * KT * P192];
  auto kt = [&](int i) { return smem + i * KT * P144; };
  auto vt = [&](int i) { return smem + 2 * KT * P144 + i * KT * P192; };

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  MMDIT_YOUNG_HALF_PRIO();
  int qtile, bh;
  map_block((S + 32 * NW - 1) / (32 * NW), BH, qtile, bh);
  const int h = bh % H;
  const int64_t b = bh / H;
  const bf16_t* Qb = Q + (int64_t)bh * S * HD;
  const bf16_t* Kb = K + (int64_t)bh * Skv * HD;
  const bf16_t* Vb = V + (int64_t)bh * Skv * HD;
  const int q = qtile * 32 * NW + wave * 32 + (lane & 31);
  const int qc = min(q, S - 1);
  const bool active = qtile * 32 * NW + wave * 32 < S;   // wave-uniform: a wave whose 32 queries are all padding only helps with the tile copies

  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ks++) qf[ks] = *(const bf16x8*)(Qb + (int64_t)qc * HD + ks * 16 + (lane >> 5) * 8);

  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) o[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int nkv = (Skv + KT - 1) / KT;
  u32x4 sk[tile_chunks<NT>()], sv[tile_chunks<NT>()];

  // scores of tile j from LDS buffer kb_ -> s[2] (masked keys = -inf).  fast: log2 domain; oracle: natural, bf16-rounded
  auto scores = [&](int j, const char* ktile, f32x16 (&s)[2]) {
#pragma unroll
    for (int kb = 0; kb < 2; kb++) {
      if (j * KT + kb * 32 >= Skv) {   // (wave-uniform) the whole 32-key block is padding: no MFMAs, all scores masked
#pragma unroll
        for (int r = 0; r < 16; r++) s[kb][r] = -INFINITY;
        continue;
      }
#pragma unroll
      for (int r = 0; r < 16; r++) s[kb][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ks++) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(ktile, P144, kb * 32, ks, lane), qf[ks], s[kb], 0, 0, 0);
      if (ORACLE) {
#pragma unroll
        for (int r = 0; r < 16; r++) s[kb][r] = bf2f(f2bf(bf2f(f2bf(s[kb][r])) * scale));   // Attention.py:277: bf16 matmul, then bf16 * scale
      }
      if ((j + 1) * KT > Skv) {   // only the last (ragged) tile has keys to mask: wave-uniform branch
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (j * KT + kb * 32 + acc_row(r, lane) >= Skv) s[kb][r] = -INFINITY;
      }
    }
  };
  auto tile_max = [&](const f32x16 (&s)[2]) {
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[kb][r]);
    return fmaxf(mx, __shfl_xor(mx, 32, 64));
  };
  auto pv = [&](int j, const f32x16 (&p)[2], const char* vtile) {
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
      if (j * KT + kb * 32 < Skv)   // (the probabilities of a padding block are all zero)
#pragma unroll
      for (int h8 = 0; h8 < 2; h8++) {
        const bf16x8 pf = pack_frag(p[kb], h8);
#pragma unroll
        for (int db = 0; db < 2; db++) o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(vtile, P192, kb * 32, h8, db, lane), pf, o[db], 0, 0, 0);
      }
  };

  for (int pass = 0; pass < (ORACLE ? 2 : 1); pass++) {
    tile_g2r<NT>(sk, Kb, 0, Skv, tid);
    tile_g2r<NT>(sv, Vb, 0, Skv, tid);
    __syncthreads();  // previous pass done with the buffers
    tile_r2s<NT>(sk, kt(0), P144, tid);
    tile_r2s<NT>(sv, vt(0), P192, tid);
    __syncthreads();
    for (int j = 0; j < nkv; j++) {
      const int cur = j & 1;
      if (j + 1 < nkv) {
        tile_g2r<NT>(sk, Kb, (j + 1) * KT, Skv, tid);
        tile_g2r<NT>(sv, Vb, (j + 1) * KT, Skv, tid);
      }
      f32x16 s[2];
      if (active) scores(j, kt(cur), s);
      if (!active) {
      } else if (!ORACLE) {
        // raw scores; m is tracked in the scaled log2 domain: p = exp2(s*c - m) as one fma + v_exp_f32
        const float c = scale * LOG2E;
        const float mn = fmaxf(m, tile_max(s) * c);
        const float alpha = fast_exp2(m - mn);
        float rs = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; kb++)
#pragma unroll
          for (int r = 0; r < 16; r++) { const float p = fast_exp2(fmaf(s[kb][r], c, -mn)); s[kb][r] = p; rs += p; }
        rs += __shfl_xor(rs, 32, 64);
        l = l * alpha + rs; m = mn;
#pragma unroll
        for (int db = 0; db < 2; db++)
#pragma unroll
          for (int r = 0; r < 16; r++) o[db][r] *= alpha;
        pv(j, s, vt(cur));
      } else if (pass == 0) {
        const float mn = fmaxf(m, tile_max(s));
        float rs = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; kb++)
#pragma unroll
          for (int r = 0; r < 16; r++) rs += expf(s[kb][r] - mn);
        rs += __shfl_xor(rs, 32, 64);
        l = l * expf(m - mn) + rs; m = mn;
      } else {
#pragma unroll
        for (int kb = 0; kb < 2; kb++)
#pragma unroll
          for (int r = 0; r < 16; r++) s[kb][r] = expf(s[kb][r] - m) / l;   // softmax output, rounded to bf16 by pack_frag
        pv(j, s, vt(cur));
      }
      if (j + 1 < nkv) {
        tile_r2s<NT>(sk, kt(cur ^ 1), P144, tid);
        tile_r2s<NT>(sv, vt(cur ^ 1), P192, tid);
        __syncthreads();
      }
    }
  }

  if (q < S) {
    const float inv = ORACLE ? 1.f : 1.f / l;
    const int n_txt = S - n_img, D = H * HD;
    bf16_t* dst = q < n_img ? Ox + ((b * n_img + q) * (int64_t)D + h * HD) : Oc + ((b * n_txt + (q - n_img)) * (int64_t)D + h * HD);
#pragma unroll
    for (int db = 0; db < 2; db++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        float v4[4] = {o[db][g * 4] * inv, o[db][g * 4 + 1] * inv, o[db][g * 4 + 2] * inv, o[db][g * 4 + 3] * inv};
        st4(dst + db * 32 + 8 * g + 4 * (lane >> 5), v4);
      }
    if (lane < 32) lse[(int64_t)bh * S + q] = ORACLE ? m + logf(l) : m * LN2 + logf(l);
  }
}

// ------------------------------------------------------------------------------------------------
// forward, LDS-DMA variant (fast mode): K/V tiles go global -> LDS with global_load_lds (no VGPR staging, no ds_write) into a
// 4-stage ring, three tiles ahead of the MFMAs -- with one tile of look-ahead the loop was bound by the L2 latency of the
// tile copy, not by MFMA or VALU work.  The LDS image of a DMA is lane-linear, so tiles are unpadded [64 keys][128 B] and the
// bank swizzle is applied to the per-lane SOURCE address and mirrored by the fragment reads:
//   K (ds_read_b128 row fragments):      16-B piece p of key row r lives at slot p ^ ((r >> 1) & 7)
//   V (ds_read_b64_tr_b16 fragments):    16-B piece p of key row r lives at slot p ^ (4 * ((r >> 1) & 1))
// Rows beyond S are clamped to the last valid row (their scores are masked / their probabilities are zero).
// One s_waitcnt vmcnt + one s_barrier per tile; every wave issues exactly two pieces per tile (8 waves = 8 + 8 KiB).
// Round 4: nothing is issued past the last tile (the ring used to reload clamped copies: 3 of 7 + 3 tile copies at S = 410), the Q loads
// go out first and share the first tile's counted wait, the first MFMA of a score block takes a constant-zero C, scale-and-shift and row
// sums are packed fp32 pairs: 70 -> 67.5 us.  Workgroup geometry, same box (profiles/r04_round4_ab.txt; waves x ring stages; the forced geometries left the source after it):
// 8x4 70.2, 8x3 69.6, 4x4 104, 4x3 101, 4x2 101 us -- four independent 4-wave workgroups per CU de-phase MFMA and VALU work but copy every
// K/V tile twice as often, and the LDS-DMA stream (64 KiB per tile step and CU) becomes the limit.
// ------------------------------------------------------------------------------------------------
constexpr int ANS = 4;   // ring stages

__device__ __forceinline__ void attn_glds16(const void* gptr, uint32_t lds_dst_) {
  const uint32_t lds_dst = __builtin_amdgcn_readfirstlane(lds_dst_);
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gptr), "s"(lds_dst) : "memory", "m0");
}
__device__ __forceinline__ void attn_glds16s(uint32_t voff, const char* sbase_, uint32_t lds_dst_) {   // wave-uniform base + 32-bit lane offset
  const uint64_t a = (uint64_t)(uintptr_t)sbase_;
  const char* sbase = (const char*)(uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(a >> 32)) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)a));
  const uint32_t lds_dst = __builtin_amdgcn_readfirstlane(lds_dst_);
  asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst) : "memory", "m0");
}
// value of lane ^ 32 without an LDS round trip: v_permlane32_swap exchanges the upper half of its first operand with the lower
// half of the second; whichever way the compiler allocates the two copies of x (one register: both results are the partner's
// value; two registers: [own | partner] and [partner | own]), the select below picks the partner
__device__ __forceinline__ float partner32(float x, int lane) {
  const auto pr = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, x), false, false);
  return __builtin_bit_cast(float, lane < 32 ? pr[1] : pr[0]);
}
// fragments of the swizzled unpadded tiles
__device__ __forceinline__ bf16x8 row_frag_sw(const char* tile, int rb, int ks, int lane) {
  const int r = rb + (lane & 31), kp = ks * 2 + (lane >> 5);
  return *LDS_PTR(const bf16x8, tile + r * 128 + ((kp ^ ((r >> 1) & 7)) << 4));
}
__device__ __forceinline__ bf16x8 tr_frag_sw(const char* tile, int rb, int h8, int cb, int lane) {
  const int row = rb + 16 * h8 + 4 * (lane >> 5) + ((lane & 15) >> 2);
  const int cbyte = (cb * 32 + 16 * ((lane >> 4) & 1) + (lane & 3) * 4) * 2;
  const char* p = tile + row * 128 + ((((cbyte >> 4) ^ (4 * ((row >> 1) & 1))) << 4) | (cbyte & 15));
  s16x4 lo = lds_tr16(p), hi = lds_tr16(p + 8 * 128);     // row + 8: same swizzle bit
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// DBG (ablation builds, tools/probes/attn_ablate.py): 1 no exponentials (p = s), 2 no P V MFMAs, 4 no K Q^T MFMAs, 8 no LDS fragment reads
// (constant operands), 16 no per-tile wait / barrier / DMA, 32 no rescale / row sums
// MXO (fp8 inference): the output leaves as MX e4m3 -- codes in place of the bf16 rows (same (B, tokens, H * 64) geometry, one byte per
// feature) plus E8M0 block scales in the GEMM's layout (mx_scale_index; a head's 64 features are two 32-blocks) -- so the out-projection
// GEMM needs no quantise pass; bit-identical to the bf16 output followed by mmdit_mxfp8_quantize.
// PAD (MXO, odd H; include/mmdit_hip_mxpad.h): the code rows have pitch H * 64 + 64; the 64 pad bytes of a token (zero codes) and the scale
// bytes of its two pad blocks (0x00) belong to no head -- the workgroups of the LAST head write them for their own query rows, so every
// pad byte has exactly one writer in the launch.
template <int DBG = 0, bool MXO = false, int NW = 8, int NS = ANS, bool KVL = false, bool PAD = false>
__global__ __launch_bounds__(64 * NW) void attn_fwd_dma_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                           int BH, int H, int S, int n_img, float scale,
                                                           bf16_t* __restrict__ Ox, bf16_t* __restrict__ Oc, float* __restrict__ lse,
                                                           unsigned char* __restrict__ scx = nullptr, unsigned char* __restrict__ scc = nullptr, int s_kv = 0) {
  const int Skv = KVL ? s_kv : S;      // key rows (see attn_fwd_kernel)
  constexpr int PPW = 8 / NW;   // 1 KiB pieces (8 key rows) of each operand tile this wave copies
  static_assert(NW * PPW == 8 && NS >= 2 && NW * 4096 <= NS * 2 * KT * 128, "tile pieces / epilogue staging");
  __shared__ __attribute__((aligned(16))) char smem[NS * 2 * KT * 128];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  MMDIT_YOUNG_HALF_PRIO();
  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(char, smem);
  int qtile, bh;
  map_block((S + 32 * NW - 1) / (32 * NW), BH, qtile, bh);
  const int h = bh % H;
  const int64_t b = bh / H;
  const bf16_t* Qb = Q + (int64_t)bh * S * HD;
  const bf16_t* Kb = K + (int64_t)bh * Skv * HD;
  const bf16_t* Vb = V + (int64_t)bh * Skv * HD;
  const int q = qtile * 32 * NW + wave * 32 + (lane & 31);
  const int qc = min(q, S - 1);
  const bool active = qtile * 32 * NW + wave * 32 < S;

  if (DBG & 64) return;   // launch floor
  const int nkv = (Skv + KT - 1) / KT;
  // this lane's part of a tile: piece p = PPW * wave + i holds key rows 8 p .. 8 p + 7; row 8 p + (lane >> 3), 16-byte slot lane & 7
  const int slot = lane & 7;
  auto issue = [&](int j, int stage) {
#pragma unroll
    for (int i = 0; i < PPW; i++) {
      const int pc = wave * PPW + i, rl = 8 * pc + (lane >> 3);
      const int kcol = (slot ^ ((rl >> 1) & 7)) * 8, vcol = (slot ^ (4 * ((rl >> 1) & 1))) * 8;
      const int row = min(j * KT + rl, Skv - 1);
      attn_glds16(Kb + (int64_t)row * HD + kcol, lds0 + stage * (2 * KT * 128) + pc * 1024);
      attn_glds16(Vb + (int64_t)row * HD + vcol, lds0 + stage * (2 * KT * 128) + KT * 128 + pc * 1024);
    }
  };
  // The Q fragments are requested FIRST and the ring's first NS - 1 tiles behind them; nothing waits here: the first tile's counted wait
  // in the loop covers the Q loads too (they are older).  The Q loads are asm so that the compiler does not put a vmcnt(0) of its own
  // in front of their first use (it cannot see the DMA queue); the empty asm after the loop's wait carries the dependence.
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ks++) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qf[ks]) : "v"(Qb + (int64_t)qc * HD + ks * 16 + (lane >> 5) * 8) : "memory");
#pragma unroll
  for (int st = 0; st < NS - 1; st++)
    if (st < nkv) issue(st, st);

  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) o[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const float c = scale * LOG2E;
  // Per-lane LDS byte offsets of the fragment reads, computed ONCE: everything that depends on the tile / key block / k-step is
  // a compile-time constant added as the ds_read immediate (the swizzles only involve lane bits), so a tile costs 6 address
  // adds instead of one per read.
  //   K row fragment (kb, ks): row 32 kb + (lane & 31), piece (2 ks + (lane >> 5)) ^ ((row >> 1) & 7)  =  [(ks ^ f) << 5] + per-lane part
  //   V^T fragment (kb, h8, db): row 32 kb + 16 h8 + 4 (lane >> 5) + rr, piece ^ 4 ((rr >> 1) & 1)      =  [(db ^ b) << 6] + per-lane part
  uint32_t kofs[4], vofs[2];
  {
    const int l31 = lane & 31, hi5 = lane >> 5, swz = (l31 >> 1) & 7, f = swz >> 1, e = hi5 ^ (swz & 1);
#pragma unroll
    for (int ks = 0; ks < 4; ks++) kofs[ks] = l31 * 128 + ((ks ^ f) << 5) + (e << 4);
    const int rr = (lane & 15) >> 2, x = (lane >> 4) & 1, y = lane & 3, bb = (rr >> 1) & 1;
#pragma unroll
    for (int db = 0; db < 2; db++) vofs[db] = KT * 128 + (4 * hi5 + rr) * 128 + ((db ^ bb) << 6) + (x << 5) + ((y >> 1) << 4) + ((y & 1) << 3);
  }
  int stage = 0;
  for (int j = 0; j < nkv; j++) {
    if (!(DBG & 16) || j == 0) {
    // tile j has landed; the min(NS - 2, nkv - 1 - j) younger tiles may be in flight (nothing is issued past the last tile)
    const int ahead = nkv - 1 - j;
    if (NS >= 3 && ahead >= NS - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPW * (NS - 2)) : "memory");
    else if (NS >= 4 && ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]));
    __builtin_amdgcn_s_barrier();                                          // ... for every wave; and everyone has left tile j-1
    if (j + NS - 1 < nkv) issue(j + NS - 1, stage == 0 ? NS - 1 : stage - 1);   // refill the stage of tile j-1
    }
    const char* tile = smem + stage * (2 * KT * 128);
    stage = stage + 1 == NS ? 0 : stage + 1;
    if (!active) continue;
    const char* kp[4] = {tile + kofs[0], tile + kofs[1], tile + kofs[2], tile + kofs[3]};
    const char* vp[2] = {tile + vofs[0], tile + vofs[1]};
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; kb++) {
      // (a fully padded second block of the last tile is multiplied too -- its rows are copies of the last key -- and masked below: a
      //  skip would cost every tile 16 speculative v_mov of -inf)
      if (DBG & 4) {
#pragma unroll
        for (int r = 0; r < 16; r++) s[kb][r] = (float)qf[r & 3][0];
      } else {
        // the first MFMA of the chain takes the constant 0 as its C operand: no 16 v_mov per block to clear the accumulator
        constexpr f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ks++)
          s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16((DBG & 8) ? qf[(ks + 1) & 3] : *LDS_PTR(const bf16x8, kp[ks] + kb * 32 * 128), qf[ks], ks == 0 ? zero16 : s[kb], 0, 0, 0);
      }
      if ((j + 1) * KT > Skv) {
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (j * KT + kb * 32 + acc_row(r, lane) >= Skv) s[kb][r] = -INFINITY;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[kb][r]);
    mx = fmaxf(mx, partner32(mx, lane)) * c;   // the two lanes of a query (l, l + 32)
    // the accumulators are rescaled only when some query's running maximum grows (exact: alpha == 1 otherwise); after the first
    // tiles that is rare, and it takes 32 multiplies per lane out of most iterations
    if (!(DBG & 32) && !__all(mx <= m)) {
      const float mn = fmaxf(m, mx);
      const float alpha = fast_exp2(m - mn);
      l *= alpha;
      m = mn;
#pragma unroll
      for (int db = 0; db < 2; db++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[db][r] *= alpha;
    }
    // p = 2^(s c - m): the scale-and-shift and the row sums as packed fp32 pairs (v_pk_fma_f32 / v_pk_add_f32: two values per issue slot);
    // the 32 v_exp_f32 stay scalar -- they are the VALU floor of a tile
#ifdef MMDIT_ATTN_SCALAR_MATH      // experiment: one-value fp32 instructions (they co-issue with the other waves' MFMAs; v_pk_* do not: tools/probes/mfma_valu_mix.hip)
    float rs = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float t = fmaf(s[kb][r], c, -m);       // (compile with -fno-slp-vectorize, or the compiler packs these again)
        const float pe = (DBG & 1) ? t : fast_exp2(t);
        s[kb][r] = pe;
        if (!(DBG & 32)) rs += pe;
      }
    l += rs + partner32(rs, lane);
#else
    f32x2 rs2 = {0.f, 0.f};
    const f32x2 c2 = {c, c}, nm2 = {-m, -m};
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const f32x2 sv = {s[kb][r], s[kb][r + 1]};
        const f32x2 t = (DBG & 1) ? sv : __builtin_elementwise_fma(sv, c2, nm2);
        const f32x2 pv = {(DBG & 1) ? t[0] : fast_exp2(t[0]), (DBG & 1) ? t[1] : fast_exp2(t[1])};
        s[kb][r] = pv[0];
        s[kb][r + 1] = pv[1];
        if (!(DBG & 32)) rs2 += pv;
      }
    const float rs = rs2[0] + rs2[1];
    l += rs + partner32(rs, lane);
#endif
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
      if (j * KT + kb * 32 < Skv)
#pragma unroll
        for (int h8 = 0; h8 < 2; h8++) {
          const bf16x8 pf = pack_frag(s[kb], h8);
#pragma unroll
          for (int db = 0; db < 2; db++) {
            if (DBG & 2) { o[db][h8] += (float)pf[0]; continue; }
            if (DBG & 8) { o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[db + h8], pf, o[db], 0, 0, 0); continue; }
            const char* q0 = vp[db] + (kb * 32 + 16 * h8) * 128;
            const s16x4 lo = lds_tr16(q0), hi = lds_tr16(q0 + 8 * 128);
            const s16x8 vr = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vr), pf, o[db], 0, 0, 0);
          }
        }
  }
  __builtin_amdgcn_s_barrier();                      // every wave has left the last tile (no DMA is in flight: the last wait was vmcnt(0))
  if (DBG & 128) { if (o[0][0] + o[1][3] + l == 12345.f) lse[0] = 1.f; return; }
  // Epilogue: the accumulators hold O^T fragments (lane = query, 4 consecutive features per register group): stored directly, every
  // instruction would touch 32 different rows with 8 bytes each (16 instructions per wave, store-issue-bound: the empty-loop
  // ablation of this kernel takes 32 of its 73 us).  Each wave stages its 32 x 64 bf16 block through a private 4 KB of the (now
  // idle) ring -- 16-byte chunk c of row r at chunk c ^ (r & 7), conflict-free both ways -- and writes it as 8 rows x 128 B per
  // instruction (whole lines).
  {
    const float inv = 1.f / l;
    char* stg = smem + wave * 4096;
    const int wr = lane & 31, wc = lane >> 5;
#pragma unroll
    for (int db = 0; db < 2; db++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const u32x2 pk = {pack_bf2(o[db][g * 4] * inv, o[db][g * 4 + 1] * inv), pack_bf2(o[db][g * 4 + 2] * inv, o[db][g * 4 + 3] * inv)};
        *LDS_PTR(u32x2, stg + wr * 128 + (((db * 4 + g) ^ (wr & 7)) << 4) + wc * 8) = pk;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private region: program order is enough
    const int n_txt = S - n_img, D = H * HD;
    const int rr = lane >> 3, rc = lane & 7;
#pragma unroll
    for (int it = 0; it < 4; it++) {
      const int r = it * 8 + rr, qq = qtile * 32 * NW + wave * 32 + r;
      const u32x4 t = *LDS_PTR(const u32x4, stg + r * 128 + ((rc ^ (r & 7)) << 4));
      if constexpr (MXO) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; e++) { v[2 * e] = __builtin_bit_cast(float, t[e] << 16); v[2 * e + 1] = __builtin_bit_cast(float, t[e] & 0xffff0000u); }
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) amax = fmaxf(amax, fabsf(v[e]));
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));     // the 32-block: four 16-byte chunks = four adjacent lanes
        amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
        float inv;
        const int ex = mx_exponent(amax, inv);
        if (qq < S) {
          const bool img = qq < n_img;
          const int64_t tok = img ? b * n_img + qq : b * n_txt + (qq - n_img);
          unsigned char* dst = (unsigned char*)(img ? Ox : Oc) + tok * (D + (PAD ? 64 : 0)) + h * HD + rc * 8;
          *(uint2*)dst = make_uint2(mx_pack4(v, inv), mx_pack4(v + 4, inv));
          if ((rc & 3) == 0) (img ? scx : scc)[mx_scale_index((int)tok, h * 2 + (rc >> 2), (BH / H) * (img ? n_img : n_txt))] = (unsigned char)(ex + 127);
          if constexpr (PAD) {
            if (h == H - 1) {      // (workgroup-uniform) lanes rc 0-3: the token's 64 pad bytes; rc 0 / 1: the scale bytes of its two pad blocks
              if (rc < 4) *(uint4*)((unsigned char*)(img ? Ox : Oc) + tok * (D + 64) + D + rc * 16) = make_uint4(0u, 0u, 0u, 0u);
              if (rc < 2) (img ? scx : scc)[mx_scale_index((int)tok, H * 2 + rc, (BH / H) * (img ? n_img : n_txt))] = 0;
            }
          }
        }
      } else if (qq < S) {
        bf16_t* dst = qq < n_img ? Ox + ((b * n_img + qq) * (int64_t)D + h * HD) : Oc + ((b * n_txt + (qq - n_img)) * (int64_t)D + h * HD);
        *(u32x4*)(dst + rc * 8) = t;
      }
    }
    if (!MXO && q < S && lane < 32) lse[(int64_t)bh * S + q] = m * LN2 + logf(l);
  }
}

// (Two forward variants of round 2 -- a persistent one, 2 workgroups per CU walking the work items, 71.6 vs 69.7 us, and one with 64 queries
//  per wave on 4 waves, 80 vs 74 us -- were measured slower and are not part of the library any more; their text is in the history of this
//  file, commit cd8583f.)

// ------------------------------------------------------------------------------------------------
// backward dQ: query-stationary, loops over KV tiles.  dQ^T[hd][q] += K^T[hd][key] dS^T[key][q]
// ------------------------------------------------------------------------------------------------
#ifndef MMDIT_DQ_WAVES
#define MMDIT_DQ_WAVES 4
#endif
template <int NW, typename TG, bool FUSE = false, bool KVL = false>
__global__ __launch_bounds__(NW * 64, NW == 8 ? MMDIT_DQ_WAVES : 1) void attn_bwd_dq_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                               const bf16_t* __restrict__ Ox, const bf16_t* __restrict__ Oc,
                                                               const bf16_t* __restrict__ dOx, const bf16_t* __restrict__ dOc,
                                                               const float* __restrict__ lse, float* __restrict__ delta,
                                                               int BH, int H, int S, int n_img, float scale, TG* __restrict__ dQ, QkFuse F = QkFuse(), int s_kv = 0) {
  static_assert(!(FUSE && KVL), "the fused QK epilogue keeps one sequence length");
  const int Skv = KVL ? s_kv : S;      // key rows (see attn_fwd_kernel)
  // delta[q] = sum_d dO[q,d] O[q,d] is formed here from the query's own dO / O rows (each lane holds half of the 64 features of its
  // query) and written out for the dK/dV kernel that follows on the same stream -- no separate preparation pass.
  constexpr int NT = NW * 64;
  // (fused epilogue: dynamic LDS of qk_lds_bytes<NW>() > 64 KB, whose head is the K / V tile pair of the main loop)
  // NW == 8: the K / V tiles arrive through a DQ_ST-stage LDS-DMA ring (global_load_lds, no staging registers, two tiles in flight behind
  // the one being multiplied) -- the register-staged copy of the other widths pays a tile's round trip between two barriers every tile.
  constexpr bool DMA = NW == 8;
#ifndef MMDIT_DQ_STAGES
#define MMDIT_DQ_STAGES 3
#endif
  constexpr int DQ_ST = MMDIT_DQ_STAGES;
  __shared__ __attribute__((aligned(16))) char smem_static[FUSE ? 16 : (DMA ? DQ_ST : 1) * 2 * KT * 128];
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  char* smem = FUSE ? smem_dyn : smem_static;
  char* ktile = smem;
  char* vtile = smem + KT * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  MMDIT_YOUNG_HALF_PRIO();
  int qtile, bh;
  map_block((S + 32 * NW - 1) / (32 * NW), BH, qtile, bh);
  const int h = bh % H;
  const int64_t b = bh / H;
  const bf16_t* Qb = Q + (int64_t)bh * S * HD;
  const bf16_t* Kb = K + (int64_t)bh * Skv * HD;
  const bf16_t* Vb = V + (int64_t)bh * Skv * HD;
  const int q = qtile * 32 * NW + wave * 32 + (lane & 31);
  const int qc = min(q, S - 1);
  const bool active = qtile * 32 * NW + wave * 32 < S;
  const bf16_t* dop = tok_ptr(dOx, dOc, b, qc, n_img, S - n_img, H * HD, h);

  bf16x8 qf[4], dof[4];
#pragma unroll
  for (int ks = 0; ks < 4; ks++) {
    qf[ks] = *(const bf16x8*)(Qb + (int64_t)qc * HD + ks * 16 + (lane >> 5) * 8);
    u32x4 z = {0, 0, 0, 0};
    dof[ks] = dop ? *(const bf16x8*)(dop + ks * 16 + (lane >> 5) * 8) : __builtin_bit_cast(bf16x8, z);
  }
  float dq_delta = 0.f;
  {
    const bf16_t* op = tok_ptr(Ox, Oc, b, qc, n_img, S - n_img, H * HD, h);
    if (dop && op) {
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
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
  f32x16 acc[2];
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[db][r] = 0.f;

  const int nkv = (Skv + KT - 1) / KT;
  u32x4 sk[DMA ? 1 : tile_chunks<NT>()], sv[DMA ? 1 : tile_chunks<NT>()];
  // DMA: this lane's 16 bytes of a tile -- key row 8 * wave + (lane >> 3), LDS slot lane & 7 holds chunk slot ^ sw2(row) (the layout
  // tile_r2s_sw writes and row_frag_d / tr_frag_d read); rows past the end re-read the last key (masked below in the ragged tile)
  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(char, smem);
  const int rl = 8 * wave + (lane >> 3), dcol = ((lane & 7) ^ sw2(rl)) * 8;
  auto issue = [&](int j, int stage) {     // wave-uniform bases (SGPR pairs) + one 32-bit lane offset: the kernel sits at its 128-VGPR cap
    const uint32_t voff = (uint32_t)min(min(j, nkv - 1) * KT + rl, Skv - 1) * (HD * 2) + dcol * 2;
    attn_glds16s(voff, (const char*)Kb, lds0 + stage * (2 * KT * 128) + wave * 1024);
    attn_glds16s(voff, (const char*)Vb, lds0 + stage * (2 * KT * 128) + KT * 128 + wave * 1024);
  };
  int stage = 0;
  if constexpr (DMA) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the Q / dO / O / lse loads above: from here on only DMA pieces are counted)
#pragma unroll
    for (int st = 0; st < DQ_ST - 1; st++) issue(st, st);
  }
  for (int j = 0; j < nkv; j++) {
    if constexpr (DMA) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (DQ_ST - 2)) : "memory");   // tile j has landed (DQ_ST - 2 younger tiles may be in flight)
      __builtin_amdgcn_s_barrier();                                             // ... for every wave; and everyone has left tile j - 1
      issue(j + DQ_ST - 1, stage == 0 ? DQ_ST - 1 : stage - 1);                 // refill the stage of tile j - 1
      ktile = smem + stage * (2 * KT * 128);
      vtile = ktile + KT * 128;
      stage = stage + 1 == DQ_ST ? 0 : stage + 1;
    } else {
      tile_g2r<NT>(sk, Kb, j * KT, Skv, tid);
      tile_g2r<NT>(sv, Vb, j * KT, Skv, tid);
      __syncthreads();
      tile_r2s_sw<NT>(sk, ktile, tid);
      tile_r2s_sw<NT>(sv, vtile, tid);
      __syncthreads();
    }
    if (!active) continue;
#pragma unroll
    for (int kb = 0; kb < 2; kb++) {
      if (j * KT + kb * 32 >= Skv) continue;   // (wave-uniform) 32 padding keys contribute nothing
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_d(ktile, kb * 32, ks, lane), qf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_d(vtile, kb * 32, ks, lane), dof[ks], dp, 0, 0, 0);
      }
      // per 8-row half: softmax arithmetic, pack, the half's two dQ MFMAs -- s / dp die as they are consumed (the kernel sits at its
      // 128-VGPR cap), and the second half's VALU work issues behind the first half's MFMAs.
      // Padding keys exist in the last K/V tile only: a wave-uniform branch.  (Written as a per-element `ragged && ...` select the
      // compiler evaluated index, compare and two selects for EVERY score of EVERY tile: 4 of the loop's ~11 VALU slots per score.)
      const bool ragged = (j + 1) * KT > Skv;
#pragma unroll
      for (int h8 = 0; h8 < 2; h8++) {
        __builtin_amdgcn_sched_barrier(0);
        f32x16 d8;      // (only elements [8 h8, 8 h8 + 8) are used: pack_frag's register window)
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const int r = 8 * h8 + i;
          const float p = fast_exp2(fmaf(s[r], scale * LOG2E, -lq));
          d8[r] = p * (dp[r] - dq_delta);
        }
        if (ragged) {
#pragma unroll
          for (int i = 0; i < 8; i++)
            if (j * KT + kb * 32 + acc_row(8 * h8 + i, lane) >= Skv) d8[8 * h8 + i] = 0.f;
        }
        const bf16x8 dsf = pack_frag(d8, h8);
#pragma unroll
        for (int db = 0; db < 2; db++) acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_d(ktile, kb * 32, h8, db, lane), dsf, acc[db], 0, 0, 0);
      }
    }
  }
  if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // trailing (clamped, unused) pieces must land before the LDS is reused / released
  if constexpr (FUSE) {
    // dQ rows -> gradient of the raw q projection (RMSNorm + RoPE backward, qk_bwd_tile), norm-weight gradient partials of this workgroup
    __syncthreads();                       // every wave has left the last K/V tile: the LDS is free
    float* sdw = (float*)(smem + NW * QK_WAVE_BYTES);             // [image | text][64]
    if (tid < 128) sdw[tid] = 0.f;
    __syncthreads();
    if (active) {
      const int q0 = qtile * 32 * NW + wave * 32;
      const bool img = q0 < n_img;                                   // wave-uniform: n_img % 32 == 0 (checked by the launcher)
      const int n_txt = S - n_img, tok0 = img ? q0 : q0 - n_img, nvalid = min(32, (img ? n_img : S) - q0);
      const int64_t pitch = 3 * (int64_t)(H * HD), off = (img ? b * n_img + tok0 : b * n_txt + tok0) * pitch + h * HD;
      float* tile = (float*)(smem + wave * QK_WAVE_BYTES);
      acc_to_lds(acc, tile, lane);
      qk_bwd_tile(tile, scale, lane, nvalid, (img ? F.qkv_x : F.qkv_c) + off, (img ? F.dqkv_x : F.dqkv_c) + off, pitch, img ? F.wq_x : F.wq_c,
                  img ? F.rcos + (int64_t)tok0 * 64 : nullptr, img ? F.rsin + (int64_t)tok0 * 64 : nullptr, sdw + (img ? 0 : 64));
    }
    __syncthreads();
    if (tid < 128 && sdw[tid] != 0.f) atomicAdd(F.dw + (tid >> 6) * 128 + (tid & 63), sdw[tid]);    // [wq_x | . | wq_c | .]  (a workgroup is all image or mostly one stream: half of the adds are exact zeros)
  } else if (q < S) {
    TG* dst = dQ + ((int64_t)bh * S + q) * HD;
#pragma unroll
    for (int db = 0; db < 2; db++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        float v4[4] = {acc[db][g * 4] * scale, acc[db][g * 4 + 1] * scale, acc[db][g * 4 + 2] * scale, acc[db][g * 4 + 3] * scale};
        st4(dst + db * 32 + 8 * g + 4 * (lane >> 5), v4);
      }
  }
}

// ------------------------------------------------------------------------------------------------
// backward dK/dV: key-stationary (each wave owns 32 keys), loops over query tiles of 64.
//   S[q][key] = Q K^T, dP[q][key] = dO V^T  (lane owns key l&31, rows = queries)
//   dV^T[d][key] += dO^T[d][q] P[q][key],  dK^T[hd][key] += Q^T[hd][q] dS[q][key]
// ------------------------------------------------------------------------------------------------
// TRACE (probes build, tools/probes/attn_bwd_trace.py): lane 0 of every wave of the first 2048 workgroups records the cycle counter at
// the phase boundaries (72 slots per wave)
template <int NW, typename TG, bool FUSE = false, bool TRACE = false, bool KVL = false>
__global__ __launch_bounds__(NW * 64) void attn_bwd_dkv_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                           const bf16_t* __restrict__ dOx, const bf16_t* __restrict__ dOc,
                                                           const float* __restrict__ lse, const float* __restrict__ delta,
                                                           int BH, int H, int S, int n_img, float scale, TG* __restrict__ dK, TG* __restrict__ dV, QkFuse F = QkFuse(),
                                                           unsigned long long* __restrict__ trace = nullptr, int s_kv = 0) {
  static_assert(!(FUSE && KVL), "the fused QK epilogue keeps one sequence length");
  const int Skv = KVL ? s_kv : S;      // key rows: the grid, the stationary fragments and the outputs of this kernel (see attn_fwd_kernel)
  int tpos = 0;
  auto stamp = [&]() {
    if constexpr (TRACE) {
      if (blockIdx.x < 2048 && (threadIdx.x & 63) == 0 && tpos < 72) trace[((int64_t)blockIdx.x * NW + (threadIdx.x >> 6)) * 72 + tpos] = __builtin_readcyclecounter();
      tpos++;
    }
  };
  stamp();                                   // 0: start
  constexpr int NT = NW * 64;
  __shared__ __attribute__((aligned(16))) char smem_static[FUSE ? 16 : 2 * KT * 128 + 2 * KT * 4];
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];      // fused epilogue: qk_lds_bytes<NW>()
  char* smem = FUSE ? smem_dyn : smem_static;
  char* qtile = smem;
  char* dotile = smem + KT * 128;
  float* lse_s = (float*)(smem + 2 * KT * 128);
  float* del_s = lse_s + KT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  MMDIT_YOUNG_HALF_PRIO();
  int ktile, bh;
  map_block((Skv + 32 * NW - 1) / (32 * NW), BH, ktile, bh);
  const int h = bh % H;
  const int64_t b = bh / H;
  const bf16_t* Qb = Q + (int64_t)bh * S * HD;
  const bf16_t* Kb = K + (int64_t)bh * Skv * HD;
  const bf16_t* Vb = V + (int64_t)bh * Skv * HD;
  const int key = ktile * 32 * NW + wave * 32 + (lane & 31);
  const bool active = ktile * 32 * NW + wave * 32 < Skv;   // wave-uniform: a wave whose 32 keys are all padding only helps with the tile copies
  const int keyc = min(key, Skv - 1);
  const int n_txt = S - n_img, D = H * HD;

  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ks++) {
    kf[ks] = *(const bf16x8*)(Kb + (int64_t)keyc * HD + ks * 16 + (lane >> 5) * 8);
    vf[ks] = *(const bf16x8*)(Vb + (int64_t)keyc * HD + ks * 16 + (lane >> 5) * 8);
  }
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) { dk[db][r] = 0.f; dv[db][r] = 0.f; }

  const int nq = (S + KT - 1) / KT;
  // The next Q / dO tile (+ its lse / delta) is requested into registers BEFORE this tile's arithmetic and parked in LDS after it: with
  // one workgroup per CU (204 VGPRs) nothing else hides the ~2 us of a tile's round trip.  (NW = 8: one 16-byte chunk of each per thread.)
  u32x4 sq[tile_chunks<NT>()], sd[tile_chunks<NT>()];
  float lv = 0.f, dl = 0.f;
  auto request = [&](int jq) {
    tile_g2r<NT>(sq, Qb, jq * KT, S, tid);
#pragma unroll
    for (int i = 0; i < tile_chunks<NT>(); i++) {
      const int c = tid + i * NT, row = c >> 3, kc = c & 7, s = jq * KT + row;
      const bf16_t* p = (c < 512 && s < S) ? tok_ptr(dOx, dOc, b, s, n_img, n_txt, D, h) : nullptr;
      sd[i] = p ? *(const u32x4*)(p + kc * 8) : (u32x4){0, 0, 0, 0};
    }
    lv = 0.f, dl = 0.f;
    if (tid < KT && jq * KT + tid < S) { lv = lse[(int64_t)bh * S + jq * KT + tid]; dl = delta[(int64_t)bh * S + jq * KT + tid]; }   // (no arithmetic on the loaded values here: it would put the wait in front of the tile's MFMAs)
  };
  request(0);
  stamp();                                   // 1: K / V fragments and the first tile requested
  for (int jq = 0; jq < nq; jq++) {
    __syncthreads();
    stamp();                                 // per tile +0: everyone has left the previous tile
    tile_r2s_sw<NT>(sq, qtile, tid);
    tile_r2s_sw<NT>(sd, dotile, tid);
    if (tid < KT) { lse_s[tid] = lv * LOG2E; del_s[tid] = dl; }
    stamp();                                 // +1: this tile's chunks have landed and are parked in LDS
    __syncthreads();
    stamp();                                 // +2: ... everybody's
    if (jq + 1 < nq) request(jq + 1);
    if (active) {
#pragma unroll
    for (int qb = 0; qb < 2; qb++) {
      if (jq * KT + qb * 32 >= S) continue;   // (wave-uniform) 32 padding queries contribute nothing
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_d(qtile, qb * 32, ks, lane), kf[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_d(dotile, qb * 32, ks, lane), vf[ks], dp, 0, 0, 0);
      }
      if constexpr (TRACE) stamp();            // +3 / +6: S / dP MFMAs issued
      f32x16 ds;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int r0 = qb * 32 + 8 * g + 4 * (lane >> 5);
        const f32x4 l4 = *LDS_PTR(const f32x4, lse_s + r0);
        const f32x4 d4 = *LDS_PTR(const f32x4, del_s + r0);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int r = g * 4 + e;
          const float p = fast_exp2(fmaf(s[r], scale * LOG2E, -l4[e]));
          s[r] = p;
          ds[r] = p * (dp[r] - d4[e]);
        }
      }
      // No per-score masks in the steady state: a lane whose key is padding (key >= Skv: the key count, S unless KVL) works on the clamped last key and its dK / dV
      // column is never stored; padding QUERIES (>= S, the query count) exist in the last Q / dO tile only (their rows are zero-filled, lse = delta = 0, so
      // they would contribute exact zeros anyway; masked in a wave-uniform branch to keep P and dS themselves zero there).
      if ((jq + 1) * KT > S) {
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
          for (int e = 0; e < 4; e++)
            if (jq * KT + qb * 32 + 8 * g + 4 * (lane >> 5) + e >= S) { s[g * 4 + e] = 0.f; ds[g * 4 + e] = 0.f; }
      }
      if constexpr (TRACE) stamp();            // +4 / +7: softmax arithmetic issued
#pragma unroll
      for (int h8 = 0; h8 < 2; h8++) {
        const bf16x8 pf = pack_frag(s, h8), dsf = pack_frag(ds, h8);
#pragma unroll
        for (int db = 0; db < 2; db++) {
          dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_d(dotile, qb * 32, h8, db, lane), pf, dv[db], 0, 0, 0);
          dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_d(qtile, qb * 32, h8, db, lane), dsf, dk[db], 0, 0, 0);
        }
      }
      if constexpr (TRACE) stamp();            // +5 / +8: dV / dK MFMAs issued
    }
    }
    if constexpr (TRACE) { const int done = !active ? 0 : (jq * KT + 32 >= S ? 1 : 2); for (int i = done * 3; i < 6; i++) stamp(); }   // (fixed slot count per tile)
  }
  stamp();                                   // loop end
  if constexpr (FUSE) {
    // dK rows -> gradient of the raw k projection (qk_bwd_tile), dV rows into the v part of the same output rows
    const int k0 = ktile * 32 * NW + wave * 32;
    const bool img = k0 < n_img;                                   // wave-uniform: n_img % 32 == 0
    const int tok0 = img ? k0 : k0 - n_img, nvalid = min(32, (img ? n_img : S) - k0);
    const int64_t pitch = 3 * (int64_t)D, off = (img ? b * n_img + tok0 : b * n_txt + tok0) * pitch + D + h * HD;
    u32x4 xk[4];                           // the raw k rows: requested here, used behind the two barriers and the parking of dK
    if (active) qk_bwd_rows(xk, lane, nvalid, (img ? F.qkv_x : F.qkv_c) + off, pitch);
    __syncthreads();                       // every wave has left the last Q / dO tile
    float* sdw = (float*)(smem + NW * QK_WAVE_BYTES);             // [image | text][64]
    if (tid < 128) sdw[tid] = 0.f;
    __syncthreads();
    if (active) {
      bf16_t* ob = (img ? F.dqkv_x : F.dqkv_c) + off;
      float* tile = (float*)(smem + wave * QK_WAVE_BYTES);
      acc_to_lds(dk, tile, lane);
      qk_bwd_tile(tile, scale, lane, nvalid, (img ? F.qkv_x : F.qkv_c) + off, ob, pitch, img ? F.wk_x : F.wk_c,
                  img ? F.rcos + (int64_t)tok0 * 64 : nullptr, img ? F.rsin + (int64_t)tok0 * 64 : nullptr, sdw + (img ? 0 : 64), xk);
      __builtin_amdgcn_wave_barrier();
      acc_to_lds(dv, tile, lane);
      rows_from_tile(tile, lane, nvalid, ob + D, pitch);
    }
    __syncthreads();
    if (tid < 128 && sdw[tid] != 0.f) atomicAdd(F.dw + (tid >> 6) * 128 + 64 + (tid & 63), sdw[tid]);   // [. | wk_x | . | wk_c]
  } else if (key < Skv) {
    TG* pk = dK + ((int64_t)bh * Skv + key) * HD;
    TG* pv = dV + ((int64_t)bh * Skv + key) * HD;
#pragma unroll
    for (int db = 0; db < 2; db++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        float k4[4] = {dk[db][g * 4] * scale, dk[db][g * 4 + 1] * scale, dk[db][g * 4 + 2] * scale, dk[db][g * 4 + 3] * scale};
        float v4[4] = {dv[db][g * 4], dv[db][g * 4 + 1], dv[db][g * 4 + 2], dv[db][g * 4 + 3]};
        st4(pk + db * 32 + 8 * g + 4 * (lane >> 5), k4);
        st4(pv + db * 32 + 8 * g + 4 * (lane >> 5), v4);
      }
  }
  if constexpr (TRACE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  stamp();                                   // stores done
}

}  // namespace

// Workgroup width of the fast-mode launches below: 8 waves (32 queries / keys each).  All waves of a workgroup share one stream of 64-row K/V (or
// Q/dO) tiles, so 8 waves instead of 2 cut the tile copies and barriers per (batch, head) from 7x to 2x (measured at S = 410: forward 115 -> 70 us,
// backward 372 -> 271 us).  7-wave workgroups would pad S = 410 less (448 instead of 512 rows) but measured slower (forward 96 vs 70 us: 448
// threads copy a 512-chunk tile in two unbalanced passes).
extern "C" int mmdit_attn_fwd(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale, int mode,
                              void* Ox, void* Oc, float* lse, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && Ox && lse && batch > 0 && heads > 0 && S > 0 && n_img > 0 && n_img <= S);
  MMDIT_CHECK_ARG(Oc || n_img == S);
  hipStream_t s = (hipStream_t)stream;
  if (mode != 0 && mode != 1) return MMDIT_ERR_ARG;
  if (mode == 1)                                     // the reference's rounding points (parity mode)
    hipLaunchKernelGGL((attn_fwd_kernel<2, true>), dim3(((S + 63) / 64) * batch * heads), dim3(128), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V,
                       batch * heads, heads, S, n_img, scale, (bf16_t*)Ox, (bf16_t*)Oc, lse);
  else
    hipLaunchKernelGGL((attn_fwd_dma_kernel<0, false, 8, 4>), dim3(((S + 255) / 256) * batch * heads), dim3(512), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V,
                       batch * heads, heads, S, n_img, scale, (bf16_t*)Ox, (bf16_t*)Oc, lse);
  return mmdit_launch_status();
}


extern "C" int mmdit_attn_fwd_mx(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale,
                                 void* Ox_fp8, void* Oc_fp8, void* scales_x, void* scales_c, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && Ox_fp8 && scales_x && batch > 0 && heads > 0 && S > 0 && n_img > 0 && n_img <= S);
  MMDIT_CHECK_ARG((Oc_fp8 && scales_c) || n_img == S);
  hipLaunchKernelGGL((attn_fwd_dma_kernel<0, true>), dim3(((S + 255) / 256) * batch * heads), dim3(512), 0, (hipStream_t)stream, (const bf16_t*)Q, (const bf16_t*)K,
                     (const bf16_t*)V, batch * heads, heads, S, n_img, scale, (bf16_t*)Ox_fp8, (bf16_t*)Oc_fp8, nullptr, (unsigned char*)scales_x, (unsigned char*)scales_c);
  return mmdit_launch_status();
}

// include/mmdit_hip_mxpad.h: mmdit_attn_fwd_mx with the code rows zero-padded to K_pad = heads * 64 rounded up to 128 (an odd head count: the
// PAD instantiation; an even one: the plain kernel, the same bytes as mmdit_attn_fwd_mx)
extern "C" int mmdit_attn_fwd_mx_pad(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale,
                                     void* Ox_fp8, void* Oc_fp8, void* scales_x, void* scales_c, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && Ox_fp8 && scales_x && batch > 0 && heads > 0 && S > 0 && n_img > 0 && n_img <= S);
  MMDIT_CHECK_ARG((Oc_fp8 && scales_c) || n_img == S);
  if ((int64_t)batch * S * ((heads + 1) / 2 * 128 / 16) > 0x7fffffffll) return MMDIT_ERR_SHAPE;      // (scale rows are indexed with int)
  if (heads % 2 == 0) return mmdit_attn_fwd_mx(Q, K, V, batch, heads, S, n_img, scale, Ox_fp8, Oc_fp8, scales_x, scales_c, stream);
  hipLaunchKernelGGL((attn_fwd_dma_kernel<0, true, 8, ANS, false, true>), dim3(((S + 255) / 256) * batch * heads), dim3(512), 0, (hipStream_t)stream, (const bf16_t*)Q,
                     (const bf16_t*)K, (const bf16_t*)V, batch * heads, heads, S, n_img, scale, (bf16_t*)Ox_fp8, (bf16_t*)Oc_fp8, nullptr, (unsigned char*)scales_x,
                     (unsigned char*)scales_c);
  return mmdit_launch_status();
}

#ifdef MMDIT_PROBES
// measurement aid (tools/probes/attn_ablate.py; not part of include/mmdit_hip.h): the forward kernel with parts of its loop removed
extern "C" int mmdit_probe_attn_fwd_dbg(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale,
                                        void* Ox, void* Oc, float* lse, int dbg, mmdit_stream_t stream) {
#define MMDIT_DBG(D) case D: hipLaunchKernelGGL(attn_fwd_dma_kernel<D>, dim3(((S + 255) / 256) * batch * heads), dim3(512), 0, (hipStream_t)stream, (const bf16_t*)Q, \
                                                 (const bf16_t*)K, (const bf16_t*)V, batch * heads, heads, S, n_img, scale, (bf16_t*)Ox, (bf16_t*)Oc, lse); break;
  switch (dbg) {
    MMDIT_DBG(0) MMDIT_DBG(1) MMDIT_DBG(2) MMDIT_DBG(4) MMDIT_DBG(8) MMDIT_DBG(16) MMDIT_DBG(32) MMDIT_DBG(33) MMDIT_DBG(6) MMDIT_DBG(39) MMDIT_DBG(24) MMDIT_DBG(57) MMDIT_DBG(63) MMDIT_DBG(64) MMDIT_DBG(191) MMDIT_DBG(128)
    default: return MMDIT_ERR_ARG;
  }
#undef MMDIT_DBG
  return mmdit_launch_status();
}

#endif

#ifdef MMDIT_PROBES
// measurement aid (tools/probes/attn_bwd_trace.py; not declared in include/mmdit_hip.h): the dK/dV kernel (plain or fused epilogue) with per-phase
// cycle stamps, trace = 2048 workgroups x 8 waves x 72 slots of 8 bytes.  delta must already hold rowsum(dO * O) (run mmdit_attn_bwd first).
extern "C" int mmdit_probe_attn_bwd_dkv_trace(const void* Q, const void* K, const void* V, const void* dOx, const void* dOc, const float* lse, const float* delta,
                                              int batch, int heads, int S, int n_img, float scale, void* dK, void* dV, void* trace, mmdit_stream_t stream) {
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<8, bf16_t, false, true>), dim3(((S + 255) / 256) * batch * heads), dim3(512), 0, (hipStream_t)stream, (const bf16_t*)Q, (const bf16_t*)K,
                     (const bf16_t*)V, (const bf16_t*)dOx, (const bf16_t*)dOc, lse, delta, batch * heads, heads, S, n_img, scale, (bf16_t*)dK, (bf16_t*)dV, QkFuse(),
                     (unsigned long long*)trace);
  return mmdit_launch_status();
}
#endif

extern "C" int mmdit_attn_bwd_qk(const void* Q, const void* K, const void* V, const void* Ox, const void* Oc, const void* dOx, const void* dOc,
                                 const float* lse, float* delta, int batch, int heads, int S, int n_img, float scale,
                                 const void* qkv_x, const void* qkv_c, const float* wq_x, const float* wk_x, const float* wq_c, const float* wk_c,
                                 const float* rope_cos, const float* rope_sin, void* dqkv_x, void* dqkv_c, float* dw, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && Ox && dOx && lse && delta && batch > 0 && heads > 0 && S > 0 && n_img > 0 && n_img <= S);
  MMDIT_CHECK_ARG(Oc || n_img == S);
  MMDIT_CHECK_ARG(qkv_x && wq_x && wk_x && rope_cos && rope_sin && dqkv_x && dw && (n_img == S || (qkv_c && wq_c && wk_c && dqkv_c)));
  if (n_img % 32) return MMDIT_ERR_SHAPE;       // a wave's 32 rows must belong to one stream
  const QkFuse F{(const bf16_t*)qkv_x, (const bf16_t*)qkv_c, wq_x, wk_x, wq_c, wk_c, rope_cos, rope_sin, (bf16_t*)dqkv_x, (bf16_t*)dqkv_c, dw};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(((S + 255) / 256) * batch * heads);
  constexpr int lds = qk_lds_bytes<8>();        // 70144 B: above the 64 KB default cap of dynamic LDS
  static unsigned long long raised = 0;            // one bit per device (the attribute is a per-device property)
  if (!mmdit_device_once(raised)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_dq_kernel<8, bf16_t, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_dkv_kernel<8, bf16_t, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;             // (positive: a HIP error code, as from mmdit_launch_status)
    mmdit_device_mark(raised);
  }
  hipLaunchKernelGGL((attn_bwd_dq_kernel<8, bf16_t, true>), grid, dim3(512), lds, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V, (const bf16_t*)Ox,
                     (const bf16_t*)Oc, (const bf16_t*)dOx, (const bf16_t*)dOc, lse, delta, batch * heads, heads, S, n_img, scale, (bf16_t*)nullptr, F);
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<8, bf16_t, true>), grid, dim3(512), lds, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V, (const bf16_t*)dOx,
                     (const bf16_t*)dOc, lse, delta, batch * heads, heads, S, n_img, scale, (bf16_t*)nullptr, (bf16_t*)nullptr, F);
  return mmdit_launch_status();
}

extern "C" int mmdit_attn_bwd(const void* Q, const void* K, const void* V, const void* Ox, const void* Oc, const void* dOx, const void* dOc,
                              const float* lse, float* delta, int batch, int heads, int S, int n_img, float scale,
                              void* dQ, void* dK, void* dV, int dq_dtype, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && Ox && dOx && lse && delta && dQ && dK && dV && batch > 0 && heads > 0 && S > 0 && n_img > 0 && n_img <= S);
  MMDIT_CHECK_ARG(Oc || n_img == S);
  hipStream_t s = (hipStream_t)stream;
  // (delta = rowsum(dO * O) is produced by the dQ kernel, which runs first)
#define MMDIT_DKV(NW, TG) hipLaunchKernelGGL((attn_bwd_dkv_kernel<NW, TG>), dim3(((S + 32 * NW - 1) / (32 * NW)) * batch * heads), dim3(NW * 64), 0, s, (const bf16_t*)Q, (const bf16_t*)K, \
                                             (const bf16_t*)V, (const bf16_t*)dOx, (const bf16_t*)dOc, lse, delta, batch * heads, heads, S, n_img, scale, (TG*)dK, (TG*)dV)
#define MMDIT_DQ(NW, TG) hipLaunchKernelGGL((attn_bwd_dq_kernel<NW, TG>), dim3(((S + 32 * NW - 1) / (32 * NW)) * batch * heads), dim3(NW * 64), 0, s, (const bf16_t*)Q, (const bf16_t*)K, \
                                            (const bf16_t*)V, (const bf16_t*)Ox, (const bf16_t*)Oc, (const bf16_t*)dOx, (const bf16_t*)dOc, lse, delta, batch * heads, heads, S, n_img, scale, (TG*)dQ)
  if (dq_dtype == MMDIT_BF16) {
    MMDIT_DQ(8, bf16_t);
    MMDIT_DKV(8, bf16_t);
  } else if (dq_dtype == MMDIT_F32) {
    MMDIT_DQ(2, float);
    MMDIT_DKV(2, float);
  } else return MMDIT_ERR_DTYPE;
#undef MMDIT_DQ
#undef MMDIT_DKV
  return mmdit_launch_status();
}

// Joint attention whose keys and values have a length of their own (Attention.py:243-251, kv_merge_attn: adjacent keys / values of each stream
// averaged, S queries against s_kv = S / 2 keys).  Same kernels as above with the KVL flag: every key-side bound is s_kv, every query-side one
// S; with s_kv == S the results are those of mmdit_attn_fwd / mmdit_attn_bwd bit for bit (same arithmetic in the same order).
extern "C" int mmdit_attn_fwd_kv(const void* Q, const void* K, const void* V, int batch, int heads, int S, int s_kv, int n_img, float scale, int mode,
                                 void* Ox, void* Oc, float* lse, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && Ox && lse && batch > 0 && heads > 0 && S > 0 && n_img > 0 && n_img <= S);
  MMDIT_CHECK_ARG(Oc || n_img == S);
  MMDIT_CHECK_ARG(mode == 0 || mode == 1);
  if (s_kv < 1 || s_kv > S) return MMDIT_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (mode == 1)
    hipLaunchKernelGGL((attn_fwd_kernel<2, true, true>), dim3(((S + 63) / 64) * batch * heads), dim3(128), 0, s, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V,
                       batch * heads, heads, S, n_img, scale, (bf16_t*)Ox, (bf16_t*)Oc, lse, s_kv);
  else
    hipLaunchKernelGGL((attn_fwd_dma_kernel<0, false, 8, ANS, true>), dim3(((S + 255) / 256) * batch * heads), dim3(512), 0, s, (const bf16_t*)Q, (const bf16_t*)K,
                       (const bf16_t*)V, batch * heads, heads, S, n_img, scale, (bf16_t*)Ox, (bf16_t*)Oc, lse, (unsigned char*)nullptr, (unsigned char*)nullptr, s_kv);
  return mmdit_launch_status();
}

extern "C" int mmdit_attn_bwd_kv(const void* Q, const void* K, const void* V, const void* Ox, const void* Oc, const void* dOx, const void* dOc,
                                 const float* lse, float* delta, int batch, int heads, int S, int s_kv, int n_img, float scale,
                                 void* dQ, void* dK, void* dV, int dq_dtype, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && Ox && dOx && lse && delta && dQ && dK && dV && batch > 0 && heads > 0 && S > 0 && n_img > 0 && n_img <= S);
  MMDIT_CHECK_ARG(Oc || n_img == S);
  if (s_kv < 1 || s_kv > S) return MMDIT_ERR_SHAPE;
  if (dq_dtype != MMDIT_BF16 && dq_dtype != MMDIT_F32) return MMDIT_ERR_DTYPE;
  hipStream_t s = (hipStream_t)stream;
  // the dQ grid covers the S queries (and writes delta), the dK/dV grid the s_kv keys
#define MMDIT_BWD_KV(NW, TG)                                                                                                                                             \
  do {                                                                                                                                                                   \
    hipLaunchKernelGGL((attn_bwd_dq_kernel<NW, TG, false, true>), dim3(((S + 32 * NW - 1) / (32 * NW)) * batch * heads), dim3(NW * 64), 0, s, (const bf16_t*)Q,          \
                       (const bf16_t*)K, (const bf16_t*)V, (const bf16_t*)Ox, (const bf16_t*)Oc, (const bf16_t*)dOx, (const bf16_t*)dOc, lse, delta, batch * heads, heads, \
                       S, n_img, scale, (TG*)dQ, QkFuse(), s_kv);                                                                                                        \
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<NW, TG, false, false, true>), dim3(((s_kv + 32 * NW - 1) / (32 * NW)) * batch * heads), dim3(NW * 64), 0, s,                 \
                       (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V, (const bf16_t*)dOx, (const bf16_t*)dOc, lse, delta, batch * heads, heads, S, n_img, scale,   \
                       (TG*)dK, (TG*)dV, QkFuse(), (unsigned long long*)nullptr, s_kv);                                                                                  \
  } while (0)
  if (dq_dtype == MMDIT_BF16) MMDIT_BWD_KV(8, bf16_t);
  else MMDIT_BWD_KV(2, float);
#undef MMDIT_BWD_KV
  return mmdit_launch_status();
}
