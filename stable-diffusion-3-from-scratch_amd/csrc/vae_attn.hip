// Mid-block self-attention of the FLUX VAE for gfx950: ONE head of width 512, non-causal, forward only, the whole batch in one launch.
//
// Flash form of  O = softmax(scale * Q K^T) V  per image: no score matrix in memory, any token count.  Both products are issued
// "transposed" (as in attention.hip) so that a query is a lane column and the accumulator of the first product is the operand of the second:
//   S^T = K Q^T   v_mfma_f32_16x16x32_bf16, A = K rows from LDS (ds_read_b128), B = Q fragments resident in registers;
//                 lane (c = l & 15, g = l >> 4) holds keys 16 kb + 4 g + {0..3} of query c
//   O^T = V^T P^T A = V^T from the row-major [key][512] LDS tile through ds_read_b64_tr_b16, B = P^T = the 8 converted S^T registers of the
//                 lane (k slot j < 4: key 4 g + j, j >= 4: key 16 + 4 g + j - 4 -- the V^T reads reproduce that order by addressing)
// A wave owns 16 queries: O^T is 32 accumulators of 4 registers (128), Q 16 fragments of 4 (64) -- twice the rows would need 384 registers
// before any staging.  4 waves = 64 queries per workgroup; K and V tiles of 32 keys x 512 (32 KiB each) are double-buffered in LDS and
// filled by register-staged copies (K of tile t + 1 is in flight during the S^T MFMAs of tile t, V during the O^T MFMAs), one barrier per tile.
// Row pitch 1056 B (1024 + 32): the ds_read_b128 of a 16-row x 4-chunk K fragment and the transposed read of two 4-row x 32-byte V blocks
// per 32-lane half both land on distinct banks of the 256-byte bank row.
// Rounding points: fp32 scores, online softmax in the log2 domain, P rounded to bf16 for the MFMA, fp32 accumulation, the row sum in fp32
// from the unrounded P, one division at the end.  Deterministic: no atomics, no workspace.
#include "common.h"

namespace {

constexpr int VA_C = 512;                    // head width (elements)
constexpr int VA_KT = 32;                    // keys per LDS tile
constexpr int VA_NW = 4;                     // waves per workgroup
constexpr int VA_NT = 64 * VA_NW;
constexpr int VA_QB = 16 * VA_NW;            // queries per workgroup
constexpr int VA_PITCH = 1056;               // LDS row pitch in bytes
constexpr int VA_TILE = VA_KT * VA_PITCH;    // 33792
constexpr int VA_STAGE = 2 * VA_TILE;        // K tile + V tile
constexpr int VA_LDS = 2 * VA_STAGE;         // 135168 B of the 160 KiB
constexpr int VA_NCH = VA_KT * (VA_C / 8) / VA_NT;   // 16-byte chunks per thread and tile (8)
constexpr float VA_LOG2E = 1.4426950408889634f;

// [32 rows][512] bf16 tile, global -> registers: 8 unconditional 16-byte loads per thread.  Rows at or past `tokens` are read from the last
// valid row, so no load leaves the operand (a tile wholly past the end -- the prefetch of the last iteration -- is 32 copies of that row).
__device__ __forceinline__ void va_g2r(u32x4 (&st)[VA_NCH], const bf16_t* g, int64_t ld, int row0, int tokens, int tid) {
#pragma unroll
  for (int i = 0; i < VA_NCH; i++) {
    const int c = tid + i * VA_NT;
    st[i] = *(const u32x4*)(g + (int64_t)min(row0 + (c >> 6), tokens - 1) * ld + (c & 63) * 8);
  }
}
__device__ __forceinline__ void va_r2s(const u32x4 (&st)[VA_NCH], char* tile, int tid) {
#pragma unroll
  for (int i = 0; i < VA_NCH; i++) {
    const int c = tid + i * VA_NT;
    *LDS_PTR(u32x4, tile + (c >> 6) * VA_PITCH + (c & 63) * 16) = st[i];
  }
}
// V tile whose rows start at key row0: the rows at or past `tokens` are overwritten with zeros (by the thread that wrote them).  A masked
// key's V row must contribute exactly 0 whatever bits lie behind it: P = 0 times a non-finite V is NaN on the matrix pipe.
__device__ __forceinline__ void va_zero_tail(char* tile, int row0, int tokens, int tid) {
  if (row0 + VA_KT > tokens) {        // (workgroup-uniform: the partial tile only)
#pragma unroll
    for (int i = 0; i < VA_NCH; i++) {
      const int c = tid + i * VA_NT;
      if (row0 + (c >> 6) >= tokens) *LDS_PTR(u32x4, tile + (c >> 6) * VA_PITCH + (c & 63) * 16) = (u32x4){0, 0, 0, 0};
    }
  }
}

// grid = query blocks x batch, flattened.  Workgroup i runs on XCD i % 8 (private L2 each): with a batch that is a multiple of 8 all query
// blocks of one image are placed on one XCD, so its K / V come from HBM once instead of once per XCD (locality only).
__global__ __launch_bounds__(VA_NT) void vae_attn_fwd_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V, int ld, int batch,
                                                            int tokens, int nqb, float c, bf16_t* __restrict__ O) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int qb, b;
  {
    const int id = blockIdx.x;
    if (batch % 8 == 0) {
      const int j = id >> 3;
      qb = j % nqb;
      b = (j / nqb) * 8 + (id & 7);
    } else {
      qb = id % nqb;
      b = id / nqb;
    }
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qc = lane & 15, g = lane >> 4;
  const int64_t base = (int64_t)b * tokens;
  const bf16_t* Kb = K + base * ld;
  const bf16_t* Vb = V + base * ld;
  const int q0 = qb * VA_QB + wave * 16;

  // Q fragments (B operand): query qc, k = 32 ks + 8 g + {0..7}; a row past the end re-reads the last query and is not stored
  bf16x8 qf[16];
  {
    const bf16_t* qp = Q + (base + min(q0 + qc, tokens - 1)) * ld + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 16; ks++) {
      qf[ks] = *(const bf16x8*)(qp + 32 * ks);
      asm volatile("" : "+a"(qf[ks]));      // resident in the accumulation half of the register file (an MFMA takes its B operand from either half)
    }
  }
  f32x4 o[32];
#pragma unroll
  for (int db = 0; db < 32; db++) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;      // running maximum (log2 domain) of query qc; this lane's share of its row sum

  const int ntile = (tokens + VA_KT - 1) / VA_KT;
  u32x4 st[VA_NCH];
  va_g2r(st, Kb, ld, 0, tokens, tid);
  va_r2s(st, smem, tid);
  va_g2r(st, Vb, ld, 0, tokens, tid);
  va_r2s(st, smem + VA_TILE, tid);
  va_zero_tail(smem + VA_TILE, 0, tokens, tid);
  __syncthreads();

  const int koff = qc * VA_PITCH + g * 16;                                    // K fragment: row qc (+ 16 kb), chunk 4 ks + g
  const int voff = (4 * g + (qc >> 2)) * VA_PITCH + (qc & 3) * 8;             // V^T fragment: row 4 g + q (+ 16), columns 16 db + 4 p
  for (int t = 0; t < ntile; t++) {
    const char* kt = smem + (t & 1) * VA_STAGE;
    const char* vt = kt + VA_TILE;
    char* nk = smem + ((t + 1) & 1) * VA_STAGE;        // stage of tile t + 1: last read in iteration t - 1, which every wave left at its barrier
    // K of tile t + 1 is in flight during the S^T MFMAs, V during the O^T MFMAs, through the same 32 staging registers (both sets resident left no
    // register for a second LDS fragment in flight).  Unconditional: the loop body stays one basic block for the staging registers; after the last
    // tile it is a clamped, unused copy.
    va_g2r(st, Kb, ld, (t + 1) * VA_KT, tokens, tid);
    // S^T: two 16-key blocks, each as two independent accumulation chains (even / odd k steps)
    f32x4 sa[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int h = 0; h < 2; h++) sa[kb][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 16; ks++)
#pragma unroll
      for (int kb = 0; kb < 2; kb++)
        sa[kb][ks & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*LDS_PTR(const bf16x8, kt + koff + kb * 16 * VA_PITCH + ks * 64), qf[ks], sa[kb][ks & 1], 0, 0, 0);
    float s[8];
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int r = 0; r < 4; r++) s[kb * 4 + r] = sa[kb][0][r] + sa[kb][1][r];
    if ((t + 1) * VA_KT > tokens) {            // last, partial tile: keys past the end -> -inf
#pragma unroll
      for (int kb = 0; kb < 2; kb++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (t * VA_KT + kb * 16 + 4 * g + r >= tokens) s[kb * 4 + r] = -INFINITY;
    }
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 8; r++) mx = fmaxf(mx, s[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));     // the four lanes of a query
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * c;
    // the accumulators are rescaled only when some query's running maximum grows (exact: alpha == 1 otherwise)
    if (!__all(mx <= m)) {
      const float mn = fmaxf(m, mx);
      const float alpha = fast_exp2(m - mn);
      l *= alpha;
      m = mn;
#pragma unroll
      for (int db = 0; db < 32; db++) o[db] *= alpha;
    }
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      s[r] = fast_exp2(fmaf(s[r], c, -m));
      rs += s[r];
    }
    l += rs;
    const u32x4 pw = {pack_bf2(s[0], s[1]), pack_bf2(s[2], s[3]), pack_bf2(s[4], s[5]), pack_bf2(s[6], s[7])};
    const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
    va_r2s(st, nk, tid);
    va_g2r(st, Vb, ld, (t + 1) * VA_KT, tokens, tid);
    // O^T += V^T P^T
#pragma unroll
    for (int db = 0; db < 32; db++) {
      const char* p = vt + voff + db * 32;
      const s16x4 lo = lds_tr16(p), hi = lds_tr16(p + 16 * VA_PITCH);
      const s16x8 vr = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vr), pf, o[db], 0, 0, 0);
    }
    va_r2s(st, nk + VA_TILE, tid);
    va_zero_tail(nk + VA_TILE, (t + 1) * VA_KT, tokens, tid);
    __syncthreads();
  }

  // Epilogue.  The lane holds 4 consecutive features of query qc per accumulator: each wave stages its 16 x 512 bf16 block in LDS (idle
  // after the last barrier) and stores whole 1 KiB rows, 16 bytes per lane.
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.f / l;
  char* stg = smem + wave * 16 * VA_PITCH;
#pragma unroll
  for (int db = 0; db < 32; db++) {
    const u32x2 pk = {pack_bf2(o[db][0] * inv, o[db][1] * inv), pack_bf2(o[db][2] * inv, o[db][3] * inv)};
    *LDS_PTR(u32x2, stg + qc * VA_PITCH + db * 32 + g * 8) = pk;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const u32x4 v = *LDS_PTR(const u32x4, stg + r * VA_PITCH + lane * 16);
    if (q0 + r < tokens) *(u32x4*)(O + (base + q0 + r) * VA_C + lane * 8) = v;
  }
}

}  // namespace

extern "C" int mmdit_vae_attn_fwd(const void* Q, const void* K, const void* V, int ld, int batch, int tokens, int C, float scale, void* O_bf16, mmdit_stream_t stream) {
  if (C != VA_C || ld < VA_C || ld % 8 != 0 || tokens < 1) return MMDIT_ERR_SHAPE;
  MMDIT_CHECK_ARG(Q && K && V && O_bf16 && batch > 0 && scale > 0.f);
  MMDIT_CHECK_ARG((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)O_bf16) & 15) == 0);
  const int nqb = (tokens + VA_QB - 1) / VA_QB;
  MMDIT_CHECK_ARG((int64_t)nqb * batch <= 0x7fffffff);
  static unsigned long long raised = 0;            // one bit per device (the attribute is a per-device property)
  if (!mmdit_device_once(raised)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&vae_attn_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, VA_LDS);
    if (e != hipSuccess) return (int)e;
    mmdit_device_mark(raised);
  }
  hipLaunchKernelGGL(vae_attn_fwd_kernel, dim3(nqb * batch), dim3(VA_NT), VA_LDS, (hipStream_t)stream, (const bf16_t*)Q, (const bf16_t*)K, (const bf16_t*)V, ld, batch, tokens, nqb,
                     scale * VA_LOG2E, (bf16_t*)O_bf16);
  return mmdit_launch_status();
}
