// Joint [image;text] softmax attention forward for gfx950 with e4m3 operands on BOTH matrix products (mmdit_attn_fwd_e4m3,
// include/mmdit_hip_ext.h; reference call site Attention.py:266-293).  Head width 64, non-causal, forward only (inference: no lse).
// Q, K, V arrive as bf16 (B, H, S, 64), exactly as the QKV epilogue leaves them; they are quantised on the tiles as they are loaded --
// no calibration state, no extra pass over HBM, no persistent buffers.
//
// Orientation as in attention.hip: S^T = K Q^T and O^T = V^T P^T, so a query's softmax statistics live in one lane pair (l, l + 32) and the
// score accumulators are already the B operand of the second product.  Both products are ONE v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3
// operands, unit E8M0 block scales, fp32 accumulate) per 32 keys x 32 queries / 32 features x 32 queries: the 64-wide K of the instruction
// is the head width for K Q^T and the key tile for V^T P^T.
//
// Rounding points (tests/test_attn_e4m3_gpu.py restates them in float64).  pow2(a) below is the power of two 2^e with
// e = floor(log2(448 / a)), i.e. a * 2^e lies in (224, 448]; pow2(0) = 1.  Every conversion is round-to-nearest-even and saturates at +-448.
//   Q   one scale per query row:  q8[i][:] = e4m3(Q[i][:] * pow2(amax_d |Q[i][d]|))
//   K   one scale per key row:    k8[j][:] = e4m3(K[j][:] * pow2(amax_d |K[j][d]|))
//   s   s[i][j] = (sum_d q8[i][d] k8[j][d], exact products, fp32 accumulate) / (pow2_q[i] pow2_k[j]) * scale, fp32; keys past S are -inf
//       before the row maximum.  Online softmax in fp32 (log2 domain, v_exp_f32), exactly like the bf16 kernel: running maximum m,
//       l = sum_j p[i][j] of the UNROUNDED p = exp(s - m).
//   P   p8[i][j] = e4m3(256 * p[i][j]): the fixed factor 256 lets small probabilities use the format's range (256 p <= 256 needs no clamp);
//       it is carried by l as well (l sums 256 p), so it leaves with the final 1 / l.  p is relative to the RUNNING maximum of the tile in
//       which key j is visited, and the accumulator is rescaled in fp32 when the maximum grows.
//   V   one scale per 64-key tile t (keys 64 t .. 64 t + 63 of the (batch, head); rows past S count as zero):
//       v8[j][:] = e4m3(V[j][:] * pow2(amax_{j in t, d} |V[j][d]|))
//   O   o[i][:] += (sum_{j in t} p8[i][j] v8[j][:], fp32 accumulate) / pow2_v[t] per tile in fp32;  O[i][:] = bf16(o[i][:] / l[i]).
//       MX outputs: the bf16 O row re-quantised as mmdit_mxfp8_quantize does it (bit-identical to that pass on output (a)).
// Every scale is a power of two built from the amax's exponent field and applied with vector multiplies.
//
// Tiling: 4 waves = 128 queries per workgroup, 64-key tiles, register-staged double buffer (global -> VGPR -> quantise -> LDS).
//   K codes: row-major [key][64 B] (pitch 80), the MFMA's A fragment of key l & 31 is the 32 bytes d = 32 (l >> 5) ..; its de-quantisation
//            factors sit beside the tile as 64 floats.
//   V codes: transposed ON THE WAY INTO LDS, [feature][64 B] (pitch 80): a thread loads 4 consecutive keys x 4 features, converts, and
//            writes four dwords (4 keys of one feature each).  Key k of the tile sits at byte 32 g + 16 kb + 4 rg + (k & 3) with
//            kb = k >> 5, g = (k >> 2) & 1, rg = (k & 31) >> 3 -- the key order of the score accumulators (acc_row), so the 32 P codes a lane
//            packs from its two score blocks pair with the 32 V bytes of lane half g without any lane movement.
//   The V scale needs the tile's amax: the threads leave their partial maxima in LDS, one extra barrier per tile.
// Not tuned: no LDS-DMA ring (the tiles must pass through registers to be converted), two barriers per tile.
#include "common.h"
#include "../../include/mmdit_hip_ext.h"
#include "../../include/mmdit_hip_mxpad.h"

namespace {

constexpr int HD = 64;
constexpr int KT = MMDIT_ATTN_E4M3_KEY_TILE;      // keys per LDS tile
constexpr int NW = 4;                              // waves per workgroup
constexpr int QT = MMDIT_ATTN_E4M3_QUERY_TILE;    // queries per workgroup
constexpr int NT = NW * 64;
constexpr int PK = 80, PV = 80;                    // row pitches of the code tiles (64 B + 16)
constexpr int BUF = KT * PK + HD * PV + KT * 4;    // K codes, V^T codes, K de-quantisation factors
constexpr int UNIT = 0x7f7f7f7f;                   // E8M0 1.0 in every byte
constexpr float LOG2E = 1.4426950408889634f;
static_assert(QT == 32 * NW && KT == 64 && NT == 256, "thread -> tile element maps below");
static_assert(2 * BUF >= NW * 4096, "epilogue staging");

__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// 2^e with amax * 2^e in (224, 448] (e = floor(log2(448 / amax)): 8 - floor(log2 amax), one less when the mantissa exceeds 1.75), and 2^-e
__device__ __forceinline__ float pow2_scale(float amax, float& inv) {
  const unsigned bits = __float_as_uint(amax), ex = (bits >> 23) & 0xff;
  if (ex == 0) { inv = 1.f; return 1.f; }                                 // zero (or denormal) row
  int e = 8 - ((int)ex - 127) - ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  e = e < -126 ? -126 : (e > 126 ? 126 : e);
  inv = __uint_as_float((unsigned)(127 - e) << 23);
  return __uint_as_float((unsigned)(127 + e) << 23);
}
__device__ __forceinline__ float sat448(float x) { return fminf(fmaxf(x, -448.f), 448.f); }
// four fp32 -> four e4m3 codes (RNE, saturating), byte i = value i
__device__ __forceinline__ int e4m3x4(float a, float b, float c, float d) {
  int pk = __builtin_amdgcn_cvt_pk_fp8_f32(sat448(a), sat448(b), 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(sat448(c), sat448(d), pk, true);
}
__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// 1-D grid -> (query tile, batch * head): all tiles of one (batch, head) on one XCD (see map_block of attention.hip; locality only)
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

// MXO: outputs as MX e4m3 codes + E8M0 block scales (the layout mmdit_attn_fwd_mx writes) instead of bf16 rows
// PAD (MXO, odd H; include/mmdit_hip_mxpad.h): code rows of pitch H * 64 + 64; a token's 64 pad bytes (zero codes) and the scale bytes of
// its two pad blocks (0x00) are written by the workgroups of the LAST head for their own query rows -- one writer per pad byte
template <bool MXO, bool PAD = false>
__global__ __launch_bounds__(NT) void attn_fwd_e4m3_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                           int BH, int H, int S, int n_img, float scale,
                                                           bf16_t* __restrict__ Ox, bf16_t* __restrict__ Oc,
                                                           unsigned char* __restrict__ scx, unsigned char* __restrict__ scc) {
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  __shared__ float vmax[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, g = lane >> 5;
  int qtile, bh;
  map_block((S + QT - 1) / QT, BH, qtile, bh);
  const int h = bh % H;
  const int64_t b = bh / H;
  const bf16_t* Qb = Q + (int64_t)bh * S * HD;
  const bf16_t* Kb = K + (int64_t)bh * S * HD;
  const bf16_t* Vb = V + (int64_t)bh * S * HD;
  const int q = qtile * QT + wave * 32 + l31;
  const int qc = min(q, S - 1);                          // ragged query tile: clamped loads, guarded stores
  const bool active = qtile * QT + wave * 32 < S;        // wave-uniform: a wave of padding queries only helps with the tile copies

  // ---- Q: 32 features of the lane's query (d = 32 g ..), one scale per row
  i32x8 qf;
  float cq;                                              // 2^-eq * scale * log2(e): raw score -> scaled score in the log2 domain (times 2^-ek below)
  {
    u32x4 w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = *(const u32x4*)(Qb + (int64_t)qc * HD + g * 32 + i * 8);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int e = 0; e < 4; e++) amax = fmaxf(amax, fmaxf(fabsf(bf_lo(w[i][e])), fabsf(bf_hi(w[i][e]))));
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    float inv;
    const float sq = pow2_scale(amax, inv);
    cq = inv * scale * LOG2E;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int e = 0; e < 2; e++)
        qf[i * 2 + e] = e4m3x4(bf_lo(w[i][2 * e]) * sq, bf_hi(w[i][2 * e]) * sq, bf_lo(w[i][2 * e + 1]) * sq, bf_hi(w[i][2 * e + 1]) * sq);
  }

  // ---- tile staging: this thread's part of a K tile (row tid >> 2, 16 features) and of a V tile (4 keys x 4 features)
  const int krow = tid >> 2, kq = tid & 3;
  const int vkg = tid >> 4, vdc = tid & 15;
  u32x4 rk[2];
  u32x2 rv[4];
  auto g2r = [&](int j) {
    const int kr = j * KT + krow;
#pragma unroll
    for (int i = 0; i < 2; i++) rk[i] = kr < S ? *(const u32x4*)(Kb + (int64_t)kr * HD + kq * 16 + i * 8) : (u32x4){0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int vr = j * KT + vkg * 4 + i;
      rv[i] = vr < S ? *(const u32x2*)(Vb + (int64_t)vr * HD + vdc * 4) : (u32x2){0, 0};
    }
  };
  // quantise the staged tile into buffer `buf`; returns the tile's V de-quantisation factor.  Two barriers: the V amax, the finished tile.
  auto r2s = [&](int buf) -> float {
    char* kt = smem + buf * BUF;
    char* vt = kt + KT * PK;
    float* ksc = (float*)(vt + HD * PV);
    float vv[4][4];
    float va = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      vv[i][0] = bf_lo(rv[i][0]); vv[i][1] = bf_hi(rv[i][0]); vv[i][2] = bf_lo(rv[i][1]); vv[i][3] = bf_hi(rv[i][1]);
#pragma unroll
      for (int e = 0; e < 4; e++) va = fmaxf(va, fabsf(vv[i][e]));
    }
    va = wave_max(va);
    if (lane == 0) vmax[wave] = va;
    // K while the partial maxima travel
    float kv[16];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int e = 0; e < 4; e++) { kv[i * 8 + 2 * e] = bf_lo(rk[i][e]); kv[i * 8 + 2 * e + 1] = bf_hi(rk[i][e]); }
    float ka = 0.f;
#pragma unroll
    for (int e = 0; e < 16; e++) ka = fmaxf(ka, fabsf(kv[e]));
    ka = fmaxf(ka, __shfl_xor(ka, 1, 64));
    ka = fmaxf(ka, __shfl_xor(ka, 2, 64));
    float kinv;
    const float sk = pow2_scale(ka, kinv);
    u32x4 kc;
#pragma unroll
    for (int e = 0; e < 4; e++) kc[e] = (unsigned)e4m3x4(kv[4 * e] * sk, kv[4 * e + 1] * sk, kv[4 * e + 2] * sk, kv[4 * e + 3] * sk);
    *LDS_PTR(u32x4, kt + krow * PK + kq * 16) = kc;
    if (kq == 0) *LDS_PTR(float, ksc + krow) = kinv;
    __syncthreads();
    float ta = vmax[0];
#pragma unroll
    for (int w = 1; w < NW; w++) ta = fmaxf(ta, vmax[w]);
    float vinv;
    const float sv = pow2_scale(ta, vinv);
    // keys 4 vkg .. + 3 are four consecutive bytes of the permuted key order
    const int kpos = (vkg & 1) * 32 + (vkg >> 3) * 16 + ((vkg & 7) >> 1) * 4;
#pragma unroll
    for (int e = 0; e < 4; e++)
      *LDS_PTR(int, vt + (vdc * 4 + e) * PV + kpos) = e4m3x4(vv[0][e] * sv, vv[1][e] * sv, vv[2][e] * sv, vv[3][e] * sv);
    __syncthreads();
    return vinv;
  };

  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; db++)
#pragma unroll
    for (int r = 0; r < 16; r++) o[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int nkv = (S + KT - 1) / KT;
  constexpr f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  g2r(0);
  float dv = r2s(0);
  for (int j = 0; j < nkv; j++) {
    const int cur = j & 1;
    if (j + 1 < nkv) g2r(j + 1);
    if (active) {
      const char* kt = smem + cur * BUF;
      const char* vt = kt + KT * PK;
      const float* ksc = (const float*)(vt + HD * PV);
      f32x16 s[2];
#pragma unroll
      for (int kb = 0; kb < 2; kb++) {
        const char* kp = kt + (kb * 32 + l31) * PK + g * 32;
        const u32x4 lo = *LDS_PTR(const u32x4, kp), hi = *LDS_PTR(const u32x4, kp + 16);
        const i32x8 kf = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        s[kb] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(kf, qf, zero16, 0, 0, 0, UNIT, 0, UNIT);
        // de-quantise: the key's factor (4 consecutive keys per register group), then the query's with scale and log2(e)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const f32x4 ks = *LDS_PTR(const f32x4, ksc + kb * 32 + 8 * rg + 4 * g);
#pragma unroll
          for (int e = 0; e < 4; e++) s[kb][rg * 4 + e] = s[kb][rg * 4 + e] * ks[e] * cq;
        }
        if ((j + 1) * KT > S) {   // only the last (ragged) tile has keys to mask: wave-uniform branch
#pragma unroll
          for (int r = 0; r < 16; r++)
            if (j * KT + kb * 32 + acc_row(r, lane) >= S) s[kb][r] = -INFINITY;
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 2; kb++)
#pragma unroll
        for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[kb][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m, mx);
      const float alpha = fast_exp2(m - mn);
      const float sh = 8.f - mn;                         // p * 256
      float rs = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; kb++)
#pragma unroll
        for (int r = 0; r < 16; r++) { const float p = fast_exp2(s[kb][r] + sh); s[kb][r] = p; rs += p; }
      rs += __shfl_xor(rs, 32, 64);
      l = l * alpha + rs;
      m = mn;
      i32x8 pf;
#pragma unroll
      for (int kb = 0; kb < 2; kb++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {                  // 0 <= 256 p <= 256: inside the format, no clamp
          const int pk = __builtin_amdgcn_cvt_pk_fp8_f32(s[kb][rg * 4], s[kb][rg * 4 + 1], 0, false);
          pf[kb * 4 + rg] = __builtin_amdgcn_cvt_pk_fp8_f32(s[kb][rg * 4 + 2], s[kb][rg * 4 + 3], pk, true);
        }
#pragma unroll
      for (int db = 0; db < 2; db++) {
        const char* vp = vt + (db * 32 + l31) * PV + g * 32;
        const u32x4 lo = *LDS_PTR(const u32x4, vp), hi = *LDS_PTR(const u32x4, vp + 16);
        const i32x8 vf = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        const f32x16 t = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, zero16, 0, 0, 0, UNIT, 0, UNIT);
#pragma unroll
        for (int r = 0; r < 16; r++) o[db][r] = fmaf(t[r], dv, o[db][r] * alpha);
      }
    }
    if (j + 1 < nkv) dv = r2s(cur ^ 1);
  }
  __syncthreads();                                       // every wave has left the last tile: the buffers become the epilogue's staging

  // Epilogue, as attn_fwd_dma_kernel: each wave stages its 32 x 64 bf16 block through a private 4 KB (16-byte chunk c of row r at chunk
  // c ^ (r & 7)) and writes whole 128-byte rows; MXO re-quantises the bf16 row per 32-block (four adjacent lanes) on the way out.
  if (!active) return;
  {
    const float inv = 1.f / l;
    char* stg = smem + wave * 4096;
#pragma unroll
    for (int db = 0; db < 2; db++)
#pragma unroll
      for (int gg = 0; gg < 4; gg++) {
        const u32x2 pk = {pack_bf2(o[db][gg * 4] * inv, o[db][gg * 4 + 1] * inv), pack_bf2(o[db][gg * 4 + 2] * inv, o[db][gg * 4 + 3] * inv)};
        *LDS_PTR(u32x2, stg + l31 * 128 + (((db * 4 + gg) ^ (l31 & 7)) << 4) + g * 8) = pk;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private region: program order is enough
    const int n_txt = S - n_img, D = H * HD;
    const int rr = lane >> 3, rc = lane & 7;
#pragma unroll
    for (int it = 0; it < 4; it++) {
      const int r = it * 8 + rr, qq = qtile * QT + wave * 32 + r;
      const u32x4 t = *LDS_PTR(const u32x4, stg + r * 128 + ((rc ^ (r & 7)) << 4));
      const bool img = qq < n_img;
      const int64_t tok = img ? b * n_img + qq : b * n_txt + (qq - n_img);
      if constexpr (MXO) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; e++) { v[2 * e] = bf_lo(t[e]); v[2 * e + 1] = bf_hi(t[e]); }
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) amax = fmaxf(amax, fabsf(v[e]));
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));     // the 32-block: four 16-byte chunks = four adjacent lanes
        amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
        float minv;
        const int ex = mx_exponent(amax, minv);
        if (qq < S) {
          unsigned char* dst = (unsigned char*)(img ? Ox : Oc) + tok * (D + (PAD ? 64 : 0)) + h * HD + rc * 8;
          *(uint2*)dst = make_uint2(mx_pack4(v, minv), mx_pack4(v + 4, minv));
          if ((rc & 3) == 0) (img ? scx : scc)[mx_scale_index((int)tok, h * 2 + (rc >> 2), (BH / H) * (img ? n_img : n_txt))] = (unsigned char)(ex + 127);
          if constexpr (PAD) {
            if (h == H - 1) {      // (workgroup-uniform) lanes rc 0-3: the token's 64 pad bytes; rc 0 / 1: the scale bytes of its two pad blocks
              if (rc < 4) *(uint4*)((unsigned char*)(img ? Ox : Oc) + tok * (D + 64) + D + rc * 16) = make_uint4(0u, 0u, 0u, 0u);
              if (rc < 2) (img ? scx : scc)[mx_scale_index((int)tok, H * 2 + rc, (BH / H) * (img ? n_img : n_txt))] = 0;
            }
          }
        }
      } else if (qq < S) {
        *(u32x4*)((img ? Ox : Oc) + tok * D + h * HD + rc * 8) = t;
      }
    }
  }
}

}  // namespace

extern "C" int mmdit_attn_fwd_e4m3(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale,
                                   void* Ox, void* Oc, void* scales_x, void* scales_c, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && batch > 0 && heads > 0);
  if (S < 1 || n_img < 0 || n_img > S) return MMDIT_ERR_SHAPE;
  MMDIT_CHECK_ARG((Ox || n_img == 0) && (Oc || n_img == S));
  MMDIT_CHECK_ARG(!scales_x || scales_c || n_img == S);
  const int64_t blocks = (int64_t)((S + QT - 1) / QT) * batch * heads;
  // (MX scale rows are indexed with int: batch * tokens of a stream must fit)
  if (blocks > 0x7fffffff || (int64_t)batch * heads > 0x7fffffff || (int64_t)batch * S > 0x7fffffff) return MMDIT_ERR_SHAPE;
#define MMDIT_E4M3(...) hipLaunchKernelGGL((attn_fwd_e4m3_kernel<__VA_ARGS__>), dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, (const bf16_t*)Q, (const bf16_t*)K, \
                                           (const bf16_t*)V, batch * heads, heads, S, n_img, scale, (bf16_t*)Ox, (bf16_t*)Oc, (unsigned char*)scales_x, (unsigned char*)scales_c)
  if (scales_x) MMDIT_E4M3(true);
  else MMDIT_E4M3(false);
  return mmdit_launch_status();
}

// include/mmdit_hip_mxpad.h: the MX-output form of mmdit_attn_fwd_e4m3 with the code rows zero-padded to K_pad = heads * 64 rounded up to 128
// (an odd head count: the PAD instantiation; an even one: the plain launch, the same bytes)
extern "C" int mmdit_attn_fwd_e4m3_mx_pad(const void* Q, const void* K, const void* V, int batch, int heads, int S, int n_img, float scale,
                                          void* Ox_fp8, void* Oc_fp8, void* scales_x, void* scales_c, mmdit_stream_t stream) {
  MMDIT_CHECK_ARG(Q && K && V && batch > 0 && heads > 0);
  if (S < 1 || n_img < 1 || n_img > S) return MMDIT_ERR_SHAPE;
  MMDIT_CHECK_ARG(Ox_fp8 && scales_x && ((Oc_fp8 && scales_c) || n_img == S));
  const int64_t blocks = (int64_t)((S + QT - 1) / QT) * batch * heads;
  if (blocks > 0x7fffffff || (int64_t)batch * S * ((heads + 1) / 2 * 128 / 16) > 0x7fffffffll) return MMDIT_ERR_SHAPE;
  if (heads % 2 == 0) return mmdit_attn_fwd_e4m3(Q, K, V, batch, heads, S, n_img, scale, Ox_fp8, Oc_fp8, scales_x, scales_c, stream);
  void* Ox = Ox_fp8; void* Oc = Oc_fp8;
  MMDIT_E4M3(true, true);
#undef MMDIT_E4M3
  return mmdit_launch_status();
}
