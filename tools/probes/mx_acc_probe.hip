// Accumulation error of ONE v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 operands, E8M0 block scales) on its 64 products against float64:
//   kappa = |D - (C + sum_k a_k b_k)| / (|C| + sum_k |a_k| |b_k|)
// per input family, worst and rms over 512 waves x 1024 outputs.  The e4m3 yardstick of tests/test_gemm_edges_gpu.py takes twice the worst
// figure as its accumulation coefficient (the GEMM kernels under test are not involved).  The operand and result layouts are checked first on
// small integers with block scales that vary along K (exact in any order): a wrong layout fails loudly instead of measuring nonsense.
//   hipcc --offload-arch=gfx950 -O3 -o mx_acc_probe mx_acc_probe.hip && ./mx_acc_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cmath>
#include <vector>
#include <random>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int W = 512;      // waves (independent 32 x 32 x 64 products) per family

// A, B: [W][32 rows][64 k] e4m3 codes; SA, SB: [W][32 rows][2 blocks] E8M0 bytes; C, D: [W][32 (A row)][32 (B row)]
__global__ void k(const unsigned char* A, const unsigned char* B, const unsigned char* SA, const unsigned char* SB, const float* C, float* D) {
  const int w = blockIdx.x, l = threadIdx.x, r = l & 31, g = l >> 5;
  // registers 0-3: k = 16 g + [0, 16), registers 4-7: k = 32 + 16 g + [0, 16) of row r (csrc/gemm_tile.h load_frag8)
  i32x8 a, b;
  for (int i = 0; i < 8; i++) {
    const int k0 = (i < 4 ? 0 : 32) + 16 * g + 4 * (i & 3);
    a[i] = *(const int*)(A + (w * 32 + r) * 64 + k0);
    b[i] = *(const int*)(B + (w * 32 + r) * 64 + k0);
  }
  // the scale of (row r, 32-block blk) comes from byte 0 of lane r + 32 blk
  const int sa = SA[(w * 32 + r) * 2 + g], sb = SB[(w * 32 + r) * 2 + g];
  // D[i][j], i = 8 (reg / 4) + 4 g + reg % 4 (row of the first operand), j = r (row of the second)
  f32x16 c;
  for (int i = 0; i < 16; i++) c[i] = C[(w * 32 + 8 * (i / 4) + 4 * g + i % 4) * 32 + r];
  c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, sa, 0, sb);
  for (int i = 0; i < 16; i++) D[(w * 32 + 8 * (i / 4) + 4 * g + i % 4) * 32 + r] = c[i];
}

static double e4m3_value(unsigned char c) {
  const int e = (c >> 3) & 15, m = c & 7;
  const double v = e ? ldexp(1.0 + m / 8.0, e - 7) : ldexp(m / 8.0, -6);
  return c & 0x80 ? -v : v;
}

static unsigned char e4m3_nearest(double x) {      // nearest code (ties: the smaller code), |x| clamped to 448
  unsigned char best = 0;
  double bd = 1e300;
  for (int c = 0; c < 0x7f; c++) { const double d = fabs(e4m3_value((unsigned char)c) - fabs(x)); if (d < bd) { bd = d; best = (unsigned char)c; } }
  return x < 0 ? best | 0x80 : best;
}

int main() {
  const size_t nA = (size_t)W * 32 * 64, nS = (size_t)W * 32 * 2, nC = (size_t)W * 32 * 32;
  std::vector<unsigned char> A(nA), B(nA), SA(nS), SB(nS);
  std::vector<float> C(nC), D(nC);
  unsigned char *dA, *dB, *dSA, *dSB; float *dC, *dD;
  hipMalloc(&dA, nA); hipMalloc(&dB, nA); hipMalloc(&dSA, nS); hipMalloc(&dSB, nS); hipMalloc(&dC, nC * 4); hipMalloc(&dD, nC * 4);
  std::mt19937 rng(1);
  std::normal_distribution<double> randn(0.0, 1.0);
  // family: 0 integers + varying scales + integer C (layout check, must be exact); 1 randn codes, unit scales, C = 0; 2 ... C = fp32 of the size of the
  // sum; 3 uniformly random codes (every exponent), unit scales; 4 randn codes, block scales 2^-8 .. 2^8, C = 0; 5 ... C of the size of the sum
  const char* names[6] = {"integers, scales 2^-2..2^2, integer C (layout check)", "randn codes, unit scales, C = 0", "randn codes, unit scales, C ~ the sum",
                          "uniform random codes, unit scales, C = 0", "randn codes, block scales 2^-8..2^8, C = 0", "randn codes, block scales 2^-8..2^8, C ~ the sum"};
  double overall = 0.0;
  for (int fam = 0; fam < 6; fam++) {
    for (size_t i = 0; i < nA; i++) {
      if (fam == 0) { A[i] = e4m3_nearest((int)(rng() % 7) - 3); B[i] = e4m3_nearest((int)(rng() % 7) - 3); }
      else if (fam == 3) { do { A[i] = rng() & 0xff; } while ((A[i] & 0x7f) == 0x7f); do { B[i] = rng() & 0xff; } while ((B[i] & 0x7f) == 0x7f); }
      else { A[i] = e4m3_nearest(64.0 * randn(rng)); B[i] = e4m3_nearest(64.0 * randn(rng)); }
    }
    for (size_t i = 0; i < nS; i++) {
      const int span = fam == 0 ? 2 : fam >= 4 ? 8 : 0;
      SA[i] = 127 + (span ? (int)(rng() % (2 * span + 1)) - span : 0);
      SB[i] = 127 + (span ? (int)(rng() % (2 * span + 1)) - span : 0);
    }
    std::vector<double> ref(nC), mag(nC);
    for (int w = 0; w < W; w++) for (int i = 0; i < 32; i++) for (int j = 0; j < 32; j++) {
      double s = 0, m = 0;
      for (int kk = 0; kk < 64; kk++) {
        const double p = e4m3_value(A[(w * 32 + i) * 64 + kk]) * ldexp(1.0, SA[(w * 32 + i) * 2 + kk / 32] - 127) *
                         e4m3_value(B[(w * 32 + j) * 64 + kk]) * ldexp(1.0, SB[(w * 32 + j) * 2 + kk / 32] - 127);
        s += p; m += fabs(p);
      }
      const size_t o = ((size_t)w * 32 + i) * 32 + j;
      C[o] = fam == 0 ? (float)((int)(rng() % 2001) - 1000) : (fam == 2 || fam == 5) ? (float)(m / 8.0 * randn(rng)) : 0.f;      // (sqrt(64) = 8: the size of the sum)
      ref[o] = s + (double)C[o]; mag[o] = m + fabs((double)C[o]);
    }
    hipMemcpy(dA, A.data(), nA, hipMemcpyHostToDevice); hipMemcpy(dB, B.data(), nA, hipMemcpyHostToDevice);
    hipMemcpy(dSA, SA.data(), nS, hipMemcpyHostToDevice); hipMemcpy(dSB, SB.data(), nS, hipMemcpyHostToDevice);
    hipMemcpy(dC, C.data(), nC * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(W), dim3(64), 0, 0, dA, dB, dSA, dSB, dC, dD);
    if (hipMemcpy(D.data(), dD, nC * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); return 1; }
    double worst = 0, sq = 0;
    size_t wrong = 0;
    for (size_t o = 0; o < nC; o++) {
      const double e = fabs((double)D[o] - ref[o]), kap = mag[o] > 0 ? e / mag[o] : (e > 0 ? 1e30 : 0.0);
      worst = kap > worst ? kap : worst; sq += kap * kap; wrong += e != 0;
    }
    printf("family %d (%s): kappa worst %.4e = 2^%.2f, rms %.4e, %zu of %zu outputs inexact\n", fam, names[fam], worst, worst > 0 ? log2(worst) : -999.0,
           sqrt(sq / nC), wrong, nC);
    if (fam == 0 && wrong) { printf("LAYOUT CHECK FAILED: the integer family must be exact\n"); return 2; }
    if (fam) overall = worst > overall ? worst : overall;
  }
  printf("kappa (worst over the families 1-5) = %.4e; twice that = %.4e = %.1f x 2^-23\n", overall, 2 * overall, 2 * overall * 8388608.0);
  return 0;
}
