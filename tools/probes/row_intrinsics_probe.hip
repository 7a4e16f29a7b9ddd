// Error of the fp32 intrinsics the row kernels (csrc/rowops.hip, csrc/common.h) lean on, each ALONE against float64 over the argument range of
// tests/test_rowops_edges_gpu.py (the row kernels under test are not involved):
//   cdf   1.f + erff(x * 0.70710678f)                 absolute error in units of 2^-23      x in [-12, 12] and +-20, +-100 (gelu_f / gelu_grad_f)
//   sigm  __builtin_amdgcn_rcpf(1.f + __expf(-x))     relative error / ((1 + |x|) 2^-23)    x in [-20, 20]                 (sigmoid_f: v_exp_f32, v_rcp_f32)
//   phi   __expf(-0.5f * x * x)                       relative error / ((1 + x^2 / 2) 2^-23) x in [-12, 12]                (gelu_grad_f: v_exp_f32)
//   rsq   rsqrtf(q)                                   relative error in units of 2^-24      q in [2^-20, 2^14]             (the norms: v_rsq_f32)
//   sin   sinf(x)                                     absolute error in units of 2^-24      x in [0, 1100]                 (time_embed_fwd / _bwd_kernel)
//   cos   cosf(x)                                     absolute error in units of 2^-24      x in [0, 1100]
// The GELU yardstick of the sweep takes twice the worst cdf figure (ERF_ABS); the other three are recorded next to the bounds derived for them;
// the time-embedding yardstick of tests/test_optim_edges_gpu.py takes twice the worse of the sin / cos figures (SINCOS_ABS).
//   hipcc --offload-arch=gfx950 -O3 -o row_intrinsics_probe row_intrinsics_probe.hip && ./row_intrinsics_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void k(const float* x, float* out, int n, int which) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  out[i] = which == 0 ? 1.f + erff(v * 0.70710678118654752440f) : which == 1 ? __builtin_amdgcn_rcpf(1.0f + __expf(-v)) : which == 2 ? __expf(-0.5f * v * v) : which == 3 ? rsqrtf(v)
           : which == 4 ? sinf(v) : cosf(v);
}

int main() {
  const int N = 1 << 22;
  std::vector<float> x(N + 4), y(N + 4);
  float *dx, *dy;
  if (hipMalloc(&dx, (N + 4) * 4) != hipSuccess || hipMalloc(&dy, (N + 4) * 4) != hipSuccess) { printf("no device memory\n"); return 1; }
  const char* names[6] = {"cdf   1 + erff(x / sqrt 2)      abs / 2^-23", "sigm  rcp(1 + exp(-x))         rel / ((1 + |x|) 2^-23)", "phi   exp(-x^2 / 2)            rel / ((1 + x^2 / 2) 2^-23)",
                          "rsq   rsqrtf(q)                rel / 2^-24", "sin   sinf(x)                  abs / 2^-24", "cos   cosf(x)                  abs / 2^-24"};
  for (int which = 0; which < 6; which++) {
    const double lo = which >= 4 ? 0.0 : which == 1 ? -20.0 : which == 3 ? -20.0 : -12.0, hi = which >= 4 ? 1100.0 : which == 1 ? 20.0 : which == 3 ? 14.0 : 12.0;
    for (int i = 0; i < N; i++) { const double t = lo + (hi - lo) * (i + 0.5) / N; x[i] = (float)(which == 3 ? exp2(t) : t); }
    const float extra[4] = {20.f, -20.f, 100.f, -100.f};
    const int n = which == 0 ? N + 4 : N;
    for (int i = 0; i < 4; i++) x[N + i] = extra[i];
    hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n, which);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
    hipMemcpy(y.data(), dy, n * 4, hipMemcpyDeviceToHost);
    double worst = 0, at = 0, sq = 0;
    for (int i = 0; i < n; i++) {
      const double v = x[i];
      double r;
      if (which == 0) r = fabs(y[i] - (1.0 + erf(v * 0.70710678118654752440))) / ldexp(1.0, -23);
      else if (which == 1) { const double t = 1.0 / (1.0 + exp(-v)); r = fabs(y[i] - t) / t / ((1 + fabs(v)) * ldexp(1.0, -23)); }
      else if (which == 2) { const double t = exp(-0.5 * v * v); r = fabs(y[i] - t) / t / ((1 + 0.5 * v * v) * ldexp(1.0, -23)); }
      else if (which == 3) { const double t = 1.0 / sqrt(v); r = fabs(y[i] - t) / t / ldexp(1.0, -24); }
      else r = fabs(y[i] - (which == 4 ? sin(v) : cos(v))) / ldexp(1.0, -24);
      sq += r * r;
      if (r > worst) { worst = r; at = v; }
    }
    printf("%s   worst %.4f at %.9g   rms %.4f   (%d points in [%g, %g]%s)\n", names[which], worst, at, sqrt(sq / n), n, which == 3 ? exp2(lo) : lo, which == 3 ? exp2(hi) : hi,
           which == 0 ? " and +-20, +-100" : "");
  }
  hipFree(dx); hipFree(dy);
  return 0;
}
