// chol_inv_tiles<128> on the XINV stage's batch at C3 (128 matrices of n = 128: X blocks, then Y
// blocks): the plain form against the form that also leaves A^-1 = L^-T L^-1 for the first half
// (the X blocks), time per launch (best of 10), and A^-1 against L^-T L^-1 formed on the host.
// Build twice for the tile map of A^-1: -DCLRSDP_SPDINV_W4=1 (default: its tiles on all seven
// workers) and =0 (none on worker 3, the wave that shares SIMD 0 with the chain wave).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form [-DCLRSDP_SPDINV_W4=0] \
//     spdinv_bench.hip -o ../../microbin/spdinv_bench && ../../microbin/spdinv_bench
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../clustered-low-rank-sdp-solver_amd/csrc/kernels_dense.h"
using namespace clrsdp;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP %s @%d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

template <bool SPD>
static float time_form(int nb, const MatDesc<double>* din, const MatDesc<double>* dout,
                       const MatDesc<double>* dg, int* info) {
  CK(hipFuncSetAttribute((const void*)chol_inv_tiles<128, SPD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                         (int)chol_inv_tiles_lds<128>()));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int rep = 0; rep < 11; ++rep) {
    CK(hipEventRecord(e0));
    chol_inv_tiles<128, SPD><<<nb, CholTiles<128>::NTH, chol_inv_tiles_lds<128>()>>>(din, dout, info, 1, dg);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (rep) best = fminf(best, ms * 1e3f);
  }
  CK(hipGetLastError());
  return best;
}

int main() {
  const int n = 128, nb = 128, ng = 64;
  std::vector<double> h((size_t)nb * n * n);
  srand(7);
  for (int b = 0; b < nb; ++b) {  // A = I + G G^T / n
    std::vector<double> G((size_t)n * n);
    for (auto& g : G) g = rand() / (double)RAND_MAX - 0.5;
    double* A = h.data() + (size_t)b * n * n;
    for (int j = 0; j < n; ++j)
      for (int i = j; i < n; ++i) {
        double s = i == j ? 1.0 : 0.0;
        for (int k = 0; k < n; ++k) s += G[i + (size_t)k * n] * G[j + (size_t)k * n] / n;
        A[i + (size_t)j * n] = A[j + (size_t)i * n] = s;
      }
  }
  double *dA, *dO, *dG;
  int* info;
  CK(hipMalloc(&dA, h.size() * 8));
  CK(hipMalloc(&dO, h.size() * 8));
  CK(hipMalloc(&dG, (size_t)ng * n * n * 8));
  CK(hipMalloc(&info, nb * 4));
  CK(hipMemcpy(dA, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  std::vector<MatDesc<double>> in(nb), out(nb), g(nb);
  for (int b = 0; b < nb; ++b) {
    in[b] = {dA + (size_t)b * n * n, n, n};
    out[b] = {dO + (size_t)b * n * n, n, n};
    g[b] = {b < ng ? dG + (size_t)b * n * n : nullptr, n, n};
  }
  MatDesc<double>*din, *dout, *dg;
  CK(hipMalloc(&din, nb * sizeof(MatDesc<double>)));
  CK(hipMalloc(&dout, nb * sizeof(MatDesc<double>)));
  CK(hipMalloc(&dg, nb * sizeof(MatDesc<double>)));
  CK(hipMemcpy(din, in.data(), nb * sizeof(MatDesc<double>), hipMemcpyHostToDevice));
  CK(hipMemcpy(dout, out.data(), nb * sizeof(MatDesc<double>), hipMemcpyHostToDevice));
  CK(hipMemcpy(dg, g.data(), nb * sizeof(MatDesc<double>), hipMemcpyHostToDevice));
  const float t0 = time_form<false>(nb, din, dout, nullptr, info);
  const float t1 = time_form<true>(nb, din, dout, dg, info);
  const float t2 = time_form<true>(nb, din, dout, nullptr, info);
  std::vector<double> X((size_t)n * n), Gd((size_t)n * n);
  double err = 0, asym = 0;
  for (int b = 0; b < 2; ++b) {
    CK(hipMemcpy(X.data(), dO + (size_t)b * n * n, (size_t)n * n * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(Gd.data(), dG + (size_t)b * n * n, (size_t)n * n * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double s = 0;
        for (int k = 0; k < n; ++k) s += X[k + (size_t)i * n] * X[k + (size_t)j * n];
        err = fmax(err, fabs(s - Gd[i + (size_t)j * n]));
        asym = fmax(asym, fabs(Gd[i + (size_t)j * n] - Gd[j + (size_t)i * n]));
      }
  }
  const bool bad = !(err < 1e-12) || asym != 0.0;
  printf("chol_inv_tiles<128> batch=%d W4=%d: plain %.1f us | with A^-1 for %d blocks %.1f us | A^-1 form, none asked %.1f us"
         " | max|G - X^T X| %.2e asym %.1e%s\n",
         nb, (int)CLRSDP_SPDINV_W4, t0, ng, t1, t2, err, asym, bad ? "  MISMATCH" : "");
  return bad;
}
