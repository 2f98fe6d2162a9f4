// The eigblk_* chain (tridiagonalisation across workgroups, one launch per column, then
// eigblk_sturm; CLRSDP_EIG_BLK=1) against the one-CU eigmin_batched on a batch of random symmetric
// n x n blocks: time per batch (HIP events around the launches, best of 7, the input copied back
// before every run outside the timed events) at strips of R = 16 / 32 / 64 rows, the largest
// |lambda_min difference| against eigmin_batched relative to the Gershgorin radius of the block,
// and whether the three R give bitwise the same lambda_min.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 eig_blk_bench.hip -o ../../microbin/eig_blk_bench
//   microbin/eig_blk_bench words n batch        (words 1, 2 or 4)
//   microbin/eig_blk_bench attr                 (hipFuncGetAttributes of eigmin_batched<T>)
// eigmin_batched is timed only where its dynamic LDS request stays within the 64 KiB a kernel may
// ask for without the attribute (it sets none).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <cmath>
#include "../../clustered-low-rank-sdp-solver_amd/csrc/kernels_dense.h"
using namespace clrsdp;
using mw::dd;
using mw::qd;
#define CK(x) do{hipError_t e_=(x); if(e_!=hipSuccess){printf("HIP %s @%d\n",hipGetErrorString(e_),__LINE__); exit(1);} }while(0)

template <class P, class K>
float timeit(P prep, K k) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  prep();
  k();
  CK(hipDeviceSynchronize());
  float best = 1e30f;
  for (int rep = 0; rep < 7; ++rep) {
    float ms;
    prep();
    CK(hipEventRecord(e0));
    k();
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    best = fminf(best, ms * 1e3f);
  }
  return best;
}

template <class T, int R>
void run_chain(const EigBlkDesc<T>* ed, int nmat, int n, T* out, bool tri) {
  eigblk_amax<T, R><<<dim3((n + R - 1) / R, nmat), 64>>>(ed);
  eigblk_sym<T, R><<<dim3((n + R - 1) / R, nmat), 64>>>(ed);
  for (int k = 0; k + 2 < n; ++k)
    eigblk_col<T, R><<<dim3((n - k - 1 + R - 1) / R, nmat), 64, eigblk_col_lds<T>(n)>>>(ed, k);
  if (tri) eigblk_sturm<T, true><<<nmat, 512, eigblk_sturm_lds<T>(n, true)>>>(ed, out, R);
  else eigblk_sturm<T, false><<<nmat, 512, eigblk_sturm_lds<T>(n, false)>>>(ed, out, R);
}

template <class T>
void run(const char* name, int n, int nmat) {
  constexpr size_t LDS_MAX = 160 * 1024;
  const size_t nn = (size_t)n * n;
  std::vector<T> h(nn * nmat);
  srand(11);
  for (int b = 0; b < nmat; ++b)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i <= j; ++i) {
        // (a second limb 2^-60 below the first, so that the multi-word kernels carry full words)
        const T v = T((double)rand() / RAND_MAX - 0.5) + T(ldexp((double)rand() / RAND_MAX - 0.5, -60));
        h[b * nn + i + (size_t)j * n] = v;
        h[b * nn + j + (size_t)i * n] = v;
      }
  T *dA, *dW, *ws, *out;
  double* am;
  CK(hipMalloc(&dA, h.size() * sizeof(T)));
  CK(hipMalloc(&dW, h.size() * sizeof(T)));
  CK(hipMalloc(&ws, nmat * eigblk_ws_words(n) * sizeof(T)));
  CK(hipMalloc(&am, (size_t)nmat * ((n + 15) / 16) * sizeof(double)));
  CK(hipMalloc(&out, 4 * nmat * sizeof(T)));
  CK(hipMemset(out, 0, 4 * nmat * sizeof(T)));
  CK(hipMemcpy(dA, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  std::vector<MatDesc<T>> md(nmat);
  std::vector<EigBlkDesc<T>> eh(nmat);
  for (int b = 0; b < nmat; ++b) {
    md[b] = {dW + b * nn, n, n};
    eh[b] = {dW + b * nn, ws + b * eigblk_ws_words(n), am + (size_t)b * ((n + 15) / 16), n, n};
  }
  MatDesc<T>* dmd;
  EigBlkDesc<T>* ded;
  CK(hipMalloc(&dmd, nmat * sizeof(MatDesc<T>)));
  CK(hipMalloc(&ded, nmat * sizeof(EigBlkDesc<T>)));
  CK(hipMemcpy(dmd, md.data(), nmat * sizeof(MatDesc<T>), hipMemcpyHostToDevice));
  CK(hipMemcpy(ded, eh.data(), nmat * sizeof(EigBlkDesc<T>), hipMemcpyHostToDevice));
  if (eigblk_col_lds<T>(n) > LDS_MAX) {
    printf("%s n=%d: past eigblk_col's on-chip vectors\n", name, n);
    return;
  }
  const bool tri = eigblk_sturm_lds<T>(n, true) <= LDS_MAX;
  CK(hipFuncSetAttribute((const void*)eigblk_col<T, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
  CK(hipFuncSetAttribute((const void*)eigblk_col<T, 32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
  CK(hipFuncSetAttribute((const void*)eigblk_col<T, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
  CK(hipFuncSetAttribute((const void*)eigblk_sturm<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
  CK(hipFuncSetAttribute((const void*)eigblk_sturm<T, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
  auto prep = [&] { CK(hipMemcpy(dW, dA, h.size() * sizeof(T), hipMemcpyDeviceToDevice)); };
  const size_t lds = sizeof(T) * (4 * (size_t)n + 256);
  const bool fits = lds <= 64 * 1024;
  float tb = 0.f;
  if (fits) tb = timeit(prep, [&] { eigmin_batched<T><<<nmat, 256, lds>>>(dmd, out); });
  const float t16 = timeit(prep, [&] { run_chain<T, 16>(ded, nmat, n, out + nmat, tri); });
  const float t32 = timeit(prep, [&] { run_chain<T, 32>(ded, nmat, n, out + 2 * nmat, tri); });
  const float t64 = timeit(prep, [&] { run_chain<T, 64>(ded, nmat, n, out + 3 * nmat, tri); });
  std::vector<T> r(4 * nmat);
  CK(hipMemcpy(r.data(), out, r.size() * sizeof(T), hipMemcpyDeviceToHost));
  double diff = 0.0;
  int same = 1;
  for (int b = 0; b < nmat; ++b) {
    same &= !memcmp(&r[nmat + b], &r[2 * nmat + b], sizeof(T)) && !memcmp(&r[nmat + b], &r[3 * nmat + b], sizeof(T));
    double rad = 0.0;  // Gershgorin radius of the block
    for (int i = 0; i < n; ++i) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += fabs(Num<T>::hi(h[b * nn + i + (size_t)j * n]));
      rad = fmax(rad, s);
    }
    if (fits) diff = fmax(diff, fabs(Num<T>::hi(r[3 * nmat + b] - r[b])) / rad);
  }
  printf("{\"tool\": \"eig_blk_bench\", \"word\": \"%s\", \"n\": %d, \"batch\": %d, \"eigmin_batched_us\": %.1f, "
         "\"chain_R16_us\": %.1f, \"chain_R32_us\": %.1f, \"chain_R64_us\": %.1f, \"rel_diff_vs_batched\": %.2e, "
         "\"bitwise_same_across_R\": %d, \"lambda_min_block0\": %.17g}\n",
         name, n, nmat, tb, t16, t32, t64, fits ? diff : -1.0, same, Num<T>::hi(r[3 * nmat]));
  fflush(stdout);
}

// what the runtime reports for eigmin_batched<T> (no launch): static LDS and the dynamic limit
template <class T>
void attr(const char* name) {
  hipFuncAttributes fa;
  CK(hipFuncGetAttributes(&fa, (const void*)eigmin_batched<T>));
  const long lim = (long)fa.maxDynamicSharedSizeBytes, st = (long)fa.sharedSizeBytes;
  printf("{\"tool\": \"eig_blk_bench\", \"kernel\": \"eigmin_batched<%s>\", \"sharedSizeBytes\": %ld, "
         "\"maxDynamicSharedSizeBytes\": %ld, \"largest_n_within\": %ld}\n",
         name, st, lim, (lim / (long)sizeof(T) - 256) / 4);
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "attr")) {
    attr<double>("double");
    attr<dd>("mw::dd");
    attr<qd>("mw::qd");
    return 0;
  }
  const int words = argc > 1 ? atoi(argv[1]) : 1;
  const int n = argc > 2 ? atoi(argv[2]) : 160, nmat = argc > 3 ? atoi(argv[3]) : 2;
  if (n < 3 || n > 4096 || nmat < 1 || nmat > 64) {
    printf("usage: eig_blk_bench words n batch (3 <= n <= 4096, 1 <= batch <= 64)\n");
    return 1;
  }
  if (words == 1) run<double>("fp64", n, nmat);
  else if (words == 2) run<dd>("dd", n, nmat);
  else if (words == 4) run<qd>("qd", n, nmat);
  else return 1;
  return 0;
}
