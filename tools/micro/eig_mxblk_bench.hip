// The mxblk route (CLRSDP_EIG_MX_BLK=1: fp64 eigblk_* chain, fp64 Cholesky chain, refinement at the
// word's width, then the flagged blocks by the replaced route) against the one-CU eigmin_batched
// and the multi-word eigblk_* chain (CLRSDP_EIG_BLK=1) on a batch of random symmetric n x n
// blocks, each through the library's own MatPlan<T>::eigmin (this file includes the library's
// translation unit, so the launch sequences are the library's): time per batch (HIP events
// around eigmin(), best of 7, the input copied back before every run outside the timed events),
// the route's split of its best run -- prepass + fp64 chain + Sturm step, factor, inverse
// iteration, refinement steps + flagged launch -- the number of flagged blocks, and the largest
// |lambda_min difference| against the multi-word chain relative to the block's Gershgorin radius.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form \
//         tools/micro/eig_mxblk_bench.hip -o microbin/eig_mxblk_bench -ldl
//   microbin/eig_mxblk_bench words n batch        (words 2 or 4)
// eigmin_batched is timed only where its dynamic LDS request stays within 64 KiB.
#include "../../clustered-low-rank-sdp-solver_amd/csrc/clrsdp.hip"

using namespace clrsdp;
#define CK(x) do{hipError_t e_=(x); if(e_!=hipSuccess){printf("HIP %s @%d\n",hipGetErrorString(e_),__LINE__); exit(1);} }while(0)

template <class T>
struct Timed {
  float us = 0.f, ph[4] = {0.f, 0.f, 0.f, 0.f};
};

template <class T>
Timed<T> timeit(MatPlan<T>& plan, T* dW, const T* dA, size_t bytes, T* out, bool phases) {
  hipEvent_t e0, e1, ph[3];
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (auto& e : ph) CK(hipEventCreate(&e));
  if (phases) plan.mx_phase_ev = ph;
  Timed<T> best;
  best.us = 1e30f;
  for (int rep = 0; rep < 8; ++rep) {  // (the first run warms up and is not counted)
    float ms;
    CK(hipMemcpy(dW, dA, bytes, hipMemcpyDeviceToDevice));
    CK(hipEventRecord(e0));
    plan.eigmin(nullptr, out);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (rep && ms * 1e3f < best.us) {
      best.us = ms * 1e3f;
      if (phases) {
        hipEvent_t seq[5] = {e0, ph[0], ph[1], ph[2], e1};
        for (int q = 0; q < 4; ++q) {
          CK(hipEventElapsedTime(&ms, seq[q], seq[q + 1]));
          best.ph[q] = ms * 1e3f;
        }
      }
    }
  }
  plan.mx_phase_ev = nullptr;
  return best;
}

template <class T>
void run(const char* name, int n, int nmat) {
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
  const size_t bytes = h.size() * sizeof(T);
  T *dA, *dW, *out;
  CK(hipMalloc(&dA, bytes));
  CK(hipMalloc(&dW, bytes));
  CK(hipMalloc(&out, 3 * nmat * sizeof(T)));
  CK(hipMemset(out, 0, 3 * nmat * sizeof(T)));
  CK(hipMemcpy(dA, h.data(), bytes, hipMemcpyHostToDevice));
  // (the two switches as given here; every other one as the environment has it)
  auto build = [&](MatPlan<T>& p, bool chain, bool mx) {
    Switches sw = Switches::read();
    sw.eig_blk = chain;
    sw.eig_mx_blk = mx;
    for (int b = 0; b < nmat; ++b) p.add(dW + b * nn, n, n);
    p.finalize(sw, MatPlan<T>::Use::EIG_ONLY);
  };
  MatPlan<T> pb, pc, pm;
  build(pb, false, false);
  build(pc, true, false);
  build(pm, false, true);
  if (pm.eig_k != CLRSDP_EIG_K_MXBLK) {
    printf("%s n=%d: outside the route's range\n", name, n);
    return;
  }
  const bool fits = MatPlan<T>::batched_lds(n) <= 64 * 1024;
  Timed<T> tb, tc, tm;
  if (fits) tb = timeit(pb, dW, dA, bytes, out, false);
  tc = timeit(pc, dW, dA, bytes, out + nmat, false);
  tm = timeit(pm, dW, dA, bytes, out + 2 * nmat, true);
  std::vector<T> r(3 * nmat);
  std::vector<int> redo(nmat);
  CK(hipMemcpy(r.data(), out, r.size() * sizeof(T), hipMemcpyDeviceToHost));
  CK(hipMemcpy(redo.data(), pm.redo, nmat * sizeof(int), hipMemcpyDeviceToHost));
  double diff = 0.0;
  int flagged = 0;
  for (int b = 0; b < nmat; ++b) {
    flagged += redo[b] != 0;
    double rad = 0.0;  // Gershgorin radius of the block
    for (int i = 0; i < n; ++i) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += fabs(Num<T>::hi(h[b * nn + i + (size_t)j * n]));
      rad = fmax(rad, s);
    }
    diff = fmax(diff, fabs(Num<T>::hi(r[2 * nmat + b] - r[nmat + b])) / rad);
  }
  printf("{\"tool\": \"eig_mxblk_bench\", \"word\": \"%s\", \"n\": %d, \"batch\": %d, \"eigmin_batched_us\": %.1f, "
         "\"chain_us\": %.1f, \"mxblk_us\": %.1f, \"mxblk_fp64_chain_us\": %.1f, \"mxblk_factor_us\": %.1f, "
         "\"mxblk_inverse_iteration_us\": %.1f, \"mxblk_refinement_us\": %.1f, \"flagged\": %d, "
         "\"rel_diff_vs_chain\": %.2e, \"lambda_min_block0\": %.17g}\n",
         name, n, nmat, tb.us, tc.us, tm.us, tm.ph[0], tm.ph[1], tm.ph[2], tm.ph[3], flagged, diff,
         Num<T>::hi(r[2 * nmat]));
  fflush(stdout);
}

int main(int argc, char** argv) {
  if (argc < 4) {
    printf("usage: eig_mxblk_bench words n batch\n");
    return 2;
  }
  const int words = atoi(argv[1]), n = atoi(argv[2]), nmat = atoi(argv[3]);
  try {
    if (words == 2) run<mw::dd>("dd", n, nmat);
    else if (words == 4) run<mw::qd>("qd", n, nmat);
    else { printf("words must be 2 or 4\n"); return 2; }
  } catch (const ClrsdpError& e) {
    printf("clrsdp error %d: %s\n", e.code, e.msg.c_str());
    return 1;
  }
  return 0;
}
