// clrsdp.hip -- device-resident interior-point iteration behind the C ABI of include/clrsdp.h.
//
// One process drives one GPU.  The handle owns every device buffer; constraint data is uploaded
// once and stays resident.  A loop body of solverank1sdp (MPMP.jl:755-887) is a fixed sequence
// of batched launches on one stream (see DESIGN.md for the stage -> kernel table); the only
// host synchronisation is the final read-back of the iteration statistics.  With
// world_size > 1 each rank owns a subset of clusters and the few cross-cluster quantities (Q,
// the n_y-vectors p and sum_j B_j^T S_j^-1 r_j, and ~10 scalars) are all-gathered through the
// registered exchange and reduced in rank order, so every rank computes identical y, dy, alpha.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <string>
#include <array>
#include <vector>

#include "../../include/clrsdp.h"
#include "kernels.h"
#include "kernels_dense.h"

using namespace clrsdp;
using mw::dd;
using mw::qd;
using mw::Num;

namespace {

std::string g_last_error;

struct ClrsdpError {
  int code;
  std::string msg;
};

// (the runtime also keeps a failed call's code for the thread's next hipGetLastError(); it is
// reported here, so it is cleared here: the launch check of a later, good call must not find it)
#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      (void)hipGetLastError();                                                      \
      throw ClrsdpError{CLRSDP_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)}; \
    }                                                                               \
  } while (0)

// zero-filled device allocation; the fill is complete on return (null stream, synchronised:
// no caller has to order it against its own non-blocking streams)
template <class X>
X* dmalloc(size_t n) {
  if (n == 0) n = 1;
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, n * sizeof(X)));
  HIPCHK(hipMemsetAsync(p, 0, n * sizeof(X), nullptr));
  HIPCHK(hipStreamSynchronize(nullptr));
  return reinterpret_cast<X*>(p);
}

// the calling thread's current device, set for the scope and restored after (the C ABI's calls
// are made from threads that may drive other devices)
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) {
      prev = -1;
      (void)hipGetLastError();
    }
    if (prev != dev) HIPCHK(hipSetDevice(dev));
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// ---------------- RCCL, loaded at run time (the library itself has no link dependency on it,
// so a single-GPU or CPU-side user never needs librccl).  Only the five entry points the
// exchange uses are resolved.
struct Rccl {
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
  decltype(&ncclCommCount) comm_count = nullptr;
};

const Rccl& rccl() {
  static Rccl api;
  static bool tried = false;
  static std::string why;
  if (!tried) {
    tried = true;
    void* so = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if ((so = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!so) {
      why = std::string("cannot load librccl: ") + dlerror();
    } else {
      api.get_unique_id = reinterpret_cast<decltype(api.get_unique_id)>(dlsym(so, "ncclGetUniqueId"));
      api.comm_init_rank = reinterpret_cast<decltype(api.comm_init_rank)>(dlsym(so, "ncclCommInitRank"));
      api.all_gather = reinterpret_cast<decltype(api.all_gather)>(dlsym(so, "ncclAllGather"));
      api.comm_destroy = reinterpret_cast<decltype(api.comm_destroy)>(dlsym(so, "ncclCommDestroy"));
      api.error_string = reinterpret_cast<decltype(api.error_string)>(dlsym(so, "ncclGetErrorString"));
      api.comm_count = reinterpret_cast<decltype(api.comm_count)>(dlsym(so, "ncclCommCount"));
      if (!api.get_unique_id || !api.comm_init_rank || !api.all_gather || !api.comm_destroy ||
          !api.error_string) {
        api = Rccl{};
        why = "librccl lacks an nccl* entry point";
      }
    }
  }
  if (!api.all_gather) throw ClrsdpError{CLRSDP_E_EXCHANGE, why};
  return api;
}

#define RCCLCHK(x)                                                                       \
  do {                                                                                   \
    ncclResult_t r_ = (x);                                                               \
    if (r_ != ncclSuccess)                                                               \
      throw ClrsdpError{CLRSDP_E_EXCHANGE, std::string(#x) + ": " + rccl().error_string(r_)}; \
  } while (0)

template <class X>
X* upload_vec(const std::vector<X>& v) {
  X* p = dmalloc<X>(v.size());
  if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(X), hipMemcpyHostToDevice));
  return p;
}

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the current device only: `seen` is
// the caller's per-kernel bitmask of the devices it was already set on
inline void lds_attr_once(std::atomic<unsigned long long>& seen, const void* fn, int bytes) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  const unsigned long long bit = 1ull << (dev & 63);
  if (seen.load(std::memory_order_acquire) & bit) return;
  HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  seen.fetch_or(bit, std::memory_order_acq_rel);
}

// --------------------------------------------------------------------------------------------
// launch plans: descriptor arrays built once at creation, replayed every iteration
// --------------------------------------------------------------------------------------------
// a development switch is on when set to anything but a value starting with '0' (so that
// NAME=0 switches it off again, for every switch alike); *set, when given, tells whether it is
// set at all
static inline bool env_on(const char* name, bool* set = nullptr) {
  const char* e = std::getenv(name);
  if (set) *set = e != nullptr;
  return e && e[0] != '0';
}
// a default-on switch is off only when set to a value starting with '0'
static inline bool env_off(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '0';
}
// an integer switch: `dflt` when unset, else the decimal number its value starts with (0 when it
// starts with none); *exact, when given, tells whether the whole value was that number
static inline long env_int(const char* name, long dflt, bool* exact = nullptr) {
  const char* e = std::getenv(name);
  if (exact) *exact = true;
  if (!e) return dflt;
  char* end = nullptr;
  const long v = std::strtol(e, &end, 10);
  if (exact) *exact = end != e && *end == '\0';
  return v;
}

// The development switches as one value: a field per switch, at its default
// until read() fills it from the environment.  That happens when a handle is created, when a
// handle first builds its LU plans and at the top of each stand-alone call; the plans take what
// they need from the value they are handed, so no captured loop body can change route behind it.
struct Switches {
  // three-state: -1 unset, 0 off, 1 on
  int chain = -1, lu_blk = -1, potrf_blk = -1, schur_fused = -1, schur_fused_one = -1, trsm_blk = -1;
  // off unless set (to anything not starting with '0')
  bool chol256 = false, cl_solve = false, eig_blk = false, eig_mx_blk = false, eigmx_stats = false,
       graph_mw = false, graph_rccl = false, no_graph = false, inject_capture_fail = false,
       xy_overlap = false;
  // on unless set to a value starting with '0'
  bool chol_spdinv = true, eig_mx = true, lu_panel_lds = true, mw_pair_upper = true, ozaki = true,
       qchol_main = true, seam_pub = true, schur_fused_d64 = true, schur_fused_y = true,
       schur_grp2 = true;
  long gemm_ts32_below = 192, trsm_kb = 128;
  // chol_lookahead's option bits (kernels_dense.h).  Default 2: one Newton step for the
  // quad-double pivot reciprocal (~2^-208 relative; the second step was a third of the chain:
  // C5 879 -> 930 it/s, round 5 A/B); bit 0 (chain priority) measured nothing.  Only bits 0 and 1
  // exist; any other value (not a number, other bits) is rejected with a message, once per
  // process, and the default kept.
  int la_opts = 2;
  // the mxblk route of MatPlan::eigmin is off with CLRSDP_EIG_MX=0, as every refined-eigenpair route
  bool mxblk() const { return eig_mx_blk && eig_mx; }

  static Switches read() {
    Switches s;
    bool set = false;
    s.chain = env_on("CLRSDP_CHAIN", &set) ? 1 : set ? 0 : -1;
    s.chol256 = env_on("CLRSDP_CHOL256");
    s.chol_spdinv = !env_off("CLRSDP_CHOL_SPDINV");
    s.cl_solve = env_on("CLRSDP_CL_SOLVE");
    s.eig_blk = env_on("CLRSDP_EIG_BLK");
    s.eig_mx_blk = env_on("CLRSDP_EIG_MX_BLK");
    s.eig_mx = !env_off("CLRSDP_EIG_MX");
    s.eigmx_stats = env_on("CLRSDP_EIGMX_STATS");
    s.gemm_ts32_below = env_int("CLRSDP_GEMM_TS32_BELOW", s.gemm_ts32_below);
    s.graph_mw = env_on("CLRSDP_GRAPH_MW");
    s.graph_rccl = env_on("CLRSDP_GRAPH_RCCL");
    s.no_graph = env_on("CLRSDP_NO_GRAPH");
    s.inject_capture_fail = env_on("CLRSDP_INJECT_CAPTURE_FAIL");
    const long la = env_int("CLRSDP_LA_OPTS", s.la_opts, &set);  // (set: the value is a number)
    static std::atomic<bool> told{false};
    if (set && la >= 0 && !(la & ~3L)) s.la_opts = (int)la;
    else if (!told.exchange(true))
      std::fprintf(stderr, "clrsdp: CLRSDP_LA_OPTS ignored (a number with bits 0 and 1 only); using 2\n");
    s.lu_blk = env_on("CLRSDP_LU_BLK", &set) ? 1 : set ? 0 : -1;
    s.lu_panel_lds = !env_off("CLRSDP_LU_PANEL_LDS");
    s.mw_pair_upper = !env_off("CLRSDP_MW_PAIR_UPPER");
    s.ozaki = !env_off("CLRSDP_OZAKI");
    s.potrf_blk = env_on("CLRSDP_POTRF_BLK", &set) ? 1 : set ? 0 : -1;
    s.qchol_main = !env_off("CLRSDP_QCHOL_MAIN");
    s.seam_pub = !env_off("CLRSDP_SEAM_PUB");
    s.schur_fused = env_on("CLRSDP_SCHUR_FUSED", &set) ? 1 : set ? 0 : -1;
    s.schur_fused_one = env_on("CLRSDP_SCHUR_FUSED_ONE", &set) ? 1 : set ? 0 : -1;
    s.schur_fused_d64 = !env_off("CLRSDP_SCHUR_FUSED_D64");
    s.schur_fused_y = !env_off("CLRSDP_SCHUR_FUSED_Y");
    s.schur_grp2 = !env_off("CLRSDP_SCHUR_GRP2");
    s.trsm_blk = env_on("CLRSDP_TRSM_BLK", &set) ? 1 : set ? 0 : -1;
    s.trsm_kb = env_int("CLRSDP_TRSM_KB", s.trsm_kb);
    s.xy_overlap = env_on("CLRSDP_XY_OVERLAP");
    return s;
  }
};
// the largest block of the on-chip factorisation path (L^-1 and products instead of solves):
// chol_inv_tiles (fp64) and chol_lookahead with the inverse (multi-word)
template <class T> constexpr int reg_nmax() {
  return std::is_same<T, double>::value ? 128 : std::is_same<T, dd>::value ? 64 : 32;
}
// eigmin_lds: A (n^2), v, NC = 8 (n <= 64) or 4 partial vectors, dg, e2, w, scalars
template <class T> size_t eig_lds_bytes(int n) {
  return sizeof(T) * ((size_t)n * n + (n <= 64 ? 14 : 10) * (size_t)n + 40);
}
constexpr size_t LDS_MAX = 160 * 1024;

// workgroup order for a batched launch: tile-major, problem fastest (see TileRef)
inline std::vector<TileRef> tile_major(const std::vector<int>& ntiles) {
  std::vector<TileRef> out;
  int mx = 0;
  for (int n : ntiles) mx = std::max(mx, n);
  for (int t = 0; t < mx; ++t)
    for (size_t p = 0; p < ntiles.size(); ++p)
      if (t < ntiles[p]) out.push_back(TileRef{(int)p, t});
  return out;
}

// work enqueued on another stream for one scope: `stream` is restored when the scope ends,
// also when a launch inside throws (a capture-abort path relies on `stream` being the main one)
struct StreamSwitch {
  hipStream_t& cur;
  hipStream_t saved;
  StreamSwitch(hipStream_t& c, hipStream_t to) : cur(c), saved(c) { cur = to; }
  ~StreamSwitch() { cur = saved; }
  StreamSwitch(const StreamSwitch&) = delete;
  StreamSwitch& operator=(const StreamSwitch&) = delete;
};

// work that one stream produces for another: an event and "somebody still has to wait for it".
// The Solver lists its hand-offs once (Solver::handoffs); creation, destruction, the drain at the
// end of a loop body and reset_body_state() walk that list
struct Handoff {
  hipEvent_t ev = nullptr;
  bool on = false;
  void create() { HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); }
  void destroy() {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
  }
  void signal(hipStream_t producer) {
    HIPCHK(hipEventRecord(ev, producer));
    on = true;
  }
  // wait: the consumer waits if armed, and a later consumer on another stream still will
  void wait(hipStream_t consumer) const {
    if (on) HIPCHK(hipStreamWaitEvent(consumer, ev, 0));
  }
  void join(hipStream_t consumer) {  // the last (usually the only) consumer
    wait(consumer);
    on = false;
  }
  void disarm() { on = false; }
  bool armed() const { return on; }
};

// the plans own their device descriptor arrays (freed with the plan; plans are never copied)
struct PlanBase {
  std::vector<void*> owned_dev;
  PlanBase() = default;
  PlanBase(const PlanBase&) = delete;
  PlanBase& operator=(const PlanBase&) = delete;
  ~PlanBase() {
    for (void* p : owned_dev) (void)hipFree(p);
  }
  template <class X>
  X* own(const std::vector<X>& v) {
    X* p = upload_vec(v);
    owned_dev.push_back(p);
    return p;
  }
};

template <class T>
struct GemmPlan : PlanBase {
  bool ta = false, tb = false;
  int tag = 0;  // 1: the Schur-stage V^T X^-1 / V^T Y launch (named separately in profiles)
  unsigned long long* stamp = nullptr;  // tag 1: earliest workgroup start (SCHUR timing)
  std::vector<GemmDesc<T>> h;
  std::vector<int> ntiles;  // per problem
  std::vector<TileRef> t2d;
  GemmDesc<T>* d = nullptr;
  TileRef* dt = nullptr;
  // gemm_f64_lds (fp64) and gemm_valu_ks (multi-word) output tiles
  static constexpr int TILE = std::is_same<T, double>::value ? 64 : 8;

  void clear() {  // back to an empty plan (a failed build_lu_plans)
    h.clear();
    ntiles.clear();
    t2d.clear();
    d = nullptr;
    dt = nullptr;
  }
  void add(const T* A, int lda, const T* B, int ldb, const T* Cin, int ldcin, T* C, int ldc, int M,
           int N, int K) {
    if (M <= 0 || N <= 0) return;
    GemmDesc<T> g;
    g.A = A; g.B = B; g.Cin = Cin; g.C = C;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldcin = ldcin; g.ldc = ldc;
    g.tn = cdiv(N, TILE);
    g.tile0 = 0;
    g.flags = 0;
    g.alpha = g.beta = 0.0;
    g.sa = g.sl = nullptr;
    ntiles.push_back((int)(cdiv(M, TILE) * g.tn));
    h.push_back(g);
  }
  // sca: op(A) = A with column k scaled by sa[k] * sl[k] (fp64, NT: the weighted-A products)
  bool sca = false;
  void add_scaled(const T* A, int lda, const T* B, int ldb, const T* Cin, int ldcin, T* C, int ldc,
                  int M, int N, int K, const T* sa, const T* sl) {
    if (M <= 0 || N <= 0) return;
    sca = true;
    add(A, lda, B, ldb, Cin, ldcin, C, ldc, M, N, K);
    h.back().sa = sa;
    h.back().sl = sl;
  }
  // dyn: a mixed batch (fp64): op(A), op(B), alpha and beta per problem (gemm_f64_dyn)
  bool dyn = false;
  void add_op(bool opa, bool opb, double al, double be, const T* A, int lda, const T* B, int ldb,
              const T* Cin, int ldcin, T* C, int ldc, int M, int N, int K) {
    if (M <= 0 || N <= 0) return;
    dyn = true;
    add(A, lda, B, ldb, Cin, ldcin, C, ldc, M, N, K);
    h.back().flags = (opa ? 1 : 0) | (opb ? 2 : 0) | 4;
    h.back().alpha = al;
    h.back().beta = be;
  }
  bool gemv = false;
  // sym: every problem square with an exactly symmetric result wanted (gemm_f64_lds SYM: the
  // lower tiles only, each written with its mirror image); fp64, beta = 0
  bool sym = false;
  // upper (multi-word, round 6): every problem square with a symmetric product of which only the
  // tiles on and above the diagonal are wanted (the Schur pairings V^T X^-1 V, V^T Y V of m = 1
  // blocks: schur_assemble reads (min, max)); the launch lists those tiles only -- half the
  // VALU-bound multi-word work
  bool upper = false;
  void finalize(const Switches& sw) {
    if (h.empty()) return;
    if (sca && (ta || !tb || !std::is_same<T, double>::value))
      throw ClrsdpError{CLRSDP_E_ARG, "scaled-A GEMM: fp64 A B^T only"};
    gemv = !dyn && !sca;  // (a mixed or scaled batch always takes the tiled kernel)
    for (const auto& g : h) gemv = gemv && g.N == 1;
    // op(B) = B^T of a 1 x K row is the gemv vector only for K = 1 (e.g. all blocks 1 x 1)
    if (gemv && tb)
      for (const auto& g : h) gemv = gemv && g.K == 1;
    if (gemv) sym = false;  // a product with one column is 1 x 1 when square: trivially symmetric
    if (gemv)  // one workgroup per 64 outputs
      for (size_t q = 0; q < h.size(); ++q) ntiles[q] = (int)cdiv(h[q].M, 64);
    if (dyn && (gemv || sym || !std::is_same<T, double>::value))
      throw ClrsdpError{CLRSDP_E_ARG, "mixed GEMM batch: fp64 matrices only"};
    if (sym) {
      if (gemv || !std::is_same<T, double>::value)
        throw ClrsdpError{CLRSDP_E_ARG, "symmetric GEMM epilogue: fp64 matrices only"};
      for (const auto& g : h)
        if (g.M != g.N) throw ClrsdpError{CLRSDP_E_ARG, "symmetric GEMM epilogue: square problems only"};
      // tile-major over the lower tiles (tm >= tn) of each problem, problem fastest
      int mx = 0;
      for (int n : ntiles) mx = std::max(mx, n);
      for (int t = 0; t < mx; ++t)
        for (size_t p = 0; p < h.size(); ++p)
          if (t < ntiles[p] && t / h[p].tn >= t % h[p].tn) t2d.push_back(TileRef{(int)p, t});
    } else if (upper && !gemv && !std::is_same<T, double>::value) {
      int mx = 0;
      for (int n : ntiles) mx = std::max(mx, n);
      for (int t = 0; t < mx; ++t)
        for (size_t p = 0; p < h.size(); ++p)
          if (t < ntiles[p] && t / h[p].tn <= t % h[p].tn) t2d.push_back(TileRef{(int)p, t});
    } else {
      t2d = tile_major(ntiles);
    }
    d = own(h);
    dt = own(t2d);
    detect_uniform(sw.gemm_ts32_below);
  }
  // fp64 batches of one shape at constant operand strides take gemm_f64_uni (no descriptor
  // chain before the first operand load)
  bool uni = false;
  int uts = 64;  // gemm_f64_uni output tile (64 or 32)
  UniGemm ug{};
  void detect_uniform(long ts32_below) {
    if constexpr (std::is_same<T, double>::value) {
      if (gemv || dyn || h.empty()) return;
      const GemmDesc<T>& g0 = h[0];
      auto stride = [&](auto get, long long& st) {
        st = h.size() > 1 ? (long long)(get(h[1]) - get(h[0])) : 0;
        for (size_t p = 1; p < h.size(); ++p)
          if ((long long)(get(h[p]) - get(h[p - 1])) != st) return false;
        return true;
      };
      for (const auto& g : h)
        if (g.M != g0.M || g.N != g0.N || g.K != g0.K || g.lda != g0.lda || g.ldb != g0.ldb ||
            g.ldc != g0.ldc || g.ldcin != g0.ldcin || (g.Cin == nullptr) != (g0.Cin == nullptr) ||
            (g.sa == nullptr) != (g0.sa == nullptr))
          return;
      UniGemm u{};
      bool ok = stride([](const GemmDesc<T>& g) { return g.A; }, u.sA) &&
                stride([](const GemmDesc<T>& g) { return g.B; }, u.sB) &&
                stride([](const GemmDesc<T>& g) { return (const T*)g.C; }, u.sC);
      if (g0.Cin) ok = ok && stride([](const GemmDesc<T>& g) { return g.Cin; }, u.sCin);
      if (g0.sa) ok = ok && stride([](const GemmDesc<T>& g) { return g.sa; }, u.sSa) &&
                      stride([](const GemmDesc<T>& g) { return g.sl; }, u.sSl);
      if (!ok) return;
      u.A = g0.A; u.B = g0.B; u.Cin = g0.Cin; u.C = g0.C; u.sa = g0.sa; u.sl = g0.sl;
      u.M = g0.M; u.N = g0.N; u.K = g0.K; u.lda = g0.lda; u.ldb = g0.ldb; u.ldcin = g0.ldcin;
      u.P = (int)h.size();
      u.ldc = g0.ldc;
      // 32x32 tiles when the 64x64 tiles would leave most CUs idle (a small batch: one CU's
      // tile is then latency-bound, ~9.4 us for a 128^3 product against 6.5 us split over four
      // CUs, tools/micro/gemm_tiles.hip); CLRSDP_GEMM_TS32_BELOW sets the threshold (tiles)
      const long t64m = (long)cdiv(g0.M, 64), t64n = (long)cdiv(g0.N, 64);
      const long tiles64 = u.P * (sym ? t64m * (t64m + 1) / 2 : t64m * t64n);
      uts = tiles64 < ts32_below ? 32 : 64;
      u.tn = (int)cdiv(g0.N, uts);
      const int tm = (int)cdiv(g0.M, uts);
      u.tsym = tm * (tm + 1) / 2;
      ug = u;
      uni = true;
    }
  }
  template <class U = T>
  void launch_uni_impl(hipStream_t s, double alpha, double beta, const double* ds, double dmult) const;
  void launch_uni(hipStream_t s, double alpha, double beta, const double* ds, double dmult) const {
    launch_uni_impl<T>(s, alpha, beta, ds, dmult);
  }
  // the kernel launch() takes after finalize() (CLRSDP_PATH_*, include/clrsdp.h; 0: empty plan),
  // from the fields it branches on, in its order
  int path() const {
    if (h.empty()) return 0;
    constexpr bool f64 = std::is_same<T, double>::value;
    if (gemv) {
      if (f64) return ta ? CLRSDP_PATH_GEMV_T_F64 : CLRSDP_PATH_GEMV_N_F64;
      if (!ta) return CLRSDP_PATH_GEMV_N_MW;
      return std::is_same<T, mw::dd>::value ? CLRSDP_PATH_GEMV_T_DD : CLRSDP_PATH_GEMV_T_QD;
    }
    if (!f64) return CLRSDP_PATH_VALU_KS;
    if (uni) return uts == 32 ? CLRSDP_PATH_UNI32 : CLRSDP_PATH_UNI64;
    if (sca) return CLRSDP_PATH_LDS;
    return dyn ? CLRSDP_PATH_DYN : CLRSDP_PATH_LDS;
  }
  // C = alpha op(A) op(B) + beta Cin (+ dmult * *dscal on the diagonal of square problems)
  void launch(hipStream_t s, double alpha, double beta, const T* dscal = nullptr,
              double dmult = 0.0) const {
    if (h.empty()) return;
    if (dscal && !std::is_same<T, double>::value)
      throw ClrsdpError{CLRSDP_E_ARG, "fused diagonal epilogue is fp64 only"};
    const unsigned grid = (unsigned)t2d.size();
    if (gemv) {  // (tb only with K = 1: B[0] is the vector either way)
      // the transposed product: DEEP is the deep load pipeline (fp64) and the thread-per-column
      // form (quad-double); double-double keeps the 16-lane reduction form
      constexpr bool deep_t = !std::is_same<T, mw::dd>::value;
      if (ta) gemv_batched<T, true, deep_t><<<grid, 256, 0, s>>>(d, dt, alpha, beta);
      else gemv_batched<T, false><<<grid, 256, 0, s>>>(d, dt, alpha, beta);
      HIPCHK(hipGetLastError());
      return;
    }
    if constexpr (std::is_same<T, double>::value) {
      const double* ds = reinterpret_cast<const double*>(dscal);
      if (uni) {
        launch_uni(s, alpha, beta, ds, dmult);
        return;
      }
      if (sca) {
        gemm_f64_lds<false, true, 0, 32, 8, false, true><<<grid, 512, 0, s>>>(d, dt, alpha, beta, ds, dmult);
        HIPCHK(hipGetLastError());
        return;
      }
      if (dyn) {  // alpha/beta come from the descriptors
        gemm_f64_dyn<><<<grid, 512, 0, s>>>(d, dt, alpha, beta);
        HIPCHK(hipGetLastError());
        return;
      }
      if (sym) {
        if (beta != 0.0 || ds) throw ClrsdpError{CLRSDP_E_ARG, "symmetric GEMM epilogue: beta = 0 only"};
        if (!ta && tb) gemm_f64_lds<false, true, 0, 32, 8, true><<<grid, 512, 0, s>>>(d, dt, alpha, 0.0);
        else if (!ta && !tb) gemm_f64_lds<false, false, 0, 32, 8, true><<<grid, 512, 0, s>>>(d, dt, alpha, 0.0);
        else throw ClrsdpError{CLRSDP_E_ARG, "symmetric GEMM epilogue: op(A) = A only"};
        HIPCHK(hipGetLastError());
        return;
      }
      if (tag == 1 && !ta && tb) gemm_f64_lds<false, true, 1><<<grid, 512, 0, s>>>(d, dt, alpha, beta, ds, dmult, stamp);
      else if (tag == 3 && !ta && tb) gemm_f64_lds<false, true, 3><<<grid, 512, 0, s>>>(d, dt, alpha, beta, ds, dmult, stamp);
      else if (!ta && !tb) gemm_f64_lds<false, false><<<grid, 512, 0, s>>>(d, dt, alpha, beta, ds, dmult);
      else if (ta && !tb) gemm_f64_lds<true, false><<<grid, 512, 0, s>>>(d, dt, alpha, beta, ds, dmult);
      else if (!ta && tb) gemm_f64_lds<false, true><<<grid, 512, 0, s>>>(d, dt, alpha, beta, ds, dmult);
      else gemm_f64_lds<true, true><<<grid, 512, 0, s>>>(d, dt, alpha, beta, ds, dmult);
    } else {
      if (!ta && !tb) gemm_valu_ks<T, false, false><<<grid, 256, 0, s>>>(d, dt, alpha, beta);
      else if (ta && !tb) gemm_valu_ks<T, true, false><<<grid, 256, 0, s>>>(d, dt, alpha, beta);
      else if (!ta && tb) gemm_valu_ks<T, false, true><<<grid, 256, 0, s>>>(d, dt, alpha, beta);
      else gemm_valu_ks<T, true, true><<<grid, 256, 0, s>>>(d, dt, alpha, beta);
    }
    HIPCHK(hipGetLastError());
  }
};

// Two dependent products of every block as one launch by column strips (chain_f64, fp64,
// uniform n x n blocks with n <= 128): T = a1 A1 op(B1)[:, S] + b1 C1[:, S], O[:, S] = A2 T
struct ChainPlan {
  bool on = false, tb1 = false, sym = false, trace = false;
  ChainGemm u{};
  // one pointer set per arena; the blocks sit at stride n^2 (checked by the caller)
  void set(int half, const double* A1, const double* B1, const double* C1, const double* A2,
           double* O) {
    u.A1[half] = A1; u.B1[half] = B1; u.C1[half] = C1; u.A2[half] = A2; u.O[half] = O;
  }
  void init(int n, int nb, int halves, bool tb, bool sy) {
    on = true;
    tb1 = tb;
    sym = sy;
    u.n = n;
    u.lda1 = u.ldb1 = u.ldc1 = u.lda2 = u.ldo = n;
    u.sA1 = u.sB1 = u.sC1 = u.sA2 = u.sO = (long long)n * n;
    u.P1 = nb;
    u.P = nb * halves;
    if (halves == 1) set(1, nullptr, nullptr, nullptr, nullptr, nullptr);
    for (const void* k : {(const void*)chain_f64<false, false>, (const void*)chain_f64<true, true>,
                          (const void*)chain_f64<false, false, true>})
      HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)chain::LDS));
  }
  void launch(hipStream_t s, double a1, double b1) const {
    const unsigned grid = (unsigned)(u.P * (int)cdiv(trace ? u.NC : u.n, chain::NS));
    if (trace) chain_f64<false, false, true><<<grid, 512, chain::LDS_TRACE, s>>>(u, a1, b1);
    else if (tb1 && sym) chain_f64<true, true><<<grid, 512, chain::LDS, s>>>(u, a1, b1);
    else if (!tb1 && !sym) chain_f64<false, false><<<grid, 512, chain::LDS, s>>>(u, a1, b1);
    else throw ClrsdpError{CLRSDP_E_ARG, "chain_f64: unsupported variant"};
    HIPCHK(hipGetLastError());
  }
};

template <int TS>
void launch_uni_ts(const UniGemm& u, hipStream_t s, bool ta, bool tb, bool sca, bool sym, int tag,
                   unsigned long long* stamp, double alpha, double beta, const double* ds, double dmult) {
  constexpr int NW = TS == 64 ? 8 : 2, NT = 64 * NW;
  const unsigned tiles = (unsigned)(u.P * (int)cdiv(u.M, TS) * u.tn);
  if (sca) {
    gemm_f64_uni<false, true, 0, 32, NW, false, true, true, TS><<<tiles, NT, 0, s>>>(u, alpha, beta, ds, dmult);
  } else if (sym) {
    if (beta != 0.0 || ds) throw ClrsdpError{CLRSDP_E_ARG, "symmetric GEMM epilogue: beta = 0 only"};
    const unsigned grid = (unsigned)(u.P * u.tsym);
    if (!ta && tb) gemm_f64_uni<false, true, 0, 32, NW, true, false, true, TS><<<grid, NT, 0, s>>>(u, alpha, 0.0);
    else if (!ta && !tb) gemm_f64_uni<false, false, 0, 32, NW, true, false, true, TS><<<grid, NT, 0, s>>>(u, alpha, 0.0);
    else throw ClrsdpError{CLRSDP_E_ARG, "symmetric GEMM epilogue: op(A) = A only"};
  } else {
    if (tag == 1 && !ta && tb) gemm_f64_uni<false, true, 1, 32, NW, false, false, true, TS><<<tiles, NT, 0, s>>>(u, alpha, beta, ds, dmult, stamp);
    else if (tag == 3 && !ta && tb) gemm_f64_uni<false, true, 3, 32, NW, false, false, true, TS><<<tiles, NT, 0, s>>>(u, alpha, beta, ds, dmult, stamp);
    else if (!ta && !tb) gemm_f64_uni<false, false, 0, 32, NW, false, false, true, TS><<<tiles, NT, 0, s>>>(u, alpha, beta, ds, dmult);
    else if (ta && !tb) gemm_f64_uni<true, false, 0, 32, NW, false, false, true, TS><<<tiles, NT, 0, s>>>(u, alpha, beta, ds, dmult);
    else if (!ta && tb) gemm_f64_uni<false, true, 0, 32, NW, false, false, true, TS><<<tiles, NT, 0, s>>>(u, alpha, beta, ds, dmult);
    else gemm_f64_uni<true, true, 0, 32, NW, false, false, true, TS><<<tiles, NT, 0, s>>>(u, alpha, beta, ds, dmult);
  }
  HIPCHK(hipGetLastError());
}

template <class T>
template <class U>
void GemmPlan<T>::launch_uni_impl(hipStream_t s, double alpha, double beta, const double* ds, double dmult) const {
  if constexpr (std::is_same<T, double>::value) {
    if (uts == 32) launch_uni_ts<32>(ug, s, ta, tb, sca, sym, tag, stamp, alpha, beta, ds, dmult);
    else launch_uni_ts<64>(ug, s, ta, tb, sca, sym, tag, stamp, alpha, beta, ds, dmult);
  }
}

template <class T>
struct TrsmPlan : PlanBase {
  // NC: right-hand sides per workgroup.  Multi-word solves with many right-hand sides
  // (W = L^-1 B) take 16 (one diagonal pass of 256 threads, and four times the workgroups of 64:
  // the panel update's multi-word products spread over more CUs).
  static constexpr int NB = 16, NCW = 64, NCN = 16;
  // LDS of trsm_batched at n: launch()'s dynamic diagonal block, solved rows and panel, and the
  // kernel's static reciprocals.  Beyond LDS_MAX (fp64 n > 1199, dd 559, qd 239) the plan takes
  // the blocked chain: super-blocks of kb rows, each solved by trsm_batched on the sub-triangle
  // (per-step descriptors) and followed by trsm_blk_update on the rows not yet solved.
  // CLRSDP_TRSM_BLK: unset that; 1 the chain at every size trsm_batched would have served; 0
  // trsm_batched only (larger matrices: E_ARG)
  static constexpr size_t lu_lds_bytes(int n) {
    return sizeof(T) * ((size_t)NB * NB + (size_t)NB * NCW + (size_t)NB * n + NB);
  }
  static bool one_cu_fits(int n) { return lu_lds_bytes(n) <= LDS_MAX; }
  // the chain's super-block height (CLRSDP_TRSM_KB overrides; rounded down to a multiple of NB
  // that fits the panel): DESIGN.md §3 has the sweep
  bool blk = false;
  int kb = 0;
  struct Step { TrsmDesc<T>* d; int* dt; unsigned grid; };
  std::vector<Step> steps;  // by super-block, top down
  // update tiles: TR rows x UC right-hand sides (vector solves: one column, no padding)
  static constexpr int TR = 64, UC = 16;
  std::vector<TrsmDesc<T>> h;
  std::vector<int> t2d;
  TrsmDesc<T>* d = nullptr;
  int* dt = nullptr;
  int nmax = 0, rmax = 0;
  bool narrow = false;
  // multi-word solves with n <= 128: trsv_wave (n <= 64) / trsv_wave128 (L through LDS in
  // 32-step chunks), one wave per right-hand side, 4 waves per workgroup for vector solves and 16
  // (four per SIMD, their chains interleaved; one LDS copy of L per 16 right-hand sides) for
  // W_j = L_j^-1 B_j; trsm_batched beyond
  static constexpr int NCV = 4, NCV16 = 16;
  bool vec = false;
  int ncv = NCV;
  bool four = false;  // four right-hand sides per workgroup whatever their number (latency first)
  // ident: the right-hand sides are the columns of the identity (L^-1 = L \ I); src: read them
  // from src (ld ldb) and write the solution to B.  Both only in the vector-solve kernels
  // (vec_rhs() after finalize); otherwise the caller fills B first.
  void add(const T* L, int ldl, T* B, int ldb, int n, int nrhs, bool ident = false,
           const T* src = nullptr) {
    if (n <= 0 || nrhs <= 0) return;
    rmax = std::max(rmax, nrhs);
    TrsmDesc<T> t;
    t.L = L; t.B = B; t.n = n; t.nrhs = nrhs; t.ldl = ldl; t.ldb = ldb;
    t.tile0 = 0;
    t.pad = ident ? 1 : 0;
    t.src = src;
    h.push_back(t);
    nmax = std::max(nmax, n);
  }
  void finalize(const Switches& sw) {
    if (h.empty()) return;
    narrow = mode == 0 && !std::is_same<T, double>::value && rmax >= 32;
    vec = mode == 0 && !std::is_same<T, double>::value && nmax <= 128;
    ncv = (rmax <= NCV || four) ? NCV : NCV16;
    const int nc = vec ? ncv : narrow ? NCN : NCW;
    if constexpr (!std::is_same<T, double>::value) {
      if (vec) {  // (outside any graph capture)
        static std::atomic<unsigned long long> a128[4], a64[4];
        lds_attr_once(a128[0], (const void*)trsv_wave128<T, true, NCV>, (int)trsv_wave128_lds<T>());
        lds_attr_once(a128[1], (const void*)trsv_wave128<T, false, NCV>, (int)trsv_wave128_lds<T>());
        lds_attr_once(a128[2], (const void*)trsv_wave128<T, true, NCV16>, (int)trsv_wave128_lds<T>());
        lds_attr_once(a128[3], (const void*)trsv_wave128<T, false, NCV16>, (int)trsv_wave128_lds<T>());
        lds_attr_once(a64[0], (const void*)trsv_wave<T, true, NCV>, (int)trsv_wave_lds<T>());
        lds_attr_once(a64[1], (const void*)trsv_wave<T, false, NCV>, (int)trsv_wave_lds<T>());
        lds_attr_once(a64[2], (const void*)trsv_wave<T, true, NCV16>, (int)trsv_wave_lds<T>());
        lds_attr_once(a64[3], (const void*)trsv_wave<T, false, NCV16>, (int)trsv_wave_lds<T>());
      }
    }
    blk = !vec && (sw.trsm_blk == 1 || (sw.trsm_blk < 0 && !one_cu_fits(nmax)));
    if (!vec && !blk && !one_cu_fits(nmax))
      throw ClrsdpError{CLRSDP_E_ARG, "triangular solve: matrix too large for the on-chip panel of trsm_batched (CLRSDP_TRSM_BLK=0)"};
    if (blk) {
      int kmax = NB;
      while (one_cu_fits(kmax + NB)) kmax += NB;
      kb = (int)(std::max<long>(NB, std::min<long>(sw.trsm_kb, kmax)) / NB * NB);
    }
    const int npan = blk ? std::min(kb, nmax) : nmax;  // rows of the largest on-chip solve
    if (lu_lds_bytes(npan) > 64 * 1024) {  // (outside any graph capture)
      static std::atomic<unsigned long long> alu[10];
      const void* fns[10] = {(const void*)trsm_batched<T, false, NB, NCW, 256, true, false>,
                            (const void*)trsm_batched<T, true, NB, NCW, 256, true, false>,
                            (const void*)trsm_batched<T, true, NB, NCW, 256, false, true>,
                            (const void*)trsm_batched<T, false, NB, NCW, 256, false, true>,
                            (const void*)trsm_batched<T, false, NB, NCN, 256>,
                            (const void*)trsm_batched<T, true, NB, NCN, 256>,
                            (const void*)trsm_batched<T, false, NB, NCW, 1024>,
                            (const void*)trsm_batched<T, true, NB, NCW, 1024>,
                            (const void*)trsm_batched<T, false, NB, NCW>,
                            (const void*)trsm_batched<T, true, NB, NCW>};
      for (int q = mode != 0 ? 0 : 4; q < (mode != 0 ? 4 : 10); ++q) lds_attr_once(alu[q], fns[q], (int)(LDS_MAX - 1024));
    }
    if (!vec_rhs())
      for (TrsmDesc<T>& t : h) { t.pad = 0; t.src = nullptr; }  // (the caller fills B)
    t2d.clear();
    for (size_t q = 0; q < h.size(); ++q) {
      h[q].tile0 = (int)t2d.size();
      for (int i = 0; i < (int)cdiv(h[q].nrhs, nc); ++i) t2d.push_back((int)q);
    }
    d = own(h);
    dt = own(t2d);
    steps.clear();
    if (!blk) return;
    // per super-block: the sub-triangles of the matrices that reach it
    for (int k0 = 0; k0 < nmax; k0 += kb) {
      std::vector<TrsmDesc<T>> hs;
      std::vector<int> ts;
      for (const TrsmDesc<T>& t : h) {
        if (t.n <= k0) continue;
        TrsmDesc<T> u = t;
        u.L = t.L + k0 + (size_t)k0 * t.ldl;
        u.B = t.B + k0;
        u.n = std::min(kb, t.n - k0);
        u.tile0 = (int)ts.size();
        for (int i = 0; i < (int)cdiv(u.nrhs, nc); ++i) ts.push_back((int)hs.size());
        hs.push_back(u);
      }
      steps.push_back(Step{own(hs), own(ts), (unsigned)ts.size()});
    }
  }
  void launch_vec(hipStream_t s, bool trans, unsigned grid) const {
    if constexpr (!std::is_same<T, double>::value) {
      if (nmax > 64) {
        const size_t l = trsv_wave128_lds<T>();
        if (ncv == NCV16) {
          if (trans) trsv_wave128<T, true, NCV16><<<grid, 64 * NCV16, l, s>>>(d, dt);
          else trsv_wave128<T, false, NCV16><<<grid, 64 * NCV16, l, s>>>(d, dt);
        } else {
          if (trans) trsv_wave128<T, true, NCV><<<grid, 64 * NCV, l, s>>>(d, dt);
          else trsv_wave128<T, false, NCV><<<grid, 64 * NCV, l, s>>>(d, dt);
        }
      } else if (ncv == NCV16) {
        if (trans) trsv_wave<T, true, NCV16><<<grid, 64 * NCV16, trsv_wave_lds<T>(), s>>>(d, dt);
        else trsv_wave<T, false, NCV16><<<grid, 64 * NCV16, trsv_wave_lds<T>(), s>>>(d, dt);
      } else {
        if (trans) trsv_wave<T, true, NCV><<<grid, 64 * NCV, trsv_wave_lds<T>(), s>>>(d, dt);
        else trsv_wave<T, false, NCV><<<grid, 64 * NCV, trsv_wave_lds<T>(), s>>>(d, dt);
      }
    }
  }
  // the vector-solve kernels take the identity / a separate source as right-hand sides
  bool vec_rhs() const { return vec; }
  // mode (the LU fallback's factors): 0 = potrf's L; 1 = unit lower L of getrf; 2 = getrf's U,
  // read transposed (forward: U^T x = b; trans: U x = b)
  int mode = 0;
  void launch(hipStream_t s, bool trans) const {
    if (h.empty()) return;
    if (!blk) {
      launch_tb(s, trans, d, dt, (unsigned)t2d.size(), nmax);
      return;
    }
    // the blocked chain: forward top-down, trans bottom-up; constant launch arguments, so the
    // loop is capture-safe
    const int ns = (int)steps.size();
    const unsigned nm = (unsigned)h.size();
    for (int q = 0; q < ns; ++q) {
      const int si = trans ? ns - 1 - q : q, k0 = si * kb;
      launch_tb(s, trans, steps[si].d, steps[si].dt, steps[si].grid, std::min(kb, nmax - k0));
      const int nr = trans ? k0 : nmax - k0 - kb;  // rows still to be solved (largest matrix)
      if (nr <= 0) continue;
      const int ntr = (int)cdiv(nr, TR);
      if (rmax == 1) {
        const dim3 g((unsigned)ntr, nm);
        if (trans) {
          if (mode == 2) trsm_blk_update<T, true, true, NB, TR, 1, TR><<<g, TR, 0, s>>>(d, k0, kb, ntr);
          else trsm_blk_update<T, true, false, NB, TR, 1, TR><<<g, TR, 0, s>>>(d, k0, kb, ntr);
        } else {
          if (mode == 2) trsm_blk_update<T, false, true, NB, TR, 1, TR><<<g, TR, 0, s>>>(d, k0, kb, ntr);
          else trsm_blk_update<T, false, false, NB, TR, 1, TR><<<g, TR, 0, s>>>(d, k0, kb, ntr);
        }
      } else {
        const dim3 g((unsigned)ntr * cdiv(rmax, UC), nm);
        if (trans) {
          if (mode == 2) trsm_blk_update<T, true, true, NB, TR, UC, 256><<<g, 256, 0, s>>>(d, k0, kb, ntr);
          else trsm_blk_update<T, true, false, NB, TR, UC, 256><<<g, 256, 0, s>>>(d, k0, kb, ntr);
        } else {
          if (mode == 2) trsm_blk_update<T, false, true, NB, TR, UC, 256><<<g, 256, 0, s>>>(d, k0, kb, ntr);
          else trsm_blk_update<T, false, false, NB, TR, UC, 256><<<g, 256, 0, s>>>(d, k0, kb, ntr);
        }
      }
      HIPCHK(hipGetLastError());
    }
  }
  // one trsm_batched launch over descriptors d / tiles dt with at most nmax rows
  void launch_tb(hipStream_t s, bool trans, const TrsmDesc<T>* d, const int* dt, unsigned grid,
                 int nmax) const {
    constexpr int NC = NCW;
    const size_t lds = sizeof(T) * ((size_t)NB * NB + (size_t)NB * NC + (size_t)NB * nmax);
    if constexpr (!std::is_same<T, double>::value) {
      if (vec && mode == 0) {
        launch_vec(s, trans, grid);
        HIPCHK(hipGetLastError());
        return;
      }
    }
    if (narrow && mode == 0) {
      const size_t ldsn = sizeof(T) * ((size_t)NB * NB + (size_t)NB * NCN + (size_t)NB * nmax);
      if (trans) trsm_batched<T, true, NB, NCN, 256><<<grid, 256, ldsn, s>>>(d, dt);
      else trsm_batched<T, false, NB, NCN, 256><<<grid, 256, ldsn, s>>>(d, dt);
      HIPCHK(hipGetLastError());
      return;
    }
    if (mode == 1) {  // (the solver's LU path solves with L forward only; clrsdp_trsm both ways)
      if (trans) trsm_batched<T, true, NB, NC, 256, true, false><<<grid, 256, lds, s>>>(d, dt);
      else trsm_batched<T, false, NB, NC, 256, true, false><<<grid, 256, lds, s>>>(d, dt);
      HIPCHK(hipGetLastError());
      return;
    }
    if (mode == 2) {
      if (trans) trsm_batched<T, true, NB, NC, 256, false, true><<<grid, 256, lds, s>>>(d, dt);
      else trsm_batched<T, false, NB, NC, 256, false, true><<<grid, 256, lds, s>>>(d, dt);
      HIPCHK(hipGetLastError());
      return;
    }
    if (mode != 0) throw ClrsdpError{CLRSDP_E_ARG, "unsupported triangular solve mode"};
    // multi-word solves with many right-hand sides (W = L^-1 B): 1024 threads, four waves per
    // SIMD for the VALU-bound panel update; vector solves keep 256
    if (!std::is_same<T, double>::value && rmax >= 32) {
      if (trans) trsm_batched<T, true, NB, NC, 1024><<<grid, 1024, lds, s>>>(d, dt);
      else trsm_batched<T, false, NB, NC, 1024><<<grid, 1024, lds, s>>>(d, dt);
    } else {
      if (trans) trsm_batched<T, true, NB, NC><<<grid, 256, lds, s>>>(d, dt);
      else trsm_batched<T, false, NB, NC><<<grid, 256, lds, s>>>(d, dt);
    }
    HIPCHK(hipGetLastError());
  }
};

template <class T>
struct MatPlan : PlanBase {  // potrf / eigmin
  static constexpr int NB = 16;
  std::vector<MatDesc<T>> h;
  MatDesc<T>* d = nullptr;
  int nmax = 0;
  void add(T* A, int n, int lda) {
    MatDesc<T> m;
    m.A = A; m.n = n; m.lda = lda;
    h.push_back(m);
    nmax = std::max(nmax, n);
  }
  // multi-word Cholesky factors on one CU: chol_lookahead without the inverse (1024 threads, the
  // whole block on chip, the pivot chain beside the trailing update) writes L in place, up to
  // n = 128 (double-double) or 64 (quad-double: a 128 instance would spill) -- against
  // potrf_batched's 16-column panels with a serial pivot chain beyond.
  static constexpr int LA_NMAX = std::is_same<T, mw::dd>::value ? 128 : 64;
  int* redo = nullptr;  // eigmin_mx's per-block fallback flags
  // blocked multi-word potrf across workgroups (potrf_blk_*, kernels_dense.h; round 6): taken
  // for the double-double blocks above 64 (CLRSDP_POTRF_BLK=0 keeps chol_lookahead there).
  // 16-column panels: n = 127 x 16 blocks 230 -> 155 us (32-column panels: 201 us), while at
  // n <= 64 the one-CU chol_lookahead stays ahead (52 against 73 us; tools/micro/potrf_blk_bench)
  static constexpr int BLK_NB = 16;
  // the fp64 chain (potrf64_*, the trailing update on the fp64 matrix cores): panel width by
  // measurement (tools/micro/potrf_blk_bench, 2 blocks, us, NB = 16 / 32 /
  // 64 against potrf_batched): n = 257 258 / 284 / 405 against 1277; n = 640 668 / 708 / 966
  // against 14180; n = 1262 1540 / 1600 / 2184 against 105903.  A panel costs its serial steps
  // (diag, the substitution) plus two launches, both growing with NB, while the update's 64 x 64
  // tiles are already spread over the chip at NB = 16.
  static constexpr int BLK64_NB = 16;
  // The kernel potrf() launches for a batch whose largest block is nmax (CLRSDP_POTRF_K_*,
  // clrsdp.h), `potrf_blk` being the three-state CLRSDP_POTRF_BLK (as CLRSDP_LU_BLK): unset
  // (-1) the chain for double-double above 64 only; 0 no chain at any word type; 1 the chain
  // also wherever potrf_batched would run (fp64 at every n, quad-double above 64 in
  // chol_lookahead's LDL form).  Only potrf_batched has a size bound (potrf_refusal).
  static int potrf_dispatch(int nmax, int potrf_blk) {
    if (std::is_same<T, double>::value) return potrf_blk == 1 ? CLRSDP_POTRF_K_BLK64 : CLRSDP_POTRF_K_BATCHED;
    if (nmax <= 64) return CLRSDP_POTRF_K_LA64;
    if (std::is_same<T, mw::dd>::value) {
      if (potrf_blk != 0) return CLRSDP_POTRF_K_BLK;
      return nmax <= LA_NMAX ? CLRSDP_POTRF_K_LA128 : CLRSDP_POTRF_K_BATCHED;
    }
    return potrf_blk == 1 ? CLRSDP_POTRF_K_BLK : CLRSDP_POTRF_K_BATCHED;
  }
  int route = -1;   // potrf()'s, stored by finalize(); -1: an EIG_ONLY plan, which potrf() refuses
  int la_opts = 2;  // chol_lookahead's option bits, as finalize() was handed them
  BlkPotrfDesc<T>* bd = nullptr;
  // potrf_batched: 256 threads, double-double 1024 (see potrf())
  static constexpr int PB_NT = std::is_same<T, mw::dd>::value ? 1024 : 256;
  static size_t pb_lds_dyn(int n) { return sizeof(T) * ((size_t)NB * NB + (size_t)NB * n); }
  // static LDS of potrf_batched (rdg[], fail), from the code object (asked once per word type)
  static size_t pb_lds_static() {
    static const size_t bytes = [] {
      hipFuncAttributes fa;
      HIPCHK(hipFuncGetAttributes(&fa, (const void*)potrf_batched<T, NB, PB_NT>));
      return (size_t)fa.sharedSizeBytes;
    }();
    return bytes;
  }
  // the largest n whose 16-column panel (dynamic) and static LDS fit one CU
  static int pb_nmax() {
    const size_t st = pb_lds_static();
    return (int)((LDS_MAX - st - sizeof(T) * NB * NB) / (sizeof(T) * NB));
  }
  // Past potrf_batched's panel the runtime would refuse the launch: the message of the refusal
  // (CLRSDP_E_ARG) for matrices up to nmax, empty where potrf() can run
  static std::string potrf_refusal(int nmax, int potrf_blk) {
    if (potrf_dispatch(nmax, potrf_blk) != CLRSDP_POTRF_K_BATCHED || pb_lds_dyn(nmax) + pb_lds_static() <= LDS_MAX)
      return std::string();
    const char* w = std::is_same<T, double>::value ? "fp64" : std::is_same<T, mw::dd>::value ? "double-double" : "quad-double";
    return std::string("Cholesky factorization: a matrix of n = ") + std::to_string(nmax) +
           " is too large for the on-chip panel of potrf_batched (" + w + ": n <= " + std::to_string(pb_nmax()) + ")";
  }
  static void check_potrf(int nmax, int potrf_blk) {
    const std::string r = potrf_refusal(nmax, potrf_blk);
    if (!r.empty()) throw ClrsdpError{CLRSDP_E_ARG, r};
  }
  std::string refused;  // potrf() throws this (before any launch) instead of launching
  // What the plan is for, which decides how finalize() treats potrf_batched's size bound:
  //   FACTOR           potrf() runs: a plan past the bound is refused by finalize();
  //   FACTOR_DEFERRED  the solver's plans: a plan past the bound is built all the same and
  //                    refused when potrf() is called, since a handle of that size still runs
  //                    every stage before FACTOR, and FACTOR itself with CLRSDP_FACT_LU_SQ
  //                    (pivoted LU has no size bound);
  //   EIG_ONLY         only eigmin() runs: no such bound
  enum class Use { FACTOR, FACTOR_DEFERRED, EIG_ONLY };
  void finalize(const Switches& sw, Use use = Use::FACTOR) {
    if (h.empty()) return;
    la_opts = sw.la_opts;
    if (use != Use::EIG_ONLY) {
      route = potrf_dispatch(nmax, sw.potrf_blk);
      refused = potrf_refusal(nmax, sw.potrf_blk);
      if (!refused.empty() && use == Use::FACTOR) throw ClrsdpError{CLRSDP_E_ARG, refused};
    }
    d = own(h);
    if (route == CLRSDP_POTRF_K_BLK64 || route == CLRSDP_POTRF_K_BLK) {
      // the L_kk^-1 scratch of potrf_blk_* (potrf64_* substitutes against L_kk: none)
      T* li = route == CLRSDP_POTRF_K_BLK ? own(std::vector<T>(h.size() * BLK_NB * BLK_NB, T(0.0))) : nullptr;
      std::vector<BlkPotrfDesc<T>> b(h.size());
      for (size_t q = 0; q < h.size(); ++q)
        b[q] = BlkPotrfDesc<T>{h[q].A, li ? li + q * BLK_NB * BLK_NB : nullptr, h[q].n, h[q].lda};
      bd = own(b);
    }
    if (!std::is_same<T, double>::value) redo = own(std::vector<int>(h.size(), 1));
    const bool eig_blk = use == Use::EIG_ONLY && sw.eig_blk;
    eig_stats = sw.eigmx_stats;
    const int ek = eig_k = eig_dispatch(nmax, eig_blk, use == Use::EIG_ONLY && sw.mxblk(), sw.eig_mx);
    // the flagged blocks of the mxblk route go to the route the switch replaced; where
    // eigmin_batched would ask for more LDS than a launch gets unasked (it then cannot run
    // today either), to the multi-word chain
    mx_fb_chain = ek == CLRSDP_EIG_K_MXBLK && (eig_blk || batched_lds(nmax) > 64 * 1024);
    if (ek == CLRSDP_EIG_K_BLK || mx_fb_chain) finalize_eig_chain();
    if (ek == CLRSDP_EIG_K_MXBLK) finalize_mxblk(sw);
  }
  static size_t batched_lds(int n) { return sizeof(T) * (4 * (size_t)n + 256); }  // eigmin_batched
  bool mx_fb_chain = false;
  // ---- multi-word lambda_min of blocks past the LDS kernels from a refined fp64 eigenpair
  // (mxblk_*, kernels_dense.h).  CLRSDP_EIG_MX_BLK=1 (off with CLRSDP_EIG_MX=0): a multi-word
  // batch that eigmin() would give to eigmin_batched (or, with CLRSDP_EIG_BLK=1, to the
  // multi-word chain) first goes through the fp64 chain, the fp64 Cholesky chain and a few
  // refinement steps at the word's width; the blocks Temple's bound does not certify are
  // flagged in `redo`, and the route the switch replaced then runs on those alone.  All of its
  // scratch is allocated when the plan is finalised.  Opt-in: DESIGN.md §1.
  // the first size of the route per word type: the first of eigmin_batched's range (the route
  // was ahead of both older routes there)
  static constexpr int MXBLK_NMIN = std::is_same<T, mw::dd>::value ? 97 : 67;
  static constexpr int MXBLK_NMAX = 4096;  // the 2^-40 margin of lam2 covers n 2^-52 up to here
  MxBlkDesc<T>* md = nullptr;
  EigBlkDesc<double>* ed64 = nullptr;
  BlkPotrfDesc<double>* bd64 = nullptr;
  int* info64 = nullptr;
  double* lam64 = nullptr;
  double* mx_st = nullptr;  // MXBLK_ST state words per block
  TrsmPlan<double> mx_ts;   // the vector solves with the factor of A_h - mu I
  // tools/micro/eig_mxblk_bench: three events recorded behind the fp64 chain with its Sturm
  // step, the factor, and the inverse iteration (null in the library: a capture records none)
  hipEvent_t* mx_phase_ev = nullptr;
  void finalize_mxblk(const Switches& sw) {
    if constexpr (!std::is_same<T, double>::value) {
      constexpr int R = EIG_R;
      const size_t nm = h.size();
      size_t sq = 0, vec = 0, parts = 0, words = 0;
      for (const MatDesc<T>& m : h) {
        sq += (size_t)m.n * m.n;
        vec += m.n;
        parts += cdiv(m.n, R);
        words += eigblk_ws_words(m.n);
      }
      double* Ah = own(std::vector<double>(sq, 0.0));
      double* Af = own(std::vector<double>(sq, 0.0));
      double* zb = own(std::vector<double>(2 * vec, 0.0));
      T* xy = own(std::vector<T>(2 * vec, T(0.0)));
      double* am = own(std::vector<double>(2 * parts, 0.0));
      double* ws = own(std::vector<double>(words, 0.0));
      mx_st = own(std::vector<double>(nm * MXBLK_ST, 0.0));
      lam64 = own(std::vector<double>(nm, 0.0));
      info64 = own(std::vector<int>(nm, 0));
      std::vector<MxBlkDesc<T>> m(nm);
      std::vector<EigBlkDesc<double>> e(nm);
      std::vector<BlkPotrfDesc<double>> b(nm);
      sq = vec = parts = words = 0;
      for (size_t q = 0; q < nm; ++q) {
        const int n = h[q].n;
        m[q] = MxBlkDesc<T>{h[q].A, Ah + sq, Af + sq, am + 2 * parts, zb + 2 * vec, zb + 2 * vec + n,
                            xy + 2 * vec, xy + 2 * vec + n, mx_st + q * MXBLK_ST, n, h[q].lda};
        e[q] = EigBlkDesc<double>{Ah + sq, ws + words, am + 2 * parts + cdiv(n, R), n, n};
        b[q] = BlkPotrfDesc<double>{Af + sq, nullptr, n, n};
        mx_ts.add(Af + sq, n, zb + 2 * vec + n, n, n, 1);
        sq += (size_t)n * n;
        vec += n;
        parts += cdiv(n, R);
        words += eigblk_ws_words(n);
      }
      md = own(m);
      ed64 = own(e);
      bd64 = own(b);
      mx_ts.finalize(sw);
      // every instance that can ask for more than 64 KiB of dynamic LDS, outside any capture
      static std::atomic<unsigned long long> ac{0}, as{0};
      lds_attr_once(ac, (const void*)eigblk_col<double, EIG_R>, (int)LDS_MAX);
      lds_attr_once(as, (const void*)mxblk_sturm<T>, (int)LDS_MAX);
    }
  }
  // the launches of the route up to the flags; eigmin() follows with the flagged blocks
  void eigmin_mxblk(hipStream_t s, T* out) const {
    if constexpr (!std::is_same<T, double>::value) {
      constexpr int R = EIG_R, NB = BLK64_NB;
      const unsigned nm = (unsigned)h.size();
      const dim3 strips(cdiv(nmax, R), nm);
      mxblk_amax<T, R><<<strips, 64, 0, s>>>(md);
      mxblk_image<T, R><<<strips, 64, 0, s>>>(md);
      eigblk_amax<double, R><<<strips, 64, 0, s>>>(ed64);
      eigblk_sym<double, R><<<strips, 64, 0, s>>>(ed64);
      const size_t lds = eigblk_col_lds<double>(nmax);
      for (int k = 0; k + 2 < nmax; ++k)
        eigblk_col<double, R><<<dim3(cdiv(nmax - k - 1, R), nm), 64, lds, s>>>(ed64, k);
      mxblk_sturm<T><<<nm, 512, mxblk_sturm_lds(nmax), s>>>(ed64, md, lam64);
      HIPCHK(hipGetLastError());
      if (mx_phase_ev) HIPCHK(hipEventRecord(mx_phase_ev[0], s));
      potrf64_first<NB><<<nm, 256, 0, s>>>(bd64, info64);
      for (int k0 = 0; k0 + NB < nmax; k0 += NB) {
        const int rows = nmax - k0 - NB, nch = cdiv(rows, 64);
        potrf64_trsm<NB><<<dim3((unsigned)nch, nm), 64, 0, s>>>(bd64, k0, info64);
        potrf64_update<NB><<<dim3(1u + (unsigned)(nch * (nch + 1) / 2), nm), 256, 0, s>>>(bd64, k0, info64);
      }
      HIPCHK(hipGetLastError());
      if (mx_phase_ev) HIPCHK(hipEventRecord(mx_phase_ev[1], s));
      for (int r = 0; r < MXBLK_INVIT; ++r) {
        mx_ts.launch(s, false);
        mx_ts.launch(s, true);
        mxblk_norm<T><<<nm, 256, 0, s>>>(md, info64, r == 0, r + 1 == MXBLK_INVIT);
      }
      if (mx_phase_ev) HIPCHK(hipEventRecord(mx_phase_ev[2], s));
      for (int it = 0; it <= MXBLK_REFINE; ++it) {
        mxblk_matvec<T><<<strips, 256, 0, s>>>(md);
        mxblk_rayleigh<T><<<nm, 256, 0, s>>>(md, out, it, it == MXBLK_REFINE);
        if (it == MXBLK_REFINE) break;
        mx_ts.launch(s, false);
        mx_ts.launch(s, true);
        mxblk_update<T><<<nm, 256, 0, s>>>(md);
      }
      mxblk_finish<T><<<cdiv(nm, 256), 256, 0, s>>>(md, (int)nm, redo);
      HIPCHK(hipGetLastError());
    }
  }
  // ---- lambda_min of blocks past the LDS kernels across workgroups (eigblk_*, kernels_dense.h)
  // CLRSDP_EIG_BLK=1: a batch that eigmin() would give to the one-CU eigmin_batched goes to the
  // chain instead -- one launch per column over strips of EIG_R rows, then eigblk_sturm.
  // Opt-in: the measurements and the crossover against eigmin_batched are in DESIGN.md §1.
  // EIG_R: one thread per row and one wave per strip, so the strip height only decides how
  // many waves share the rows (tools/micro/eig_blk_bench)
  static constexpr int EIG_R = 64;
  bool eig_stats = false;  // CLRSDP_EIGMX_STATS: eigmin_mx's diagnostics instance
  int eig_k = -1;          // eigmin()'s kernel (eig_dispatch), stored by finalize()
  bool eig_tri = true;  // eigblk_sturm keeps the tridiagonal in LDS
  EigBlkDesc<T>* ed = nullptr;
  // the largest n whose v_k and w (eigblk_col's dynamic LDS) fit one CU
  static constexpr int eig_chain_nmax() { return (int)(LDS_MAX / (2 * sizeof(T))); }
  // The kernel eigmin() launches for a batch whose largest block is nmax (CLRSDP_EIG_K_*,
  // clrsdp.h), `chain` being CLRSDP_EIG_BLK, `mxblk` CLRSDP_EIG_MX_BLK (off with CLRSDP_EIG_MX=0)
  // and `mx` CLRSDP_EIG_MX as the plan was handed them
  static int eig_dispatch(int nmax, bool chain, bool mxblk, bool mx) {
    if (std::is_same<T, double>::value && nmax <= 128) return CLRSDP_EIG_K_SPLIT;  // matrix in registers
    if (!std::is_same<T, double>::value) {
      // n <= 64: an fp64 eigenpair refined at the word's width (eigmin_mx; the blocks it cannot
      // certify go to eigmin_lds2 in a second, flagged launch) unless CLRSDP_EIG_MX=0
      if (mx && nmax <= 64 && eigmx_lds_bytes<T>(nmax) + EIGMX_STATIC_LDS <= LDS_MAX &&
          eig2_lds_bytes<T>(nmax) <= LDS_MAX)
        return CLRSDP_EIG_K_MX;
      // eigmin_lds2 (two barriers per column) where its column slots fit (qd: 8 column slots
      // per lane, n <= 64)
      if (eig2_lds_bytes<T>(nmax) <= LDS_MAX && (sizeof(T) <= 16 || nmax <= 64)) return CLRSDP_EIG_K_LDS2;
    }
    if (eig_lds_bytes<T>(nmax) <= LDS_MAX) return CLRSDP_EIG_K_LDS;
    if (!std::is_same<T, double>::value && mxblk && nmax >= MXBLK_NMIN && nmax <= MXBLK_NMAX)
      return CLRSDP_EIG_K_MXBLK;
    return chain ? CLRSDP_EIG_K_BLK : CLRSDP_EIG_K_BATCHED;
  }
  void finalize_eig_chain() {
    if (nmax > eig_chain_nmax())
      throw ClrsdpError{CLRSDP_E_ARG, "eigenvalues: a block of n = " + std::to_string(nmax) +
                                          " is too large for the on-chip vectors of eigblk_col (n <= " +
                                          std::to_string(eig_chain_nmax()) + ")"};
    size_t words = 0, parts = 0;
    for (const MatDesc<T>& m : h) {
      words += eigblk_ws_words(m.n);
      parts += cdiv(m.n, EIG_R);
    }
    T* ws = own(std::vector<T>(words, T(0.0)));
    double* am = own(std::vector<double>(parts, 0.0));
    std::vector<EigBlkDesc<T>> e(h.size());
    words = parts = 0;
    for (size_t q = 0; q < h.size(); ++q) {
      e[q] = EigBlkDesc<T>{h[q].A, ws + words, am + parts, h[q].n, h[q].lda};
      words += eigblk_ws_words(h[q].n);
      parts += cdiv(h[q].n, EIG_R);
    }
    ed = own(e);
    eig_tri = eigblk_sturm_lds<T>(nmax, true) <= LDS_MAX;
    // every instance that can ask for more than 64 KiB of dynamic LDS, outside any capture
    static std::atomic<unsigned long long> ac{0}, at{0}, ag{0};
    lds_attr_once(ac, (const void*)eigblk_col<T, EIG_R>, (int)LDS_MAX);
    lds_attr_once(at, (const void*)eigblk_sturm<T, true>, (int)LDS_MAX);
    lds_attr_once(ag, (const void*)eigblk_sturm<T, false>, (int)LDS_MAX);
  }
  // (flags: the fallback behind eigmin_mxblk, on the blocks with flags[block] != 0 only)
  void eigmin_chain(hipStream_t s, T* out, const int* flags = nullptr) const {
    constexpr int R = EIG_R;
    const unsigned nm = (unsigned)h.size();
    eigblk_amax<T, R><<<dim3(cdiv(nmax, R), nm), 64, 0, s>>>(ed, flags);
    eigblk_sym<T, R><<<dim3(cdiv(nmax, R), nm), 64, 0, s>>>(ed, flags);
    const size_t lds = eigblk_col_lds<T>(nmax);
    for (int k = 0; k + 2 < nmax; ++k)
      eigblk_col<T, R><<<dim3(cdiv(nmax - k - 1, R), nm), 64, lds, s>>>(ed, k, flags);
    if (eig_tri) eigblk_sturm<T, true><<<nm, 512, eigblk_sturm_lds<T>(nmax, true), s>>>(ed, out, R, flags);
    else eigblk_sturm<T, false><<<nm, 512, eigblk_sturm_lds<T>(nmax, false), s>>>(ed, out, R, flags);
    HIPCHK(hipGetLastError());
  }
  void potrf(hipStream_t s, int* info) const {
    if (h.empty()) return;
    if (!refused.empty()) throw ClrsdpError{CLRSDP_E_ARG, refused};
    const unsigned nm = (unsigned)h.size();
    switch (route) {
      case CLRSDP_POTRF_K_BLK64:
        if constexpr (std::is_same<T, double>::value) {
          constexpr int NB = BLK64_NB;
          potrf64_first<NB><<<nm, 256, 0, s>>>(bd, info);
          for (int k0 = 0; k0 + NB < nmax; k0 += NB) {
            const int rows = nmax - k0 - NB, nch = cdiv(rows, 64);
            potrf64_trsm<NB><<<dim3((unsigned)nch, nm), 64, 0, s>>>(bd, k0, info);
            potrf64_update<NB><<<dim3(1u + (unsigned)(nch * (nch + 1) / 2), nm), 256, 0, s>>>(bd, k0, info);
          }
        }
        break;
      case CLRSDP_POTRF_K_BLK:
        if constexpr (!std::is_same<T, double>::value) {
          // (quad-double: the diagonal step in the LDL form of its chol_lookahead instances)
          constexpr bool LDL = std::is_same<T, mw::qd>::value;
          constexpr int NB = BLK_NB, DT = NB / 16;
          potrf_blk_first<T, LDL, NB><<<nm, 256, 0, s>>>(bd, info, la_opts);
          for (int k0 = 0; k0 + NB < nmax; k0 += NB) {
            const int rows = nmax - k0 - NB, ntr = cdiv(rows, 16);
            int tiles = 0;  // lower 16-tiles of the trailing matrix outside the next diagonal block
            for (int I = DT; I < ntr; ++I) tiles += I + 1;
            potrf_blk_trsm<T, NB><<<dim3((unsigned)ntr, nm), 256, 0, s>>>(bd, k0);
            potrf_blk_update<T, LDL, NB><<<dim3(1u + tiles, nm), 256, 0, s>>>(bd, k0, info, la_opts);
          }
        }
        break;
      case CLRSDP_POTRF_K_LA64:
        // at n <= 64 the bulk waves on the chain's SIMD stay idle (SKIP0, round 6: qd n = 51
        // 138 -> 126 us, dd n = 64 63 -> 61 us); quad-double in the square-root-free LDL form
        if constexpr (std::is_same<T, mw::dd>::value)
          chol_lookahead<T, false, false, 64, 15, true><<<nm, 1024, 0, s>>>(d, nullptr, d, info, la_opts);
        else if constexpr (std::is_same<T, mw::qd>::value)
          chol_lookahead<T, false, true, 64, 15, true><<<nm, 1024, 0, s>>>(d, nullptr, d, info, la_opts);
        break;
      case CLRSDP_POTRF_K_LA128:
        if constexpr (std::is_same<T, mw::dd>::value)
          chol_lookahead<T, false, false, 128><<<nm, 1024, 0, s>>>(d, nullptr, d, info, la_opts);
        break;
      case CLRSDP_POTRF_K_BATCHED:
        // double-double: 1024 threads, so the trailing update (VALU bound) has four waves per
        // SIMD (C4 factor stage 806 -> 724 us); quad-double keeps 256 (its registers, 3 % slower
        // at 1024)
        potrf_batched<T, NB, PB_NT><<<nm, PB_NT, pb_lds_dyn(nmax), s>>>(d, info);
        break;
      default:
        throw ClrsdpError{CLRSDP_E_STATE, "potrf on a plan finalised for eigmin only"};
    }
    HIPCHK(hipGetLastError());
  }
  void eigmin(hipStream_t s, T* out) const {
    if (h.empty()) return;
    const unsigned nm = (unsigned)h.size();
    switch (eig_k) {
      case CLRSDP_EIG_K_SPLIT:
        if constexpr (std::is_same<T, double>::value) {
          // eigmin_split: one reflector chain wave + 8 bulk waves, the last 24 columns on the
          // chain wave alone (no barriers)
          eigmin_split<0, 24><<<nm, 576, 0, s>>>(d, out);
        }
        break;
      case CLRSDP_EIG_K_MX:
        if constexpr (!std::is_same<T, double>::value) {
          static std::atomic<unsigned long long> attrm{0}, attr2r{0};
          if (eig_stats) {  // (the diagnostics instance: per-block eta / lambda / Temple width)
            static std::atomic<unsigned long long> attrd{0};
            lds_attr_once(attrd, (const void*)eigmin_mx<T, 1>, (int)(LDS_MAX - EIGMX_STATIC_LDS));
            eigmin_mx<T, 1><<<nm, 576, eigmx_lds_bytes<T>(nmax), s>>>(d, out, redo);
          } else {
            lds_attr_once(attrm, (const void*)eigmin_mx<T>, (int)(LDS_MAX - EIGMX_STATIC_LDS));
            eigmin_mx<T><<<nm, 576, eigmx_lds_bytes<T>(nmax), s>>>(d, out, redo);
          }
          HIPCHK(hipGetLastError());
          // the flagged blocks (clustered lambda_min) at the full width; the others exit at once
          lds_attr_once(attr2r, (const void*)eigmin_lds2<T>, (int)LDS_MAX);
          eigmin_lds2<T><<<nm, 512, eig2_lds_bytes<T>(nmax), s>>>(d, out, redo);
        }
        break;
      case CLRSDP_EIG_K_LDS2:
        if constexpr (!std::is_same<T, double>::value) {
          static std::atomic<unsigned long long> attr2{0};
          lds_attr_once(attr2, (const void*)eigmin_lds2<T>, (int)LDS_MAX);
          eigmin_lds2<T><<<nm, 512, eig2_lds_bytes<T>(nmax), s>>>(d, out);
        }
        break;
      case CLRSDP_EIG_K_LDS: {
        static std::atomic<unsigned long long> attr_t{0};
        lds_attr_once(attr_t, (const void*)eigmin_lds<T, true>, (int)LDS_MAX);
        eigmin_lds<T, true><<<nm, 512, eig_lds_bytes<T>(nmax), s>>>(d, out);
        break;
      }
      case CLRSDP_EIG_K_BLK:
        eigmin_chain(s, out);
        return;
      case CLRSDP_EIG_K_MXBLK:
        // the flagged blocks by the route the switch replaced; the others exit at once
        eigmin_mxblk(s, out);
        if (mx_fb_chain) {
          eigmin_chain(s, out, redo);
          return;
        }
        eigmin_batched<T><<<nm, 256, batched_lds(nmax), s>>>(d, out, redo);
        break;
      default:  // CLRSDP_EIG_K_BATCHED
        eigmin_batched<T><<<nm, 256, sizeof(T) * (4 * (size_t)nmax + 256), s>>>(d, out);
        break;
    }
    HIPCHK(hipGetLastError());
  }
};


// pivoted LU in place (the approx_lu! / approx_inv! fallback): getrf_batched, one workgroup per
// matrix, wherever its panel and U12 fit in LDS (fp64 n <= 624, dd 312, qd 156), and the blocked
// chain across workgroups beyond (getrf_blk_panel / _swap / _update per 16-column panel, looped
// here up to the batch's nmax: constant launch arguments, so the loop is capture-safe)
template <class T>
struct LuPlan : PlanBase {
  static constexpr int NB = 16, TL = 32;
  // the static LDS of the kernels (pivot search, pivots) comes on top of the dynamic panel
  static constexpr size_t LDS_DYN = LDS_MAX - 4096;
  std::vector<LuDesc<T>> h;
  LuDesc<T>* d = nullptr;
  int nmax = 0;
  void add(T* A, int* perm, int n, int lda) {
    h.push_back(LuDesc<T>{A, perm, n, lda});
    nmax = std::max(nmax, n);
  }
  static bool one_cu_fits(int n) { return getrf_lds_bytes<T, NB>(n) <= LDS_DYN; }
  // which kernel factors matrices up to n: the chain (true) or getrf_batched; E_ARG when neither.
  // `m` is CLRSDP_LU_BLK: unset (-1) the blocked LU chain (getrf_blk_*) where getrf_batched's
  // on-chip panel does not fit; 1 the chain at every size; 0 getrf_batched only
  static bool takes_chain(int n, int m) {
    if (m == 1 || (m < 0 && !one_cu_fits(n))) return true;
    if (!one_cu_fits(n))
      throw ClrsdpError{CLRSDP_E_ARG, "LU factorization: matrix too large for the on-chip panel of getrf_batched (CLRSDP_LU_BLK=0)"};
    return false;
  }
  size_t lds = 0;
  bool blk = false;
  bool panel_lds = true;  // CLRSDP_LU_PANEL_LDS=0: the chain's panel in global memory at every size
  int* pivs = nullptr;    // the chain's pivot rows of the current panel, NB per matrix
  // (outside any graph capture: the LDS attributes are set and the pivot scratch allocated here)
  void finalize(const Switches& sw) {
    if (h.empty()) return;
    blk = takes_chain(nmax, sw.lu_blk);
    d = own(h);
    if (blk) {
      pivs = own(std::vector<int>(h.size() * NB, 0));
      panel_lds = sw.lu_panel_lds;
      static std::atomic<unsigned long long> attr{0};
      lds_attr_once(attr, (const void*)getrf_blk_panel<T, NB, 256>, (int)LDS_DYN);
      return;
    }
    lds = getrf_lds_bytes<T, NB>(nmax);
    if (lds > 64 * 1024)
      HIPCHK(hipFuncSetAttribute((const void*)getrf_batched<T, NB, 256>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  void launch(hipStream_t s, int* info) const {
    if (h.empty()) return;
    if (!blk) {
      getrf_batched<T, NB, 256><<<(unsigned)h.size(), 256, lds, s>>>(d, info);
      HIPCHK(hipGetLastError());
      return;
    }
    const unsigned nm = (unsigned)h.size();
    for (int k0 = 0; k0 < nmax; k0 += NB) {
      // the panel of the largest matrix in LDS when it fits, else in place (smaller ones follow)
      const size_t pl = sizeof(T) * (size_t)NB * (nmax - k0);
      const bool in_lds = panel_lds && pl <= LDS_DYN;
      getrf_blk_panel<T, NB, 256><<<nm, 256, in_lds ? pl : 0, s>>>(d, pivs, info, k0, in_lds ? 1 : 0);
      if (nmax > NB) getrf_blk_swap<T, NB, 256><<<dim3(cdiv(nmax, 256), nm), 256, 0, s>>>(d, pivs, info, k0);
      const int nr = nmax - k0 - NB;
      if (nr > 0) {
        const int ntr = (int)cdiv(nr, TL);
        getrf_blk_update<T, NB, TL, 256><<<dim3((unsigned)(ntr * ntr), nm), 256, 0, s>>>(d, info, k0, ntr);
      }
    }
    HIPCHK(hipGetLastError());
  }
};

// row gathers out = in[perm, :] (or P I with ident)
template <class T>
struct PermPlan : PlanBase {
  std::vector<PermDesc<T>> h;
  PermDesc<T>* d = nullptr;
  long long emax = 0;
  void add(const T* in, int ldi, T* out, int ldo, const int* perm, int n, int ncol) {
    h.push_back(PermDesc<T>{in, out, perm, n, ncol, ldi, ldo});
    emax = std::max(emax, (long long)n * ncol);
  }
  void finalize() {
    if (!h.empty()) d = own(h);
  }
  void launch(hipStream_t s, bool ident = false) const {
    if (h.empty()) return;
    dim3 g(std::min<unsigned>(cdiv(emax, 256), 64), (unsigned)h.size());
    perm_rows<T><<<g, 256, 0, s>>>(d, ident ? 1 : 0);
    HIPCHK(hipGetLastError());
  }
};

template <class T>
struct CholInvPlan : PlanBase {  // A_b -> L_b^-1 (and optionally L_b, or A_b^-1)
  std::vector<MatDesc<T>> hin, hout, hl, hg;
  MatDesc<T>*din = nullptr, *dout = nullptr, *dl = nullptr, *dg = nullptr;
  // Whether a batch takes the form of chol_inv_tiles that also leaves A^-1 = L^-T L^-1 (the
  // product formed in the factorisation's launch instead of a GEMM behind it): fp64 on-chip
  // blocks up to 128, never where the inverse comes from the pivoted LU (lu_x() / lu_sq()), and
  // CLRSDP_CHOL_SPDINV=0 (`sw` false) keeps the GEMM.
  static bool spdinv_dispatch(int nmax, bool lu, bool sw) {
    return std::is_same<T, double>::value && sw && !lu && nmax >= 1 && nmax <= 128;
  }
  void add(T* A, int n, int lda, T* out, int ldo, T* L = nullptr) {
    hin.push_back(MatDesc<T>{A, n, lda});
    hout.push_back(MatDesc<T>{out, n, ldo});
    nmax = std::max(nmax, n);
    if (L) hl.push_back(MatDesc<T>{L, n, ldo});
  }
  // A_b^-1 of the matrix added last into G (pitch ldg), which must not alias its input or its
  // L^-1; matrices without one run the plain form.  Read by launch(.., true) only.
  void want_inverse(T* G, int ldg) {
    hg.resize(hin.size(), MatDesc<T>{nullptr, 0, 0});
    hg.back() = MatDesc<T>{G, hin.back().n, ldg};
  }
  int la_opts = 2;  // chol_lookahead's option bits, as finalize() was handed them
  void finalize(const Switches& sw) {
    if (hin.empty()) return;
    la_opts = sw.la_opts;
    din = own(hin);
    dout = own(hout);
    if (!hl.empty()) dl = own(hl);
    if (!hg.empty()) {
      hg.resize(hin.size(), MatDesc<T>{nullptr, 0, 0});
      dg = own(hg);
    }
  }
  int nmax = 0;
  // spdinv: the matrices that asked for A^-1 (want_inverse) get it; the caller decides by
  // spdinv_dispatch
  void launch(hipStream_t s, int* info, bool spdinv = false) const {
    if (hin.empty()) return;
    const unsigned nb = (unsigned)hin.size();
    if constexpr (std::is_same<T, double>::value) {
      if (spdinv) {
        if (!dg || nmax > 128) throw ClrsdpError{CLRSDP_E_ARG, "chol_inv_tiles with A^-1: n <= 128 and a target only"};
        if (nmax <= 32) go<32, true>(s, nb, info);
        else if (nmax <= 64) go<64, true>(s, nb, info);
        else go<128, true>(s, nb, info);
      } else if (nmax <= 32) go<32>(s, nb, info);
      else if (nmax <= 64) go<64>(s, nb, info);
      else if (nmax <= 128) go<128>(s, nb, info);
      else if (nmax <= 256) go<256>(s, nb, info);
      else throw ClrsdpError{CLRSDP_E_ARG, "on-chip fp64 factorisation with inverse (chol_inv_tiles): n <= 256 only"};
    } else {
      // chol_lookahead with L^-1 (quad-double: the square-root-free LDL form).  Blocks n <= 32
      // on 4 waves -- one per SIMD, the chain alone on its SIMD -- instead of 16 (C5's X/Y
      // blocks <= 18: 980 -> 1007 it/s, round 5); SKIP0 at 64 as potrf's
      constexpr bool LDL = std::is_same<T, mw::qd>::value;
      if (nmax <= 32) chol_lookahead<T, true, LDL, 32, 3><<<nb, 256, 0, s>>>(din, dout, dl, info, la_opts);
      else if (nmax <= 64) chol_lookahead<T, true, LDL, 64, 15, true><<<nb, 1024, 0, s>>>(din, dout, dl, info, la_opts);
      else throw ClrsdpError{CLRSDP_E_ARG, "on-chip multi-word factorisation with inverse: n <= 64 only"};
    }
    HIPCHK(hipGetLastError());
  }
  template <int NP, bool SPDINV = false>
  void go(hipStream_t s, unsigned nb, int* info) const {
    static_assert(sizeof(double) * CholTiles<NP>::END + sizeof(int) * CholTiles<NP>::NFLAGS <= LDS_MAX,
                  "chol_inv_tiles: LDS");
    const size_t lds = chol_inv_tiles_lds<NP>();
    // raised wave priority: the factorisation's chains keep their issue slots against the side
    // streams' GEMM waves on the same SIMDs
    constexpr int prio = 1;
    static std::atomic<unsigned long long> attr{0};
    lds_attr_once(attr, (const void*)chol_inv_tiles<NP, SPDINV>, (int)lds);
    chol_inv_tiles<NP, SPDINV><<<nb, CholTiles<NP>::NTH, lds, s>>>(
        reinterpret_cast<const MatDesc<double>*>(din), reinterpret_cast<const MatDesc<double>*>(dout), info,
        prio, SPDINV ? reinterpret_cast<const MatDesc<double>*>(dg) : nullptr);
  }
};

// ---- the launches of the reductions, the slab sums and the state update: one place for each
// kernel's grid, block, LDS size and op mapping, shared by the Solver's stages and by
// clrsdp_reduce / clrsdp_slab_sum / clrsdp_update_state
constexpr int RED_G = 256;  // fixed chunking of the flat reductions (deterministic)

// per-workgroup partials of sum a.*b (op 0), sum (a+da).*(b+db) (1) or max |a| (2) -> part[RED_G]
template <class T>
void launch_flat_reduce(hipStream_t s, const T* A, const T* B_, const T* dA, const T* dB,
                        long long n, int op, T* part) {
  flat_reduce<T><<<RED_G, 256, 0, s>>>(A, B_, dA, dB, n, op, part);
}
// one workgroup: sum a.*b (op 0), max |a| (2) or sum a (3) over [0, n) -> *dst
template <class T>
void launch_vec_reduce(hipStream_t s, const T* a, const T* b, long long n, int op, T* dst) {
  vec_reduce<T><<<1, vec_reduce_threads<T>(), 0, s>>>(a, b, n, op, dst);
}
// one-workgroup fixed-tree reduction of n partials of a flat op (sum, or max for op 2)
template <class T>
void launch_vec_reduce_tree(hipStream_t s, const T* in, int n, int op, T* dst) {
  launch_vec_reduce<T>(s, in, in, n, op == 2 ? 2 : 3, dst);
}
// the fold of RED_G flat_reduce partials of a flat op, as blk_dot queues it
template <class T>
FoldRed<T> flat_fold(const T* part, int op, int dst) {
  return FoldRed<T>{part, 1, RED_G, op == 2 ? 2 : 0, dst, 0};
}
// the pending folds in scalar_kernel launches of at most six; the last launch runs the scalar
// logic `which` (-1: none), the first one clears p.zero_n status words.  No fold: one launch.
template <class T>
void launch_folds(hipStream_t s, T* sc, ScalarParams<T> p, const std::vector<FoldRed<T>>& pend,
                  int which) {
  size_t q = 0;
  while (q < pend.size() || q == 0) {
    const size_t cnt = std::min<size_t>(6, pend.size() - q);
    p.nred = (int)cnt;
    for (size_t i = 0; i < cnt; ++i) p.red[i] = pend[q + i];
    q += cnt;
    const bool last = q >= pend.size();
    scalar_kernel<T><<<1, 64, 0, s>>>(sc, p, last ? which : -1);
    p.zero_n = 0;
    if (last) break;
  }
}
template <class T>
void launch_ordered_reduce(hipStream_t s, const T* in, int cnt, long long stride, int op, T* out) {
  ordered_reduce<T><<<1, 1, 0, s>>>(in, cnt, stride, op, out);
}
template <class T>
void launch_slab_sum4(hipStream_t s, const T* in, int cnt, long long stride, long long n, T* out,
                      const T* base = nullptr, double cbase = 0.0, double csum = 1.0,
                      T* out2 = nullptr) {
  slab_sum4<T><<<cdiv(n, 64), 256, 0, s>>>(in, cnt, stride, n, out, base, cbase, csum, out2);
}
inline size_t slab_qsolve_lds(long long n) { return ((size_t)n + 256) * sizeof(double); }
inline void launch_slab_qsolve(hipStream_t s, const double* in, int cnt, long long stride, int n,
                               const double* base, double cbase, double csum, const double* Q,
                               int ldq, double* out) {
  slab_qsolve<<<cdiv(n, 64), 256, slab_qsolve_lds(n), s>>>(in, cnt, stride, n, base, cbase, csum, Q,
                                                           ldq, out);
}
template <class T>
void launch_update_state(hipStream_t s, T* X, const T* dX, T* Y, const T* dY, long long nel, T* x,
                         const T* dx, long long nx, const T* cv, T* y, const T* dy, long long ny,
                         const T* bv, const T* alpha_p, const T* alpha_d, const int* info, int ninfo,
                         T* part, const StepAlpha<T>& sa) {
  update_state<T><<<RED_G, 256, 0, s>>>(X, dX, Y, dY, nel, x, dx, nx, cv, y, dy, ny, bv, alpha_p,
                                        alpha_d, info, ninfo, part, sa);
}

// What clrsdp_handoff_state needs of a handle, whatever its word type: the four state arrays
// (arrays of limb structs, `words` doubles per element), their counts, and a signature of the
// description, rank, world size and owned set (equal signatures: equal local layouts).
struct StateView {
  void *x = nullptr, *X = nullptr, *Y = nullptr, *y = nullptr;
  int64_t nx = 0, nblk_el = 0, n_y = 0;
  int words = 0, dev = 0, inflight = 0;
  bool has_state = false;
  hipStream_t stream = nullptr;
  std::vector<int64_t> sig;
};

template <class TS, class TD>
void launch_state_convert(hipStream_t s, const StateView& src, const StateView& dst) {
  const long long tot = (long long)src.nx + 2 * (long long)src.nblk_el + (long long)src.n_y;
  if (tot <= 0) return;
  const StateSegs<const TS> a{static_cast<const TS*>(src.x), static_cast<const TS*>(src.X),
                              static_cast<const TS*>(src.Y), static_cast<const TS*>(src.y),
                              src.nx, src.nblk_el, src.n_y};
  const StateSegs<TD> b{static_cast<TD*>(dst.x), static_cast<TD*>(dst.X), static_cast<TD*>(dst.Y),
                        static_cast<TD*>(dst.y), dst.nx, dst.nblk_el, dst.n_y};
  state_convert<TS, TD><<<(unsigned)std::min<long long>((tot + 255) / 256, 2048), 256, 0, s>>>(a, b);
}
// the nine (source, destination) word pairs, by the index of the width (1, 2, 4 words)
using StateConvertFn = void (*)(hipStream_t, const StateView&, const StateView&);
inline int width_index(int words) { return words == 1 ? 0 : words == 2 ? 1 : words == 4 ? 2 : -1; }
static const StateConvertFn state_convert_fn[3][3] = {
    {launch_state_convert<double, double>, launch_state_convert<double, dd>, launch_state_convert<double, qd>},
    {launch_state_convert<dd, double>, launch_state_convert<dd, dd>, launch_state_convert<dd, qd>},
    {launch_state_convert<qd, double>, launch_state_convert<qd, dd>, launch_state_convert<qd, qd>}};

struct HandleBase {
  // the switches as they stood when the handle was created: its plans, the members a switch
  // decides and every loop body captured later follow them (the LU plans: Solver::lu_sw)
  const Switches sw = Switches::read();
  std::string err;
  int dev = 0;  // the handle's HIP device (every C-ABI call on the handle runs with it current)
  virtual StateView state_view() const = 0;
  virtual void adopt_state() = 0;  // the bookkeeping of set_state after the state was written on the device
  virtual ~HandleBase() {}
  virtual void upload(const double* V, const double* lam, const double* B, const double* c,
                      const double* b, const double* C) = 0;
  virtual void set_state(const double* x, const double* X, const double* y, const double* Y) = 0;
  virtual void get_state(double* x, double* X, double* y, double* Y) = 0;
  virtual int initial(const clrsdp_params* prm, clrsdp_iter_stats* st) = 0;
  virtual int iterate(const clrsdp_params* prm, int pd_feas, clrsdp_iter_stats* st) = 0;
  virtual void set_control(const clrsdp_control* c) = 0;
  virtual int iterate_async(const clrsdp_params* prm) = 0;
  virtual int iterate_wait(clrsdp_iter_stats* st, int* ran) = 0;
  virtual int run_stage(int stage, const clrsdp_params* prm, int pd_feas) = 0;
  virtual void get_buffer(int buf, double* host, int64_t* count) = 0;
  virtual int64_t exchange_bytes() const = 0;
  virtual void set_exchange(clrsdp_exchange_fn fn, void* ctx, void* send, void* recv) = 0;
  virtual void comm_init(const uint8_t* id) = 0;
  virtual void set_stream(void* s) = 0;
  virtual void* get_stream() const = 0;
  virtual void synchronize() = 0;
  virtual void set_timing(int on) = 0;
  virtual void save_state() = 0;
  virtual void restore_state() = 0;
  virtual void set_factorization(int flags) = 0;
  virtual int get_factorization() const = 0;
  virtual void set_graph(int on) = 0;
  virtual void comm_info(int* nranks, int* backend) const = 0;
  virtual void schur_info(struct clrsdp_schur_info* out) const = 0;
  virtual void apply_operator(int op, const clrsdp_operands* a, int32_t* route) = 0;
};

template <class T>
struct Solver final : HandleBase {
  // ---------------- configuration / global description
  int rank = 0, world = 1, timing = 0, W = Num<T>::W;
  int64_t J = 0, n_y = 0;
  std::vector<int64_t> m, Lc, Ns, Ds, xoff_g;    // per cluster
  std::vector<int64_t> jl_first;                 // first (j,l) index of cluster j
  std::vector<int64_t> delta, Kb, nb_g, blkoff_g, voff_g, koff_g;  // per (j,l)
  std::vector<int64_t> rkoff_g;                  // offset into ranks[] of (j,l)
  std::vector<int64_t> ranks_all;
  std::vector<int64_t> Boff_g;                   // per cluster offset in global B
  int64_t tot_x = 0, tot_blk = 0, tot_V = 0, tot_K = 0, tot_B = 0;
  double dimtot = 0;

  // ---------------- local (owned) layout
  std::vector<int> oc;                       // owned clusters (global ids)
  struct LBlk { int c, l; int64_t gjl; int n, del, K, m, N; int64_t off, voff, koff, toff, boff, ayoff, rsoff; };
  std::vector<LBlk> lb;
  std::vector<int64_t> c_xoff, c_Soff, c_Boff;   // per local cluster
  int64_t nx = 0, nblk_el = 0, nV = 0, nK = 0, nT = 0, nBX = 0, nAY = 0, nS = 0, nB = 0, nRS = 0;
  bool anyMgt1 = false, hasC = false;
  bool mw_pair_upper = false;  // BX / BY hold their upper triangles only (schur_assemble reads (min, max))
  int nc2 = 0;  // clusters factorised as 2x2 blocks (s_single < dim_S <= 256, fp64)
  // the largest fp64 S_j factorised (and inverted) by ONE chol_inv_tiles launch: 256 with
  // CLRSDP_CHOL256=1 (chol_inv_tiles<256>, 768 threads: no 2x2 blocking, no X21 / W1 side
  // products), else 128
  const int s_single = (std::is_same<T, double>::value && sw.chol256) ? 256 : 128;
  bool s_lower = false;  // the last SCHUR enqueued assembled the lower triangle of S only
  int schur_full = -1;   // the `full` of the last SCHUR enqueued (-1: none yet), for schur_info

  // ---------------- device memory
  hipStream_t own_stream = nullptr, stream = nullptr;
  T *X, *Y, *Xinv, *LX, *LY, *R, *P, *dX, *dY, *Z, *tA, *tB, *Cm;
  T *V, *lam, *TX, *TY, *BX, *BY, *AY, *tval, *S, *Wm, *Bm, *Qslab, *Q, *Qf, *Qinv;
  T *TU, *TW;  // trace_A products U = Z V and the scaled vectors of compute_weighted_A (own
               // buffers: they are produced on the side stream while SCHUR uses TX/TY)
  T *cvec, *x, *dx, *dvec, *rhs, *tvec, *tmpv, *pslab, *y, *bvec, *dyv, *pvec, *uvec;
  T *sc, *bpart, *upart = nullptr, *eigX, *eigY, *tmpsc, *tC = nullptr, *Stmp = nullptr;
  T* Vt = nullptr;  // per block V^T (K x delta), fused Schur path only
  int *ksamp, *rsums, *info;
  T *xsend = nullptr, *xrecv = nullptr, *own_send = nullptr;
  int64_t xcap = 0;  // exchange capacity in T values
  clrsdp_exchange_fn xfn = nullptr;
  void* xctx = nullptr;
  ncclComm_t comm = nullptr;    // native RCCL communicator (clrsdp_comm_init)
  T* comm_recv = nullptr;       // world * xcap values, rank r's partials at r * cnt
  int device = 0;
  bool uploaded = false;
  int info_count = 0, info_S0 = 0, info_Q0 = 0, info_Y0 = 0, info_H = 0;
  int info_L0 = 0;  // status words of X^-1 by LU (one per block)
  int info_G = 0;   // world > 1: the failure bits of every rank, OR-ed (STEP's exchange)
  // ---------------- the LU fallback (approx_lu! / approx_inv!, MPMP.jl:774-786, 1436, 1501):
  // Cholesky first; when a Cholesky status word fires, the loop body is re-run with pivoted LU
  // for S_j and Q (or for X^-1), and LU stays on for the rest of the solve, as the reference
  // switches spd_inv! off.  CLRSDP_FACT_LU_SQ from the start is the reference's own choice.
  int fact_flags = CLRSDP_FACT_FALLBACK;
  bool lu_built = false;
  int* lperm = nullptr;  // row permutations: S_j (at the cluster's x offset), Q, X blocks
  T* W2m = nullptr;      // U_j^-T B_j  (the transposed B_j^T U_j^-1, MPMP.jl:1457-1460)
  bool lu_sq() const { return (fact_flags & CLRSDP_FACT_LU_SQ) != 0; }
  bool lu_x() const { return (fact_flags & CLRSDP_FACT_LU_X) != 0; }
  // pipelined loop (iterate_async / iterate_wait): device-side loop control and results copy
  T gap_thr{}, p_thr{}, d_thr{};
  int need_p = 0, need_d = 0;
  T *Pres = nullptr, *pres = nullptr, *dres = nullptr;  // P, p, d of the last loop body that ran
  bool res_from_copy = false;

  // ---------------- plans
  PlanBase descs;  // owner of the stage descriptor arrays below (d_blk, d_pair, ...)
  GemmPlan<T> p_XY, p_dXdY, p_xinv, p_s1x, p_s1y, p_s2x, p_s2y, p_Q, p_wA_P, p_wA_dX, p_trU_Z,
      p_trU_Y, p_By, p_Btx, p_Wt, p_Wdy, p_PY, p_Z, p_dXY, p_dY;
  TrsmPlan<T> t_Linv, t_W, t_t, t_Q, t_sX1, t_sX2, t_sY1, t_sY2;
  MatPlan<T> f_X, f_Y, f_S, f_Q, e_X, e_Y;
  // on-chip factorisation path (all sizes <= reg_nmax<T>()): L^-1 and MFMA products
  bool reg_blk = false, reg_S = false, reg_Q = false;
  // fp64: chol_inv_tiles leaves X^-1 / Q^-1 beside L^-1 (CholInvPlan::spdinv_dispatch; without
  // the LU fallback, which st_xinv / factor_q_ look at when they launch); CLRSDP_CHOL_SPDINV=0:
  // the GEMMs q_xinv / p_xir and q_qinv behind the factorisation (per handle: tests switch it)
  bool spd_xy = false, spd_q = false;
  CholInvPlan<T> ci_XY, ci_S, ci_S22, ci_Q;
  GemmPlan<T> q_xinv, q_sx1, q_sx2, q_sy1, q_sy2, q_W, q_t, q_Wdy, q_dx, q_q1, q_q2, q_qinv, q_qdy;
  // fp64, uniform blocks: Z, dY and the step-length products as one strip-chain launch each
  ChainPlan c_Z, c_dY, c_step, c_trZ;
  ChainPlan c_stepX, c_stepY;             // the step-length congruences apart (xy_ov)
  MatPlan<T> e_Xs, e_Ys;                  // their eigen launches apart
  bool xy_ov_ok = false;   // the overlapped step length is configured (small batches, opt-in)
  // fp64 FACTOR with every dim_S <= 256 (fac2): f_a = {W = L^-1 B | L21^T = L11^-1 S12, W1} and
  // f_b = {W^T W | S22 - L21 L21^T, W1^T W1, B2 - L21 W1} as mixed batches, then (dim_S > 128)
  // chol_inv(S22), f_c: W2 = L22^-1 B2', f_d: slab += W2^T W2 (measured 1% faster than one
  // W^T W product after W2); f_x1/f_x2: X21 (side stream)
  GemmPlan<T> f_a, f_b, f_c, f_d, f_x1, f_x2;
  // the 2x2-blocked clusters' {W1 = L11^-1 B1} and {W1^T W1, B2 - L21 W1}: off the chain
  // chol(S11) -> L21^T -> S22 - L21 L21^T -> chol(S22'), so a loop body runs them on a second side
  // stream beside it (joined before W2 = L22^-1 B2')
  GemmPlan<T> f_w, f_w2;
  bool fac2 = false;
  T* B2p = nullptr;
  // weighted A with the column scaling inside the GEMM's slab staging (fp64, every local block
  // m = L = 1 with rank-1 samples): no scale_cols launch, no scaled copy of V
  bool wa_fused = false;
  GemmPlan<T> p_wA_Ps, p_wA_dXs;
  // multi-word S_j / Q beyond reg_nmax in the split form: potrf on the critical path,
  // L^-1 by four-wave triangular solves of the identity (S_j: on aux2, off the critical path),
  // then the same GEMV solves as the explicit-inverse path
  bool s_split = false, q_split = false;
  bool qf_fresh = false;  // sum_q_slabs wrote Qf = Q for this iteration's factor_q_
  T *SLi = nullptr, *QLi = nullptr;  // L^-1 of the S_j and of Q
  TrsmPlan<T> t_Sinv, t_Qinv;
  GemmPlan<T> q_t2, q_dx2, q_qinv2;
  MatPlan<T> e_XY;                        // both step-length eigenproblems in one launch
  // LU fallback plans (built on the first switch)
  LuPlan<T> lu_S, lu_Q, lu_X;
  PermPlan<T> pm_B, pm_rhs, pm_r, pm_I;
  TrsmPlan<T> tl_W1, tl_W2, tl_t, tl_dx, tl_Q1, tl_Q2, tl_X1, tl_X2;
  GemmPlan<T> lq_slab, lq_Wt;
  BlkDesc* d_blk = nullptr;      // all local blocks
  BlkDesc* d_blk_m = nullptr;    // local blocks with m > 1
  int n_blk_m = 0;
  // fused Schur path (fp64, every local block m = 1): TXt/TYt = V^T X^-1 / V^T Y, then the
  // paired Hadamard tiles; clusters with L > 1 or ranks != 1 are summed from G (BX arena)
  bool fast_schur = false;
  GemmPlan<T> p_txy, p_ty;  // V^T X^-1 (SCHUR) and V^T Y (ahead on the side stream in a loop body)
  PairTileDesc* d_ptd = nullptr;
  TileRef* d_pt2d = nullptr;
  int n_ptiles = 0;
  // schur_fused_f64 (every local block delta <= 128): V^T X^-1 formed on chip, one workgroup
  // per 64-row block; CLRSDP_SCHUR_FUSED=0 keeps the V^T X^-1 GEMM + schur_pairs_f64 pair
  bool schur_fused = false;
  bool fused_one = false;   // schur_fused_f64<.., .., .., true>: one column tile per workgroup (small batches)
  bool fused_d64 = false;   // schur_fused_f64<.., .., .., true, true>: the ONE form at delta <= 64
  bool fused_grp2 = false;  // schur_fused_f64<.., .., true>: the rank-2 group-sum epilogue (every block grp = 2)
  bool fused_y = false;  // schur_fused_f64<0, true>: V^T Y on chip too (no p_ty); CLRSDP_SCHUR_FUSED_Y=0
  FusedPairDesc* d_fpd = nullptr;
  TileRef* d_fpt2d = nullptr;
  int n_fwg = 0;
  SchurClusterDesc* d_gcd = nullptr;  // clusters summed by schur_gsum
  int n_gsum = 0, max_gD = 0;
  SchurClusterDesc* d_scd = nullptr;
  SchurBlockDesc* d_sbd = nullptr;
  long long n_pairs = 0;
  AYDesc* d_ayd = nullptr;
  PairDesc* d_pair = nullptr;
  // <X + dX, Y + dY> partials from the predictor's dY chain (dotp, dy_dot_cnt of them)
  T* dotp = nullptr;
  int dy_dot_cnt = 0;
  bool dy_dot_ok = false;
  // fp64 cluster solves in two launches (cl_solve_t / cl_solve_dx): one descriptor per cluster,
  // cls_nrb 64-row blocks per cluster (the partial slabs: nc x cls_nrb x n_y in pslab)
  std::vector<ClSolveDesc> h_cls;
  ClSolveDesc* d_cls = nullptr;
  int cls_nrb = 0;
  bool cls_on = false;
  bool trivial_tuples = false;
  int n_pair = 0, max_K = 0;
  ScaleDesc* d_scale = nullptr;
  TupleDesc* d_td = nullptr;
  TupleBlock* d_tb = nullptr;
  hipEvent_t ev[CLRSDP_NUM_STAGES + 1];
  // timing mode 1: inner buckets (CLRSDP_INNER_*), one event pair per segment, recorded on the
  // stream the segment's launches go to (so side-stream work is measured on its own stream)
  std::vector<hipEvent_t> seg_pool;
  std::vector<std::array<int, 3>> segs;  // (bucket, begin event, end event)
  template <class F>
  void seg(int bucket, F&& work) {
    if (timing != 1) {
      work();
      return;
    }
    const int b = (int)segs.size() * 2;
    while ((int)seg_pool.size() < b + 2) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      seg_pool.push_back(e);
    }
    HIPCHK(hipEventRecord(seg_pool[b], stream));
    work();
    HIPCHK(hipEventRecord(seg_pool[b + 1], stream));
    segs.push_back({bucket, b, b + 1});
  }
  // side stream: the local residuals overlap the Schur factorisation, chol(Q) overlaps the
  // first part of the predictor (iterate only; run_stage stays serial)
  hipStream_t aux = nullptr, aux2 = nullptr;
  // events that only order a fork (fork() below) or a join written out where it happens (EV_R in
  // enqueue_iteration, EV_JOIN / EV_JOIN2 after a failed capture): nobody keeps a flag for them
  enum ForkEv { EV_M, EV_S, EV_QA, EV_R, EV_FA, EV_X2, EV_SP, EV_DXO, EV_JOIN, EV_JOIN2, N_FORK_EV };
  hipEvent_t fev[N_FORK_EV] = {};
  // work on `to` behind everything enqueued on `stream` so far: `stream` is `to` while work() runs
  template <class F>
  void fork(hipEvent_t e, hipStream_t to, F&& work) {
    HIPCHK(hipEventRecord(e, stream));
    HIPCHK(hipStreamWaitEvent(to, e, 0));
    StreamSwitch on_to(stream, to);  // restored on scope exit, also when a launch throws
    work();
  }
  // The hand-offs of a loop body: each is signalled on the stream that produced the work and
  // joined where it is first read.  A new one is a new member and one line in handoffs[]; the
  // order of handoffs[] is the order of the drain at the end of enqueue_iteration.
  Handoff h_stx;   // aux -> main: lambda_min of the X step (direction_rest, xy_ov); joined by st_step
  Handoff h_q;     // aux -> main: L_Q^-1, Q^-1 (enqueue_iteration, !q_main); joined before the Q solve
  Handoff h_x21;   // aux2 -> the stream of solve_head / direction_solves: X21 (factor_local, fac2 with S22)
  Handoff h_sinv;  // aux2 -> the stream of solve_head: L_j^-1 (factor_local, s_split)
  Handoff h_ty;    // aux -> main: V^T Y (enqueue_iteration, ty_side); joined by st_schur
  Handoff h_w;     // aux2 -> main (factor_local, wait) and aux (enqueue_iteration, join): W1^T W1, B2'
  Handoff* const handoffs[6] = {&h_stx, &h_q, &h_x21, &h_sinv, &h_ty, &h_w};
  // What changes how ONE loop body is enqueued; all false between bodies (reset_body_state()).
  //   fuse_r       set by enqueue_iteration before MU_R (fp64, not timing mode 1), cleared by it
  //                after XINV: R = mu_p I - XY rides in XINV's launch (st_mu_r, st_xinv)
  //   fuse_alpha   set by enqueue_iteration before CORRECTOR_R (not timing mode 1), cleared by it
  //                after UPDATE: st_step leaves alpha to UPDATE's launch
  //   alpha_fused  set by st_step when it did so, cleared by the st_update that forms alpha
  //   xy_ov_body   set and cleared by enqueue_iteration beside fuse_alpha: the corrector's
  //                direction_rest may fork the X step length (it then signals h_stx)
  //   r_late       set by st_xinv in a fuse_r body whose XINV is one launch (spd_xy: no GEMM to
  //                carry R), cleared by enqueue_iteration, which forms R at the head of the side
  //                stream's work after SCHUR
  //   head_ahead   set by enqueue_iteration (q_main) after solve_head ran on the side stream,
  //                cleared by the predictor's direction_solves, which then skips it
  //   dy_dot_ready set by the predictor's direction_rest when its dY chain left the
  //                <X + dX, Y + dY> partials, cleared by st_corrector_r (and by a new state:
  //                set_state, restore_state)
  struct BodyFlags {
    bool fuse_r = false, fuse_alpha = false, alpha_fused = false, xy_ov_body = false,
         head_ahead = false, dy_dot_ready = false, r_late = false;
  } body;
  float phase_ms[CLRSDP_NUM_STAGES];

  int nb() const { return (int)lb.size(); }
  int nc() const { return (int)oc.size(); }

  Solver(const clrsdp_desc* desc, const clrsdp_config* cfg) {
    rank = cfg->rank;
    world = std::max(1, (int)cfg->world_size);
    timing = cfg->timing;
    device = cfg->device;
    dev = cfg->device;
    HIPCHK(hipSetDevice(cfg->device));  // (clrsdp_create restores the caller's device)
    J = desc->J;
    n_y = desc->n_y;
    if (J <= 0 || n_y <= 0) throw ClrsdpError{CLRSDP_E_ARG, "J and n_y must be positive"};
    m.assign(desc->m, desc->m + J);
    Lc.assign(desc->L, desc->L + J);
    Ns.assign(desc->n_samples, desc->n_samples + J);
    int64_t njl = 0;
    for (int64_t j = 0; j < J; ++j) {
      if (m[j] <= 0 || Lc[j] <= 0 || Ns[j] <= 0) throw ClrsdpError{CLRSDP_E_ARG, "bad m/L/N"};
      Ds.push_back(m[j] * (m[j] + 1) / 2 * Ns[j]);
      xoff_g.push_back(tot_x);
      tot_x += Ds[j];
      jl_first.push_back(njl);
      njl += Lc[j];
      Boff_g.push_back(tot_B);
      tot_B += Ds[j] * n_y;
    }
    jl_first.push_back(njl);
    int64_t rk = 0;
    for (int64_t j = 0; j < J; ++j)
      for (int64_t l = 0; l < Lc[j]; ++l) {
        const int64_t g = jl_first[j] + l;
        const int64_t del = desc->delta[g];
        if (del <= 0) throw ClrsdpError{CLRSDP_E_ARG, "bad delta"};
        delta.push_back(del);
        rkoff_g.push_back(rk);
        int64_t K = 0;
        for (int64_t k = 0; k < Ns[j]; ++k) {
          if (desc->ranks[rk + k] < 0) throw ClrsdpError{CLRSDP_E_ARG, "negative rank"};
          K += desc->ranks[rk + k];
          ranks_all.push_back(desc->ranks[rk + k]);
        }
        rk += Ns[j];
        if (K <= 0) throw ClrsdpError{CLRSDP_E_ARG, "block without vectors"};
        Kb.push_back(K);
        const int64_t n = m[j] * del;
        nb_g.push_back(n);
        blkoff_g.push_back(tot_blk);
        tot_blk += n * n;
        voff_g.push_back(tot_V);
        tot_V += del * K;
        koff_g.push_back(tot_K);
        tot_K += K;
        dimtot += (double)n;
      }
    // owned clusters
    if (cfg->owned && cfg->n_owned > 0) {
      for (int i = 0; i < cfg->n_owned; ++i) {
        if (cfg->owned[i] < 0 || cfg->owned[i] >= J) throw ClrsdpError{CLRSDP_E_ARG, "bad owned id"};
        oc.push_back(cfg->owned[i]);
      }
      std::sort(oc.begin(), oc.end());
    } else if (world == 1) {
      for (int j = 0; j < J; ++j) oc.push_back(j);
    }
    // local layout
    for (int c = 0; c < (int)oc.size(); ++c) {
      const int j = oc[c];
      c_xoff.push_back(nx);
      nx += Ds[j];
      c_Soff.push_back(nS);
      nS += Ds[j] * Ds[j];
      c_Boff.push_back(nB);
      nB += Ds[j] * n_y;
      if (std::is_same<T, double>::value && Ds[j] > s_single && Ds[j] <= 256) ++nc2;
      if (m[j] > 1) anyMgt1 = true;
      for (int l = 0; l < Lc[j]; ++l) {
        LBlk b;
        b.c = c; b.l = l; b.gjl = jl_first[j] + l;
        b.n = (int)nb_g[b.gjl]; b.del = (int)delta[b.gjl]; b.K = (int)Kb[b.gjl];
        b.m = (int)m[j]; b.N = (int)Ns[j];
        b.off = nblk_el; nblk_el += (int64_t)b.n * b.n;
        b.voff = nV; nV += (int64_t)b.del * b.K;
        b.koff = nK; nK += b.K;
        b.toff = nT; nT += (int64_t)b.n * b.m * b.K;
        b.boff = nBX; nBX += (int64_t)b.m * b.K * b.m * b.K;
        b.ayoff = nAY; nAY += (int64_t)b.m * (b.m + 1) / 2 * b.K;
        b.rsoff = nRS; nRS += b.N + 1;
        max_K = std::max(max_K, b.K);
        lb.push_back(b);
      }
    }
    fast_schur = std::is_same<T, double>::value && !anyMgt1 && nb() > 0;
    HIPCHK(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
    stream = own_stream;
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&aux2, hipStreamNonBlocking));
    for (hipEvent_t& e : fev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (Handoff* h : handoffs) h->create();
    allocate();
    build_plans();
  }

  ~Solver() override {
    // device memory is released with the process / hipDeviceReset; free what we own explicitly
    T* bufs[] = {X, Y, Xinv, LX, LY, R, P, dX, dY, Z, tA, tB, Cm, V, lam, TX, TY, TU, TW, BX, BY, AY,
                 tval, S, Wm, Bm, Qslab, Q, Qf, Qinv, cvec, x, dx, dvec, rhs, tvec, tmpv, pslab, y,
                 bvec, dyv, pvec, uvec, bpart, upart, eigX, tmpsc, tC, Stmp, B2p, own_send, Vt, Pres, pres, dres,
                 W2m};
    for (T* p : bufs)
      if (p) (void)hipFree(p);
    if (comm) {
      (void)hipStreamSynchronize(stream);
      (void)rccl().comm_destroy(comm);
    }
    if (comm_recv) (void)hipFree(comm_recv);
    if (snap) (void)hipFree(snap);
    if (dotp) (void)hipFree(dotp);
    (void)hipFree(ksamp);
    (void)hipFree(rsums);
    if (lperm) (void)hipFree(lperm);
    if (stat_dev) (void)hipFree(stat_dev);
    if (stat_host) (void)hipHostFree(stat_host);
    for (char* r : ring_host)
      if (r) (void)hipHostFree(r);
    for (auto& e : ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : seg_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : fev)
      if (e) (void)hipEventDestroy(e);
    for (Handoff* h : handoffs) h->destroy();
    for (hipEvent_t e : ring_ev)
      if (e) (void)hipEventDestroy(e);
    for (hipGraphExec_t g : gexec)
      if (g) (void)hipGraphExecDestroy(g);
    if (aux) (void)hipStreamDestroy(aux);
    if (aux2) (void)hipStreamDestroy(aux2);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }

  void allocate() {
    const int64_t B = std::max<int64_t>(nblk_el, 1);
    X = dmalloc<T>(B); Y = dmalloc<T>(B); Xinv = dmalloc<T>(B); LX = dmalloc<T>(B);
    LY = dmalloc<T>(B); R = dmalloc<T>(B); P = dmalloc<T>(B); dX = dmalloc<T>(B);
    dY = dmalloc<T>(B); Z = dmalloc<T>(B); tA = dmalloc<T>(B); tB = dmalloc<T>(B);
    Cm = dmalloc<T>(B);
    V = dmalloc<T>(nV); lam = dmalloc<T>(nK);
    // TX / TY: the Schur-stage products; TU / TW (same slot layout, m(m+1)/2 * delta*K <=
    // (m delta)(m K) per block): the trace_A products U and the scaled vectors of
    // compute_weighted_A
    TX = dmalloc<T>(nT); TY = dmalloc<T>(nT); TU = dmalloc<T>(nT); TW = dmalloc<T>(nT);
    BX = dmalloc<T>(nBX); BY = dmalloc<T>(nBX);
    AY = dmalloc<T>(nAY); tval = dmalloc<T>(nAY);
    S = dmalloc<T>(nS); Wm = dmalloc<T>(nB); Bm = dmalloc<T>(nB);
    Qslab = dmalloc<T>((size_t)std::max(nc(), 1) * n_y * n_y);
    Q = dmalloc<T>(n_y * n_y); Qf = dmalloc<T>(n_y * n_y); Qinv = dmalloc<T>(n_y * n_y);
    cvec = dmalloc<T>(nx); x = dmalloc<T>(nx); dx = dmalloc<T>(nx); dvec = dmalloc<T>(nx);
    rhs = dmalloc<T>(nx); tvec = dmalloc<T>(nx); tmpv = dmalloc<T>(nx);
    pslab = dmalloc<T>((size_t)std::max(nc(), 1) * 4 * n_y);  // (x 4: cl_solve_t's row blocks)
    y = dmalloc<T>(n_y); bvec = dmalloc<T>(n_y); dyv = dmalloc<T>(n_y); pvec = dmalloc<T>(n_y);
    Pres = dmalloc<T>(std::max<int64_t>(nblk_el, 1)); pres = dmalloc<T>(std::max<int64_t>(n_y, 1));
    dres = dmalloc<T>(std::max<int64_t>(nx, 1));
    uvec = dmalloc<T>(n_y);
    // sc and the status words share one allocation (one D2H copy per iteration, pinned host
    // mirror) -- see stat_alloc()
    bpart = dmalloc<T>(std::max(nb(), 256));
    upart = dmalloc<T>(3 * RED_G);  // update_state's partial sums
    eigX = dmalloc<T>(2 * std::max(nb(), 1));
    eigY = eigX + std::max(nb(), 1);  // X-side and Y-side minima of one batched eigen launch
    tC = dmalloc<T>(B);
    {
      int64_t ns = 0;
      for (int c = 0; c < nc(); ++c)
        if (std::is_same<T, double>::value && Ds[oc[c]] > s_single && Ds[oc[c]] <= 256) ns += 2 * (Ds[oc[c]] - 128) * 128;
      Stmp = dmalloc<T>(ns);
      int64_t nb2 = 0;
      for (int c = 0; c < nc(); ++c)
        if (std::is_same<T, double>::value && Ds[oc[c]] > s_single && Ds[oc[c]] <= 256) nb2 += (Ds[oc[c]] - 128) * n_y;
      B2p = dmalloc<T>(nb2);
    }
    tmpsc = dmalloc<T>(8);
    ksamp = dmalloc<int>(nK);
    rsums = dmalloc<int>(nRS);
    if (fast_schur) Vt = dmalloc<T>(std::max<int64_t>(nV, 1));
    // info layout: [X: nb][Y: nb][S: nc single + nc2 second blocks][Q: 1][X by LU: nb]
    // [gathered failure bits: 1][halt: 1 (last; not zeroed)]
    info_count = 3 * nb() + nc() + nc2 + 1 + 1 + 1;
    info_H = info_count - 1;
    info_Y0 = nb();
    info_S0 = 2 * nb();
    info_Q0 = 2 * nb() + nc() + nc2;
    info_L0 = info_Q0 + 1;
    info_G = info_L0 + nb();
    stat_alloc();
    xcap = n_y * n_y + n_y + 16;
    own_send = dmalloc<T>(xcap);
    xsend = own_send;
    xrecv = own_send;
    // sample index of every vector column and the rank prefix sums, per local block
    std::vector<int> ks(nK), rs(nRS);
    for (const LBlk& b : lb) {
      const int64_t r0 = rkoff_g[b.gjl];
      int acc = 0, col = 0;
      for (int k = 0; k < b.N; ++k) {
        rs[b.rsoff + k] = acc;
        for (int q = 0; q < ranks_all[r0 + k]; ++q) ks[b.koff + col++] = k;
        acc += (int)ranks_all[r0 + k];
      }
      rs[b.rsoff + b.N] = acc;
    }
    if (nK) HIPCHK(hipMemcpy(ksamp, ks.data(), nK * sizeof(int), hipMemcpyHostToDevice));
    if (nRS) HIPCHK(hipMemcpy(rsums, rs.data(), nRS * sizeof(int), hipMemcpyHostToDevice));
  }

  void build_plans() {
    {
      int nmax_b = 0, nmax_S = 0;
      for (const LBlk& b : lb) nmax_b = std::max(nmax_b, b.n);
      for (int c = 0; c < nc(); ++c) nmax_S = std::max(nmax_S, (int)Ds[oc[c]]);
      reg_blk = nmax_b <= reg_nmax<T>();
      reg_S = nmax_S <= (std::is_same<T, double>::value ? 2 : 1) * reg_nmax<T>();
      reg_Q = n_y <= reg_nmax<T>();
      spd_xy = reg_blk && nb() && CholInvPlan<T>::spdinv_dispatch(nmax_b, false, sw.chol_spdinv);
      spd_q = reg_Q && CholInvPlan<T>::spdinv_dispatch((int)n_y, false, sw.chol_spdinv);
      // multi-word S_j / Q beyond the on-chip inverse: GEMV solves with L^-1 instead of the
      // serial multi-word vector solves (four 41-us trsv_wave chains per direction at C5), in the
      // split form: potrf on the critical path and L^-1 = L \ I by four-wave solves (S_j's beside
      // W_j and the Q chain).  Double-double S_j up to 128: trsv_wave128 forms L^-1 as it does
      // the vector solves.  (DESIGN.md §13 has the round-5 A/B against the other forms.)
      if (!std::is_same<T, double>::value) {
        s_split = !reg_S && nmax_S <= (std::is_same<T, mw::dd>::value ? 128 : 64);
        q_split = !reg_Q && n_y <= 64;
      }
    }
    q_xinv.ta = true;
    q_sx2.tb = q_sy2.tb = true;
    // L^-1 dM L^-T exactly symmetric: eigmin_split reads it without a transposed copy
    q_sx2.sym = std::is_same<T, double>::value;
    f_d.ta = true;
    f_x1.tb = true;
    fac2 = std::is_same<T, double>::value && reg_S;
    q_dx.ta = true;
    q_q2.ta = true;
    p_xinv.ta = true;
    p_s2x.ta = p_s2y.ta = true;
    // (multi-word, every block m = 1: only the upper tiles of the symmetric pairings; CLRSDP_MW_PAIR_UPPER=0
    // computes both triangles)
    mw_pair_upper = !std::is_same<T, double>::value && !anyMgt1 && sw.mw_pair_upper;
    p_s2x.upper = p_s2y.upper = mw_pair_upper;
    p_Q.ta = true;
    p_wA_P.tb = p_wA_dX.tb = true;
    p_Btx.ta = true;
    p_Wt.ta = true;
    std::vector<BlkDesc> bd, bdm;
    std::vector<AYDesc> ayd;
    std::vector<PairDesc> pd;
    std::vector<ScaleDesc> sd;
    for (const LBlk& b : lb) {
      const int n = b.n, del = b.del, K = b.K, mm = b.m;
      BlkDesc d{b.off, n, 0};
      bd.push_back(d);
      if (mm > 1) bdm.push_back(d);
      p_XY.add(X + b.off, n, Y + b.off, n, nullptr, n, R + b.off, n, n, n, n);
      p_dXdY.add(dX + b.off, n, dY + b.off, n, R + b.off, n, R + b.off, n, n, n, n);
      p_xinv.add(tA + b.off, n, tA + b.off, n, nullptr, n, Xinv + b.off, n, n, n, n);
      p_PY.add(P + b.off, n, Y + b.off, n, R + b.off, n, tA + b.off, n, n, n, n);
      p_Z.add(Xinv + b.off, n, tA + b.off, n, nullptr, n, Z + b.off, n, n, n, n);
      p_dXY.add(dX + b.off, n, Y + b.off, n, R + b.off, n, tA + b.off, n, n, n, n);
      p_dY.add(Xinv + b.off, n, tA + b.off, n, nullptr, n, dY + b.off, n, n, n, n);
      t_Linv.add(LX + b.off, n, tA + b.off, n, n, n);
      t_sX1.add(LX + b.off, n, tA + b.off, n, n, n);
      t_sX2.add(LX + b.off, n, tB + b.off, n, n, n);
      t_sY1.add(LY + b.off, n, tA + b.off, n, n, n);
      t_sY2.add(LY + b.off, n, tB + b.off, n, n, n);
      f_X.add(LX + b.off, n, n);
      f_Y.add(LY + b.off, n, n);
      ci_XY.add(X + b.off, n, n, LX + b.off, n);
      // (Xinv aliases neither X nor LX; the Y blocks below ask for no inverse)
      if (spd_xy) ci_XY.want_inverse(Xinv + b.off, n);
      q_xinv.add(LX + b.off, n, LX + b.off, n, nullptr, n, Xinv + b.off, n, n, n, n);
      if constexpr (std::is_same<T, double>::value) {
        p_xir.add_op(true, false, 1.0, 0.0, LX + b.off, n, LX + b.off, n, nullptr, n, Xinv + b.off, n, n, n, n);
        p_xir.add_op(false, false, -1.0, 0.0, X + b.off, n, Y + b.off, n, nullptr, n, R + b.off, n, n, n, n);
        if (!p_xir.h.empty()) {
          p_xir.h.back().flags |= 16;  // + mu_p I
          p_xir.h.back().sa = sc + SC_MU_P;
        }
      }
      // step length: L^-1 dM L^-T for X and Y in the same two launches (Y's middle product in Z)
      q_sx1.add(LX + b.off, n, dX + b.off, n, nullptr, n, tA + b.off, n, n, n, n);
      q_sx1.add(LY + b.off, n, dY + b.off, n, nullptr, n, Z + b.off, n, n, n, n);
      q_sx2.add(tA + b.off, n, LX + b.off, n, nullptr, n, tB + b.off, n, n, n, n);
      q_sx2.add(Z + b.off, n, LY + b.off, n, nullptr, n, tC + b.off, n, n, n, n);
      e_X.add(tB + b.off, n, n);
      e_Y.add(tB + b.off, n, n);
      e_XY.add(tB + b.off, n, n);
      const int ldT = n;           // TX_b is (m delta) x (m K)
      const int ldBX = mm * K;     // BX_b is (m K) x (m K)
      for (int s = 0; s < mm; ++s) {
        p_s1x.add(Xinv + b.off + (int64_t)s * del * n, n, V + b.voff, del, nullptr, 0,
                  TX + b.toff + (int64_t)s * K * ldT, ldT, n, K, del);
        p_s1y.add(Y + b.off + (int64_t)s * del * n, n, V + b.voff, del, nullptr, 0,
                  TY + b.toff + (int64_t)s * K * ldT, ldT, n, K, del);
        for (int r = 0; r < mm; ++r) {
          p_s2x.add(V + b.voff, del, TX + b.toff + r * del + (int64_t)s * K * ldT, ldT, nullptr, 0,
                    BX + b.boff + r * K + (int64_t)s * K * ldBX, ldBX, K, K, del);
          p_s2y.add(V + b.voff, del, TY + b.toff + r * del + (int64_t)s * K * ldT, ldT, nullptr, 0,
                    BY + b.boff + r * K + (int64_t)s * K * ldBX, ldBX, K, K, del);
        }
      }
      ayd.push_back(AYDesc{b.boff, b.ayoff, K, mm});
      const int64_t xo = c_xoff[b.c];
      for (int r = 0; r < mm; ++r)
        for (int s = 0; s <= r; ++s) {
          const int rsi = s + r * (r + 1) / 2;
          const int64_t uoff = b.toff + (int64_t)rsi * del * K;  // U / Vs slot in TU / TW
          // trace_A: U = Z[r,s] V   (Z block rows r, cols s)
          p_trU_Z.add(Z + b.off + r * del + (int64_t)s * del * n, n, V + b.voff, del, nullptr, 0,
                      TU + uoff, del, del, K, del);
          p_trU_Y.add(Y + b.off + r * del + (int64_t)s * del * n, n, V + b.voff, del, nullptr, 0,
                      TU + uoff, del, del, K, del);
          pd.push_back(PairDesc{uoff, b.voff, b.ayoff + (int64_t)rsi * K, del, K, (int)b.koff,
                                -1});
          // weighted A: block (s, r) = Vs V^T  (MPMP.jl:1659-1667)
          ScaleDesc s_;
          s_.v_off = b.voff; s_.vs_off = uoff; s_.delta = del; s_.K = K;
          s_.ks_off = (int)b.koff; s_.lam_off = (int)b.koff;
          s_.a_off = (int)(xo + (int64_t)rsi * b.N);
          s_.scale = (r != s) ? 0.5 : 1.0;
          sd.push_back(s_);
          // P = WA(x) - X and dX = WA(dx) + P: the second term rides in the GEMM's Cin
          const int64_t so = s * del + (int64_t)r * del * n;
          p_wA_P.add(TW + uoff, del, V + b.voff, del, X + b.off + so, n, P + b.off + so, n, del,
                     del, K);
          p_wA_dX.add(TW + uoff, del, V + b.voff, del, P + b.off + so, n, dX + b.off + so, n,
                      del, del, K);
        }
    }
    for (const LBlk& b : lb) ci_XY.add(Y + b.off, b.n, b.n, LY + b.off, b.n);
    for (const LBlk& b : lb) e_XY.add(tC + b.off, b.n, b.n);
    if constexpr (std::is_same<T, double>::value) {
      // the strip chains need one block size n <= 128 at stride n^2 (one cluster shape: C3 and
      // its shards); by default taken for 64 < n (C2's n = 64 keeps the tiled GEMMs); Z only for
      // m = 1 (no symmetrisation of Z); CLRSDP_CHAIN=0 / 1 forces either
      bool uni_blk = !lb.empty() && !anyMgt1;
      for (size_t q = 0; q < lb.size() && uni_blk; ++q)
        uni_blk = lb[q].n == lb[0].n && lb[q].off == lb[0].off + (int64_t)q * lb[0].n * lb[0].n;
      const int n0 = lb.empty() ? 0 : lb[0].n;
      const bool chains = uni_blk && n0 <= 128 && reg_blk && sw.chain != 0 && (sw.chain == 1 || n0 > 64);
      if (chains) {
        const int nbk = (int)lb.size();
        c_Z.init(n0, nbk, 1, false, false);
        c_Z.set(0, P, Y, R, Xinv, Z);            // Z = X^-1 (P Y - R)
        c_dY.init(n0, nbk, 1, false, false);
        c_dY.set(0, dX, Y, R, Xinv, dY);         // dY = X^-1 (R - dX Y)
        // the predictor's dY launch also leaves the partials of <X + dX, Y + dY> (CORRECTOR_R's
        // mu; a flat sum over both triangles, so dY before its symmetrisation gives the same
        // value); one rank only (else the separate flat_reduce)
        dy_dot_cnt = nbk * (int)cdiv(n0, chain::NS);
        dy_dot_ok = world == 1;
        if (dy_dot_ok) {
          if (!dotp) dotp = dmalloc<T>(dy_dot_cnt);
          c_dY.u.DA[0] = X; c_dY.u.DdA[0] = dX; c_dY.u.DB[0] = Y;
        }
        c_step.init(n0, nbk, 2, true, true);
        c_step.set(0, dX, LX, nullptr, LX, tB);  // L_X^-1 dX L_X^-T
        c_step.set(1, dY, LY, nullptr, LY, tC);  // L_Y^-1 dY L_Y^-T
        // the X and Y halves apart, for the overlapped step length of small batches (below)
        c_stepX.init(n0, nbk, 1, true, true);
        c_stepX.set(0, dX, LX, nullptr, LX, tB);
        c_stepY.init(n0, nbk, 1, true, true);
        c_stepY.set(0, dY, LY, nullptr, LY, tC);
        for (const LBlk& b : lb) {
          e_Xs.add(tB + b.off, b.n, b.n);
          e_Ys.add(tC + b.off, b.n, b.n);
        }
        e_Xs.finalize(sw, MatPlan<T>::Use::EIG_ONLY);
        e_Ys.finalize(sw, MatPlan<T>::Use::EIG_ONLY);
        // CLRSDP_XY_OVERLAP=1 (round 6): with at most 32 local blocks the
        // X step length (its congruence and eigen launch) runs on the side stream as soon as the
        // corrector's dX exists, beside dY and the Y step length.  Measured, not the default
        // (DESIGN.md §7).
        xy_ov_ok = sw.xy_overlap && nb() <= 32;
      }
    }
    n_blk_m = (int)bdm.size();
    if (std::is_same<T, double>::value) {
      int nmx = 0;
      for (const LBlk& b : lb) nmx = std::max(nmx, b.n);
      const int nt = (nmx + 31) / 32;
      sym_pairs = nt * (nt + 1) / 2;
    }
    d_blk = descs.own(bd);
    if (n_blk_m) d_blk_m = descs.own(bdm);
    d_ayd = descs.own(ayd);
    build_ozaki();
    n_pair = (int)pd.size();
    // tuples <-> columns 1:1 in every local cluster (m = L = 1, every rank 1): fused trace_A
    trivial_tuples = n_pair > 0;
    {
      int bi = 0, pi = 0;
      for (int c = 0; c < nc() && trivial_tuples; ++c) {
        const int j = oc[c];
        trivial_tuples = m[j] == 1 && Lc[j] == 1;
        for (int k = 0; k < Ns[j] && trivial_tuples; ++k)
          trivial_tuples = ranks_all[rkoff_g[lb[bi].gjl] + k] == 1;
        if (trivial_tuples) pd[pi].x_off = (int)c_xoff[c];
        bi += (int)Lc[j];
        pi += 1;
      }
    }
    d_pair = descs.own(pd);
    d_scale = descs.own(sd);
    // U = Z V and the column sums of the right-hand side in one launch (chain_f64 TRACE): with
    // the Z chain, trivial tuples and every block's K, lambda and tuple slices at fixed strides
    if constexpr (std::is_same<T, double>::value) {
      bool tr = c_Z.on && trivial_tuples && (int)pd.size() == (int)lb.size();
      for (size_t q = 0; q < pd.size() && tr; ++q)
        tr = pd[q].K == pd[0].K && pd[q].delta == lb[0].n && pd[q].v_off == pd[0].v_off + (long long)q * pd[0].delta * pd[0].K &&
             (long long)pd[q].lam_off == pd[0].lam_off + (long long)q * pd[0].K &&
             (long long)pd[q].x_off == pd[0].x_off + (long long)q * pd[0].K;
      if (tr) {
        c_trZ.init(lb[0].n, (int)lb.size(), 1, false, false);
        c_trZ.trace = true;
        c_trZ.set(0, Z, V + pd[0].v_off, nullptr, nullptr, nullptr);
        c_trZ.u.ldb1 = pd[0].delta;
        c_trZ.u.sB1 = (long long)pd[0].delta * pd[0].K;
        c_trZ.u.NC = pd[0].K;
        c_trZ.u.lam = lam + pd[0].lam_off;
        c_trZ.u.sLam = pd[0].K;
        c_trZ.u.din = dvec + pd[0].x_off;
        c_trZ.u.rout = rhs + pd[0].x_off;
        c_trZ.u.sX = pd[0].K;
        c_trZ.u.c_in = -1.0;  // rhs_x = -d - Tr(A_* Z)  (MPMP.jl:1733-1739)
        c_trZ.u.c_agg = -1.0;
      }
    }
    // trivial tuples + fp64 + the fused Schur layout: x_i / dx_i of column p is entry p of the
    // cluster's slice, lambda_p entry p of the block's
    wa_fused = std::is_same<T, double>::value && trivial_tuples && fast_schur;
    if (wa_fused) {
      p_wA_Ps.tb = p_wA_dXs.tb = true;
      for (const LBlk& b : lb) {
        const int n = b.n, del = b.del, K = b.K;
        const int64_t xo = c_xoff[b.c];
        p_wA_Ps.add_scaled(V + b.voff, del, V + b.voff, del, X + b.off, n, P + b.off, n, del, del, K,
                           x + xo, lam + b.koff);
        p_wA_dXs.add_scaled(V + b.voff, del, V + b.voff, del, P + b.off, n, dX + b.off, n, del, del, K,
                            dx + xo, lam + b.koff);
      }
    }
    // per cluster plans
    std::vector<SchurClusterDesc> scd;
    std::vector<SchurBlockDesc> sbd;
    h_cls.clear();
    cls_nrb = 0;
    cls_on = false;
    std::vector<TupleDesc> td;
    std::vector<TupleBlock> tbk;
    int bi = 0;
    int64_t s2off = 0, b2off = 0;
    std::vector<MatDesc<T>> s11;  // S11 blocks of the 2x2-blocked clusters (chol_inv in ci_S)
    if (s_split || q_split) {
      q_dx2.ta = true;
      q_qinv2.ta = true;
      t_W.four = t_Sinv.four = t_Qinv.four = true;
      // (the solves take the identity's columns as right-hand sides themselves: vec_rhs())
      if (s_split) {
        int64_t len = 1;
        for (int c = 0; c < nc(); ++c)
          len = std::max(len, c_Soff[c] + (int64_t)Ds[oc[c]] * Ds[oc[c]]);
        SLi = dmalloc<T>(len);
      }
      if (q_split) QLi = dmalloc<T>(std::max<int64_t>(n_y * n_y, 1));
    }
    for (int c = 0; c < nc(); ++c) {
      const int j = oc[c];
      const int D = (int)Ds[j];
      T* Sc = S + c_Soff[c];
      T* Wc = Wm + c_Boff[c];
      T* Bc = Bm + c_Boff[c];
      const int64_t xo = c_xoff[c];
      f_S.add(Sc, D, D);
      T* slab = Qslab + (int64_t)c * n_y * n_y;
      const int ny = (int)n_y;
      if (!std::is_same<T, double>::value || D <= s_single) {
        ci_S.add(Sc, D, D, Sc, D);
        q_W.add(Sc, D, Bc, D, nullptr, 0, Wc, D, D, ny, D);
        if (std::is_same<T, double>::value) {  // (mixed batches are fp64 only)
          f_a.add_op(false, false, 1.0, 0.0, Sc, D, Bc, D, nullptr, 0, Wc, D, D, ny, D);    // W = L^-1 B
          f_b.add_op(true, false, 1.0, 0.0, Wc, D, Wc, D, nullptr, 0, slab, ny, ny, ny, D); // W^T W
        }
        q_t.add(Sc, D, rhs + xo, D, nullptr, 0, tvec + xo, D, D, 1, D);
        q_dx.add(Sc, D, tmpv + xo, D, nullptr, 0, dx + xo, D, D, 1, D);
      } else if (D <= 256) {
        // S = [S11 S12; S21 S22] = L L^T with L = [L11 0; L21 L22] (SURVEY.md §3D with Cholesky):
        // the critical path only needs W = L^-1 B and Q's slab; X21 = -L22^-1 L21 L11^-1 (the
        // lower-left block of L^-1, for the solves) is formed on the side stream
        const int D1 = 128, D2 = D - 128;
        T* S11 = Sc;
        T* S12 = Sc + (int64_t)D1 * D;
        T* S21 = Sc + D1;
        T* S22 = Sc + D1 + (int64_t)D1 * D;
        T* T12 = Stmp + s2off;               // L11^-1 S12 = L21^T   (D1 x D2)
        T* Mb = T12 + (int64_t)D2 * D1;      // L22^-1 L21           (D2 x D1)
        T* B2 = B2p + b2off;                 // B2 - L21 W1          (D2 x n_y)
        s2off += 2 * (int64_t)D2 * D1;
        b2off += (int64_t)D2 * n_y;
        s11.push_back(MatDesc<T>{S11, D1, D});                                          // S11 <- L11^-1
        // (S21^T, not S12: the fused Schur kernel may assemble only the lower triangle)
        f_a.add_op(false, true, 1.0, 0.0, S11, D, S21, D, nullptr, 0, T12, D1, D1, D2, D1);
        f_w.add_op(false, false, 1.0, 0.0, S11, D, Bc, D, nullptr, 0, Wc, D, D1, ny, D1);  // W1
        f_b.add_op(true, false, -1.0, 1.0, T12, D1, T12, D1, S22, D, S22, D, D2, D2, D1);  // S22 - L21 L21^T
        f_w2.add_op(true, false, 1.0, 0.0, Wc, D, Wc, D, nullptr, 0, slab, ny, ny, ny, D1); // W1^T W1
        f_w2.add_op(true, false, -1.0, 1.0, T12, D1, Wc, D, Bc + D1, D, B2, D2, D2, ny, D1);  // B2'
        ci_S22.add(S22, D2, D, S22, D);                                                 // S22 <- L22^-1
        f_c.add(S22, D, B2, D2, nullptr, 0, Wc + D1, D, D2, ny, D2);                   // W2 = L22^-1 B2'
        f_d.add(Wc + D1, D, Wc + D1, D, slab, ny, slab, ny, ny, ny, D2);               // slab += W2^T W2
        f_x1.add(S22, D, T12, D1, nullptr, 0, Mb, D2, D2, D1, D2);                      // M = L22^-1 L21
        f_x2.add(Mb, D2, S11, D, nullptr, 0, S21, D, D2, D1, D1);                       // S21 <- -M L11^-1
        // S12 is not part of L^-1: the products with L^-1 below are split so that none reads it
        q_t.add(S11, D, rhs + xo, D, nullptr, 0, tvec + xo, D, D1, 1, D1);
        q_t.add(Sc + D1, D, rhs + xo, D, nullptr, 0, tvec + xo + D1, D, D2, 1, D);
        // dx = (L^-1)^T u: columns 0..D1-1 of L^-1 are [L11^-1; X21], the rest L22^-1
        q_dx.add(Sc, D, tmpv + xo, D, nullptr, 0, dx + xo, D, D1, 1, D);
        q_dx.add(S22, D, tmpv + xo + D1, D2, nullptr, 0, dx + xo + D1, D2, D2, 1, D2);
      } else {
        q_t.add(Sc, D, rhs + xo, D, nullptr, 0, tvec + xo, D, D, 1, D);
        q_dx.add(Sc, D, tmpv + xo, D, nullptr, 0, dx + xo, D, D, 1, D);
      }
      q_Wdy.add(Wc, D, dyv, (int)n_y, tvec + xo, D, tmpv + xo, D, D, 1, (int)n_y);
      t_W.add(Sc, D, Wc, D, D, (int)n_y, false, Bc);
      t_t.add(Sc, D, tvec + xo, D, D, 1);
      if (s_split) {
        T* Li = SLi + c_Soff[c];
        t_Sinv.add(Sc, D, Li, D, D, D, true);                                        // L^-1 = L \ I
        q_t2.add(Li, D, rhs + xo, D, nullptr, 0, tvec + xo, D, D, 1, D);
        q_dx2.add(Li, D, tmpv + xo, D, nullptr, 0, dx + xo, D, D, 1, D);
      }
      p_Q.add(Wc, D, Wc, D, nullptr, 0, slab, ny, ny, ny, D);
      p_By.add(Bc, D, y, (int)n_y, nullptr, 0, tmpv + xo, D, D, 1, (int)n_y);
      p_Btx.add(Bc, D, x + xo, D, nullptr, 0, pslab + (int64_t)c * n_y, (int)n_y, (int)n_y, 1, D);
      p_Wt.add(Wc, D, tvec + xo, D, nullptr, 0, pslab + (int64_t)c * n_y, (int)n_y, (int)n_y, 1, D);
      p_Wdy.add(Wc, D, dyv, (int)n_y, tvec + xo, D, dx + xo, D, D, 1, (int)n_y);
      if constexpr (std::is_same<T, double>::value) {
        ClSolveDesc cs{};
        cs.L = Sc; cs.W = Wc; cs.rhs = rhs + xo; cs.t = tvec + xo; cs.dx = dx + xo; cs.D = D;
        h_cls.push_back(cs);
        cls_nrb = std::max(cls_nrb, (int)cdiv(D, 64));
      }
      SchurClusterDesc cdsc;
      cdsc.m = (int)m[j]; cdsc.N = (int)Ns[j]; cdsc.D = D;
      cdsc.blk0 = bi; cdsc.nblk = (int)Lc[j];
      cdsc.pair0 = (int)n_pairs;
      cdsc.S_off = c_Soff[c];
      scd.push_back(cdsc);
      n_pairs += (long long)D * (D + 1) / 2;
      TupleDesc tdc;
      tdc.x_off = (int)xo; tdc.N = (int)Ns[j]; tdc.m = (int)m[j];
      tdc.blk0 = bi; tdc.nblk = (int)Lc[j]; tdc.t0 = (int)xo;
      td.push_back(tdc);
      for (int l = 0; l < Lc[j]; ++l, ++bi) {
        const LBlk& b = lb[bi];
        SchurBlockDesc s;
        s.bx_off = b.boff; s.K = b.K; s.rs_off = (int)b.rsoff; s.lam_off = (int)b.koff; s.pad = 0;
        sbd.push_back(s);
        TupleBlock t;
        t.val_off = b.ayoff; t.K = b.K; t.rs_off = (int)b.rsoff; t.lam_off = (int)b.koff; t.pad = 0;
        tbk.push_back(t);
      }
    }
    for (const MatDesc<T>& m1 : s11) ci_S.add(m1.A, m1.n, m1.lda, m1.A, m1.lda);  // after the single blocks
    t_Q.add(Qf, (int)n_y, dyv, (int)n_y, (int)n_y, 1);
    t_dxadd_init();
    f_Q.add(Qf, (int)n_y, (int)n_y);
    ci_Q.add(Q, (int)n_y, (int)n_y, Qf, (int)n_y);
    if (spd_q) ci_Q.want_inverse(Qinv, (int)n_y);  // (Qinv aliases neither Q nor Qf)
    q_q1.add(Qf, (int)n_y, dyv, (int)n_y, nullptr, 0, uvec, (int)n_y, (int)n_y, 1, (int)n_y);
    q_q2.add(Qf, (int)n_y, uvec, (int)n_y, nullptr, 0, dyv, (int)n_y, (int)n_y, 1, (int)n_y);
    // Q^-1 = L_Q^-T L_Q^-1 once per iteration (side stream), then one GEMV per direction
    q_qinv.ta = true;
    q_qinv.add(Qf, (int)n_y, Qf, (int)n_y, nullptr, 0, Qinv, (int)n_y, (int)n_y, (int)n_y, (int)n_y);
    q_qdy.add(Qinv, (int)n_y, uvec, (int)n_y, nullptr, 0, dyv, (int)n_y, (int)n_y, 1, (int)n_y);
    if (q_split) {
      t_Qinv.add(Qf, (int)n_y, QLi, (int)n_y, (int)n_y, (int)n_y, true);            // L_Q^-1 = L_Q \ I
      q_qinv2.add(QLi, (int)n_y, QLi, (int)n_y, nullptr, 0, Qinv, (int)n_y, (int)n_y, (int)n_y, (int)n_y);
    }
    {
      // (fp64 explicit inverses of S_j (<= 256) and Q; opt-in, CLRSDP_CL_SOLVE=1: at C3 the two
      // launches ran 14.8 + 21.4 us against 13.4 + 11.8 for the four GEMVs, and slab_qsolve
      // summing four partial slabs per cluster 13.7 against 9.0 us: 1195-1232 against 1248-1270
      // it/s, A/B round 5 -- fewer workgroups with longer load chains lose to more, shorter ones)
      int max_D = 0;
      for (const ClSolveDesc& cs : h_cls) max_D = std::max(max_D, cs.D);
      cls_on = sw.cl_solve &&std::is_same<T, double>::value && reg_S && reg_Q &&
               cl_solve_ok(nc(), cls_nrb, max_D, n_y);
      if (cls_on) d_cls = descs.own(h_cls);
    }
    if (nc()) {
      d_scd = descs.own(scd);
      d_sbd = descs.own(sbd);
      d_td = descs.own(td);
      d_tb = descs.own(tbk);
    }
    if (fast_schur) build_fast_schur();
    for (GemmPlan<T>* g : {&p_txy, &p_ty, &p_XY, &p_dXdY, &p_xinv, &p_s1x, &p_s1y, &p_s2x, &p_s2y, &p_Q, &p_wA_P,
                           &p_wA_dX, &p_trU_Z, &p_trU_Y, &p_By, &p_Btx, &p_Wt, &p_Wdy, &p_PY,
                           &p_Z, &p_dXY, &p_dY, &q_xinv, &q_sx1, &q_sx2, &q_sy1, &q_sy2, &q_W,
                           &q_t, &q_Wdy, &q_dx, &q_q1, &q_q2, &q_qinv, &q_qdy, &f_a, &f_b, &f_c, &f_d, &f_x1, &f_x2, &f_w, &f_w2,
                           &q_t2, &q_dx2, &q_qinv2,
                           &p_wA_Ps, &p_wA_dXs, &p_xir})
      g->finalize(sw);
    for (CholInvPlan<T>* c : {&ci_XY, &ci_S, &ci_S22, &ci_Q}) c->finalize(sw);
    e_XY.finalize(sw, MatPlan<T>::Use::EIG_ONLY);
    for (TrsmPlan<T>* t : {&t_Linv, &t_W, &t_t, &t_Q, &t_sX1, &t_sX2, &t_sY1, &t_sY2, &t_dx, &t_Sinv, &t_Qinv})
      t->finalize(sw);
    for (MatPlan<T>* f : {&f_X, &f_Y, &f_S, &f_Q}) f->finalize(sw, MatPlan<T>::Use::FACTOR_DEFERRED);
    for (MatPlan<T>* f : {&e_X, &e_Y}) f->finalize(sw, MatPlan<T>::Use::EIG_ONLY);
  }

  // ---- double-double Schur products on the int8 matrix cores (Ozaki scheme, oz_split / oz_gemm in
  // kernels_dense.h; round 6): every block m = 1.  Four launches replace the four gemm_valu_ks
  // launches of p_s1x, p_s1y, p_s2x, p_s2y: the digits of the rows of X^-1_b and Y_b and of the
  // columns of V_b; TX_b = X^-1_b V_b and TY_b = Y_b V_b; the digits of the columns of TX_b, TY_b;
  // BX_b = V_b^T TX_b and BY_b = V_b^T TY_b on their upper 16-tiles (the rows of V_b^T are the
  // columns of V_b, so their digits serve twice).  CLRSDP_OZAKI=0 keeps the VALU products.
  bool use_oz = false;
  OzSplitDesc* d_ozs1 = nullptr;
  OzSplitDesc* d_ozs2 = nullptr;
  OzGemmDesc* d_ozg1 = nullptr;
  OzGemmDesc* d_ozg2 = nullptr;
  TileRef *d_ozs1t = nullptr, *d_ozs2t = nullptr, *d_ozg1t = nullptr, *d_ozg2t = nullptr;
  int n_ozs1 = 0, n_ozs2 = 0, n_ozg1 = 0, n_ozg2 = 0;
  // the equilibration exponents of the contraction index (oz_split's kx): one arena, the del
  // exponents of local block q at oz_kx + oz_kxoff[q] (-1: the block has no products)
  int* oz_kx = nullptr;
  std::vector<int64_t> oz_kxoff;
  int64_t oz_nkx = 0;
  void build_ozaki() {
    use_oz = false;
    oz_kx = nullptr;
    oz_nkx = 0;
    if constexpr (std::is_same<T, mw::dd>::value) {
      if (anyMgt1 || lb.empty() || !sw.ozaki) return;
      std::vector<OzSplitDesc> s1, s2;
      std::vector<OzGemmDesc> g1, g2;
      std::vector<TileRef> s1t, s2t, g1t, g2t;
      auto pad = [](int v, int q) { return (v + q - 1) / q * q; };
      auto digits = [&](int nv, int K) {
        signed char* D = dmalloc<signed char>((size_t)OZ_S * pad(nv, 16) * pad(K, 64));
        descs.owned_dev.push_back(D);
        return D;
      };
      auto expo = [&](int nv) {
        int* E = dmalloc<int>((size_t)pad(nv, 16));
        descs.owned_dev.push_back(E);
        return E;
      };
      auto add_split = [&](std::vector<OzSplitDesc>& v, std::vector<TileRef>& t, const T* X, long long sv,
                           long long sk, int nv, int K, signed char* D, int* E, const int* kx, int ks) {
        v.push_back(OzSplitDesc{X, sv, sk, D, E, nv, K, pad(nv, 16), pad(K, 64), kx, ks, 0});
        for (int g = 0; g < cdiv(nv, 4); ++g) t.push_back(TileRef{(int)v.size() - 1, g});
      };
      auto add_gemm = [&](std::vector<OzGemmDesc>& v, std::vector<TileRef>& t, const signed char* DA,
                          const int* EA, int RA, const signed char* DB, const int* EB, int RB, int Kp,
                          T* C, int ldc, int M, int N, bool upper) {
        const int tn = cdiv(N, 16);
        v.push_back(OzGemmDesc{DA, EA, DB, EB, C, RA, RB, Kp, ldc, M, N, tn, 0});
        for (int q = 0; q < cdiv(M, 16) * tn; ++q)
          if (!upper || q / tn <= q % tn) t.push_back(TileRef{(int)v.size() - 1, q});
      };
      oz_kxoff.assign(lb.size(), -1);
      oz_nkx = 0;
      for (size_t q = 0; q < lb.size(); ++q)
        if (lb[q].K > 0 && lb[q].del > 0) {
          oz_kxoff[q] = oz_nkx;
          oz_nkx += lb[q].del;
        }
      oz_kx = expo((int)oz_nkx);  // (zero until upload() sets them)
      for (size_t q = 0; q < lb.size(); ++q) {
        const LBlk& b = lb[q];
        const int n = b.n, del = b.del, K = b.K;
        if (K <= 0 || del <= 0) continue;
        const int* kx = oz_kx + oz_kxoff[q];
        signed char *Dx = digits(n, del), *Dy = digits(n, del), *Gv = digits(K, del);
        signed char *Gtx = digits(K, del), *Gty = digits(K, del);
        int *Ex = expo(n), *Ey = expo(n), *Fv = expo(K), *Ftx = expo(K), *Fty = expo(K);
        // rows of X^-1_b, Y_b (n x n, ld n: row v, element k at v + k n); columns of V_b (del x K)
        add_split(s1, s1t, Xinv + b.off, 1, n, n, del, Dx, Ex, kx, 1);
        add_split(s1, s1t, Y + b.off, 1, n, n, del, Dy, Ey, kx, 1);
        add_split(s1, s1t, V + b.voff, del, 1, K, del, Gv, Fv, kx, -1);
        // columns of TX_b, TY_b (del x K, ld n)
        add_split(s2, s2t, TX + b.toff, n, 1, K, del, Gtx, Ftx, kx, 1);
        add_split(s2, s2t, TY + b.toff, n, 1, K, del, Gty, Fty, kx, 1);
        const int Kp = pad(del, 64);
        add_gemm(g1, g1t, Dx, Ex, pad(n, 16), Gv, Fv, pad(K, 16), Kp, TX + b.toff, n, n, K, false);
        add_gemm(g1, g1t, Dy, Ey, pad(n, 16), Gv, Fv, pad(K, 16), Kp, TY + b.toff, n, n, K, false);
        add_gemm(g2, g2t, Gv, Fv, pad(K, 16), Gtx, Ftx, pad(K, 16), Kp, BX + b.boff, K, K, K, mw_pair_upper);
        add_gemm(g2, g2t, Gv, Fv, pad(K, 16), Gty, Fty, pad(K, 16), Kp, BY + b.boff, K, K, K, mw_pair_upper);
      }
      if (g1.empty()) return;
      d_ozs1 = descs.own(s1); d_ozs2 = descs.own(s2); d_ozg1 = descs.own(g1); d_ozg2 = descs.own(g2);
      d_ozs1t = descs.own(s1t); d_ozs2t = descs.own(s2t); d_ozg1t = descs.own(g1t); d_ozg2t = descs.own(g2t);
      n_ozs1 = (int)s1t.size(); n_ozs2 = (int)s2t.size(); n_ozg1 = (int)g1t.size(); n_ozg2 = (int)g2t.size();
      use_oz = true;
    }
  }
  void launch_ozaki() {
    oz_split<<<(unsigned)n_ozs1, 256, 0, stream>>>(d_ozs1, d_ozs1t);
    oz_gemm<<<(unsigned)cdiv(n_ozg1, 4), 256, 0, stream>>>(d_ozg1, d_ozg1t, n_ozg1);
    oz_split<<<(unsigned)n_ozs2, 256, 0, stream>>>(d_ozs2, d_ozs2t);
    oz_gemm<<<(unsigned)cdiv(n_ozg2, 4), 256, 0, stream>>>(d_ozg2, d_ozg2t, n_ozg2);
    HIPCHK(hipGetLastError());
  }

  bool any_grp2 = false;
  void build_fast_schur() {
    if constexpr (std::is_same<T, double>::value) {
      p_txy.tag = 1;
      p_txy.stamp = stamps;  // the SCHUR stage's start (clock stamps in the stat block)
      p_txy.tb = true;  // TXt = Vt * X^-1^T (X^-1 and Y are symmetric)
      p_ty.tag = 3;
      p_ty.stamp = stamps + 2;
      p_ty.tb = true;
      for (const LBlk& b : lb)
        if (b.K > 0) {
          p_txy.add(Vt + b.voff, b.K, Xinv + b.off, b.n, nullptr, 0, TX + b.toff, b.K, b.K, b.del, b.del);
          p_ty.add(Vt + b.voff, b.K, Y + b.off, b.n, nullptr, 0, TY + b.toff, b.K, b.K, b.del, b.del);
        }
      std::vector<PairTileDesc> ptd;
      std::vector<int> pnt;
      std::vector<SchurClusterDesc> gcd;
      int bi = 0;
      for (int c = 0; c < nc(); ++c) {
        const int j = oc[c];
        bool direct = Lc[j] == 1, grp2 = Lc[j] == 1;
        for (int l = 0; l < Lc[j] && (direct || grp2); ++l) {
          const LBlk& b = lb[bi + l];
          for (int k = 0; k < b.N; ++k) {
            direct = direct && ranks_all[rkoff_g[b.gjl] + k] == 1;
            grp2 = grp2 && ranks_all[rkoff_g[b.gjl] + k] == 2;
          }
        }
        // every sample of rank 2 (C2): the pairs kernel sums the 2 x 2 groups into S itself
        // (CLRSDP_SCHUR_GRP2=0: G and schur_gsum, for A/B)
        grp2 = grp2 && sw.schur_grp2;
        for (int l = 0; l < Lc[j]; ++l) {
          const LBlk& b = lb[bi + l];
          if (b.K == 0) continue;
          PairTileDesc t;
          t.Vt = Vt + b.voff; t.TXt = TX + b.toff; t.TYt = TY + b.toff; t.lam = lam + b.koff;
          t.G = (direct || grp2) ? S + c_Soff[c] : BX + b.boff;
          t.ldG = grp2 ? (int)Ds[j] : b.K;
          t.grp = grp2 ? 2 : 1;
          t.pad = 0;
          t.AY = AY + b.ayoff;
          t.K = b.K; t.del = b.del; t.tile0 = 0;
          const int nt = cdiv(b.K, 64);
          pnt.push_back(nt * (nt + 1) / 2);
          ptd.push_back(t);
        }
        if (grp2) any_grp2 = true;
        if (!direct && !grp2) {
          SchurClusterDesc g;
          g.m = 1; g.N = (int)Ns[j]; g.D = (int)Ds[j]; g.blk0 = bi; g.nblk = (int)Lc[j];
          g.pair0 = 0; g.S_off = c_Soff[c];
          gcd.push_back(g);
          max_gD = std::max(max_gD, g.D);
        }
        bi += (int)Lc[j];
      }
      const std::vector<TileRef> pt2d = tile_major(pnt);
      n_ptiles = (int)pt2d.size();
      if (n_ptiles) { d_ptd = descs.own(ptd); d_pt2d = descs.own(pt2d); }
      // the fused kernel: same blocks, one workgroup per 64-row block of each
      // Taken when it fills at least half the CUs with 64 < delta <= 128 (C3 and its 2-rank
      // shards), and in its ONE form below half the CUs (small cluster counts; at delta <= 64, C2,
      // the D64 instance).  Otherwise the unfused pair, with more and smaller workgroups.
      // CLRSDP_SCHUR_FUSED=0 / 1 forces either.
      schur_fused = sw.schur_fused != 0 && !ptd.empty();
      int fwg = 0;
      for (const PairTileDesc& t : ptd) {
        schur_fused = schur_fused && t.del <= 128;
        fwg += cdiv(t.K, 64);
      }
      // round 6: below half the CUs, with 64 < delta, the one-tile-per-workgroup form (ONE) is
      // taken (8-cluster shard of C3: 1572-1601 -> 1607-1681 it/s against the unfused pair, three
      // A/B pairs; at C2's delta = 64 it lost 2 %: 24.9 against 22.6 us)
      // (CLRSDP_SCHUR_FUSED_ONE=0: never, =1: whenever the fused kernel runs)
      fused_one = fwg < 128 && sw.schur_fused_one != 0;
      // (round 6, late: with every delta <= 64 the D64 instance of the ONE form -- half the MFMAs
      // of the padded one -- replaces the unfused pair below half the CUs, C2;
      // CLRSDP_SCHUR_FUSED_D64=0 keeps the padded instance wherever the fused kernel runs)
      fused_d64 = sw.schur_fused_d64;
      for (const PairTileDesc& t : ptd) fused_d64 = fused_d64 && t.del <= 64;
      for (const PairTileDesc& t : ptd) fused_one = fused_one && (t.del > 64 || fused_d64);
      if (sw.schur_fused_one == 1) fused_one = true;
      if (sw.schur_fused != 1 && !fused_one) {
        for (const PairTileDesc& t : ptd) schur_fused = schur_fused && t.del > 64;
        schur_fused = schur_fused && fwg >= 128;
      }
      // The fused kernel's rank-2 group-sum epilogue is a template parameter of the whole launch
      // (GRP2: every descriptor grp = 2), not a branch on d.grp.  A handle that mixes all-rank-2
      // clusters with others (grp = 1: S written per entry, or G for schur_gsum) would have the
      // group sums applied to those too, so it takes the unfused pair, whose schur_pairs_f64
      // branches per descriptor -- also under CLRSDP_SCHUR_FUSED=1.
      {
        bool all_grp2 = true;
        for (const PairTileDesc& t : ptd) all_grp2 = all_grp2 && t.grp == 2;
        if (any_grp2 && !all_grp2) schur_fused = false;
      }
      if (schur_fused) {
        std::vector<FusedPairDesc> fpd;
        std::vector<int> fnt;
        int q = 0;
        for (const LBlk& b : lb) {
          if (b.K == 0) continue;
          const PairTileDesc& t = ptd[q++];
          FusedPairDesc f;
          f.Vt = t.Vt; f.Xinv = Xinv + b.off; f.TYt = t.TYt; f.Y = Y + b.off; f.lam = t.lam;
          f.G = t.G; f.AY = t.AY;
          f.K = t.K; f.del = t.del; f.ldG = t.ldG; f.ldx = b.n; f.ldy = b.n;
          f.grp = t.grp; f.pad = 0;
          fpd.push_back(f);
          fnt.push_back(cdiv(b.K, 64));
        }
        fused_y = sw.schur_fused_y;
        fused_one = fused_one && fused_y;  // (instantiated with V^T Y on chip only)
        fused_d64 = fused_d64 && fused_one;   // (instantiated in the ONE form only)
        std::vector<TileRef> ft2d = tile_major(fnt);
        if (fused_one) {  // every (row block a, tile s of its share): t = a + st s, st = max(64, nr)
          // (the stride the kernel decodes with, schur_fused_f64: 64 up to 64 row blocks, K <= 4096,
          // and the row-block count itself above, so that row blocks 64, 65, ... are launched too)
          std::vector<int> fnt1;
          for (int nr : fnt) fnt1.push_back(std::max(64, nr) * (nr / 2 + 1));
          ft2d.clear();
          for (const TileRef& r : tile_major(fnt1)) {
            const int nr = fnt[r.p], st = std::max(64, nr), a = r.t % st, sidx = r.t / st;
            const int nbt = (nr % 2 == 0 && a >= nr / 2) ? nr / 2 : nr / 2 + 1;
            if (a < nr && sidx < nbt) ft2d.push_back(r);
          }
        }
        n_fwg = (int)ft2d.size();
        d_fpd = descs.own(fpd);
        d_fpt2d = descs.own(ft2d);
        fused_grp2 = any_grp2;
        for (const void* k : {(const void*)schur_fused_f64<0>, (const void*)schur_fused_f64<0, true>,
                              (const void*)schur_fused_f64<0, false, true>,
                              (const void*)schur_fused_f64<0, true, true>,
                              (const void*)schur_fused_f64<0, true, false, true>,
                              (const void*)schur_fused_f64<0, true, true, true>,
                              (const void*)schur_fused_f64<0, true, false, true, true>,
                              (const void*)schur_fused_f64<0, true, true, true, true>})
          HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)schur_fused::LDS));
      }
      n_gsum = (int)gcd.size();
      if (n_gsum) d_gcd = descs.own(gcd);
    }
  }

  TrsmPlan<T> t_dx;
  void t_dxadd_init() {
    for (int c = 0; c < nc(); ++c) {
      const int D = (int)Ds[oc[c]];
      t_dx.add(S + c_Soff[c], D, dx + c_xoff[c], D, D, 1);
    }
  }

  // The LU fallback's buffers and launch plans (first switch, or set_factorization).
  //   FACTOR:  S_j[perm_j] = L_j U_j (getrf); W1_j = L_j^-1 B_j[perm_j]; W2_j = U_j^-T B_j;
  //            slab_j = W2_j^T W1_j; Q = sum_j slab_j; Q[perm] = L_Q U_Q     (MPMP.jl:1429-1505)
  //   solves:  t_j = L_j^-1 rhs_j[perm_j]; u = sum_j W2_j^T t_j; dy = U_Q^-1 L_Q^-1 (p - u)[perm];
  //            dx_j = U_j^-1 (t_j + W1_j dy)                                  (MPMP.jl:1743-1776)
  //   X^-1:    X_b[perm_b] = L_b U_b; X_b^-1 = U_b^-1 L_b^-1 (P_b I)          (approx_inv!, 781)
  // Neither the factorisation nor its triangular solves have a size bound: beyond the on-chip
  // panels (getrf_batched: fp64 624, dd 312, qd 156; trsm_batched: fp64 1199, dd 559, qd 239) the
  // blocked chains across workgroups take over, unless CLRSDP_LU_BLK=0 / CLRSDP_TRSM_BLK=0 keep
  // the on-chip kernels alone.
  int lu_nmax() const {
    int nmax = (int)n_y;
    for (int c = 0; c < nc(); ++c) nmax = std::max(nmax, (int)Ds[oc[c]]);
    for (const LBlk& b : lb) nmax = std::max(nmax, b.n);
    return nmax;
  }
  // the switches as read when the LU plans are first built (lazily, after creation): whether the
  // handle fits, the error text and every plan finalised there take this one value
  Switches lu_sw;
  bool lu_fits() const {
    const int nmax = lu_nmax();
    if (lu_sw.lu_blk == 0 && !LuPlan<T>::one_cu_fits(nmax)) return false;
    return lu_sw.trsm_blk != 0 || TrsmPlan<T>::one_cu_fits(nmax);
  }
  // false (E_ARG when `must`): a matrix beyond the panels CLRSDP_LU_BLK=0 / CLRSDP_TRSM_BLK=0 keep it to
  bool build_lu_plans(bool must = true) {
    if (lu_built) return true;
    lu_sw = Switches::read();
    if (!lu_fits()) {
      if (!must) return false;
      if (lu_sw.trsm_blk == 0 && !TrsmPlan<T>::one_cu_fits(lu_nmax()))
        throw ClrsdpError{CLRSDP_E_ARG, "LU factorization: a matrix is too large for the on-chip panel of the LU triangular solves (CLRSDP_TRSM_BLK=0)"};
      throw ClrsdpError{CLRSDP_E_ARG, "LU factorization: a matrix is too large for the on-chip panel of getrf_batched (CLRSDP_LU_BLK=0)"};
    }
    try {
      build_lu_plans_();
    } catch (...) {  // transactional: no half-built plans or buffers survive a failure
      for (LuPlan<T>* l : {&lu_S, &lu_Q, &lu_X}) l->h.clear();
      for (PermPlan<T>* q : {&pm_B, &pm_rhs, &pm_r, &pm_I}) q->h.clear();
      for (TrsmPlan<T>* t : {&tl_W1, &tl_W2, &tl_t, &tl_dx, &tl_Q1, &tl_Q2, &tl_X1, &tl_X2}) t->h.clear();
      for (GemmPlan<T>* g : {&lq_slab, &lq_Wt}) g->clear();
      if (lperm) (void)hipFree(lperm);
      if (W2m) (void)hipFree(W2m);
      lperm = nullptr;
      W2m = nullptr;
      throw;
    }
    return true;
  }
  void build_lu_plans_() {
    int64_t np = nx + n_y;
    for (const LBlk& b : lb) np += b.n;
    lperm = dmalloc<int>(std::max<int64_t>(np, 1));
    W2m = dmalloc<T>(std::max<int64_t>(nB, 1));
    const int ny = (int)n_y;
    for (int c = 0; c < nc(); ++c) {
      const int D = (int)Ds[oc[c]];
      T* Sc = S + c_Soff[c];
      T* Wc = Wm + c_Boff[c];
      T* W2c = W2m + c_Boff[c];
      const T* Bc = Bm + c_Boff[c];
      int* pc = lperm + c_xoff[c];
      const int64_t xo = c_xoff[c];
      lu_S.add(Sc, pc, D, D);
      pm_B.add(Bc, D, Wc, D, pc, D, ny);                                          // B_j[perm_j]
      tl_W1.add(Sc, D, Wc, D, D, ny);                                             // L_j^-1 (.)
      tl_W2.add(Sc, D, W2c, D, D, ny);                                            // U_j^-T B_j
      lq_slab.add(W2c, D, Wc, D, nullptr, 0, Qslab + (int64_t)c * n_y * n_y, ny, ny, ny, D);
      pm_rhs.add(rhs + xo, D, tvec + xo, D, pc, D, 1);                            // rhs_j[perm_j]
      tl_t.add(Sc, D, tvec + xo, D, D, 1);
      lq_Wt.add(W2c, D, tvec + xo, D, nullptr, 0, pslab + (int64_t)c * n_y, ny, ny, 1, D);
      tl_dx.add(Sc, D, dx + xo, D, D, 1);                                         // U_j^-1 (.)
    }
    int* qp = lperm + nx;
    lu_Q.add(Qf, qp, ny, ny);
    pm_r.add(uvec, ny, dyv, ny, qp, ny, 1);
    tl_Q1.add(Qf, ny, dyv, ny, ny, 1);
    tl_Q2.add(Qf, ny, dyv, ny, ny, 1);
    int* xp = qp + n_y;
    for (const LBlk& b : lb) {
      lu_X.add(tA + b.off, xp, b.n, b.n);
      pm_I.add(nullptr, 0, Xinv + b.off, b.n, xp, b.n, b.n);
      tl_X1.add(tA + b.off, b.n, Xinv + b.off, b.n, b.n, b.n);
      tl_X2.add(tA + b.off, b.n, Xinv + b.off, b.n, b.n, b.n);
      xp += b.n;
    }
    lq_slab.ta = lq_Wt.ta = true;
    for (TrsmPlan<T>* t : {&tl_W1, &tl_t, &tl_Q1, &tl_X1}) t->mode = 1;
    for (TrsmPlan<T>* t : {&tl_W2, &tl_dx, &tl_Q2, &tl_X2}) t->mode = 2;
    for (LuPlan<T>* l : {&lu_S, &lu_Q, &lu_X}) l->finalize(lu_sw);
    for (PermPlan<T>* q : {&pm_B, &pm_rhs, &pm_r, &pm_I}) q->finalize();
    for (TrsmPlan<T>* t : {&tl_W1, &tl_W2, &tl_t, &tl_dx, &tl_Q1, &tl_Q2, &tl_X1, &tl_X2}) t->finalize(lu_sw);
    lq_slab.finalize(lu_sw);
    lq_Wt.finalize(lu_sw);
    lu_built = true;
  }
  void set_factorization(int flags) override {
    if (inflight) throw ClrsdpError{CLRSDP_E_STATE, "set_factorization with loop bodies in flight"};
    if (flags & ~(CLRSDP_FACT_FALLBACK | CLRSDP_FACT_LU_SQ | CLRSDP_FACT_LU_X))
      throw ClrsdpError{CLRSDP_E_ARG, "unknown factorization flags"};
    if (flags & (CLRSDP_FACT_LU_SQ | CLRSDP_FACT_LU_X)) build_lu_plans();
    if (flags != fact_flags) drop_graphs();
    fact_flags = flags;
  }
  int get_factorization() const override { return fact_flags; }
  // what build_fast_schur / build_ozaki / upload decided, and the last SCHUR's store form
  void schur_info(struct clrsdp_schur_info* o) const override {
    o->fast = fast_schur;
    o->fused = schur_fused;
    o->one = schur_fused && fused_one;
    o->d64 = schur_fused && fused_d64;
    o->grp2 = schur_fused ? fused_grp2 : any_grp2;
    o->fused_y = schur_fused && fused_y;
    o->n_fwg = schur_fused ? n_fwg : 0;
    o->n_ptiles = n_ptiles;
    o->n_gsum = n_gsum;
    o->ozaki = use_oz;
    o->pair_upper = mw_pair_upper;
    o->full = schur_full;
    o->s_lower = schur_full < 0 ? -1 : (s_lower ? 1 : 0);
  }

  // ---------------- host <-> device conversion
  void put(T* dst, const double* planes, int64_t nplane, int64_t first, int64_t count) {
    if (count <= 0) return;
    std::vector<T> tmp(count);
    for (int64_t i = 0; i < count; ++i) Num<T>::pack(planes, nplane, first + i, &tmp[i]);
    HIPCHK(hipMemcpyAsync(dst, tmp.data(), count * sizeof(T), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  void get(const T* src, double* planes, int64_t nplane, int64_t first, int64_t count) {
    if (count <= 0) return;
    std::vector<T> tmp(count);
    HIPCHK(hipMemcpyAsync(tmp.data(), src, count * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int64_t i = 0; i < count; ++i) Num<T>::unpack(tmp[i], planes, nplane, first + i);
  }

  void upload(const double* Vh, const double* lamh, const double* Bh, const double* ch,
              const double* bh, const double* Ch) override {
    for (const LBlk& b : lb) {
      put(V + b.voff, Vh, tot_V, voff_g[b.gjl], (int64_t)b.del * b.K);
      put(lam + b.koff, lamh, tot_K, koff_g[b.gjl], b.K);
      if (fast_schur && b.K > 0) {  // V^T for the fused Schur path (fp64: one plane)
        std::vector<double> vt((size_t)b.del * b.K);
        const double* src = Vh + voff_g[b.gjl];
        for (int i = 0; i < b.del; ++i)
          for (int p = 0; p < b.K; ++p) vt[p + (size_t)i * b.K] = src[i + (size_t)p * b.del];
        put(Vt + b.voff, vt.data(), (int64_t)vt.size(), 0, (int64_t)vt.size());
      }
    }
    // the Ozaki products' equilibration of the contraction index (oz_split): per row k of V_b the
    // exponent of its largest entry, from the leading plane (0 for a row of zeros)
    // (every block's into one host image of the arena, one copy)
    if (oz_kx && oz_nkx > 0) {
      std::vector<int> kx((size_t)oz_nkx, 0);
      for (size_t q = 0; q < lb.size() && q < oz_kxoff.size(); ++q) {
        const LBlk& b = lb[q];
        if (oz_kxoff[q] < 0) continue;
        const double* src = Vh + voff_g[b.gjl];
        for (int i = 0; i < b.del; ++i) {
          double mx = 0.0;
          for (int p = 0; p < b.K; ++p) mx = std::max(mx, std::fabs(src[i + (size_t)p * b.del]));
          if (mx > 0.0 && std::isfinite(mx)) kx[(size_t)oz_kxoff[q] + i] = std::ilogb(mx);
        }
      }
      HIPCHK(hipMemcpyAsync(oz_kx, kx.data(), kx.size() * sizeof(int), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    for (int c = 0; c < nc(); ++c) {
      const int j = oc[c];
      put(Bm + c_Boff[c], Bh, tot_B, Boff_g[j], Ds[j] * n_y);
      put(cvec + c_xoff[c], ch, tot_x, xoff_g[j], Ds[j]);
    }
    put(bvec, bh, n_y, 0, n_y);
    hasC = (Ch != nullptr);
    if (hasC)
      for (const LBlk& b : lb) put(Cm + b.off, Ch, tot_blk, blkoff_g[b.gjl], (int64_t)b.n * b.n);
    uploaded = true;
  }

  void set_state(const double* xh, const double* Xh, const double* yh, const double* Yh) override {
    for (int c = 0; c < nc(); ++c) put(x + c_xoff[c], xh, tot_x, xoff_g[oc[c]], Ds[oc[c]]);
    for (const LBlk& b : lb) {
      put(X + b.off, Xh, tot_blk, blkoff_g[b.gjl], (int64_t)b.n * b.n);
      put(Y + b.off, Yh, tot_blk, blkoff_g[b.gjl], (int64_t)b.n * b.n);
    }
    put(y, yh, n_y, 0, n_y);
    adopt_state();
  }
  bool has_state = false;  // set_state or a hand-off has given the handle an iterate
  // after the state was written (set_state's uploads, clrsdp_handoff_state's launch)
  void adopt_state() override {
    body.dy_dot_ready = false;  // (a new state: CORRECTOR_R sums <X + dX, Y + dY> itself)
    has_state = true;
    refresh_xy_part();
    HIPCHK(hipStreamSynchronize(stream));
  }
  StateView state_view() const override {
    StateView v;
    v.x = x; v.X = X; v.Y = Y; v.y = y;
    v.nx = nx; v.nblk_el = nblk_el; v.n_y = n_y;
    v.words = Num<T>::W; v.dev = device; v.inflight = inflight; v.has_state = has_state;
    v.stream = stream;
    // every vector behind its length, so that two signatures agree only part by part
    auto add = [&](const auto& a) {
      v.sig.push_back((int64_t)a.size());
      for (const auto& e : a) v.sig.push_back((int64_t)e);
    };
    v.sig = {J, n_y, (int64_t)rank, (int64_t)world};
    add(m); add(Lc); add(Ns); add(delta); add(ranks_all); add(oc);
    return v;
  }
  void get_state(double* xh, double* Xh, double* yh, double* Yh) override {
    if (xh)
      for (int c = 0; c < nc(); ++c) get(x + c_xoff[c], xh, tot_x, xoff_g[oc[c]], Ds[oc[c]]);
    for (const LBlk& b : lb) {
      if (Xh) get(X + b.off, Xh, tot_blk, blkoff_g[b.gjl], (int64_t)b.n * b.n);
      if (Yh) get(Y + b.off, Yh, tot_blk, blkoff_g[b.gjl], (int64_t)b.n * b.n);
    }
    if (yh) get(y, yh, n_y, 0, n_y);
  }

  // ---------------- exchange
  // Partials are written to xsend[0..cnt); after the exchange rank r's copy is at
  // xrecv[r*cnt..].  world == 1: xrecv == xsend, nothing to do.
  void exchange(int tag, int64_t cnt) {
    if (comm) {  // native: one all-gather on the library stream (graph-capturable)
      RCCLCHK(rccl().all_gather(xsend, xrecv, (size_t)(cnt * (int64_t)sizeof(T)), ncclUint8, comm,
                                stream));
      return;
    }
    if (world == 1) return;
    if (!xfn) throw ClrsdpError{CLRSDP_E_EXCHANGE, "world_size > 1 but no exchange registered"};
    const int rc = xfn(xctx, tag, cnt * (int64_t)sizeof(T), (void*)stream);
    if (rc != 0) throw ClrsdpError{CLRSDP_E_EXCHANGE, "exchange callback failed"};
  }
  // reduce slot `slot` of every rank's partial vector (length cnt) in rank order into dst
  // rank-ordered reduction of slot `slot` of every rank's partials into sc[dst]; folded into
  // the next scalar_kernel launch (flush_scalars() at the latest, before xsend is reused)
  std::vector<FoldRed<T>> pend;
  void reduce_ranks(int64_t cnt, int64_t slot, int op, int dst) {
    pend.push_back(FoldRed<T>{xrecv + slot, cnt, world, op, dst, 0});
  }
  void fold(const T* src, int cnt, int op, int dst) {
    pend.push_back(FoldRed<T>{src, 1, cnt, op, dst, 0});
  }
  void flush_scalars() {
    if (!pend.empty()) scalars(nullptr, 0, -1);
  }

  // ---------------- kernels shorthands
  // out = a*A + b*B over all local blocks (flat), then += s I if scal
  void blk_lin(T* out, const T* A, double a, const T* B_, double b, const T* scal = nullptr,
               double sm = 1.0) {
    if (!nb()) return;
    if (!(scal && A == out && a == 1.0 && !B_))
      vec_lin<T><<<std::min<unsigned>(cdiv(nblk_el, 256), 4096), 256, 0, stream>>>(out, A, a, B_, b, nullptr, 0.0, nblk_el);
    if (scal) diag_add<T><<<nb(), 128, 0, stream>>>(d_blk, out, scal, sm);
  }
  void vlin(T* out, const T* a_, double ca, const T* b_, double cb, const T* c_, double cc,
            int64_t n) {
    if (n > 0) vec_lin<T><<<cdiv(n, 256), 256, 0, stream>>>(out, a_, ca, b_, cb, c_, cc, n);
  }
  void copy_guarded(T* dst, const T* src, int64_t n) {
    if (n > 0)
      vec_copy_guard<T><<<std::min<unsigned>(cdiv(n, 256), 2048), 256, 0, stream>>>(dst, src, n, info + info_H);
  }
  // two guarded copies in one launch (16-byte moves)
  void copy_guarded2(T* d0, const T* s0, int64_t n0, T* d1, const T* s1, int64_t n1) {
    if (n0 <= 0 && n1 <= 0) return;
    auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (n0 <= 0 || !a16(d0) || !a16(s0) || (n1 > 0 && (!a16(d1) || !a16(s1)))) {
      copy_guarded(d0, s0, n0);
      copy_guarded(d1, s1, n1);
      return;
    }
    const long long b0 = (long long)n0 * (long long)sizeof(T), b1 = n1 > 0 ? (long long)n1 * (long long)sizeof(T) : 0;
    const long long chunks = std::max(b0, b1) / 16 + 1;
    const unsigned g = (unsigned)std::min<long long>((chunks + 255) / 256, 1024);
    copy_guard2<<<g, 256, 0, stream>>>(d0, s0, b0, n1 > 0 ? d1 : nullptr, s1, b1, info + info_H);
  }
  void fill(T* out, double v, int64_t n) {
    if (n > 0) vec_fill<T><<<cdiv(n, 256), 256, 0, stream>>>(out, v, n);
  }
  int sym_pairs = 0;  // lower 32x32 tiles of the largest local block (blk_sym_tiles grid)
  void sym(T* out, const T* Zm, int mode, bool only_m = false) {
    if (only_m) {
      if (n_blk_m) blk_sym2<T><<<dim3(n_blk_m, 32), 128, 0, stream>>>(d_blk_m, out, Zm, mode);
    } else if (std::is_same<T, double>::value && mode == 0 && nb() && sym_pairs) {
      // (fp64: coalesced tile pairs)
      blk_sym_tiles<<<dim3(nb(), sym_pairs), 256, 0, stream>>>(
          d_blk, reinterpret_cast<double*>(out), reinterpret_cast<const double*>(Zm));
    } else if (nb()) {
      blk_sym2<T><<<dim3(nb(), 32), 128, 0, stream>>>(d_blk, out, Zm, mode);
    }
  }
  static T limbs(const double* l) {
    T v = T(l[0]);
    for (int i = 1; i < Num<T>::W && i < 4; ++i) v += T(l[i]);
    return v;
  }
  ScalarParams<T> sparams(const clrsdp_params* prm, int pd_feas) {
    ScalarParams<T> p{};
    p.beta_inf = limbs(prm->beta_infeasible);
    p.beta_feas = limbs(prm->beta_feasible);
    p.gamma = limbs(prm->gamma);
    p.b0 = limbs(prm->b0);
    p.gap_thr = gap_thr;
    p.p_thr = p_thr;
    p.d_thr = d_thr;
    p.need_p = need_p;
    p.need_d = need_d;
    p.dim = dimtot;
    p.pd_feas = pd_feas;
    p.fold_all = 1;
    return p;
  }
  void set_control(const clrsdp_control* c) override {
    if (inflight) throw ClrsdpError{CLRSDP_E_STATE, "set_control with loop bodies in flight"};
    gap_thr = limbs(c->duality_gap_threshold);
    p_thr = limbs(c->primal_error_threshold);
    d_thr = limbs(c->dual_error_threshold);
    need_p = c->need_primal_feasible != 0;
    need_d = c->need_dual_feasible != 0;
    // the thresholds travel by value in the ScalarParams of the captured scalar launches, so
    // every graph captured with the previous ones is stale
    drop_graphs();
  }
  bool zero_cy = false, zero_info = false;
  // ---- scalar slots + status words: one device block, one pinned host mirror
  char* stat_dev = nullptr;
  char* stat_host = nullptr;
  size_t stat_bytes = 0, stat_info_off = 0, stat_stamp_off = 0;
  unsigned long long* stamps = nullptr;
  void stat_alloc() {
    stat_info_off = ((SC_COUNT * sizeof(T)) + 63) / 64 * 64;
    // + the OR (update guard), then the SCHUR clock stamps (8-byte aligned)
    stat_stamp_off = (stat_info_off + (info_count + 1) * sizeof(int) + 7) / 8 * 8;
    stat_bytes = stat_stamp_off + 6 * sizeof(unsigned long long);
    // (both blocks carry one more 8-byte word behind the copied bytes: the device's count of
    // published bodies and the host's sequence word, see publish_ok())
    stat_dev = dmalloc<char>(stat_bytes + 8);
    HIPCHK(hipMemset(stat_dev + stat_bytes, 0, 8));
    HIPCHK(hipHostMalloc((void**)&stat_host, stat_bytes + 8,
                         hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(stat_host, 0, stat_bytes + 8);
    HIPCHK(hipHostGetDevicePointer((void**)&stat_host_dev, stat_host, 0));
    sc = reinterpret_cast<T*>(stat_dev);
    info = reinterpret_cast<int*>(stat_dev + stat_info_off);
    stamps = reinterpret_cast<unsigned long long*>(stat_dev + stat_stamp_off);
  }
  // ---- the synchronous fp64 loop body at one rank publishes its stat block itself: its last
  // scalar launch (which == 3) stores the block into the host mirror and then a sequence word,
  // and iterate_once() polls that word -- no copy node and no stream sync between two bodies.
  // Every other path (the pipelined loop, run_stage, initial(), multi-word, sharded, per-stage
  // timing, the LU-fallback plans, a handle without graph replay) keeps stat_fetch().  A body
  // whose capture failed and that was enqueued eagerly instead publishes like the replayed one.
  char* stat_host_dev = nullptr;  // the mirror's device address
  bool pub_body = false;          // the body being enqueued publishes (read by scalars(.., 3))
  bool publish_ok(int pd_feas) const {
    return sw.seam_pub && std::is_same<T, double>::value && world == 1 && pd_feas >= 0 &&
           graph_ok() && !lu_sq() && !lu_x();
  }
  unsigned long long pub_seq_now() const {
    return __atomic_load_n(reinterpret_cast<const unsigned long long*>(stat_host + stat_bytes),
                           __ATOMIC_ACQUIRE);
  }
  // wait until the sequence word leaves `last`; the stream is queried between polls, so a stream
  // that has completed or failed without publishing is an error and not a spin
  void pub_wait(unsigned long long last) {
    for (unsigned spin = 1;; ++spin) {
      if (pub_seq_now() != last) return;
      if ((spin & 1023u) == 0) {
        const hipError_t q = hipStreamQuery(stream);
        if (q == hipSuccess) {
          if (pub_seq_now() != last) return;
          throw ClrsdpError{CLRSDP_E_HIP, "the loop body completed without publishing its stat block"};
        }
        if (q != hipErrorNotReady) HIPCHK(q);
        (void)hipGetLastError();  // ("not ready" is no error for the launches checked later)
      }
    }
  }
  // copy scalars + status to the host mirror and wait
  void stat_fetch() {
    HIPCHK(hipMemcpyAsync(stat_host, stat_dev, stat_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  void scalars(const clrsdp_params* prm, int pd_feas, int which) {
    ScalarParams<T> p = prm ? sparams(prm, pd_feas) : ScalarParams<T>{};
    p.zero_cy = zero_cy ? 1 : 0;
    p.zero_n = zero_info ? info_count - 1 : 0;  // status words of this iteration (not the halt word)
    p.zero_ptr = info;
    p.halt_ptr = zero_info ? info + info_H : nullptr;  // which == 0 at the start of a loop body
    p.stamps = zero_info ? stamps : nullptr;
    p.guard = info;
    p.nguard = info_count;
    if (which == 3 && pub_body) {
      p.pub_n8 = (int)(stat_bytes / 8);
      p.pub_src = reinterpret_cast<const unsigned long long*>(stat_dev);
      p.pub_dst = reinterpret_cast<unsigned long long*>(stat_host_dev);
      p.pub_cnt = reinterpret_cast<unsigned long long*>(stat_dev + stat_bytes);
      p.pub_seq = reinterpret_cast<unsigned long long*>(stat_host_dev + stat_bytes);
    }
    zero_info = false;
    launch_folds<T>(stream, sc, p, pend, which);  // at most 6 folded reductions per launch
    pend.clear();
  }
  // local block-sum (op 0/1) or block-max (op 2) into *dst
  void local_blk_reduce(const T* A, const T* B_, const T* dA, const T* dB, int op, T* dst) {
    if (nb()) {
      launch_flat_reduce<T>(stream, A, B_, dA, dB, nblk_el, op, bpart);
      vec_reduce_tree(bpart, RED_G, op, dst);
    } else {
      fill(dst, 0.0, 1);
    }
  }

  // one-workgroup fixed-tree reduction of n <= 256 partials
  void vec_reduce_tree(const T* in, int n, int op, T* dst) {
    launch_vec_reduce_tree<T>(stream, in, n, op, dst);
  }

  // trace_A with the products U already in TX -> val (tval) -> aggregate
  void trace_aggregate(const T* val, const T* in, double c_in, const T* in2, double c_in2,
                       double c_agg, T* out) {
    if (nx > 0)
      tuple_aggregate<T><<<cdiv(nx, 256), 256, 0, stream>>>(d_td, nc(), d_tb, rsums, lam, val, in,
                                                            c_in, in2, c_in2, c_agg, out, nx);
  }
  void colsums() {
    if (n_pair) {
      dim3 g(cdiv(max_K, 4), n_pair);
      colsum_dot<T><<<g, 256, 0, stream>>>(d_pair, TU, V, tval);
    }
  }
  void weighted_A(const T* a, const GemmPlan<T>& plan, T* out, double beta = 0.0) {
    if (wa_fused) {
      (a == x ? p_wA_Ps : p_wA_dXs).launch(stream, 1.0, beta);
      return;
    }
    if (n_pair) {
      dim3 g(64, n_pair);
      scale_cols<T><<<g, 256, 0, stream>>>(d_scale, V, lam, ksamp, a, TW);
    }
    plan.launch(stream, 1.0, beta);
    if (anyMgt1) sym(out, out, 1, true);  // Symmetric(.) on blocks with m != 1 (MPMP.jl:1671-1674)
  }

  // ---------------- stages
  void st_mu_r(const clrsdp_params* prm, int pd_feas) {
    mu_scalars(prm, pd_feas);
    if (!body.fuse_r) mu_r_gemm();
  }
  // (round 6) a loop body at fp64 forms R = mu_p I - XY in XINV's launch, beside
  // X^-1 = L^-T L^-1: a mixed batch (gemm_f64_dyn, the mu_p diagonal from the scalar slot) instead
  // of a 128^3 GEMM launch of its own on the critical path before chol_inv(X, Y) -- R is first
  // read by the predictor's Z after SCHUR.  (The per-stage timing mode keeps the separate launch.)
  GemmPlan<T> p_xir;
  // mu = <X,Y>/dim, mu_p (and the status words cleared, the halt word decided)
  void mu_scalars(const clrsdp_params* prm, int pd_feas) {
    blk_dot(X, Y, nullptr, nullptr, 0, SC_DOT_XY, 1, upart);
    zero_info = true;  // the first scalar launch of an iteration clears the status words
    scalars(prm, pd_feas, 0);
  }
  void mu_r_gemm() { gemm_diag(p_XY, -1.0, 0.0, SC_MU_P); }  // R = mu_p I - XY
  // sum/max over the local blocks into sc[slot], all-gathered and rank-reduced when world > 1;
  // part: the flat_reduce partials are already there (<X,Y>, from update_state)
  void blk_dot(const T* A, const T* B_, const T* dA, const T* dB, int op, int slot, int tag,
               const T* part = nullptr) {
    if (world == 1 && nb()) {
      if (!part) launch_flat_reduce<T>(stream, A, B_, dA, dB, nblk_el, op, bpart);
      pend.push_back(flat_fold<T>(part ? part : bpart, op, slot));  // folded into the next scalar launch
      return;
    }
    if (part && nb()) vec_reduce_tree(part, RED_G, op, xsend);
    else local_blk_reduce(A, B_, dA, dB, op, xsend);
    exchange(tag, 1);
    reduce_ranks(1, 0, op == 2 ? 2 : 0, slot);
  }
  // plan.launch + "s I" on the block diagonals (fused into the fp64 GEMM epilogue)
  void gemm_diag(const GemmPlan<T>& plan, double alpha, double beta, int slot) {
    if constexpr (std::is_same<T, double>::value) {
      plan.launch(stream, alpha, beta, sc + slot, 1.0);
    } else {
      plan.launch(stream, alpha, beta);
      if (nb()) diag_add<T><<<nb(), 128, 0, stream>>>(d_blk, R, sc + slot, 1.0);
    }
  }
  void st_xinv() {
    if (reg_blk) {  // L_X^-1 and L_Y^-1 on chip in one launch, X^-1 = L^-T L^-1 on MFMA
      // (spd_xy: X^-1 comes out of the same launch, and a loop body forms R on the side stream)
      const bool spd = CholInvPlan<T>::spdinv_dispatch(ci_XY.nmax, lu_x(), spd_xy);
      ci_XY.launch(stream, info, spd);
      if (lu_x()) {
        xinv_lu();
        if (body.fuse_r) mu_r_gemm();
      } else if (spd) {
        body.r_late = body.fuse_r;
      } else if (body.fuse_r) {
        p_xir.launch(stream, 1.0, 0.0);  // {X^-1 = L^-T L^-1 | R = mu_p I - XY}
      } else {
        q_xinv.launch(stream, 1.0, 0.0);
      }
      return;
    }
    if (body.fuse_r) mu_r_gemm();
    blk_lin(LX, X, 1.0, nullptr, 0.0);
    f_X.potrf(stream, info);
    if (lu_x()) {
      xinv_lu();
      return;
    }
    if (nb()) blk_identity<T><<<nb(), 256, 0, stream>>>(d_blk, tA);
    t_Linv.launch(stream, false);             // tA = L^-1
    p_xinv.launch(stream, 1.0, 0.0);          // X^-1 = L^-T L^-1
  }
  // approx_inv! (MPMP.jl:781, 788): X_b^-1 = U_b^-1 L_b^-1 P_b by pivoted LU (the Cholesky factor
  // above stays: the step length needs it, cho! MPMP.jl:1846)
  void xinv_lu() {
    blk_lin(tA, X, 1.0, nullptr, 0.0);
    lu_X.launch(stream, info + info_L0);
    pm_I.launch(stream, true);                // Xinv = P I
    tl_X1.launch(stream, false);              // L^-1 (P I)
    tl_X2.launch(stream, true);               // U^-1 (L^-1 P I)
  }
  void st_schur() {
    if constexpr (std::is_same<T, double>::value) {
      if (fast_schur) {
        if (!schur_fused) p_txy.launch(stream, 1.0, 0.0);
        if (h_ty.armed()) {  // V^T Y came from the side stream
          h_ty.join(stream);
        } else if (!(schur_fused && fused_y)) {
          p_ty.launch(stream, 1.0, 0.0);
        }
        // the fused kernel writes the lower triangle of S only when every reader takes that
        // triangle (the fp64 Cholesky FACTOR: chol_inv_tiles, and L21^T = L11^-1 S21^T); the
        // pivoted LU and the rank-group sums read all of it
        const bool full = !fac2 || n_gsum > 0 || lu_sq();
        s_lower = schur_fused && !full;
        schur_full = (full || !schur_fused) ? 1 : 0;  // (schur_pairs_f64 always stores both triangles)
        if (schur_fused && fused_d64 && fused_grp2)
          schur_fused_f64<0, true, true, true, true><<<n_fwg, 512, schur_fused::LDS, stream>>>(d_fpd, d_fpt2d, stamps + 4, full);
        else if (schur_fused && fused_d64)
          schur_fused_f64<0, true, false, true, true><<<n_fwg, 512, schur_fused::LDS, stream>>>(d_fpd, d_fpt2d, stamps + 4, full);
        else if (schur_fused && fused_one && fused_grp2)
          schur_fused_f64<0, true, true, true><<<n_fwg, 512, schur_fused::LDS, stream>>>(d_fpd, d_fpt2d, stamps + 4, full);
        else if (schur_fused && fused_one)
          schur_fused_f64<0, true, false, true><<<n_fwg, 512, schur_fused::LDS, stream>>>(d_fpd, d_fpt2d, stamps + 4, full);
        else if (schur_fused && fused_y && fused_grp2)
          schur_fused_f64<0, true, true><<<n_fwg, 512, schur_fused::LDS, stream>>>(d_fpd, d_fpt2d, stamps + 4, full);
        else if (schur_fused && fused_y)
          schur_fused_f64<0, true><<<n_fwg, 512, schur_fused::LDS, stream>>>(d_fpd, d_fpt2d, stamps + 4, full);
        else if (schur_fused && fused_grp2)
          schur_fused_f64<0, false, true><<<n_fwg, 512, schur_fused::LDS, stream>>>(d_fpd, d_fpt2d, stamps + 4, full);
        else if (schur_fused)
          schur_fused_f64<0><<<n_fwg, 512, schur_fused::LDS, stream>>>(d_fpd, d_fpt2d, stamps + 4, full);
        else if (n_ptiles)
          schur_pairs_f64<16><<<n_ptiles, 256, 0, stream>>>(d_ptd, d_pt2d, stamps + 4);
        if (n_gsum) {
          dim3 g((unsigned)std::min<int64_t>(cdiv((int64_t)max_gD * max_gD, 256), 64), n_gsum);
          schur_gsum<T><<<g, 256, 0, stream>>>(d_gcd, d_sbd, rsums, BX, S);
        }
        HIPCHK(hipGetLastError());
        return;
      }
    }
    schur_full = 1;  // schur_assemble writes both triangles
    if (use_oz) {
      launch_ozaki();
    } else {
      p_s1x.launch(stream, 1.0, 0.0);
      p_s1y.launch(stream, 1.0, 0.0);
      p_s2x.launch(stream, 1.0, 0.0);
      p_s2y.launch(stream, 1.0, 0.0);
    }
    if (nb()) extract_AY<T><<<nb(), 256, 0, stream>>>(d_ayd, BY, AY);
    if (n_pairs)
      schur_assemble<T><<<cdiv(n_pairs, 256), 256, 0, stream>>>(d_scd, nc(), d_sbd, rsums, lam, BX,
                                                                 BY, S, n_pairs, mw_pair_upper ? 1 : 0);
  }
  void st_factor() {
    factor_local();
    factor_q();
  }
  // side_x21: X21 on the side stream (the loop body), joined before the first solve
  void factor_local(bool side_x21 = false) {
    s_lower = false;  // S now turns into L^-1 (or the LU factors)
    h_w.disarm();
    // (inner timing buckets: a mixed batch counts where most of its work is; the reference's
    // chol_S / CinvB / Q split, MPMP.jl:1429-1495)
    if (lu_sq()) {                            // approx_lu! (MPMP.jl:1433-1494)
      seg(CLRSDP_INNER_CHOL_S, [&] { lu_S.launch(stream, info + info_S0); });
      seg(CLRSDP_INNER_CINVB, [&] {
        pm_B.launch(stream);
        tl_W1.launch(stream, false);          // W1_j = L_j^-1 B_j[perm_j]
        vlin(W2m, Bm, 1.0, nullptr, 0, nullptr, 0, nB);
        tl_W2.launch(stream, false);          // W2_j = U_j^-T B_j
      });
      seg(CLRSDP_INNER_Q, [&] {
        lq_slab.launch(stream, 1.0, 0.0);     // slab_j = W2_j^T W1_j
        sum_q_slabs();
      });
      return;
    }
    if (fac2) {                               // fp64: S_j <- L_j^-1 in place, W_j and Q's slabs
      seg(CLRSDP_INNER_CHOL_S, [&] { ci_S.launch(stream, info + info_S0); });  // S / S11 blocks
      seg(CLRSDP_INNER_CINVB, [&] { f_a.launch(stream, 1.0, 0.0); });          // {L21^T | W}
      // W1 = L11^-1 B1, then W1^T W1 and B2' = B2 - L21 W1: beside the S22 chain in a loop body
      const bool split = side_x21 && nc2;
      auto w_work = [&] {
        seg(CLRSDP_INNER_CINVB, [&] { f_w.launch(stream, 1.0, 0.0); });
        seg(CLRSDP_INNER_Q, [&] { f_w2.launch(stream, 1.0, 0.0); });
      };
      if (split) {
        fork(fev[EV_FA], aux2, w_work);
        h_w.signal(aux2);
      } else {
        w_work();
      }
      seg(CLRSDP_INNER_CHOL_S, [&] { f_b.launch(stream, 1.0, 0.0); });         // S22 - L21 L21^T | W^T W
      if (nc2) {
        seg(CLRSDP_INNER_CHOL_S, [&] { ci_S22.launch(stream, info + info_S0 + nc()); });
        if (side_x21) {
          // X21 on the second side stream when W1's products went there (it is idle by now), so
          // that the first side stream is free for the right-hand side and chol(Q) as soon as Q
          // is summed
          const hipStream_t xs = split ? aux2 : aux;
          fork(fev[EV_X2], xs, [&] {
            seg(CLRSDP_INNER_CHOL_S, [&] {
              f_x1.launch(stream, 1.0, 0.0);
              f_x2.launch(stream, -1.0, 0.0);
            });
          });
          h_x21.signal(xs);
        } else {
          seg(CLRSDP_INNER_CHOL_S, [&] {
            f_x1.launch(stream, 1.0, 0.0);
            f_x2.launch(stream, -1.0, 0.0);
          });
        }
        h_w.wait(stream);  // (stays armed: the loop body's side stream joins it too)
        seg(CLRSDP_INNER_CINVB, [&] { f_c.launch(stream, 1.0, 0.0); });
        seg(CLRSDP_INNER_Q, [&] { f_d.launch(stream, 1.0, 1.0); });
      }
      seg(CLRSDP_INNER_Q, [&] { sum_q_slabs(); });
      return;
    }
    if (reg_S) {                              // S_j <- L_j^-1 in place; W_j = L_j^-1 B_j (MFMA)
      seg(CLRSDP_INNER_CHOL_S, [&] { ci_S.launch(stream, info + info_S0); });
      seg(CLRSDP_INNER_CINVB, [&] { q_W.launch(stream, 1.0, 0.0); });
    } else {
      seg(CLRSDP_INNER_CHOL_S, [&] { f_S.potrf(stream, info + info_S0); });
      if (s_split) {  // L_j^-1 for the GEMV solves, beside W_j and the Q chain
        const hipStream_t ls = side_x21 && aux2 ? aux2 : stream;  // (a loop body only)
        if (ls != stream) {
          fork(fev[EV_SP], ls, [&] { t_Sinv.launch(stream, false); });
          h_sinv.signal(ls);
        } else {
          t_Sinv.launch(stream, false);
        }
      }
      seg(CLRSDP_INNER_CINVB, [&] {
        if (!t_W.vec_rhs()) vlin(Wm, Bm, 1.0, nullptr, 0, nullptr, 0, nB);
        t_W.launch(stream, false);            // W_j = L_j^-1 B_j
      });
    }
    seg(CLRSDP_INNER_Q, [&] {
      p_Q.launch(stream, 1.0, 0.0);           // slab_j = W_j^T W_j
      sum_q_slabs();
    });
  }
  // Q = sum_j slab_j (all-gathered over the ranks)
  void sum_q_slabs() {
    const int64_t q2 = n_y * n_y;
    // (potrf factors Q in place in Qf: the slab sum writes that copy too, one launch fewer on the
    // critical path)
    T* q_dual = !reg_Q && Qf ? Qf : nullptr;
    qf_fresh = q_dual != nullptr;
    gather_sum(Qslab, nc(), q2, 2, Q, nullptr, 0.0, 1.0, q_dual);
  }
  // The sum over all clusters of `cnt` local slabs of n numbers each (stride n): where to read it.
  // One rank with slabs: the slabs themselves; otherwise this rank's sum (zeros without slabs)
  // is all-gathered and the slabs are the ranks' sums in xrecv.
  std::pair<const T*, int> gather_slabs(const T* slabs, int cnt, int64_t n, int tag) {
    if (world == 1 && cnt) return {slabs, cnt};
    if (cnt) launch_slab_sum4<T>(stream, slabs, cnt, n, n, xsend);
    else fill(xsend, 0.0, n);
    exchange(tag, n);
    return {xrecv, world};
  }
  // out = cbase * base + csum * (that sum), out2 (if any) the same: one launch at one rank
  void gather_sum(const T* slabs, int cnt, int64_t n, int tag, T* out, const T* base = nullptr,
                  double cbase = 0.0, double csum = 1.0, T* out2 = nullptr) {
    const auto [src, k] = gather_slabs(slabs, cnt, n, tag);
    launch_slab_sum4<T>(stream, src, k, n, n, out, base, cbase, csum, out2);
  }
  void factor_q() {
    seg(CLRSDP_INNER_CHOL_Q, [&] { factor_q_(); });
  }
  void factor_q_() {
    const int64_t q2 = n_y * n_y;
    const bool fresh = qf_fresh;  // Qf = Q written by this iteration's slab sum
    qf_fresh = false;
    if (lu_sq()) {                            // approx_lu!(perm, Q) (MPMP.jl:1499-1505)
      if (!fresh) vlin(Qf, Q, 1.0, nullptr, 0, nullptr, 0, q2);
      lu_Q.launch(stream, info + info_Q0);
      return;
    }
    if (reg_Q) {
      const bool spd = CholInvPlan<T>::spdinv_dispatch(ci_Q.nmax, lu_sq(), spd_q);
      ci_Q.launch(stream, info + info_Q0, spd);  // Qf = L_Q^-1 (spd: and Q^-1 beside it)
      if (!spd) q_qinv.launch(stream, 1.0, 0.0);  // Q^-1 = L_Q^-T L_Q^-1
    } else {
      if (!fresh) vlin(Qf, Q, 1.0, nullptr, 0, nullptr, 0, q2);
      f_Q.potrf(stream, info + info_Q0);
      if (q_split) {  // Q^-1 = L_Q^-T L_Q^-1 with L_Q^-1 = L_Q \ I
        t_Qinv.launch(stream, false);
        q_qinv2.launch(stream, 1.0, 0.0);
      }
    }
  }
  void st_residuals(bool use_AY) {
    residuals_local(use_AY);
    residuals_finish();
  }
  // P, d, the p-slabs and the local error maxima (no exchange: may run on the side stream)
  void residuals_local(bool use_AY) {
    residuals_P();
    residuals_rest(use_AY);
  }
  // P = sum_i x_i A_i - X - C (the state only)
  void residuals_P() {
    weighted_A(x, p_wA_P, P, -1.0);
    if (hasC) blk_lin(P, P, 1.0, Cm, -1.0);
  }
  // d, the p-slabs, the maxima of |P| and |d| (A_Y from SCHUR when use_AY)
  void residuals_rest(bool use_AY) {
    // d = c - B y - Tr(A_* Y)
    p_By.launch(stream, 1.0, 0.0);
    if (!use_AY) {
      p_trU_Y.launch(stream, 1.0, 0.0);
      colsums();
    }
    trace_aggregate(use_AY ? AY : tval, cvec, 1.0, tmpv, -1.0, -1.0, dvec);
    // p partial = sum_j B_j^T x_j (slabs) ; local maxima of |P| and |d| into tmpsc[0..1]
    p_Btx.launch(stream, 1.0, 0.0);
    local_blk_reduce(P, nullptr, nullptr, nullptr, 2, tmpsc);
    if (nx > 0) launch_vec_reduce<T>(stream, dvec, nullptr, nx, 2, tmpsc + 1);
    else fill(tmpsc + 1, 0.0, 1);
  }
  // defer (a loop body at one rank): the three error maxima are only read by the log and the
  // loop control at UPDATE, so their folds ride in CORRECTOR_R's scalar launch instead of a launch
  // of their own on the critical path before the predictor's solves (their sources, tmpsc and p,
  // are not written again before it; with world > 1 they come from the exchange buffer, which the
  // solves' all-gathers overwrite, so they are flushed here)
  void residuals_finish(bool defer = false) {
    const int64_t k = n_y + 2;
    if (world == 1 && nc()) {  // p = b - sum_j B_j^T x_j in one launch; maxima folded
      gather_sum(pslab, nc(), n_y, 3, pvec, bvec, 1.0, -1.0);
      fold(tmpsc, 1, 2, SC_ERR_PMAT);
      fold(tmpsc + 1, 1, 2, SC_ERR_DVEC);
      fold(pvec, (int)n_y, 4, SC_ERR_PVEC);
      if (!defer) flush_scalars();
      return;
    }
    if (nc()) launch_slab_sum4<T>(stream, pslab, nc(), n_y, n_y, xsend);
    else fill(xsend, 0.0, n_y);
    vlin(xsend + n_y, tmpsc, 1.0, nullptr, 0, nullptr, 0, 2);
    exchange(3, k);
    launch_slab_sum4<T>(stream, xrecv, world, k, n_y, uvec);
    vlin(pvec, bvec, 1.0, uvec, -1.0, nullptr, 0, n_y);      // p = b - sum B^T x
    reduce_ranks(k, n_y, 2, SC_ERR_PMAT);
    reduce_ranks(k, n_y + 1, 2, SC_ERR_DVEC);
    fold(pvec, (int)n_y, 4, SC_ERR_PVEC);
    flush_scalars();
  }
  void st_direction(int tag) {
    direction_Z();
    direction_rhs();
    direction_rest(tag);
  }
  // Z = sym(X^-1 (P Y - R)) and the trace_A products U = Z V (no factorisation needed: in a
  // loop body the predictor's share runs on the side stream during FACTOR)
  void direction_Z() {
    seg(CLRSDP_INNER_Z, [&] { direction_Z_(); });
  }
  void direction_Z_() {
    if (c_Z.on) {
      c_Z.launch(stream, 1.0, -1.0);
    } else {
      p_PY.launch(stream, 1.0, -1.0);
      p_Z.launch(stream, 1.0, 0.0);
    }
    // Z is only consumed by trace_A: v^T Z v = v^T sym(Z) v, so the symmetrisation
    // (MPMP.jl:1704-1716) matters only for the off-diagonal (r != s) blocks of m > 1
    if (anyMgt1) sym(Z, Z, 0);
    trace_products_Z_();
  }
  // U = Z V for trace_A (also what clrsdp_apply_operator's RHS runs on a Z given as it is)
  void trace_products_Z_() {
    if (!c_trZ.on) p_trU_Z.launch(stream, 1.0, 0.0);  // (else U stays on chip, direction_rhs_)
  }
  // rhs_x = -d - Tr(A_* Z)   (MPMP.jl:1733-1739)
  void direction_rhs() {
    seg(CLRSDP_INNER_RHS_X, [&] { direction_rhs_(); });
  }
  void direction_rhs_() {
    if (c_trZ.on) {
      c_trZ.launch(stream, 1.0, 0.0);   // rhs = -d - lambda (V^T Z V)_tt, U = Z V on chip
    } else if (trivial_tuples) {
      dim3 g(cdiv(max_K, 4), n_pair);
      colsum_rhs<T><<<g, 256, 0, stream>>>(d_pair, TU, V, lam, dvec, -1.0, nullptr, 0.0, -1.0, rhs);
    } else {
      colsums();
      trace_aggregate(tval, dvec, -1.0, nullptr, 0.0, -1.0, rhs);
    }
  }
  // the block solve (MPMP.jl:1743-1776), dX and dY
  void direction_rest(int tag) {
    seg(CLRSDP_INNER_SOLVE, [&] { direction_solves(tag); });
    // dX = P + sum_i dx_i A_i
    seg(CLRSDP_INNER_DX, [&] { weighted_A(dx, p_wA_dX, dX, 1.0); });
    if (tag == 6 && body.xy_ov_body && xy_ov_ok) {
      // the X step length beside dY and the Y one (STEP joins it)
      fork(fev[EV_DXO], aux, [&] {
        c_stepX.launch(stream, 1.0, 0.0);
        e_Xs.eigmin(stream, eigX);
      });
      h_stx.signal(aux);
    }
    // dY = sym(X^-1 (R - dX Y))
    seg(CLRSDP_INNER_DY, [&] {
      if (c_dY.on) {
        body.dy_dot_ready = dy_dot_ok && tag == 4;
        c_dY.u.dot_part = body.dy_dot_ready ? reinterpret_cast<double*>(dotp) : nullptr;
        c_dY.launch(stream, -1.0, 1.0);
      } else {
        p_dXY.launch(stream, -1.0, 1.0);
        p_dY.launch(stream, 1.0, 0.0);
      }
      sym(dY, dY, 0);
    });
  }
  // t_j = L_j^-1 rhs_j and the slabs W_j^T t_j: the part of the batched solve that needs no Q^-1
  // (it waits for X21 / L_j^-1 where a side stream produced them).  body.head_ahead: the loop body
  // has run it on the side stream already, beside chol(Q)
  void solve_head() {
    h_x21.join(stream);
    h_sinv.join(stream);
    if (reg_S) {
      q_t.launch(stream, 1.0, 0.0);
    } else if (s_split) {
      q_t2.launch(stream, 1.0, 0.0);
    } else {
      vlin(tvec, rhs, 1.0, nullptr, 0, nullptr, 0, nx);
      t_t.launch(stream, false);
    }
    p_Wt.launch(stream, 1.0, 0.0);
  }
  // the three-stage solve and dx as separate batched launches (any word type / rank count)
  void direction_solves(int tag) {
    // t_j = L_j^-1 rhs_j ;  u = sum_j W_j^T t_j ;  dy = Q^-1 (p - u) ; dx_j = L_j^-T (t_j + W_j dy)
    h_x21.join(stream);  // X21 (lower-left block of L^-1) comes from the side stream
    if (lu_sq()) {
      direction_solves_lu(tag);
      return;
    }
    if constexpr (std::is_same<T, double>::value) {
      if (cls_on) {  // t and the partial slabs | dy = Q^-1 (p - sum) | u and dx: three launches
        launch_cl_solve_t(stream, d_cls, nc(), cls_nrb, (int)n_y, pslab);
        const auto [src, cnt] = gather_slabs(pslab, nc() * cls_nrb, n_y, tag);  // (cls_on: nc() > 0)
        h_q.join(stream);
        launch_slab_qsolve(stream, src, cnt, n_y, (int)n_y, pvec, 1.0, -1.0, Qinv, (int)n_y, dyv);
        launch_cl_solve_dx(stream, d_cls, nc(), cls_nrb, (int)n_y, dyv);
        HIPCHK(hipGetLastError());
        return;
      }
    }
    if (body.head_ahead) body.head_ahead = false;  // (the loop body ran it on the side stream, beside chol(Q))
    else solve_head();
    // fp64 with the explicit Q^-1: r = p - sum of the slabs and dy = Q^-1 r in one launch
    // (slab_qsolve)
    bool fused_done = false;
    if constexpr (std::is_same<T, double>::value) {
      const size_t lds = slab_qsolve_lds(n_y);
      // every workgroup re-forms all of r: cdiv(n_y, 64) x cnt x n_y slab reads in all.  Fused
      // only while those stay small (C3: 2 x 64 x 128); otherwise slab_sum4 forms r once
      const long long cnt_x = (world == 1 && nc()) ? nc() : world;
      const bool small_sum = (long long)cdiv(n_y, 64) * cnt_x * n_y <= (1LL << 20);
      if (reg_Q && small_sum && lds <= 64 * 1024) {
        const auto [src, cnt] = gather_slabs(pslab, nc(), n_y, tag);
        h_q.join(stream);
        launch_slab_qsolve(stream, src, cnt, n_y, (int)n_y, pvec, 1.0, -1.0, Qinv, (int)n_y, dyv);
        HIPCHK(hipGetLastError());
        fused_done = true;
      }
    }
    if (!fused_done) {
      // r = p - sum_j W_j^T t_j  (-> uvec with the explicit Q^-1, -> dyv for the two solves)
      T* rv = (reg_Q || q_split) ? uvec : dyv;
      gather_sum(pslab, nc(), n_y, tag, rv, pvec, 1.0, -1.0);
      h_q.join(stream);  // L_Q^-1 and Q^-1 are being computed on the side stream (iterate)
      if (reg_Q || q_split) {
        q_qdy.launch(stream, 1.0, 0.0);         // dy = Q^-1 r
      } else {
        t_Q.launch(stream, false);
        t_Q.launch(stream, true);
      }
    }
    // dx_j = L_j^-T (t_j + W_j dy)
    if (reg_S || s_split) {
      q_Wdy.launch(stream, 1.0, 1.0);
      (s_split ? q_dx2 : q_dx).launch(stream, 1.0, 0.0);
    } else {
      p_Wdy.launch(stream, 1.0, 1.0);
      t_dx.launch(stream, true);
    }
  }
  // the same with the LU factors (approx_solve_tril!/approx_solve_lu_precomp!/approx_solve_triu!,
  // MPMP.jl:1751-1773)
  void direction_solves_lu(int tag) {
    pm_rhs.launch(stream);                    // t_j = rhs_j[perm_j]
    tl_t.launch(stream, false);               // t_j = L_j^-1 t_j
    lq_Wt.launch(stream, 1.0, 0.0);           // slab_j = W2_j^T t_j  (B_j^T U_j^-1 t_j)
    gather_sum(pslab, nc(), n_y, tag, uvec, pvec, 1.0, -1.0);
    h_q.join(stream);
    pm_r.launch(stream);                      // dy = (p - u)[perm_Q]
    tl_Q1.launch(stream, false);              // L_Q^-1
    tl_Q2.launch(stream, true);               // U_Q^-1
    p_Wdy.launch(stream, 1.0, 1.0);           // dx_j = t_j + W1_j dy
    tl_dx.launch(stream, true);               // dx_j = U_j^-1 (.)
  }
  void st_corrector_r(const clrsdp_params* prm, int pd_feas) {
    if (body.dy_dot_ready) fold(dotp, dy_dot_cnt, 0, SC_DOT_XDY);  // (from the predictor's dY chain)
    else blk_dot(X, Y, dX, dY, 1, SC_DOT_XDY, 5);
    body.dy_dot_ready = false;
    scalars(prm, pd_feas, 1);
    if constexpr (std::is_same<T, double>::value) {
      // R still holds mu_p I - XY from MU_R (the predictor only reads it), so one GEMM:
      // R = (mu_p I - XY) - dX dY + (mu_c - mu_p) I, without forming XY again
      gemm_diag(p_dXdY, -1.0, 1.0, SC_DMU);
    } else {  // multi-word: the reference's order of operations (MPMP.jl:1209-1214)
      p_XY.launch(stream, -1.0, 0.0);
      gemm_diag(p_dXdY, -1.0, 1.0, SC_MU_C);    // R = mu_c I - XY - dX dY
    }
  }
  void st_step(const clrsdp_params* prm, int pd_feas) {
    if (reg_blk) {
      // L_X^-1, L_Y^-1 from the X^-1 stage;  M = L^-1 dM L^-T on MFMA; one eigen launch
      if (h_stx.armed()) {  // (the X half is on the side stream since dX)
        c_stepY.launch(stream, 1.0, 0.0);
        e_Ys.eigmin(stream, eigY);
        h_stx.join(stream);
      } else {
        if (c_step.on) {
          c_step.launch(stream, 1.0, 0.0);        // X and Y blocks together, one launch
        } else {
          q_sx1.launch(stream, 1.0, 0.0);         // X and Y blocks together
          q_sx2.launch(stream, 1.0, 0.0);
        }
        e_XY.eigmin(stream, eigX);
      }
    } else {
      // X: L_X from the X^-1 stage
      blk_lin(tA, dX, 1.0, nullptr, 0.0);
      t_sX1.launch(stream, false);
      sym(tB, tA, 2);
      t_sX2.launch(stream, false);
      e_X.eigmin(stream, eigX);
      // Y
      blk_lin(LY, Y, 1.0, nullptr, 0.0);
      f_Y.potrf(stream, info + info_Y0);
      blk_lin(tA, dY, 1.0, nullptr, 0.0);
      t_sY1.launch(stream, false);
      sym(tB, tA, 2);
      t_sY2.launch(stream, false);
      e_Y.eigmin(stream, eigY);
    }
    if (world == 1 && nb() && body.fuse_alpha) {
      // (a loop body: the minima and alpha are formed by UPDATE's update_state, one launch less)
      flush_scalars();
      body.alpha_fused = true;
      return;
    }
    if (world == 1 && nb()) {  // min over the blocks straight into the scalar slots
      fold(eigX, nb(), 3, SC_MINEIG_X);
      fold(eigY, nb(), 3, SC_MINEIG_Y);
    } else {
      if (nb()) {
        launch_ordered_reduce<T>(stream, eigX, nb(), 1, 3, xsend);
        launch_ordered_reduce<T>(stream, eigY, nb(), 1, 3, xsend + 1);
      } else {
        fill(xsend, 1e300, 2);  // no local blocks: neutral element of min
      }
      // + this rank's failure bits: every rank guards its update and reports (and falls back)
      // on the OR over all ranks, so the ranks stay in step
      status_bits<T><<<1, 256, 0, stream>>>(info, nb(), nc() + nc2, info_S0, info_Q0, info_L0, xsend + 2);
      exchange(8, 3);
      status_gather<T><<<1, 64, 0, stream>>>(xrecv, world, 3, 2, info + info_G);
      reduce_ranks(3, 0, 3, SC_MINEIG_X);
      reduce_ranks(3, 1, 3, SC_MINEIG_Y);
    }
    scalars(prm, pd_feas, 2);
  }
  void objectives(const clrsdp_params* prm, int pd_feas, int which = 3) {
    zero_cy = !hasC;
    if (world == 1) {
      if (nx > 0) launch_vec_reduce<T>(stream, cvec, x, nx, 0, sc + SC_DOT_CX);
      else fill(sc + SC_DOT_CX, 0.0, 1);
      if (hasC) local_blk_reduce(Cm, Y, nullptr, nullptr, 0, sc + SC_DOT_CY);
    } else {
      if (nx > 0) launch_vec_reduce<T>(stream, cvec, x, nx, 0, xsend);
      else fill(xsend, 0.0, 1);
      if (hasC) local_blk_reduce(Cm, Y, nullptr, nullptr, 0, xsend + 1);
      else fill(xsend + 1, 0.0, 1);
      exchange(9, 2);
      reduce_ranks(2, 0, 0, SC_DOT_CX);
      reduce_ranks(2, 1, 0, SC_DOT_CY);
    }
    launch_vec_reduce<T>(stream, bvec, y, n_y, 0, sc + SC_DOT_BY);
    scalars(prm, pd_feas, which);
    zero_cy = false;
  }
  void st_update(const clrsdp_params* prm, int pd_feas) {
    // one launch updates x, y, X, Y (guarded by the status words: no update after a failed
    // factorisation) and leaves the partial sums <X,Y> (next MU_R), <c,x> and <b,y>
    StepAlpha<T> sa{};
    if (body.alpha_fused) {
      sa.eigX = eigX;
      sa.eigY = eigY;
      sa.nb = nb();
      sa.pd_feas = pd_feas;
      sa.gamma = limbs(prm->gamma);
      sa.sc = sc;
      sa.sx = SC_MINEIG_X;
      sa.sy = SC_MINEIG_Y;
      sa.sap = SC_ALPHA_P;
      sa.sad = SC_ALPHA_D;
      sa.pdslot = SC_PDFEAS;
      body.alpha_fused = false;
    }
    launch_update_state<T>(stream, X, dX, Y, dY, nblk_el, x, dx, nx, cvec, y, dyv, n_y, bvec,
                           sc + SC_ALPHA_P, sc + SC_ALPHA_D, info, info_count, upart, sa);
    if (world == 1 && !hasC) {  // the objectives from the partials, folded into one scalar launch
      zero_cy = true;
      fold(upart + RED_G, RED_G, 0, SC_DOT_CX);
      fold(upart + 2 * RED_G, RED_G, 0, SC_DOT_BY);
      scalars(prm, pd_feas, 3);
      zero_cy = false;
      return;
    }
    objectives(prm, pd_feas);
  }
  // <X,Y> partials of the current state, as update_state leaves them (after a state change
  // from the host: set_state, restore_state)
  void refresh_xy_part() {
    launch_flat_reduce<T>(stream, X, Y, nullptr, nullptr, nblk_el, 0, upart);
    HIPCHK(hipGetLastError());
  }

  void stage(int s, const clrsdp_params* prm, int pd_feas) {
    switch (s) {
      case CLRSDP_STAGE_MU_R: st_mu_r(prm, pd_feas); break;
      case CLRSDP_STAGE_XINV: st_xinv(); break;
      case CLRSDP_STAGE_SCHUR: st_schur(); break;
      case CLRSDP_STAGE_FACTOR: st_factor(); break;
      case CLRSDP_STAGE_RESIDUALS: st_residuals(true); break;
      case CLRSDP_STAGE_PREDICTOR: st_direction(4); break;
      case CLRSDP_STAGE_CORRECTOR_R: st_corrector_r(prm, pd_feas); break;
      case CLRSDP_STAGE_CORRECTOR: st_direction(6); break;
      case CLRSDP_STAGE_STEP: st_step(prm, pd_feas); break;
      case CLRSDP_STAGE_UPDATE: st_update(prm, pd_feas); break;
      default: throw ClrsdpError{CLRSDP_E_ARG, "bad stage"};
    }
    HIPCHK(hipGetLastError());
  }

  // both parse the host mirror filled by stat_fetch().  Failure bits: 1 S_j, 2 Q, 4 X
  // (Cholesky), 8 X^-1 by LU, 16 Y (step length); with world > 1 the OR over all ranks
  // (info_G, STEP's exchange), so every rank returns the same code
  int fail_bits(const int* h) const {
    int b = 0;
    for (int i = 0; i < nb(); ++i) {
      if (h[i]) b |= 4;
      if (h[info_Y0 + i]) b |= 16;
      if (h[info_L0 + i]) b |= 8;
    }
    for (int i = 0; i < nc() + nc2; ++i)
      if (h[info_S0 + i]) b |= 1;
    if (h[info_Q0]) b |= 2;
    return b;
  }
  int check_info(const char* blk = nullptr) {
    const int* h = reinterpret_cast<const int*>((blk ? blk : stat_host) + stat_info_off);
    // local bits always (run_stage reports a failure at the stage where it happens); with
    // world > 1 also the OR over all ranks, which STEP's exchange wrote into info_G
    const int b = fail_bits(h) | ((world > 1 && (comm || xfn)) ? h[info_G] : 0);
    if (b & 4) {
      if (lu_x()) {  // X^-1 came from LU; cho!(X) of the step length failed (MPMP.jl:1846-1882)
        err = "The step length could not be calculated correctly (X not PD).";
        return CLRSDP_E_STEP;
      }
      err = "X block not positive definite (spd_inv! failed)";
      return CLRSDP_E_NOT_PD_X;
    }
    if (b & 8) { err = "The inverse was not computed correctly. Try again with higher precision"; return CLRSDP_E_NOT_PD_X; }
    if (b & 1) { err = "S was not decomposed succesfully, try again with higher precision"; return CLRSDP_E_NOT_PD_S; }
    if (b & 2) { err = "Q was not decomposed correctly. Try restarting with a higher precision."; return CLRSDP_E_NOT_PD_Q; }
    if (b & 16) { err = "The step length could not be calculated correctly (Y not PD)."; return CLRSDP_E_STEP; }
    return CLRSDP_OK;
  }
  // A Cholesky failure the LU fallback covers: switch (for the rest of the solve) and report
  // true, so the caller re-runs the loop body (its update was skipped, the state is unchanged)
  bool fallback(int rc) {
    if (!(fact_flags & CLRSDP_FACT_FALLBACK)) return false;
    int add = 0;
    if ((rc == CLRSDP_E_NOT_PD_S || rc == CLRSDP_E_NOT_PD_Q) && !lu_sq()) add = CLRSDP_FACT_LU_SQ;
    else if (rc == CLRSDP_E_NOT_PD_X && !lu_x()) add = CLRSDP_FACT_LU_X;
    // beyond the LU solves' panel (or getrf_batched's with CLRSDP_LU_BLK=0): the reference's
    // error stands
    if (!add || !build_lu_plans(false)) return false;
    fact_flags |= add;
    drop_graphs();
    ++fallbacks;
    return true;
  }
  int fallbacks = 0;

  void read_stats(clrsdp_iter_stats* st, const char* blk = nullptr) {
    const T* h = reinterpret_cast<const T*>(blk ? blk : stat_host);
    auto f = [&](int i) { return Num<T>::hi(h[i]); };
    st->mu = f(SC_MU);
    st->P_err = f(SC_ERR_PMAT);
    st->p_err = f(SC_ERR_PVEC);
    st->d_err = f(SC_ERR_DVEC);
    st->alpha_p = f(SC_ALPHA_P);
    st->alpha_d = f(SC_ALPHA_D);
    st->beta_c = f(SC_BETA_C);
    st->p_obj = f(SC_POBJ);
    st->d_obj = f(SC_DOBJ);
    auto limbs_of = [&](int i, double* dst) {
      const double* l = reinterpret_cast<const double*>(&h[i]);
      for (int q = 0; q < 4; ++q) dst[q] = q < Num<T>::W ? l[q] : 0.0;
    };
    limbs_of(SC_GAP, st->gap_w);
    limbs_of(SC_ERR_PMAT, st->P_err_w);
    limbs_of(SC_ERR_PVEC, st->p_err_w);
    limbs_of(SC_ERR_DVEC, st->d_err_w);
  }

  int initial(const clrsdp_params* prm, clrsdp_iter_stats* st) override {
    if (!uploaded) { err = "constraints not uploaded"; return CLRSDP_E_STATE; }
    std::memset(st, 0, sizeof(*st));
    st_residuals(false);
    objectives(prm, 0, 4);   // + gap / pd_feas / terminate of the initial point (device control)
    stat_fetch();
    read_stats(st);
    return CLRSDP_OK;
  }

  // Enqueue one loop body (all stages) on `stream`, with the side stream joined back in.
  void enqueue_iteration(const clrsdp_params* prm, int pd_feas) {
    segs.clear();
    // (the status words are cleared by the first scalar launch of MU_R)
    auto mark = [&](int s) {
      if (timing == 1) HIPCHK(hipEventRecord(ev[s], stream));
    };
    // pipelined loop: P, p, d of every body that runs are copied aside (guarded by the halt
    // word), so a skipped body leaves the residuals of the last iteration that ran, which the
    // reference returns (MPMP.jl:1014-1024)
    const bool keep_res = pd_feas < 0;
    // The side stream runs everything of RESIDUALS and of the predictor's right-hand side that
    // does not need the Schur factorisation, as soon as its inputs exist, so that it overlaps
    // XINV, SCHUR and FACTOR (whose on-chip factorisations leave most CUs idle):
    //   after MU_R:  P = sum x_i A_i - X - C                      (state only)
    //   after SCHUR: d, the p-slabs, the maxima (A_Y from SCHUR); Z = X^-1 (P Y - R), U = Z V
    //                and rhs = -d - Tr(A_* Z)                     (the predictor's trace_A)
    //   after FACTOR's Q sum: chol(Q) -> L_Q^-1, Q^-1 -- or, with q_main below, p, the guarded
    //                copy and the head of the predictor's solve while the main stream factors Q
    const hipStream_t main_s = stream;
    body.fuse_r = std::is_same<T, double>::value && timing != 1 && !p_xir.h.empty();
    mark(CLRSDP_STAGE_MU_R);
    stage(CLRSDP_STAGE_MU_R, prm, pd_feas);
    // V^T Y of the Schur stage only needs the state: it runs beside chol_inv(X, Y), which leaves
    // half the CUs idle, and SCHUR waits for it (h_ty) before the pairs launch
    const bool ty_side = fast_schur && !p_ty.h.empty() && !(schur_fused && fused_y);
    // P = sum x_i A_i - X - C is first read by the side stream's Z after SCHUR: enqueued there
    // (one fork of the critical path fewer) unless V^T Y needs the fork anyway
    const bool p_late = !ty_side;
    if (!p_late)
      fork(fev[EV_M], aux, [&] {
        if (ty_side) {
          p_ty.launch(stream, 1.0, 0.0);
          h_ty.signal(stream);
        }
        residuals_P();
      });
    mark(CLRSDP_STAGE_XINV);
    stage(CLRSDP_STAGE_XINV, prm, pd_feas);
    body.fuse_r = false;
    mark(CLRSDP_STAGE_SCHUR);
    stage(CLRSDP_STAGE_SCHUR, prm, pd_feas);
    // (Z waits for SCHUR although it could start after XINV: beside the MFMA-bound Schur
    // products it only slowed them down, beside FACTOR's latency-bound factorisations it is free)
    // The predictor's Z first (its MFMA chain fills the CUs that chol(S11) leaves idle), then the
    // residuals; the right-hand side (U = Z V and its column sums) after FACTOR's side products
    // W1^T W1 and B2' (h_w), which are on the critical path to W2 = L22^-1 B2'
    fork(fev[EV_S], aux, [&] {
      if (body.r_late) mu_r_gemm();  // R = mu_p I - XY, first read by Z below
      body.r_late = false;
      if (p_late) residuals_P();
      direction_Z();
      residuals_rest(true);
      if (keep_res) {
        copy_guarded2(Pres, P, nblk_el, dres, dvec, nx);
      }
    });
    mark(CLRSDP_STAGE_FACTOR);
    factor_local(true);
    // fp64 at one rank with the batched Cholesky solves: chol(Q) -> L_Q^-1, Q^-1 stays on the main
    // stream right behind the Q sum (they are the critical path), and what the main stream used
    // to run meanwhile goes to the side stream behind the right-hand side: p and the error folds,
    // the guarded copy of p, and the head of the predictor's solve (t = L^-1 rhs, the slabs
    // W^T t), none of which reads Q.  One join, just before the Q solve; no fork for chol(Q).
    const bool q_main = sw.qchol_main && std::is_same<T, double>::value && world == 1 && timing != 1 &&
                        nc() && !lu_sq() && !cls_on;
    {
      h_w.join(aux);
      StreamSwitch on_aux(stream, aux);
      direction_rhs();
      if (!q_main) HIPCHK(hipEventRecord(fev[EV_R], aux));
    }
    if (q_main) {
      fork(fev[EV_QA], aux, [] {});  // (the side stream goes on below, once Q is being factored)
      factor_q();
      if (capturing && inject_capture_fail)
        throw ClrsdpError{CLRSDP_E_HIP, "injected capture failure (CLRSDP_INJECT_CAPTURE_FAIL)"};
      {
        // (behind EV_QA: W, L^-1 and the halt word come from the main stream)
        StreamSwitch on_aux(stream, aux);
        residuals_finish(true);
        if (keep_res) copy_guarded(pres, pvec, n_y);
        solve_head();
        body.head_ahead = true;
        HIPCHK(hipEventRecord(fev[EV_R], aux));
      }
      HIPCHK(hipStreamWaitEvent(main_s, fev[EV_R], 0));
    } else {
      // side stream: chol(Q) -> L_Q^-1, waited for just before the first Q solve
      fork(fev[EV_QA], aux, [&] { factor_q(); });
      h_q.signal(aux);
      if (capturing && inject_capture_fail)
        throw ClrsdpError{CLRSDP_E_HIP, "injected capture failure (CLRSDP_INJECT_CAPTURE_FAIL)"};
      mark(CLRSDP_STAGE_RESIDUALS);
      HIPCHK(hipStreamWaitEvent(main_s, fev[EV_R], 0));
      residuals_finish(timing != 1);
      if (keep_res) copy_guarded(pres, pvec, n_y);
    }
    HIPCHK(hipGetLastError());
    mark(CLRSDP_STAGE_PREDICTOR);
    direction_rest(4);   // Z, U and rhs came from the side stream
    // (STEP's alpha is formed inside UPDATE's launch; the per-stage timing mode keeps the scalar
    // launch so STEP's time includes alpha)
    body.fuse_alpha = timing != 1;
    body.xy_ov_body = timing != 1;
    for (int s = CLRSDP_STAGE_CORRECTOR_R; s < CLRSDP_NUM_STAGES; ++s) {
      mark(s);
      stage(s, prm, pd_feas);
    }
    body.fuse_alpha = false;
    body.xy_ov_body = false;
    // whatever no stage joined (a hand-off whose consumer did not run) joins the main stream here
    for (Handoff* h : handoffs) h->join(stream);
    if (timing == 1) HIPCHK(hipEventRecord(ev[CLRSDP_NUM_STAGES], stream));
  }

  // One hipGraph per pd_feas value replays the whole loop body with a single launch (one
  // process per GPU with no exchange, and no per-stage timing).  The scalar parameters are
  // baked into the graph, so a change of them re-captures.
  // pd_feas 0, 1 and decided on the device (two instances of that one, used alternately, so a
  // launch never waits for the previous launch of the same executable graph)
  hipGraphExec_t gexec[4] = {nullptr, nullptr, nullptr, nullptr};
  clrsdp_params gprm[4];
  bool gpub[4] = {false, false, false, false};  // captured as a publishing body (publish_ok())
  unsigned graph_launches = 0;
  // multi-word bodies are enqueued eagerly by default: C5 (qd) 719-730 against 672-706 it/s,
  // C4 (dd) 620-625 against 600-617 with the replayed graph (A/B, round 4); fp64 keeps the
  // replay (C3 equal, C2 2288-2315 against 2122-2288 eager); CLRSDP_GRAPH_MW=1 replays
  // multi-word bodies too
  bool use_graph = !sw.no_graph && (sizeof(T) == 8 || sw.graph_mw);
  // multi-rank loop bodies with the native communicator are enqueued eagerly by default (the
  // pipelined host loop hides the enqueue); CLRSDP_GRAPH_RCCL=1 captures the all-gathers into
  // the replayed graph as well
  bool graph_rccl = sw.graph_rccl;
  void set_graph(int on) override {
    if (inflight) throw ClrsdpError{CLRSDP_E_STATE, "set_graph with loop bodies in flight"};
    use_graph = on != 0;
  }
  // the exchange the loop body uses: backend 0 none (one rank), 1 the native RCCL communicator
  // (nranks = ncclCommCount), 2 the registered callback (nranks = world_size)
  void comm_info(int* nranks, int* backend) const override {
    *backend = comm ? 1 : (xfn ? 2 : 0);
    *nranks = world;
    if (comm && rccl().comm_count) {
      int n = 0;
      if (rccl().comm_count(comm, &n) == ncclSuccess) *nranks = n;
    }
  }
  bool graph_ok() const { return use_graph && timing != 1 && (world == 1 || (comm && graph_rccl)); }
  // forget every captured loop body (they are re-captured on their next use)
  void drop_graphs() {
    for (hipGraphExec_t& g : gexec)
      if (g) {
        HIPCHK(hipGraphExecDestroy(g));
        g = nullptr;
      }
  }
  void launch_graph(const clrsdp_params* prm, int pd_feas) {
    // (one executable for every pipelined body measured the same as two alternating, round 4)
    const int g = pd_feas < 0 ? 2 + (graph_launches++ & 1) : (pd_feas ? 1 : 0);
    if (!gexec[g] || std::memcmp(&gprm[g], prm, sizeof(*prm)) != 0 || gpub[g] != pub_body) {
      if (gexec[g]) HIPCHK(hipGraphExecDestroy(gexec[g]));
      gexec[g] = nullptr;
      hipGraph_t graph = nullptr;
      HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
      try {
        capturing = true;
        enqueue_iteration(prm, pd_feas);
        capturing = false;
      } catch (...) {
        capturing = false;
        // join the side stream (it may have been forked into the capture) so that the capture
        // ends cleanly and the streams stay usable
        if (hipEventRecord(fev[EV_JOIN], aux) == hipSuccess)
          (void)hipStreamWaitEvent(stream, fev[EV_JOIN], 0);
        if (hipEventRecord(fev[EV_JOIN2], aux2) == hipSuccess)
          (void)hipStreamWaitEvent(stream, fev[EV_JOIN2], 0);
        (void)hipStreamEndCapture(stream, &graph);
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        throw;
      }
      HIPCHK(hipStreamEndCapture(stream, &graph));
      HIPCHK(hipGraphInstantiate(&gexec[g], graph, nullptr, nullptr, 0));
      HIPCHK(hipGraphDestroy(graph));
      gprm[g] = *prm;
      gpub[g] = pub_body;
    }
    HIPCHK(hipGraphLaunch(gexec[g], stream));
  }

  // A sharded body whose capture fails (CLRSDP_GRAPH_RCCL with an RCCL that cannot be captured)
  // is enqueued eagerly instead, and the handle stays eager from then on; one rank rethrows (its
  // capture has no collective in it, so a failure there is a real error)
  // CLRSDP_INJECT_CAPTURE_FAIL=1 (tests only, read per handle): the first capture of a loop body
  // throws half-way through its enqueue, after the side streams were forked and the pending
  // flags set, and the body takes the sharded path's eager fallback even at one rank
  bool inject_capture_fail = sw.inject_capture_fail;
  bool capturing = false;
  // the per-body enqueue state a failed (partial) capture may have left set; an eager re-enqueue
  // must not wait on events recorded only inside the aborted capture
  void reset_body_state() {
    body = {};
    for (Handoff* h : handoffs) h->disarm();
  }
  void launch_graph_or_eager(const clrsdp_params* prm, int pd_feas) {
    if (world == 1 && !inject_capture_fail) {
      launch_graph(prm, pd_feas);
      return;
    }
    try {
      launch_graph(prm, pd_feas);
    } catch (const ClrsdpError& e) {
      std::fprintf(stderr, "clrsdp: graph capture of the sharded loop body failed (%s); "
                           "enqueueing it eagerly from now on\n", e.msg.c_str());
      graph_rccl = false;
      inject_capture_fail = false;
      reset_body_state();
      enqueue_iteration(prm, pd_feas);
    }
  }
  int iterate(const clrsdp_params* prm, int pd_feas, clrsdp_iter_stats* st) override {
    if (!uploaded) { err = "constraints not uploaded"; return CLRSDP_E_STATE; }
    if (inflight) { err = "iterate with loop bodies in flight (call iterate_wait)"; return CLRSDP_E_STATE; }
    for (;;) {
      const int rc = iterate_once(prm, pd_feas, st);
      if (!fallback(rc)) return rc;
    }
  }
  int iterate_once(const clrsdp_params* prm, int pd_feas, clrsdp_iter_stats* st) {
    // (a publishing body: its last scalar launch fills the host mirror, see publish_ok())
    const bool pub = publish_ok(pd_feas);
    const unsigned long long seq0 = pub ? pub_seq_now() : 0ull;
    if (graph_ok()) {
      pub_body = pub;
      try {
        launch_graph_or_eager(prm, pd_feas);
      } catch (...) {
        pub_body = false;
        throw;
      }
      pub_body = false;
    } else {
      enqueue_iteration(prm, pd_feas);
    }
    res_from_copy = false;
    std::memset(st, 0, sizeof(*st));
    if (pub) pub_wait(seq0);
    else stat_fetch();
    read_stats(st);
    if (timing == 2) {  // the SCHUR stage of the body that just ran (device clock stamps)
      const unsigned long long* t = reinterpret_cast<const unsigned long long*>(stat_host + stat_stamp_off);
      // the durations of its three launches (V^T X^-1, V^T Y -- ahead on the side stream in a
      // loop body -- and the pairs), first workgroup start to last workgroup end each
      double ticks = 0.0;
      for (int q = 0; q < 3; ++q)
        if (t[2 * q + 1] > t[2 * q]) ticks += (double)(t[2 * q + 1] - t[2 * q]);
      st->phase_ms[CLRSDP_STAGE_SCHUR] = ticks * 1e-5;  // 100 MHz
    }
    if (timing == 1) {
      for (int s = 0; s < CLRSDP_NUM_STAGES; ++s) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev[s], ev[s + 1]));
        st->phase_ms[s] = ms;
      }
      for (const auto& g : segs) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, seg_pool[g[1]], seg_pool[g[2]]));
        st->inner_ms[g[0]] += ms;
      }
      st->inner_ms[CLRSDP_INNER_SCHUR] = st->phase_ms[CLRSDP_STAGE_SCHUR];
    }
    const int rc = check_info();
    st->status = rc;
    // (a failed body may be followed by fallback(), which destroys the graphs: the replay has
    // published, but the runtime may not have retired it yet)
    if (pub && rc != CLRSDP_OK) HIPCHK(hipStreamSynchronize(stream));
    return rc;
  }
  // 0: off (graph replay); 1: every stage between HIP events, no graph; 2: graph replay, and the
  // SCHUR stage timed inside the replayed body by the 100 MHz clock: the sum over its launches of
  // first workgroup start to last workgroup end (atomics in the stat block)
  void set_timing(int on) override {
    if (on < 0 || on > 2) throw ClrsdpError{CLRSDP_E_ARG, "timing mode must be 0, 1 or 2"};
    timing = on;
  }

  // device-side snapshot of the iterate (x, X, y, Y) and the scalar slots, stream-ordered
  T* snap = nullptr;
  bool snapped = false;
  void snap_copy(bool save) {
    const int64_t B = nblk_el;
    T* dst[5] = {snap, snap + nx, snap + nx + B, snap + nx + 2 * B, snap + nx + 2 * B + n_y};
    T* src[5] = {x, X, Y, y, sc};
    const int64_t cnt[5] = {nx, B, B, n_y, (int64_t)SC_COUNT};
    for (int i = 0; i < 5; ++i)
      if (cnt[i])
        HIPCHK(hipMemcpyAsync(save ? dst[i] : src[i], save ? src[i] : dst[i], cnt[i] * sizeof(T),
                              hipMemcpyDeviceToDevice, stream));
  }
  void save_state() override {
    if (!snap) snap = dmalloc<T>((size_t)nx + 2 * (size_t)nblk_el + (size_t)n_y + SC_COUNT);
    snap_copy(true);
    snapped = true;
  }
  void restore_state() override {
    body.dy_dot_ready = false;
    if (!snapped) throw ClrsdpError{CLRSDP_E_STATE, "restore_state without save_state"};
    snap_copy(false);
    refresh_xy_part();
  }

  // ---- pipelined loop: the host enqueues loop body k+1 before it reads the log row of body k.
  // pd_feas and terminate() are evaluated on the device at the end of each update (and by
  // initial_residuals); a body enqueued after the device decided to terminate changes no
  // state (the halt word guards every update like a failed factorisation) and reports ran = 0.
  char* ring_host[2] = {nullptr, nullptr};
  hipEvent_t ring_ev[2] = {nullptr, nullptr};
  int ring_head = 0, inflight = 0;
  clrsdp_params last_prm{};
  int iterate_async(const clrsdp_params* prm) override {
    if (!uploaded) { err = "constraints not uploaded"; return CLRSDP_E_STATE; }
    last_prm = *prm;
    if (inflight >= 2) { err = "two loop bodies already in flight (call iterate_wait)"; return CLRSDP_E_STATE; }
    if (!ring_host[0]) {
      for (int i = 0; i < 2; ++i) {
        HIPCHK(hipHostMalloc((void**)&ring_host[i], stat_bytes, hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&ring_ev[i], hipEventDisableTiming));
      }
    }
    if (graph_ok()) launch_graph_or_eager(prm, -1);
    else enqueue_iteration(prm, -1);
    const int slot = (ring_head + inflight) % 2;
    HIPCHK(hipMemcpyAsync(ring_host[slot], stat_dev, stat_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(ring_ev[slot], stream));
    ++inflight;
    return CLRSDP_OK;
  }
  int iterate_wait(clrsdp_iter_stats* st, int* ran) override {
    if (!inflight) { err = "no loop body in flight"; return CLRSDP_E_STATE; }
    const int slot = ring_head;
    ring_head = (ring_head + 1) % 2;
    --inflight;
    HIPCHK(hipEventSynchronize(ring_ev[slot]));
    std::memset(st, 0, sizeof(*st));
    read_stats(st, ring_host[slot]);
    const int* h = reinterpret_cast<const int*>(ring_host[slot] + stat_info_off);
    const bool halted = h[info_H] != 0;
    if (ran) *ran = halted ? 0 : 1;
    res_from_copy = true;
    if (halted) return CLRSDP_OK;   // skipped body: its factorisations may fail, nothing applied
    const int rc = check_info(ring_host[slot]);
    st->status = rc;
    const int behind = inflight;
    // a failed body: the bodies behind it may still execute (from the replayed graphs), so they
    // are waited for before fallback() destroys any graph
    if (rc != CLRSDP_OK)
      for (int q = 0; q < behind; ++q) HIPCHK(hipEventSynchronize(ring_ev[(ring_head + q) % 2]));
    if (fallback(rc)) {
      // the bodies behind this one ran on the same (unchanged) state and failed alike:
      // re-enqueue this body and those behind it with the LU factorisations
      inflight = 0;
      const clrsdp_params prm = last_prm;
      for (int q = 0; q <= behind; ++q) {
        const int r2 = iterate_async(&prm);
        if (r2) return r2;
      }
      return iterate_wait(st, ran);
    }
    return rc;
  }

  int run_stage(int s, const clrsdp_params* prm, int pd_feas) override {
    if (!uploaded) { err = "constraints not uploaded"; return CLRSDP_E_STATE; }
    if (s == 0) {
      HIPCHK(hipMemsetAsync(info, 0, info_count * sizeof(int), stream));
      segs.clear();
    }
    stage(s, prm, pd_feas);
    flush_scalars();
    stat_fetch();
    return check_info();
  }

  void get_buffer(int buf, double* host, int64_t* count) override {
    const T* src = nullptr;
    int64_t n = 0;
    switch (buf) {
      case CLRSDP_BUF_X: src = X; n = nblk_el; break;
      case CLRSDP_BUF_Y: src = Y; n = nblk_el; break;
      case CLRSDP_BUF_XINV: src = Xinv; n = nblk_el; break;
      case CLRSDP_BUF_R: src = R; n = nblk_el; break;
      case CLRSDP_BUF_S: src = S; n = nS; break;
      case CLRSDP_BUF_AY: src = AY; n = nAY; break;
      case CLRSDP_BUF_Q: src = Q; n = n_y * n_y; break;
      case CLRSDP_BUF_P: src = res_from_copy ? Pres : P; n = nblk_el; break;
      case CLRSDP_BUF_PVEC: src = res_from_copy ? pres : pvec; n = n_y; break;
      case CLRSDP_BUF_DVEC: src = res_from_copy ? dres : dvec; n = nx; break;
      case CLRSDP_BUF_DX: src = dx; n = nx; break;
      case CLRSDP_BUF_DXMAT: src = dX; n = nblk_el; break;
      case CLRSDP_BUF_DY: src = dyv; n = n_y; break;
      case CLRSDP_BUF_DYMAT: src = dY; n = nblk_el; break;
      case CLRSDP_BUF_XVEC: src = x; n = nx; break;
      case CLRSDP_BUF_YVEC: src = y; n = n_y; break;
      case CLRSDP_BUF_SCALARS: src = sc; n = SC_COUNT; break;
      case CLRSDP_BUF_LXINV: src = LX; n = nblk_el; break;
      case CLRSDP_BUF_LQINV: src = Qf; n = n_y * n_y; break;
      case CLRSDP_BUF_QINV: src = Qinv; n = n_y * n_y; break;
      default: throw ClrsdpError{CLRSDP_E_ARG, "bad buffer id"};
    }
    if (count) *count = n;
    if (host) get(src, host, n, 0, n);
    if (host && buf == CLRSDP_BUF_S && s_lower) {  // (fp64 only) the full symmetric S_j
      for (int c = 0; c < nc(); ++c) {
        const int64_t D = Ds[oc[c]];
        double* Sc = host + c_Soff[c];
        for (int64_t j = 0; j < D; ++j)
          for (int64_t i = 0; i < j; ++i) Sc[i + j * D] = Sc[j + i * D];
      }
    }
  }

  // ---------------- the low-rank operators and block kernels on operands the caller gives
  // (clrsdp_apply_operator): raw limbs into the work buffers, the loop body's own methods with
  // its own descriptors and plans, raw limbs back.  Limbs are bit copies (a NaN keeps its payload).
  void put_raw(T* dst, const double* planes, int64_t n) {
    if (n <= 0) return;
    constexpr int Wd = Num<T>::W;
    std::vector<double> h((size_t)n * Wd);
    for (int q = 0; q < Wd; ++q)
      for (int64_t e = 0; e < n; ++e)
        std::memcpy(&h[(size_t)e * Wd + q], &planes[(size_t)q * n + e], sizeof(double));
    HIPCHK(hipMemcpyAsync(dst, h.data(), (size_t)n * sizeof(T), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  void get_raw(const T* src, double* planes, int64_t n) {
    if (n <= 0) return;
    constexpr int Wd = Num<T>::W;
    std::vector<double> h((size_t)n * Wd);
    HIPCHK(hipMemcpyAsync(h.data(), src, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int q = 0; q < Wd; ++q)
      for (int64_t e = 0; e < n; ++e)
        std::memcpy(&planes[(size_t)q * n + e], &h[(size_t)e * Wd + q], sizeof(double));
  }
  void apply_operator(int op, const clrsdp_operands* a, int32_t* route) override {
    static_assert(sizeof(T) == Num<T>::W * sizeof(double), "limb structs");
    if (!uploaded) throw ClrsdpError{CLRSDP_E_STATE, "apply_operator: constraints not uploaded"};
    if (inflight) throw ClrsdpError{CLRSDP_E_STATE, "apply_operator with loop bodies in flight"};
    auto need = [](const void* p, const char* what) {
      if (!p) throw ClrsdpError{CLRSDP_E_ARG, std::string("apply_operator: ") + what + " is NULL"};
    };
    need(route, "route");
    switch (op) {
      case CLRSDP_APPLY_RHS: {
        need(a->blocks, "blocks (Z)");
        need(a->tuples, "tuples (d)");
        need(a->tuples_out, "tuples_out (rhs)");
        put_raw(Z, a->blocks, nblk_el);
        put_raw(dvec, a->tuples, nx);
        put_raw(rhs, a->tuples_out, nx);
        trace_products_Z_();
        direction_rhs_();
        *route = c_trZ.on ? 0 : trivial_tuples ? 1 : 2;
        HIPCHK(hipGetLastError());
        get_raw(rhs, a->tuples_out, nx);
        break;
      }
      case CLRSDP_APPLY_WEIGHTED: {
        need(a->tuples, "tuples (a)");
        need(a->blocks, "blocks (the base)");
        need(a->blocks_out, "blocks_out");
        put_raw(dx, a->tuples, nx);
        put_raw(P, a->blocks, nblk_el);
        put_raw(dX, a->blocks_out, nblk_el);
        weighted_A(dx, p_wA_dX, dX, 1.0);
        *route = wa_fused ? 0 : 1;
        HIPCHK(hipGetLastError());
        get_raw(dX, a->blocks_out, nblk_el);
        break;
      }
      case CLRSDP_APPLY_SYM: {
        need(a->blocks, "blocks");
        need(a->blocks_out, "blocks_out");
        if (a->mode < 0 || a->mode > 2) throw ClrsdpError{CLRSDP_E_ARG, "apply_operator: SYM mode must be 0, 1 or 2"};
        const bool only_m = a->only_m != 0;
        put_raw(Z, a->blocks, nblk_el);
        T* out = Z;  // modes 0 and 1 run in place, as sym(dY, dY, 0) and weighted_A's mirror do
        if (a->mode == 2) {
          out = tA;
          put_raw(tA, a->blocks_out, nblk_el);
        }
        sym(out, Z, a->mode, only_m);
        *route = (!only_m && std::is_same<T, double>::value && a->mode == 0 && nb() && sym_pairs) ? 0 : 1;
        HIPCHK(hipGetLastError());
        get_raw(out, a->blocks_out, nblk_el);
        break;
      }
      case CLRSDP_APPLY_LIN: {
        need(a->blocks, "blocks");
        need(a->blocks_out, "blocks_out");
        if (a->mode == CLRSDP_LIN_COPY) {          // as LX = X before a factorisation
          put_raw(Z, a->blocks, nblk_el);
          put_raw(tA, a->blocks_out, nblk_el);
          blk_lin(tA, Z, 1.0, nullptr, 0.0);
          HIPCHK(hipGetLastError());
          get_raw(tA, a->blocks_out, nblk_el);
        } else if (a->mode == CLRSDP_LIN_SUB) {    // as P = P - C
          need(a->blocks2, "blocks2");
          put_raw(P, a->blocks, nblk_el);
          put_raw(tB, a->blocks2, nblk_el);
          blk_lin(P, P, 1.0, tB, -1.0);
          HIPCHK(hipGetLastError());
          get_raw(P, a->blocks_out, nblk_el);
        } else if (a->mode == CLRSDP_LIN_DIAG) {   // as R += mu I at multi-word
          need(a->scalar, "scalar");
          put_raw(R, a->blocks, nblk_el);
          put_raw(tmpsc, a->scalar, 1);
          blk_lin(R, R, 1.0, nullptr, 0.0, tmpsc, a->mult);
          HIPCHK(hipGetLastError());
          get_raw(R, a->blocks_out, nblk_el);
        } else {
          throw ClrsdpError{CLRSDP_E_ARG, "apply_operator: LIN mode must be CLRSDP_LIN_COPY, _SUB or _DIAG"};
        }
        *route = 0;
        break;
      }
      default:
        throw ClrsdpError{CLRSDP_E_ARG, "apply_operator: unknown op"};
    }
  }

  int64_t exchange_bytes() const override { return xcap * (int64_t)sizeof(T); }
  void set_exchange(clrsdp_exchange_fn fn, void* ctx, void* send, void* recv) override {
    if (comm) throw ClrsdpError{CLRSDP_E_STATE, "the handle exchanges over its own RCCL communicator"};
    xfn = fn;
    xctx = ctx;
    if (send && recv) {
      xsend = reinterpret_cast<T*>(send);
      xrecv = reinterpret_cast<T*>(recv);
    } else {
      xsend = xrecv = own_send;
    }
  }
  void comm_init(const uint8_t* id) override {
    if (comm) throw ClrsdpError{CLRSDP_E_STATE, "RCCL communicator already initialised"};
    if (inflight) throw ClrsdpError{CLRSDP_E_STATE, "loop bodies in flight"};
    ncclUniqueId uid;
    static_assert(sizeof(uid) == CLRSDP_COMM_ID_BYTES, "ncclUniqueId size");
    std::memcpy(&uid, id, sizeof(uid));
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamSynchronize(stream));
    if (world > 1 && !comm_recv) comm_recv = dmalloc<T>((size_t)world * xcap);
    ncclComm_t c = nullptr;
    RCCLCHK(rccl().comm_init_rank(&c, world, uid, rank));  // on failure the handle keeps no comm
    comm = c;
    xsend = own_send;
    xrecv = world > 1 ? comm_recv : own_send;
    // one eager all-gather of the full capacity: RCCL connects its channels on first use, which
    // must not happen inside a graph capture
    RCCLCHK(rccl().all_gather(xsend, xrecv, (size_t)(xcap * (int64_t)sizeof(T)), ncclUint8, comm,
                              stream));
    HIPCHK(hipStreamSynchronize(stream));
    // graphs captured before carry no all-gathers
    drop_graphs();
  }
  void set_stream(void* s) override { stream = s ? reinterpret_cast<hipStream_t>(s) : own_stream; }
  void* get_stream() const override { return (void*)stream; }
  void synchronize() override { HIPCHK(hipStreamSynchronize(stream)); }
};

// Stand-alone compute_step_length (MPMP.jl:1829-1898) of a block-diagonal pair (M, dM), fp64:
// the same kernels as STAGE_STEP (L^-1 on chip and two MFMA products for blocks <= 128, potrf +
// two triangular solves above), then lambda_min per block and alpha.
struct DevBuf {
  std::vector<void*> p;
  ~DevBuf() {
    for (void* q : p) (void)hipFree(q);
  }
  template <class X>
  X* alloc(size_t n) {
    X* q = dmalloc<X>(n);
    p.push_back(q);
    return q;
  }
};
// the stream a stand-alone entry launches on
struct StreamOwner {
  hipStream_t s = nullptr;
  StreamOwner() { HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~StreamOwner() { (void)hipStreamDestroy(s); }
};

// planes of an arena of `cnt` numbers <-> the interleaved limbs of T (bit copies: a NaN keeps
// its payload)
template <class T>
std::vector<double> interleave(const double* planes, int64_t cnt) {
  constexpr int W = Num<T>::W;
  std::vector<double> h((size_t)cnt * W);
  for (int q = 0; q < W; ++q)
    for (int64_t e = 0; e < cnt; ++e)
      std::memcpy(&h[(size_t)e * W + q], &planes[(size_t)q * cnt + e], sizeof(double));
  return h;
}
template <class T>
T* upload_planes(DevBuf& mem, const double* planes, int64_t cnt) {
  T* d = mem.alloc<T>((size_t)cnt);
  const std::vector<double> h = interleave<T>(planes, cnt);
  if (cnt) HIPCHK(hipMemcpy(d, h.data(), (size_t)cnt * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
template <class T>
void download_planes(const T* d, double* planes, int64_t cnt) {
  constexpr int W = Num<T>::W;
  std::vector<double> h((size_t)cnt * W);
  if (cnt) HIPCHK(hipMemcpy(h.data(), d, (size_t)cnt * sizeof(T), hipMemcpyDeviceToHost));
  for (int q = 0; q < W; ++q)
    for (int64_t e = 0; e < cnt; ++e)
      std::memcpy(&planes[(size_t)q * cnt + e], &h[(size_t)e * W + q], sizeof(double));
}

// lambda_min of each symmetric block at the word type T (the eigenvalue part of
// compute_step_length, MPMP.jl:1857-1870): planes in, planes out
template <class T>
void eigmin_words(int device, int64_t nblk, const int64_t* n, const double* Ap, double* ep,
                  int32_t* route = nullptr) {
  const Switches sw = Switches::read();
  DeviceGuard dg(device);
  std::vector<int64_t> off(nblk + 1, 0);
  for (int64_t b = 0; b < nblk; ++b) {
    if (n[b] <= 0 || n[b] > 4096) throw ClrsdpError{CLRSDP_E_ARG, "block size out of range"};
    off[b + 1] = off[b] + n[b] * n[b];
  }
  DevBuf mem;
  T* A = upload_planes<T>(mem, Ap, off[nblk]);
  T* eig = mem.alloc<T>(nblk);
  MatPlan<T> eg;
  for (int64_t b = 0; b < nblk; ++b) eg.add(A + off[b], (int)n[b], (int)n[b]);
  eg.finalize(sw, MatPlan<T>::Use::EIG_ONLY);
  StreamOwner so;
  eg.eigmin(so.s, eig);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(so.s));
  download_planes<T>(eig, ep, nblk);
  if (!route) return;
  // per block: 0 certified by the refinement, 1 flagged and computed by the fallback launch;
  // -1 for a batch whose kernel has no certification step
  const int ek = eg.eig_k;
  if ((ek != CLRSDP_EIG_K_MX && ek != CLRSDP_EIG_K_MXBLK) || !eg.redo) {
    for (int64_t b = 0; b < nblk; ++b) route[b] = -1;
    return;
  }
  static_assert(sizeof(int) == sizeof(int32_t), "the flags are 32-bit");
  HIPCHK(hipMemcpy(route, eg.redo, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost));
  if (ek == CLRSDP_EIG_K_MXBLK && sw.eigmx_stats) {
    std::vector<double> st((size_t)nblk * MXBLK_ST);
    HIPCHK(hipMemcpy(st.data(), eg.mx_st, st.size() * sizeof(double), hipMemcpyDeviceToHost));
    int flagged = 0, steps = 0;
    for (int64_t b = 0; b < nblk; ++b) {
      flagged += route[b] != 0;
      if (route[b] == 0) steps = std::max(steps, (int)st[(size_t)b * MXBLK_ST + 6]);
    }
    std::fprintf(stderr, "clrsdp: eigmin_mxblk: %d of %lld blocks flagged, most refinement steps of a certified block %d\n",
                 flagged, (long long)nblk, steps);
  }
}

// Pivoted LU of each block at the word type T through LuPlan, as the solver's LU path runs it
// (getrf_batched, or the blocked chain beyond its panel / with CLRSDP_LU_BLK=1): planes in and out
template <class T>
void getrf_words(int device, int64_t nblk, const int64_t* n, double* Ap, int32_t* perm, int32_t* info) {
  const Switches sw = Switches::read();
  std::vector<int64_t> off(nblk + 1, 0), poff(nblk + 1, 0);
  for (int64_t b = 0; b < nblk; ++b) {
    off[b + 1] = off[b] + n[b] * n[b];
    poff[b + 1] = poff[b] + n[b];
  }
  DeviceGuard dg(device);
  const int64_t tot = off[nblk], np = poff[nblk];
  DevBuf mem;
  T* A = upload_planes<T>(mem, Ap, tot);
  int* dperm = mem.alloc<int>(np);
  int* dinfo = mem.alloc<int>(nblk);
  LuPlan<T> lu;
  for (int64_t b = 0; b < nblk; ++b) lu.add(A + off[b], dperm + poff[b], (int)n[b], (int)n[b]);
  lu.finalize(sw);
  StreamOwner so;
  lu.launch(so.s, dinfo);
  HIPCHK(hipStreamSynchronize(so.s));
  static_assert(sizeof(int) == sizeof(int32_t), "perm and info are 32-bit");
  HIPCHK(hipMemcpy(perm, dperm, (size_t)np * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(info, dinfo, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost));
  download_planes<T>(A, Ap, tot);
}

// Cholesky factor of each block at the word type T, as the solver runs it: in place through
// MatPlan::potrf (inverse = 0), or L^-1 through CholInvPlan into a buffer of its own that holds
// NaN bytes before the launch, so every entry that comes back was written by the kernel
// (inverse = 1); planes in and out
template <class T>
void potrf_words(int device, int inverse, int64_t nblk, const int64_t* n, double* Ap, int32_t* info) {
  const Switches sw = Switches::read();
  std::vector<int64_t> off(nblk + 1, 0);
  for (int64_t b = 0; b < nblk; ++b) off[b + 1] = off[b] + n[b] * n[b];
  DeviceGuard dg(device);
  // potrf_batched's size bound (E_ARG) before any buffer is allocated or copied; fac.finalize()
  // below makes the same comparison again, on the cached figure
  if (!inverse) MatPlan<T>::check_potrf((int)*std::max_element(n, n + nblk), sw.potrf_blk);
  const int64_t tot = off[nblk];
  DevBuf mem;
  T* A = upload_planes<T>(mem, Ap, tot);
  T* X = inverse ? mem.alloc<T>(tot) : nullptr;
  int* dinfo = mem.alloc<int>(nblk);
  MatPlan<T> fac;
  CholInvPlan<T> ci;
  for (int64_t b = 0; b < nblk; ++b) {
    if (inverse) ci.add(A + off[b], (int)n[b], (int)n[b], X + off[b], (int)n[b]);
    else fac.add(A + off[b], (int)n[b], (int)n[b]);
  }
  fac.finalize(sw);
  ci.finalize(sw);
  StreamOwner so;
  if (inverse) {
    HIPCHK(hipMemsetAsync(X, 0xFF, (size_t)tot * sizeof(T), so.s));
    ci.launch(so.s, dinfo);
  } else {
    fac.potrf(so.s, dinfo);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(so.s));
  static_assert(sizeof(int) == sizeof(int32_t), "info is 32-bit");
  HIPCHK(hipMemcpy(info, dinfo, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost));
  download_planes<T>(inverse ? X : A, Ap, tot);
}

// L^-1 and (want[b]) A^-1 of fp64 blocks by one launch of CholInvPlan's SPDINV form; the output
// buffers go to the device as the caller filled them, so what the kernel leaves alone comes back
// unchanged
static void chol_spdinv_f64(int device, int64_t nblk, const int64_t* n, const int64_t* ld, const int32_t* want,
                     const double* Ap, double* Linv, double* Ainv, int32_t* info) {
  const Switches sw = Switches::read();
  std::vector<int64_t> off(nblk + 1, 0), ooff(nblk + 1, 0);
  for (int64_t b = 0; b < nblk; ++b) {
    off[b + 1] = off[b] + n[b] * n[b];
    ooff[b + 1] = ooff[b] + (ld ? ld[b] : n[b]) * n[b];
  }
  DeviceGuard dg(device);
  const int64_t tot = off[nblk], otot = ooff[nblk];
  DevBuf mem;
  double* A = mem.alloc<double>(tot);
  double* X = mem.alloc<double>(otot);
  double* G = Ainv ? mem.alloc<double>(otot) : nullptr;
  int* dinfo = mem.alloc<int>(nblk);
  HIPCHK(hipMemcpy(A, Ap, (size_t)tot * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(X, Linv, (size_t)otot * sizeof(double), hipMemcpyHostToDevice));
  if (G) HIPCHK(hipMemcpy(G, Ainv, (size_t)otot * sizeof(double), hipMemcpyHostToDevice));
  CholInvPlan<double> ci;
  bool any = false;
  for (int64_t b = 0; b < nblk; ++b) {
    const int pitch = (int)(ld ? ld[b] : n[b]);
    ci.add(A + off[b], (int)n[b], (int)n[b], X + ooff[b], pitch);
    if (want && want[b]) {
      ci.want_inverse(G + ooff[b], pitch);
      any = true;
    }
  }
  if (!any) ci.want_inverse(nullptr, 0);  // (a descriptor list of nulls: the same instance)
  ci.finalize(sw);
  StreamOwner so;
  ci.launch(so.s, dinfo, true);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(so.s));
  static_assert(sizeof(int) == sizeof(int32_t), "info is 32-bit");
  HIPCHK(hipMemcpy(info, dinfo, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(Linv, X, (size_t)otot * sizeof(double), hipMemcpyDeviceToHost));
  if (G) HIPCHK(hipMemcpy(Ainv, G, (size_t)otot * sizeof(double), hipMemcpyDeviceToHost));
}

// Triangular solves of each block at the word type T through TrsmPlan, as the solver runs them
// (trsv_wave / trsm_batched, or the blocked chain beyond the on-chip panel / with
// CLRSDP_TRSM_BLK=1): planes in, B planes in and out
template <class T>
void trsm_words(int device, int mode, int trans, int64_t nblk, const int64_t* n, const int64_t* nrhs,
                const double* Ap, double* Bp) {
  const Switches sw = Switches::read();
  std::vector<int64_t> off(nblk + 1, 0), boff(nblk + 1, 0);
  for (int64_t b = 0; b < nblk; ++b) {
    off[b + 1] = off[b] + n[b] * n[b];
    boff[b + 1] = boff[b] + n[b] * nrhs[b];
  }
  DeviceGuard dg(device);
  const int64_t tot = off[nblk], totb = boff[nblk];
  DevBuf mem;
  T* A = upload_planes<T>(mem, Ap, tot);
  T* B = upload_planes<T>(mem, Bp, totb);
  TrsmPlan<T> tp;
  tp.mode = mode;
  for (int64_t b = 0; b < nblk; ++b)
    tp.add(A + off[b], (int)n[b], B + boff[b], (int)n[b], (int)n[b], (int)nrhs[b]);
  tp.finalize(sw);
  StreamOwner so;
  tp.launch(so.s, trans != 0);
  HIPCHK(hipStreamSynchronize(so.s));
  download_planes<T>(B, Bp, totb);
}

// the arguments of clrsdp_gemm, checked by the caller (gemm_check)
struct GemmCall {
  int form, ta, tb;
  double alpha, beta;
  const double* dscal;
  double dmult;
  int64_t nprob;
  const clrsdp_gemm_problem* pr;
  const double *A, *B, *Cin, *sa, *sl;
  double* C;
  int64_t na, nb, nc, ncin, ns;
};

// One GemmPlan<T> from the records, built as build_plans() builds the solver's, launched once
template <class T>
int gemm_words(int device, const GemmCall& c) {
  const Switches sw = Switches::read();
  DeviceGuard dg(device);
  DevBuf mem;
  const T* A = upload_planes<T>(mem, c.A, c.na);
  const T* B = upload_planes<T>(mem, c.B, c.nb);
  T* C = upload_planes<T>(mem, c.C, c.nc);
  const T* Cin = c.Cin ? upload_planes<T>(mem, c.Cin, c.ncin) : nullptr;
  const T* sa = c.sa ? upload_planes<T>(mem, c.sa, c.ns) : nullptr;
  const T* sl = c.sl ? upload_planes<T>(mem, c.sl, c.ns) : nullptr;
  const T* ds = nullptr;
  if (c.dscal) {
    T* d1 = mem.alloc<T>(1);
    const T v = T(*c.dscal);
    HIPCHK(hipMemcpy(d1, &v, sizeof(T), hipMemcpyHostToDevice));
    ds = d1;
  }
  GemmPlan<T> g;
  g.ta = c.ta != 0;
  g.tb = c.tb != 0;
  g.sym = c.form == CLRSDP_GEMM_SYM;
  g.upper = c.form == CLRSDP_GEMM_UPPER;
  for (int64_t p = 0; p < c.nprob; ++p) {
    const clrsdp_gemm_problem& r = c.pr[p];
    const double be = c.form == CLRSDP_GEMM_MIXED ? r.beta : c.beta;
    const bool inplace = !Cin || r.offcin < 0;
    const T* ci = be == 0.0 && inplace ? nullptr : inplace ? C + r.offc : Cin + r.offcin;
    const int ldci = (int)(inplace ? r.ldc : r.ldcin);
    const int M = (int)r.M, N = (int)r.N, K = (int)r.K;
    if (c.form == CLRSDP_GEMM_SCALED) {
      g.add_scaled(A + r.offa, (int)r.lda, B + r.offb, (int)r.ldb, ci, ldci, C + r.offc, (int)r.ldc,
                   M, N, K, sa + r.offs, sl + r.offs);
    } else if (c.form == CLRSDP_GEMM_MIXED) {
      g.add_op(r.transa != 0, r.transb != 0, r.alpha, r.beta, A + r.offa, (int)r.lda, B + r.offb,
               (int)r.ldb, ci, ldci, C + r.offc, (int)r.ldc, M, N, K);
      if (r.diag) {  // + *dscal on the diagonal, as XINV's R = mu_p I - X Y
        g.h.back().flags |= 16;
        g.h.back().sa = ds;
      }
    } else {
      g.add(A + r.offa, (int)r.lda, B + r.offb, (int)r.ldb, ci, ldci, C + r.offc, (int)r.ldc, M, N, K);
    }
  }
  g.finalize(sw);
  StreamOwner so;
  g.launch(so.s, c.alpha, c.beta, c.form == CLRSDP_GEMM_MIXED ? nullptr : ds, c.dmult);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(so.s));
  download_planes<T>(C, c.C, c.nc);
  return g.path();
}

// the argument checks of clrsdp_gemm: an empty string, or what is wrong (no device call)
std::string gemm_check(int words, const GemmCall& c) {
  if (c.nprob <= 0 || c.nprob > 65536 || !c.pr || !c.A || !c.B || !c.C) return "null argument or no problems";
  if (words != 1 && words != 2 && words != 4) return "words must be 1, 2 or 4";
  if (c.form < CLRSDP_GEMM_PLAIN || c.form > CLRSDP_GEMM_MIXED) return "unknown form";
  const bool sym = c.form == CLRSDP_GEMM_SYM, upper = c.form == CLRSDP_GEMM_UPPER,
             sca = c.form == CLRSDP_GEMM_SCALED, mixed = c.form == CLRSDP_GEMM_MIXED;
  if ((sym || sca || mixed || c.dscal) && words != 1)
    return "SYM, SCALED, MIXED and the diagonal scalar are fp64 only";
  if (upper && words == 1) return "UPPER is multi-word only";
  if (sca && (c.ta || !c.tb)) return "scaled-A GEMM: fp64 A B^T only";
  if (sca && (!c.sa || !c.sl)) return "scaled-A GEMM: sa and sl required";
  if (sym && c.ta) return "symmetric GEMM epilogue: op(A) = A only";
  if (sym && (c.beta != 0.0 || c.dscal)) return "symmetric GEMM epilogue: beta = 0 only";
  if (c.na < 0 || c.nb < 0 || c.nc < 0 || (c.Cin && c.ncin < 0) || (sca && c.ns < 0)) return "negative arena length";
  constexpr int64_t LDMAX = 1 << 24;
  bool gemv = !mixed && !sca;
  std::vector<std::pair<int64_t, int64_t>> cs;
  // footprint of a column-major rows x cols matrix at `off` inside an arena of `len` numbers
  auto inside = [](int64_t off, int64_t rows, int64_t cols, int64_t ld, int64_t len) {
    return off >= 0 && off <= len && (cols - 1) * ld + rows <= len - off;
  };
  for (int64_t p = 0; p < c.nprob; ++p) {
    const clrsdp_gemm_problem& r = c.pr[p];
    if (r.M < 1 || r.M > 4096 || r.N < 1 || r.N > 4096) return "M and N must be 1 .. 4096";
    if (r.K < 1 || r.K > 4096) return "K must be 1 .. 4096 (block without vectors)";
    if ((sym || upper) && r.M != r.N) return "symmetric GEMM epilogue: square problems only";
    const bool ta = mixed ? r.transa != 0 : c.ta != 0, tb = mixed ? r.transb != 0 : c.tb != 0;
    const double be = mixed ? r.beta : c.beta;
    const int64_t ar = ta ? r.K : r.M, ac = ta ? r.M : r.K, br = tb ? r.N : r.K, bc = tb ? r.K : r.N;
    const bool separate = be != 0.0 && c.Cin && r.offcin >= 0;
    if (r.lda < ar || r.ldb < br || r.ldc < r.M || (separate && r.ldcin < r.M))
      return "leading dimension smaller than the stored row count";
    if (r.lda > LDMAX || r.ldb > LDMAX || r.ldc > LDMAX || (separate && r.ldcin > LDMAX))
      return "leading dimension above 2^24";
    if (mixed && r.diag && (r.M != r.N || !c.dscal)) return "diag: a square problem and dscal required";
    if (!inside(r.offa, ar, ac, r.lda, c.na) || !inside(r.offb, br, bc, r.ldb, c.nb) ||
        !inside(r.offc, r.M, r.N, r.ldc, c.nc) ||
        (separate && !inside(r.offcin, r.M, r.N, r.ldcin, c.ncin)) ||
        (sca && !inside(r.offs, r.K, 1, r.K, c.ns)))
      return "operand outside its arena";
    cs.emplace_back(r.offc, r.offc + (r.N - 1) * r.ldc + r.M);
    gemv = gemv && r.N == 1 && (!tb || r.K == 1);
  }
  std::sort(cs.begin(), cs.end());
  for (size_t q = 1; q < cs.size(); ++q)
    if (cs[q].first < cs[q - 1].second) return "the C regions of two problems overlap";
  if (gemv && c.dscal) return "diagonal scalar: not with a batch that takes the GEMV kernel";
  return "";
}

// the arguments of clrsdp_gemm_chain, checked by the caller
struct ChainCall {
  int form, n, nprob, halves, ncols;
  double a1, b1, c_agg, c_in;
  const double *A1, *B1, *C1, *A2, *DA, *DdA, *DB, *lam, *din;
  double *O, *dot_part, *rout;
};

int chain_run(int device, const ChainCall& c) {
  DeviceGuard dg(device);
  DevBuf mem;
  const int n = c.n, nb = c.nprob;
  const int64_t nn = (int64_t)n * n * nb;  // one pointer set
  auto up = [&](const double* h, int64_t cnt) { return h ? upload_planes<double>(mem, h, cnt) : (double*)nullptr; };
  ChainPlan ch;
  const bool trace = c.form == CLRSDP_CHAIN_TRACE, sym = c.form == CLRSDP_CHAIN_SYM;
  ch.init(n, nb, c.halves, sym, sym);
  double* O[2] = {nullptr, nullptr};
  double *rout = nullptr, *dotp = nullptr;
  const int64_t ndot = (int64_t)nb * cdiv(n, chain::NS), nx = (int64_t)nb * c.ncols;
  if (trace) {
    ch.trace = true;
    ch.set(0, up(c.A1, nn), up(c.B1, (int64_t)n * nx), nullptr, nullptr, nullptr);
    ch.u.ldb1 = n;
    ch.u.sB1 = (long long)n * c.ncols;
    ch.u.NC = c.ncols;
    ch.u.lam = up(c.lam, nx);
    ch.u.sLam = c.ncols;
    ch.u.din = up(c.din, nx);
    ch.u.rout = rout = up(c.rout, nx);
    ch.u.sX = c.ncols;
    ch.u.c_in = c.c_in;
    ch.u.c_agg = c.c_agg;
  } else {
    for (int hf = 0; hf < c.halves; ++hf) {  // each pointer set a device allocation of its own
      const int64_t o = hf * nn;
      O[hf] = up(c.O + o, nn);
      ch.set(hf, up(c.A1 + o, nn), up(c.B1 + o, nn), !sym && c.C1 ? up(c.C1 + o, nn) : nullptr,
             up(c.A2 + o, nn), O[hf]);
    }
    if (c.dot_part) {
      ch.u.DA[0] = up(c.DA, nn);
      ch.u.DdA[0] = up(c.DdA, nn);
      ch.u.DB[0] = up(c.DB, nn);
      ch.u.dot_part = dotp = up(c.dot_part, ndot);
    }
  }
  StreamOwner so;
  ch.launch(so.s, c.a1, c.b1);
  HIPCHK(hipStreamSynchronize(so.s));
  if (trace) download_planes<double>(rout, c.rout, nx);
  for (int hf = 0; hf < (trace ? 0 : c.halves); ++hf) download_planes<double>(O[hf], c.O + hf * nn, nn);
  if (dotp) download_planes<double>(dotp, c.dot_part, ndot);
  return CLRSDP_OK;
}

int step_length_f64(int device, int64_t nblk, const int64_t* n, const double* Mh, const double* dMh,
                    double gamma, double* alpha, double* min_eig, std::string& err) {
  const Switches sw = Switches::read();
  DeviceGuard dg(device);
  std::vector<int64_t> off(nblk + 1, 0);
  int nmax = 0;
  for (int64_t b = 0; b < nblk; ++b) {
    if (n[b] <= 0 || n[b] > 4096) throw ClrsdpError{CLRSDP_E_ARG, "block size out of range"};
    off[b + 1] = off[b] + n[b] * n[b];
    nmax = std::max(nmax, (int)n[b]);
  }
  const int64_t tot = off[nblk];
  DevBuf mem;
  double* M = mem.alloc<double>(tot);
  double* dM = mem.alloc<double>(tot);
  double* L = mem.alloc<double>(tot);
  double* t1 = mem.alloc<double>(tot);
  double* t2 = mem.alloc<double>(tot);
  double* eig = mem.alloc<double>(nblk);
  int* info = mem.alloc<int>(nblk);
  HIPCHK(hipMemcpy(M, Mh, tot * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dM, dMh, tot * sizeof(double), hipMemcpyHostToDevice));
  CholInvPlan<double> ci;
  GemmPlan<double> g1, g2;
  g2.tb = true;
  g2.sym = true;  // exactly symmetric L^-1 dM L^-T (eigmin_split reads only A(i, j))
  MatPlan<double> fac, eg;
  TrsmPlan<double> s1, s2;
  std::vector<BlkDesc> big;
  for (int64_t b = 0; b < nblk; ++b) {
    const int nb = (int)n[b];
    const int64_t o = off[b];
    if (nb <= 128) {
      ci.add(M + o, nb, nb, L + o, nb);                                    // L <- L_M^-1
      g1.add(L + o, nb, dM + o, nb, nullptr, nb, t1 + o, nb, nb, nb, nb);  // t1 = L^-1 dM
      g2.add(t1 + o, nb, L + o, nb, nullptr, nb, t2 + o, nb, nb, nb, nb);  // t2 = t1 L^-T
    } else {
      fac.add(L + o, nb, nb);          // L <- chol(M)
      s1.add(L + o, nb, t1 + o, nb, nb, nb);
      s2.add(L + o, nb, t2 + o, nb, nb, nb);
      big.push_back(BlkDesc{o, nb, 0});
    }
    eg.add(t2 + o, nb, nb);
  }
  ci.finalize(sw); g1.finalize(sw); g2.finalize(sw); fac.finalize(sw); eg.finalize(sw, MatPlan<double>::Use::EIG_ONLY);
  s1.finalize(sw); s2.finalize(sw);
  PlanBase bd_owner;
  BlkDesc* d_big = big.empty() ? nullptr : bd_owner.own(big);
  StreamOwner so;
  const hipStream_t s = so.s;
  ci.launch(s, info);
  g1.launch(s, 1.0, 0.0);
  g2.launch(s, 1.0, 0.0);
  if (!big.empty()) {
    for (size_t q = 0; q < big.size(); ++q) {
      const int64_t o = big[q].off, nn = (int64_t)big[q].n * big[q].n;
      HIPCHK(hipMemcpyAsync(L + o, M + o, nn * sizeof(double), hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(t1 + o, dM + o, nn * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    // the chol-inverse launch wrote info[0 .. #small); the potrf flags follow
    fac.potrf(s, info + ci.hin.size());
    s1.launch(s, false);                                             // t1 = L^-1 dM
    blk_sym2<double><<<dim3((unsigned)big.size(), 32), 128, 0, s>>>(d_big, t2, t1, 2);  // t2 = t1^T
    s2.launch(s, false);                                             // t2 = L^-1 dM^T L^-T
  }
  eg.eigmin(s, eig);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  std::vector<int> hinfo(nblk);
  std::vector<double> he(nblk);
  HIPCHK(hipMemcpy(hinfo.data(), info, nblk * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(he.data(), eig, nblk * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t b = 0; b < nblk; ++b)
    if (hinfo[b]) {
      err = "The step length could not be calculated correctly (M not positive definite).";
      return CLRSDP_E_STEP;
    }
  // the eigen kernels run in the (j,l) order of the plan: small blocks and large ones alike
  double mn = INFINITY;
  for (int64_t b = 0; b < nblk; ++b) {
    if (min_eig) min_eig[b] = he[b];
    mn = std::min(mn, he[b]);
  }
  *alpha = (mn > -gamma) ? 1.0 : -gamma / mn;  // MPMP.jl:1893-1897
  return CLRSDP_OK;
}

// ---- clrsdp_reduce / clrsdp_slab_sum / clrsdp_update_state: the launch helpers above on planes
template <class T>
T from_limbs(const double* l) {
  T v = T(l[0]);
  for (int i = 1; i < Num<T>::W; ++i) v += T(l[i]);
  return v;
}

// the kernel's own code of a public op for a kind, or -1 where the solver never issues the pair
int reduce_op_code(int kind, int op) {
  switch (kind) {
    case CLRSDP_RED_FLAT_FOLD:
    case CLRSDP_RED_FLAT_TREE:  // flat_reduce: 0 dot, 1 dot of sums, 2 max |a|
      return op == CLRSDP_OP_DOT ? 0 : op == CLRSDP_OP_DOTSUM ? 1 : op == CLRSDP_OP_MAXABS ? 2 : -1;
    case CLRSDP_RED_VEC:  // vec_reduce: 0 dot, 2 max |a| (3, the plain sum, is the tree's)
      return op == CLRSDP_OP_DOT ? 0 : op == CLRSDP_OP_MAXABS ? 2 : -1;
    case CLRSDP_RED_FOLD:  // FoldRed: 0 sum, 2 max, 3 min, 4 max |.|
      return op == CLRSDP_OP_SUM ? 0 : op == CLRSDP_OP_MAX ? 2 : op == CLRSDP_OP_MIN ? 3
             : op == CLRSDP_OP_MAXABS ? 4 : -1;
    case CLRSDP_RED_ORDERED:  // ordered_reduce: the solver takes minima with it (op 3)
      return op == CLRSDP_OP_MIN ? 3 : -1;
  }
  return -1;
}

struct ReduceCall {
  int kind, op;
  int64_t n, stride;
  const double *a, *b, *da, *db;
  int64_t nfold;
  const clrsdp_fold* folds;
  double *out, *part;
};

constexpr int64_t RED_MAX_N = 1LL << 28;

std::string reduce_check(int words, const ReduceCall& c) {
  if (words != 1 && words != 2 && words != 4) return "words must be 1, 2 or 4";
  if (c.kind < CLRSDP_RED_FLAT_FOLD || c.kind > CLRSDP_RED_ORDERED) return "unknown kind";
  if (!c.a || !c.out) return "null argument";
  if (c.n < 1 || c.n > RED_MAX_N) return "n out of range";
  if (c.kind == CLRSDP_RED_FOLD) {
    if (c.nfold < 1 || c.nfold > 12 || !c.folds) return "FOLD: 1 .. 12 folds";
    for (int64_t q = 0; q < c.nfold; ++q) {
      const clrsdp_fold& f = c.folds[q];
      if (reduce_op_code(c.kind, f.op) < 0) return "FOLD: op must be sum, max, min or max-abs";
      if (f.cnt < 1 || f.cnt > c.n || f.stride < 1 || f.stride > c.n || f.off < 0 || f.off >= c.n ||
          f.off + (f.cnt - 1) * f.stride >= c.n)
        return "FOLD: a fold does not lie inside the source";
    }
    if (c.part) return "part: FLAT kinds only";
    return "";
  }
  if (c.nfold != 0 || c.folds) return "folds: FOLD only";
  if (reduce_op_code(c.kind, c.op) < 0) return "the solver issues no such op with this kind";
  if (c.kind == CLRSDP_RED_ORDERED) {
    if (c.stride < 1 || c.stride > RED_MAX_N || (c.n - 1) * c.stride + 1 > RED_MAX_N)
      return "ORDERED: stride out of range";
    if (c.part) return "part: FLAT kinds only";
    return "";
  }
  if (c.stride != 1) return "stride: 1 with this kind";
  if (c.op != CLRSDP_OP_MAXABS && !c.b) return "null argument";
  if (c.op == CLRSDP_OP_DOTSUM && (!c.da || !c.db)) return "null argument";
  if (c.part && c.kind == CLRSDP_RED_VEC) return "part: FLAT kinds only";
  return "";
}

template <class T>
void reduce_words(int device, const ReduceCall& c) {
  DeviceGuard dg(device);
  DevBuf mem;
  const int code = c.kind == CLRSDP_RED_FOLD ? 0 : reduce_op_code(c.kind, c.op);
  const int64_t na = c.kind == CLRSDP_RED_ORDERED ? (c.n - 1) * c.stride + 1 : c.n;
  const int64_t nout = c.kind == CLRSDP_RED_FOLD ? c.nfold : 1;
  const bool flat = c.kind == CLRSDP_RED_FLAT_FOLD || c.kind == CLRSDP_RED_FLAT_TREE;
  const T* a = upload_planes<T>(mem, c.a, na);
  const T* b = c.b && (flat || c.kind == CLRSDP_RED_VEC) && c.op != CLRSDP_OP_MAXABS
                   ? upload_planes<T>(mem, c.b, c.n) : nullptr;
  const T* da = c.op == CLRSDP_OP_DOTSUM && flat ? upload_planes<T>(mem, c.da, c.n) : nullptr;
  const T* db = c.op == CLRSDP_OP_DOTSUM && flat ? upload_planes<T>(mem, c.db, c.n) : nullptr;
  T* out = upload_planes<T>(mem, c.out, nout);
  T* part = flat ? mem.alloc<T>(RED_G) : nullptr;
  if (flat && c.part) {
    const std::vector<double> h = interleave<T>(c.part, RED_G);
    HIPCHK(hipMemcpy(part, h.data(), RED_G * sizeof(T), hipMemcpyHostToDevice));
  }
  StreamOwner so;
  ScalarParams<T> p{};
  p.fold_all = 1;
  switch (c.kind) {
    case CLRSDP_RED_FLAT_FOLD:  // blk_dot at one rank
      launch_flat_reduce<T>(so.s, a, b, da, db, c.n, code, part);
      launch_folds<T>(so.s, out, p, {flat_fold<T>(part, code, 0)}, -1);
      break;
    case CLRSDP_RED_FLAT_TREE:  // local_blk_reduce
      launch_flat_reduce<T>(so.s, a, b, da, db, c.n, code, part);
      launch_vec_reduce_tree<T>(so.s, part, RED_G, code, out);
      break;
    case CLRSDP_RED_VEC:
      launch_vec_reduce<T>(so.s, a, b, c.n, code, out);
      break;
    case CLRSDP_RED_FOLD: {
      std::vector<FoldRed<T>> pend;
      for (int64_t q = 0; q < c.nfold; ++q) {
        const clrsdp_fold& f = c.folds[q];
        pend.push_back(FoldRed<T>{a + f.off, f.stride, (int)f.cnt, reduce_op_code(c.kind, f.op), (int)q, 0});
      }
      launch_folds<T>(so.s, out, p, pend, -1);
      break;
    }
    default:
      launch_ordered_reduce<T>(so.s, a, (int)c.n, c.stride, code, out);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(so.s));
  download_planes<T>(out, c.out, nout);
  if (flat && c.part) download_planes<T>(part, c.part, RED_G);
}

struct SlabCall {
  int64_t cnt, stride, n;
  const double *in, *base;
  double cbase, csum;
  const double* Q;
  int64_t ldq;
  double *out, *out2;
  int64_t nout, offout;
};

std::string slab_check(int words, const SlabCall& c) {
  if (words != 1 && words != 2 && words != 4) return "words must be 1, 2 or 4";
  if (!c.in || !c.out) return "null argument";
  if (c.cnt < 1 || c.cnt > 65536) return "cnt must be 1 .. 65536";
  if (c.n < 1 || c.n > RED_MAX_N) return "n out of range";
  if (c.stride < c.n || c.stride > RED_MAX_N || c.cnt * c.stride > RED_MAX_N) return "stride out of range";
  if (c.offout < 0 || c.nout > RED_MAX_N || c.offout + c.n > c.nout) return "the result does not lie inside out";
  if (c.Q) {
    if (words != 1) return "slab_qsolve: fp64 only";
    if (c.n > 128) return "slab_qsolve: n must be 1 .. 128";
    if (c.ldq < c.n || c.ldq > (1 << 24)) return "slab_qsolve: ldq out of range";
    if (c.out2) return "slab_qsolve: no second output";
  }
  return "";
}

template <class T>
void slab_words(int device, const SlabCall& c) {
  DeviceGuard dg(device);
  DevBuf mem;
  const T* in = upload_planes<T>(mem, c.in, c.cnt * c.stride);
  const T* base = c.base ? upload_planes<T>(mem, c.base, c.n) : nullptr;
  T* out = upload_planes<T>(mem, c.out, c.nout);
  T* out2 = c.out2 ? upload_planes<T>(mem, c.out2, c.nout) : nullptr;
  const double* Q = nullptr;
  if constexpr (std::is_same<T, double>::value)
    if (c.Q) Q = upload_planes<double>(mem, c.Q, c.ldq * c.n);
  StreamOwner so;
  if constexpr (std::is_same<T, double>::value) {
    if (Q)
      launch_slab_qsolve(so.s, in, (int)c.cnt, c.stride, (int)c.n, base, c.cbase, c.csum, Q,
                         (int)c.ldq, out + c.offout);
  }
  if (!Q)
    launch_slab_sum4<T>(so.s, in, (int)c.cnt, c.stride, c.n, out + c.offout, base, c.cbase, c.csum,
                        out2 ? out2 + c.offout : nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(so.s));
  download_planes<T>(out, c.out, c.nout);
  if (out2) download_planes<T>(out2, c.out2, c.nout);
}

struct UpdateCall {
  int64_t nel, nx, ny, ninfo, nblk;
  double *X, *Y, *x, *y;
  const double *dX, *dY, *dx, *c, *dy, *b;
  const int32_t* info;
  const double *alpha_p, *alpha_d, *eigX, *eigY, *gamma;
  int pd_feas;
  double *part, *step;
};

std::string update_check(int words, const UpdateCall& c) {
  if (words != 1 && words != 2 && words != 4) return "words must be 1, 2 or 4";
  if (c.nel < 1 || c.nel > RED_MAX_N) return "nel out of range";
  if (c.nx < 0 || c.nx > RED_MAX_N) return "nx out of range";
  if (c.ny < 1 || c.ny > RED_MAX_N) return "ny out of range";
  if (c.ninfo < 1 || c.ninfo > (1 << 24)) return "ninfo out of range";
  if (c.nblk < 0 || c.nblk > (1 << 24)) return "nblk out of range";
  if (!c.X || !c.dX || !c.Y || !c.dY || !c.y || !c.dy || !c.b || !c.info || !c.part) return "null argument";
  if (c.nx > 0 && (!c.x || !c.dx || !c.c)) return "null argument";
  if (c.nblk == 0) {
    if (!c.alpha_p || !c.alpha_d) return "the slot path needs alpha_p and alpha_d";
    if (c.eigX || c.eigY || c.gamma || c.step) return "the slot path takes no eigenvalues";
  } else {
    if (!c.eigX || !c.eigY || !c.gamma || !c.step) return "the fused path needs eigX, eigY, gamma and step";
    if (c.alpha_p || c.alpha_d) return "the fused path forms alpha itself";
    if (c.pd_feas != 0 && c.pd_feas != 1) return "pd_feas must be 0 or 1";
  }
  return "";
}

template <class T>
void update_words(int device, const UpdateCall& c) {
  DeviceGuard dg(device);
  DevBuf mem;
  T* X = upload_planes<T>(mem, c.X, c.nel);
  T* Y = upload_planes<T>(mem, c.Y, c.nel);
  const T* dX = upload_planes<T>(mem, c.dX, c.nel);
  const T* dY = upload_planes<T>(mem, c.dY, c.nel);
  T* x = upload_planes<T>(mem, c.x, c.nx);
  const T* dx = upload_planes<T>(mem, c.dx, c.nx);
  const T* cv = upload_planes<T>(mem, c.c, c.nx);
  T* y = upload_planes<T>(mem, c.y, c.ny);
  const T* dy = upload_planes<T>(mem, c.dy, c.ny);
  const T* bv = upload_planes<T>(mem, c.b, c.ny);
  static_assert(sizeof(int) == sizeof(int32_t), "status words are 32-bit");
  int* info = mem.alloc<int>((size_t)c.ninfo);
  HIPCHK(hipMemcpy(info, c.info, (size_t)c.ninfo * sizeof(int), hipMemcpyHostToDevice));
  T* part = upload_planes<T>(mem, c.part, 3 * RED_G);
  // the four slots of the fused path (mineig_X, mineig_Y, alpha_p, alpha_d), or the two alphas
  T* sc = c.nblk ? upload_planes<T>(mem, c.step, 4) : mem.alloc<T>(4);
  StepAlpha<T> sa{};
  const T *ap = sc + 2, *ad = sc + 3;
  if (c.nblk) {
    sa.eigX = upload_planes<T>(mem, c.eigX, c.nblk);
    sa.eigY = upload_planes<T>(mem, c.eigY, c.nblk);
    sa.nb = (int)c.nblk;
    sa.pd_feas = c.pd_feas;
    sa.gamma = from_limbs<T>(c.gamma);
    sa.sc = sc;
    sa.sx = 0;
    sa.sy = 1;
    sa.sap = 2;
    sa.sad = 3;
    sa.pdslot = 0;  // (read with pd_feas < 0 only)
  } else {
    ap = upload_planes<T>(mem, c.alpha_p, 1);
    ad = upload_planes<T>(mem, c.alpha_d, 1);
  }
  StreamOwner so;
  launch_update_state<T>(so.s, X, dX, Y, dY, c.nel, x, dx, c.nx, cv, y, dy, c.ny, bv, ap, ad, info,
                         (int)c.ninfo, part, sa);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(so.s));
  download_planes<T>(X, c.X, c.nel);
  download_planes<T>(Y, c.Y, c.nel);
  download_planes<T>(x, c.x, c.nx);
  download_planes<T>(y, c.y, c.ny);
  download_planes<T>(part, c.part, 3 * RED_G);
  if (c.nblk) download_planes<T>(sc, c.step, 4);
}

struct ClSolveCall {
  int64_t ncl;
  const int64_t* D;
  int64_t ny;
  const double *Linv, *W, *rhs, *dy;
  double *t, *slabs, *dx;
};

std::string cl_solve_check(const ClSolveCall& c) {
  if (!c.D || !c.Linv || !c.W || !c.rhs || !c.dy || !c.t || !c.slabs || !c.dx) return "null argument";
  if (c.ncl < 1 || c.ncl > 4096) return "ncl must be 1 .. 4096";
  if (c.ny < 1) return "ny must be at least 1";
  int64_t mx = 0;
  for (int64_t q = 0; q < c.ncl; ++q) {
    if (c.D[q] < 1 || c.D[q] > 256) return "every D must be 1 .. 256";
    mx = std::max(mx, c.D[q]);
  }
  if (!cl_solve_ok(c.ncl, (int)cdiv(mx, 64), (int)mx, c.ny))
    return "ny too large for the slab sum behind the cluster solve";
  return "";
}

void cl_solve_run(int device, const ClSolveCall& c) {
  DeviceGuard dg(device);
  DevBuf mem;
  int64_t nS = 0, nW = 0, nX = 0, mx = 0;
  for (int64_t q = 0; q < c.ncl; ++q) {
    nS += c.D[q] * c.D[q];
    nW += c.D[q] * c.ny;
    nX += c.D[q];
    mx = std::max(mx, c.D[q]);
  }
  const int nrb = (int)cdiv(mx, 64);
  const int64_t nslab = c.ncl * nrb * c.ny;
  const double* L = upload_planes<double>(mem, c.Linv, nS);
  const double* W = upload_planes<double>(mem, c.W, nW);
  const double* rhs = upload_planes<double>(mem, c.rhs, nX);
  const double* dy = upload_planes<double>(mem, c.dy, c.ny);
  double* t = upload_planes<double>(mem, c.t, nX);
  double* slabs = upload_planes<double>(mem, c.slabs, nslab);
  double* dx = upload_planes<double>(mem, c.dx, nX);
  std::vector<ClSolveDesc> h((size_t)c.ncl);
  int64_t so = 0, wo = 0, xo = 0;
  for (int64_t q = 0; q < c.ncl; ++q) {
    const int64_t D = c.D[q];
    ClSolveDesc cs{};
    cs.L = L + so; cs.W = W + wo; cs.rhs = rhs + xo; cs.t = t + xo; cs.dx = dx + xo; cs.D = (int)D;
    h[(size_t)q] = cs;
    so += D * D; wo += D * c.ny; xo += D;
  }
  ClSolveDesc* ds = mem.alloc<ClSolveDesc>((size_t)c.ncl);
  HIPCHK(hipMemcpy(ds, h.data(), h.size() * sizeof(ClSolveDesc), hipMemcpyHostToDevice));
  StreamOwner so_;
  launch_cl_solve_t(so_.s, ds, (int)c.ncl, nrb, (int)c.ny, slabs);
  launch_cl_solve_dx(so_.s, ds, (int)c.ncl, nrb, (int)c.ny, dy);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(so_.s));
  download_planes<double>(t, c.t, nX);
  download_planes<double>(slabs, c.slabs, nslab);
  download_planes<double>(dx, c.dx, nX);
}

}  // namespace

struct clrsdp_handle {
  std::unique_ptr<HandleBase> impl;
};

#define GUARD(h, body)                                          \
  try {                                                         \
    DeviceGuard dg_(guard_dev(h));                              \
    body                                                        \
  } catch (const ClrsdpError& e) {                              \
    g_last_error = e.msg;                                       \
    if (h) (h)->impl->err = e.msg;                              \
    return e.code;                                              \
  } catch (const std::exception& e) {                           \
    g_last_error = e.what();                                    \
    if (h) (h)->impl->err = e.what();                           \
    return CLRSDP_E_HIP;                                        \
  }

static int guard_dev(const clrsdp_handle* h) {
  if (h) return h->impl->dev;
  int d = 0;
  (void)hipGetDevice(&d);
  return d;
}

// clrsdp_handoff_state: refusals first (nothing is touched before the last of them)
static void handoff_state(clrsdp_handle* dst, clrsdp_handle* src) {
  if (dst == src) throw ClrsdpError{CLRSDP_E_ARG, "handoff_state: source and destination are the same handle"};
  const StateView s = src->impl->state_view();
  const StateView d = dst->impl->state_view();
  if (s.dev != d.dev) throw ClrsdpError{CLRSDP_E_ARG, "handoff_state: the handles are on different devices"};
  if (s.sig != d.sig || s.nx != d.nx || s.nblk_el != d.nblk_el || s.n_y != d.n_y)
    throw ClrsdpError{CLRSDP_E_ARG, "handoff_state: the handles differ in their description, rank, "
                                    "world size or owned clusters"};
  if (s.inflight || d.inflight) throw ClrsdpError{CLRSDP_E_STATE, "handoff_state with loop bodies in flight"};
  if (!s.has_state) throw ClrsdpError{CLRSDP_E_STATE, "handoff_state: the source handle has no state yet"};
  const int si = width_index(s.words);
  const int di = width_index(d.words);
  if (si < 0 || di < 0) throw ClrsdpError{CLRSDP_E_ARG, "handoff_state: unknown word width"};
  // after the source's stream work, on the destination's stream; adopt_state waits for it, so
  // the source may be destroyed once this returns
  HIPCHK(hipStreamSynchronize(s.stream));
  state_convert_fn[si][di](d.stream, s, d);
  HIPCHK(hipGetLastError());
  dst->impl->adopt_state();
}

extern "C" {

int32_t clrsdp_version(void) { return 100; }

const char* clrsdp_last_error(const clrsdp_handle* h) {
  if (h && !h->impl->err.empty()) return h->impl->err.c_str();
  return g_last_error.c_str();
}

int32_t clrsdp_create(const clrsdp_desc* desc, const clrsdp_config* cfg, clrsdp_handle** out) {
  clrsdp_handle* h = nullptr;
  if (!desc || !cfg || !out) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, {
    DeviceGuard dg(cfg->device);
    auto* hh = new clrsdp_handle();
    if (cfg->precision_words == 1) hh->impl.reset(new Solver<double>(desc, cfg));
    else if (cfg->precision_words == 2) hh->impl.reset(new Solver<dd>(desc, cfg));
    else if (cfg->precision_words == 4) hh->impl.reset(new Solver<qd>(desc, cfg));
    else { delete hh; g_last_error = "precision_words must be 1, 2 or 4"; return CLRSDP_E_ARG; }
    *out = hh;
    return CLRSDP_OK;
  })
}

int32_t clrsdp_upload_constraints(clrsdp_handle* h, const double* V, const double* lambda,
                                  const double* B, const double* c, const double* b,
                                  const double* C) {
  if (!h || !V || !lambda || !B || !c || !b) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->upload(V, lambda, B, c, b, C); return CLRSDP_OK; })
}

int32_t clrsdp_set_state(clrsdp_handle* h, const double* x, const double* X, const double* y,
                         const double* Y) {
  if (!h || !x || !X || !y || !Y) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->set_state(x, X, y, Y); return CLRSDP_OK; })
}

int32_t clrsdp_get_state(clrsdp_handle* h, double* x, double* X, double* y, double* Y) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->get_state(x, X, y, Y); return CLRSDP_OK; })
}

int32_t clrsdp_initial_residuals(clrsdp_handle* h, const clrsdp_params* prm, clrsdp_iter_stats* st) {
  if (!h || !prm || !st) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, { return h->impl->initial(prm, st); })
}

int32_t clrsdp_iterate(clrsdp_handle* h, const clrsdp_params* prm, int32_t pd_feas,
                       clrsdp_iter_stats* st) {
  if (!h || !prm || !st) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  if (pd_feas != 0 && pd_feas != 1) { g_last_error = "pd_feas must be 0 or 1"; return CLRSDP_E_ARG; }
  GUARD(h, { return h->impl->iterate(prm, pd_feas, st); })
}

int32_t clrsdp_set_control(clrsdp_handle* h, const clrsdp_control* ctl) {
  if (!h || !ctl) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->set_control(ctl); return CLRSDP_OK; })
}

int32_t clrsdp_iterate_async(clrsdp_handle* h, const clrsdp_params* prm) {
  if (!h || !prm) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, { return h->impl->iterate_async(prm); })
}

int32_t clrsdp_iterate_wait(clrsdp_handle* h, clrsdp_iter_stats* st, int32_t* ran) {
  if (!h || !st) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, {
    int r = 0;
    const int rc = h->impl->iterate_wait(st, &r);
    if (ran) *ran = r;
    return rc;
  })
}

int32_t clrsdp_run_stage(clrsdp_handle* h, int32_t stage, const clrsdp_params* prm, int32_t pd_feas) {
  if (!h || !prm) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, { return h->impl->run_stage(stage, prm, pd_feas); })
}

int32_t clrsdp_get_buffer(clrsdp_handle* h, int32_t buf, double* host, int64_t* count) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->get_buffer(buf, host, count); return CLRSDP_OK; })
}

int32_t clrsdp_exchange_bytes(const clrsdp_handle* h, int64_t* bytes) {
  if (!h || !bytes) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  *bytes = h->impl->exchange_bytes();
  return CLRSDP_OK;
}

int32_t clrsdp_set_exchange(clrsdp_handle* h, clrsdp_exchange_fn fn, void* ctx, void* send_dev,
                            void* recv_dev) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->set_exchange(fn, ctx, send_dev, recv_dev); return CLRSDP_OK; })
}

int32_t clrsdp_comm_unique_id(uint8_t* id) {
  if (!id) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  try {
    ncclUniqueId uid;
    RCCLCHK(rccl().get_unique_id(&uid));
    std::memcpy(id, &uid, sizeof(uid));
    return CLRSDP_OK;
  } catch (const ClrsdpError& e) {
    g_last_error = e.msg;
    return e.code;
  }
}

int32_t clrsdp_comm_init(clrsdp_handle* h, const uint8_t* id) {
  if (!h || !id) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->comm_init(id); return CLRSDP_OK; })
}

int32_t clrsdp_set_stream(clrsdp_handle* h, void* stream) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->set_stream(stream); return CLRSDP_OK; })
}

void* clrsdp_get_stream(const clrsdp_handle* h) { return h ? h->impl->get_stream() : nullptr; }

int32_t clrsdp_synchronize(clrsdp_handle* h) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->synchronize(); return CLRSDP_OK; })
}

int32_t clrsdp_save_state(clrsdp_handle* h) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->save_state(); return CLRSDP_OK; })
}

int32_t clrsdp_restore_state(clrsdp_handle* h) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->restore_state(); return CLRSDP_OK; })
}

int32_t clrsdp_handoff_state(clrsdp_handle* dst, clrsdp_handle* src) {
  if (!dst || !src) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(dst, { handoff_state(dst, src); return CLRSDP_OK; })
}

int32_t clrsdp_step_length(int32_t device, int64_t nblocks, const int64_t* n, const double* M,
                           const double* dM, double gamma, double* alpha, double* min_eig) {
  if (nblocks <= 0 || !n || !M || !dM || !alpha) { g_last_error = "null argument or no blocks"; return CLRSDP_E_ARG; }
  try {
    std::string err;
    const int rc = step_length_f64(device, nblocks, n, M, dM, gamma, alpha, min_eig, err);
    if (rc) g_last_error = err;
    return rc;
  } catch (const ClrsdpError& e) {
    g_last_error = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return CLRSDP_E_HIP;
  }
}

int32_t clrsdp_eigmin_kernel(int32_t words, int64_t nmax, int32_t* kernel) {
  if (!kernel || nmax <= 0 || nmax > 4096) { g_last_error = "null argument or nmax outside 1 .. 4096"; return CLRSDP_E_ARG; }
  const Switches sw = Switches::read();
  if (words == 1) *kernel = MatPlan<double>::eig_dispatch((int)nmax, sw.eig_blk, sw.mxblk(), sw.eig_mx);
  else if (words == 2) *kernel = MatPlan<mw::dd>::eig_dispatch((int)nmax, sw.eig_blk, sw.mxblk(), sw.eig_mx);
  else if (words == 4) *kernel = MatPlan<mw::qd>::eig_dispatch((int)nmax, sw.eig_blk, sw.mxblk(), sw.eig_mx);
  else { g_last_error = "words must be 1, 2 or 4"; return CLRSDP_E_ARG; }
  return CLRSDP_OK;
}

// fn<word type>(...) for `words` (checked by the caller: 1, 2 or 4), errors into the return code
#define WORDS_CALL(fn, ...)                                   \
  try {                                                       \
    if (words == 1) fn<double>(__VA_ARGS__);                  \
    else if (words == 2) fn<mw::dd>(__VA_ARGS__);             \
    else fn<mw::qd>(__VA_ARGS__);                             \
    return CLRSDP_OK;                                         \
  } catch (const ClrsdpError& e) {                            \
    g_last_error = e.msg;                                     \
    return e.code;                                            \
  } catch (const std::exception& e) {                         \
    g_last_error = e.what();                                  \
    return CLRSDP_E_HIP;                                      \
  }

int32_t clrsdp_eigmin(int32_t device, int32_t words, int64_t nblocks, const int64_t* n,
                      const double* A, double* min_eig) {
  if (nblocks <= 0 || !n || !A || !min_eig) { g_last_error = "null argument or no blocks"; return CLRSDP_E_ARG; }
  if (words != 1 && words != 2 && words != 4) { g_last_error = "words must be 1, 2 or 4"; return CLRSDP_E_ARG; }
  WORDS_CALL(eigmin_words, device, nblocks, n, A, min_eig)
}

int32_t clrsdp_eigmin_routes(int32_t device, int32_t words, int64_t nblocks, const int64_t* n,
                             const double* A, double* min_eig, int32_t* route) {
  if (nblocks <= 0 || !n || !A || !min_eig || !route) { g_last_error = "null argument or no blocks"; return CLRSDP_E_ARG; }
  if (words != 1 && words != 2 && words != 4) { g_last_error = "words must be 1, 2 or 4"; return CLRSDP_E_ARG; }
  WORDS_CALL(eigmin_words, device, nblocks, n, A, min_eig, route)
}

int32_t clrsdp_getrf(int32_t device, int32_t words, int64_t nblocks, const int64_t* n, double* A,
                     int32_t* perm, int32_t* info) {
  if (nblocks <= 0 || !n || !A || !perm || !info) { g_last_error = "null argument or no blocks"; return CLRSDP_E_ARG; }
  if (words != 1 && words != 2 && words != 4) { g_last_error = "words must be 1, 2 or 4"; return CLRSDP_E_ARG; }
  for (int64_t b = 0; b < nblocks; ++b)
    if (n[b] <= 0 || n[b] > 4096) { g_last_error = "block size out of range"; return CLRSDP_E_ARG; }
  WORDS_CALL(getrf_words, device, nblocks, n, A, perm, info)
}

int32_t clrsdp_potrf(int32_t device, int32_t words, int32_t inverse, int64_t nblocks,
                     const int64_t* n, double* A, int32_t* info) {
  if (nblocks <= 0 || !n || !A || !info) { g_last_error = "null argument or no blocks"; return CLRSDP_E_ARG; }
  if (words != 1 && words != 2 && words != 4) { g_last_error = "words must be 1, 2 or 4"; return CLRSDP_E_ARG; }
  if (inverse != 0 && inverse != 1) { g_last_error = "inverse must be 0 or 1"; return CLRSDP_E_ARG; }
  const int64_t inv_max = words == 1 ? 256 : 64;  // chol_inv_tiles / chol_lookahead with L^-1
  for (int64_t b = 0; b < nblocks; ++b) {
    if (n[b] <= 0 || n[b] > 4096) { g_last_error = "block size out of range"; return CLRSDP_E_ARG; }
    if (inverse && n[b] > inv_max) {
      g_last_error = words == 1 ? "L^-1 on chip (chol_inv_tiles): n <= 256 only"
                                : "L^-1 on chip (chol_lookahead with the inverse): n <= 64 only";
      return CLRSDP_E_ARG;
    }
  }
  WORDS_CALL(potrf_words, device, inverse, nblocks, n, A, info)
}

int32_t clrsdp_potrf_kernel(int32_t words, int64_t nmax, int32_t* kernel) {
  if (!kernel || nmax <= 0 || nmax > 4096) { g_last_error = "null argument or nmax outside 1 .. 4096"; return CLRSDP_E_ARG; }
  const int potrf_blk = Switches::read().potrf_blk;
  if (words == 1) *kernel = MatPlan<double>::potrf_dispatch((int)nmax, potrf_blk);
  else if (words == 2) *kernel = MatPlan<mw::dd>::potrf_dispatch((int)nmax, potrf_blk);
  else if (words == 4) *kernel = MatPlan<mw::qd>::potrf_dispatch((int)nmax, potrf_blk);
  else { g_last_error = "words must be 1, 2 or 4"; return CLRSDP_E_ARG; }
  return CLRSDP_OK;
}

int32_t clrsdp_chol_spdinv(int32_t device, int64_t nblocks, const int64_t* n, const int64_t* ld,
                           const int32_t* want, const double* A, double* Linv, double* Ainv,
                           int32_t* info) {
  if (nblocks <= 0 || !n || !A || !Linv || !info) { g_last_error = "null argument or no blocks"; return CLRSDP_E_ARG; }
  for (int64_t b = 0; b < nblocks; ++b) {
    if (n[b] <= 0 || n[b] > 128) { g_last_error = "A^-1 on chip (chol_inv_tiles): 1 <= n <= 128 only"; return CLRSDP_E_ARG; }
    if (ld && (ld[b] < n[b] || ld[b] > 4096)) { g_last_error = "pitch out of range"; return CLRSDP_E_ARG; }
    if (want && want[b] && !Ainv) { g_last_error = "A^-1 asked for without a buffer"; return CLRSDP_E_ARG; }
  }
  try {
    chol_spdinv_f64(device, nblocks, n, ld, want, A, Linv, Ainv, info);
    return CLRSDP_OK;
  } catch (const ClrsdpError& e) {
    g_last_error = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return CLRSDP_E_HIP;
  }
}

int32_t clrsdp_spdinv_kernel(int32_t words, int64_t nmax, int32_t lu, int32_t* fused) {
  if (!fused || nmax <= 0 || nmax > 4096) { g_last_error = "null argument or nmax outside 1 .. 4096"; return CLRSDP_E_ARG; }
  const bool sw = Switches::read().chol_spdinv;
  if (words == 1) *fused = CholInvPlan<double>::spdinv_dispatch((int)nmax, lu != 0, sw);
  else if (words == 2) *fused = CholInvPlan<mw::dd>::spdinv_dispatch((int)nmax, lu != 0, sw);
  else if (words == 4) *fused = CholInvPlan<mw::qd>::spdinv_dispatch((int)nmax, lu != 0, sw);
  else { g_last_error = "words must be 1, 2 or 4"; return CLRSDP_E_ARG; }
  return CLRSDP_OK;
}

int32_t clrsdp_trsm(int32_t device, int32_t words, int32_t mode, int32_t trans, int64_t nblocks,
                    const int64_t* n, const int64_t* nrhs, const double* A, double* B) {
  if (nblocks <= 0 || !n || !nrhs || !A || !B) { g_last_error = "null argument or no blocks"; return CLRSDP_E_ARG; }
  if (words != 1 && words != 2 && words != 4) { g_last_error = "words must be 1, 2 or 4"; return CLRSDP_E_ARG; }
  if (mode < 0 || mode > 2) { g_last_error = "mode must be 0, 1 or 2"; return CLRSDP_E_ARG; }
  for (int64_t b = 0; b < nblocks; ++b) {
    if (n[b] <= 0 || n[b] > 4096) { g_last_error = "block size out of range"; return CLRSDP_E_ARG; }
    if (nrhs[b] <= 0 || nrhs[b] > 4096) { g_last_error = "number of right-hand sides out of range"; return CLRSDP_E_ARG; }
  }
  WORDS_CALL(trsm_words, device, mode, trans, nblocks, n, nrhs, A, B)
}

int32_t clrsdp_gemm(int32_t device, int32_t words, int32_t form, int32_t transa, int32_t transb,
                    double alpha, double beta, const double* dscal, double dmult, int64_t nprob,
                    const clrsdp_gemm_problem* prob, const double* A, int64_t na, const double* B,
                    int64_t nb, double* C, int64_t nc, const double* Cin, int64_t ncin,
                    const double* sa, const double* sl, int64_t ns, int32_t* path) {
  const GemmCall c{form, transa, transb, alpha, beta, dscal, dmult, nprob, prob, A, B, Cin,
                   form == CLRSDP_GEMM_SCALED ? sa : nullptr, form == CLRSDP_GEMM_SCALED ? sl : nullptr,
                   C, na, nb, nc, ncin, ns};
  const std::string bad = gemm_check(words, c);
  if (!bad.empty()) { g_last_error = bad; return CLRSDP_E_ARG; }
  try {
    const int pth = words == 1 ? gemm_words<double>(device, c)
                    : words == 2 ? gemm_words<mw::dd>(device, c) : gemm_words<mw::qd>(device, c);
    if (path) *path = pth;
    return CLRSDP_OK;
  } catch (const ClrsdpError& e) {
    g_last_error = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return CLRSDP_E_HIP;
  }
}

int32_t clrsdp_gemm_chain(int32_t device, int32_t form, int64_t n, int64_t nprob, int32_t halves,
                          int64_t ncols, double a1, double b1, const double* A1, const double* B1,
                          const double* C1, const double* A2, double* O, const double* DA,
                          const double* DdA, const double* DB, double* dot_part, const double* lam,
                          const double* din, double c_agg, double c_in, double* rout) {
  if (form < CLRSDP_CHAIN || form > CLRSDP_CHAIN_TRACE) { g_last_error = "unknown form"; return CLRSDP_E_ARG; }
  if (n < 1 || n > 128) { g_last_error = "chain_f64: n must be 1 .. 128"; return CLRSDP_E_ARG; }
  if (nprob < 1 || nprob > 4096) { g_last_error = "chain_f64: nprob must be 1 .. 4096"; return CLRSDP_E_ARG; }
  if (halves != 1 && !(halves == 2 && form == CLRSDP_CHAIN_SYM)) {
    g_last_error = "chain_f64: halves must be 1 (2: CHAIN_SYM only)";
    return CLRSDP_E_ARG;
  }
  if (!A1 || !B1) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  if (form == CLRSDP_CHAIN_TRACE) {
    if (ncols < 1 || ncols > 4096) { g_last_error = "chain_f64: ncols must be 1 .. 4096"; return CLRSDP_E_ARG; }
    if (!lam || !rout) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  } else {
    if (!A2 || !O) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
    if (form == CLRSDP_CHAIN_SYM && dot_part) { g_last_error = "chain_f64: no dot epilogue with CHAIN_SYM"; return CLRSDP_E_ARG; }
    if (dot_part && (!DA || !DdA || !DB)) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  }
  const ChainCall c{form, (int)n, (int)nprob, halves, (int)ncols, a1, b1, c_agg, c_in, A1, B1, C1, A2,
                    DA, DdA, DB, lam, din, O, form == CLRSDP_CHAIN ? dot_part : nullptr, rout};
  try {
    return chain_run(device, c);
  } catch (const ClrsdpError& e) {
    g_last_error = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return CLRSDP_E_HIP;
  }
}

int32_t clrsdp_reduce(int32_t device, int32_t words, int32_t kind, int32_t op, int64_t n,
                      int64_t stride, const double* a, const double* b, const double* da,
                      const double* db, int64_t nfold, const clrsdp_fold* folds, double* out,
                      double* part) {
  const ReduceCall c{kind, op, n, stride, a, b, da, db, nfold, folds, out, part};
  const std::string bad = reduce_check(words, c);
  if (!bad.empty()) { g_last_error = bad; return CLRSDP_E_ARG; }
  WORDS_CALL(reduce_words, device, c)
}

int32_t clrsdp_slab_sum(int32_t device, int32_t words, int64_t cnt, int64_t stride, int64_t n,
                        const double* in, const double* base, double cbase, double csum,
                        const double* Q, int64_t ldq, double* out, double* out2, int64_t nout,
                        int64_t offout) {
  const SlabCall c{cnt, stride, n, in, base, cbase, csum, Q, ldq, out, out2, nout, offout};
  const std::string bad = slab_check(words, c);
  if (!bad.empty()) { g_last_error = bad; return CLRSDP_E_ARG; }
  WORDS_CALL(slab_words, device, c)
}

int32_t clrsdp_update_state(int32_t device, int32_t words, int64_t nel, double* X, const double* dX,
                            double* Y, const double* dY, int64_t nx, double* x, const double* dx,
                            const double* c, int64_t ny, double* y, const double* dy,
                            const double* b, int64_t ninfo, const int32_t* info,
                            const double* alpha_p, const double* alpha_d, int64_t nblk,
                            const double* eigX, const double* eigY, const double* gamma,
                            int32_t pd_feas, double* part, double* step) {
  const UpdateCall u{nel, nx, ny, ninfo, nblk, X, Y, x, y, dX, dY, dx, c, dy, b, info,
                     alpha_p, alpha_d, eigX, eigY, gamma, pd_feas, part, step};
  const std::string bad = update_check(words, u);
  if (!bad.empty()) { g_last_error = bad; return CLRSDP_E_ARG; }
  WORDS_CALL(update_words, device, u)
}

int32_t clrsdp_apply_operator(clrsdp_handle* h, int32_t op, const clrsdp_operands* a,
                              int32_t* route) {
  if (!h || !a || !route) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->apply_operator(op, a, route); return CLRSDP_OK; })
}

int32_t clrsdp_cl_solve(int32_t device, int64_t ncl, const int64_t* D, int64_t ny,
                        const double* Linv, const double* W, const double* rhs, const double* dy,
                        double* t, double* slabs, double* dx) {
  const ClSolveCall c{ncl, D, ny, Linv, W, rhs, dy, t, slabs, dx};
  const std::string bad = cl_solve_check(c);
  if (!bad.empty()) { g_last_error = bad; return CLRSDP_E_ARG; }
  try {
    cl_solve_run(device, c);
    return CLRSDP_OK;
  } catch (const ClrsdpError& e) {
    g_last_error = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return CLRSDP_E_HIP;
  }
}

int32_t clrsdp_set_timing(clrsdp_handle* h, int32_t on) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->set_timing(on); return CLRSDP_OK; })
}

int32_t clrsdp_set_graph(clrsdp_handle* h, int32_t on) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->set_graph(on); return CLRSDP_OK; })
}

int32_t clrsdp_comm_info(const clrsdp_handle* h, int32_t* nranks, int32_t* backend) {
  if (!h || !nranks || !backend) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  int n = 0, b = 0;
  h->impl->comm_info(&n, &b);
  *nranks = n;
  *backend = b;
  return CLRSDP_OK;
}

int32_t clrsdp_schur_info(const clrsdp_handle* h, struct clrsdp_schur_info* out) {
  if (!h || !out) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  h->impl->schur_info(out);
  return CLRSDP_OK;
}

int32_t clrsdp_set_factorization(clrsdp_handle* h, int32_t flags) {
  if (!h) { g_last_error = "null handle"; return CLRSDP_E_ARG; }
  GUARD(h, { h->impl->set_factorization(flags); return CLRSDP_OK; })
}

int32_t clrsdp_get_factorization(const clrsdp_handle* h, int32_t* flags) {
  if (!h || !flags) { g_last_error = "null argument"; return CLRSDP_E_ARG; }
  *flags = h->impl->get_factorization();
  return CLRSDP_OK;
}

int32_t clrsdp_destroy(clrsdp_handle* h) {
  if (!h) return CLRSDP_OK;
  // CLRSDP_EIGMX_STATS=1 when the handle was created: how many blocks eigmin_mx and the mxblk
  // route handed to the multi-word path so far (all handles of the process; diagnostics only)
  if (h->impl && h->impl->sw.eigmx_stats) {
    unsigned int fb = 0, ms = 0;
    if (hipMemcpyFromSymbol(&fb, HIP_SYMBOL(g_eigmx_fallbacks), sizeof(fb)) == hipSuccess &&
        hipMemcpyFromSymbol(&ms, HIP_SYMBOL(g_mxblk_steps), sizeof(ms)) == hipSuccess)
      std::fprintf(stderr, "clrsdp: eigmin_mx multi-word fallbacks so far: %u (mxblk route: most refinement steps %u)\n", fb, ms);
    std::vector<double> z(256 * 24);
    if (hipMemcpyFromSymbol(z.data(), HIP_SYMBOL(g_eigmx_dbg), z.size() * sizeof(double)) == hipSuccess)
      for (int b = 0; b < 64; ++b) {
        const double* q = &z[b * 24];
        if (q[20] == 0.0 && q[23] == 0.0) continue;
        std::fprintf(stderr, "  block %d (last launch): eta %.2e %.2e %.2e %.2e lam %.17g lam2 %.17g rho %.17g temple %.2e\n",
                     b, q[16], q[17], q[18], q[19], q[20], q[21], q[22], q[23]);
      }
  }
  GUARD(h, { delete h; return CLRSDP_OK; })
}

}  // extern "C"
