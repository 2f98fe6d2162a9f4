// kernels_dense.h -- small dense factorisations kept on chip (registers / LDS).
//
//   chol_lookahead A = L L^T (or L D L^T) and optionally L^-1 of a multi-word block n <= 128, the
//                  matrix held in registers, the pivot chain on a wave of its own beside the
//                  trailing update.  With chol_inv_tiles (fp64) it replaces spd_inv!
//                  (MPMP.jl:766), cho! (1846) and the LU solves of S_j / Q (1436-1463, 1501,
//                  1752-1772): every later solve becomes a GEMM with L^-1.
//   potrf_blk_*, potrf64_*  the blocked Cholesky chains across workgroups (multi-word / fp64)
//                  for blocks past the on-chip kernels: diag, trsm and update steps per panel.
//   eigmin_lds     lambda_min of a symmetric n <= 128 matrix held in LDS: Householder
//                  tridiagonalisation + Sturm multisection (approx_eig_qr!, MPMP.jl:1857-1870).
//   eigblk_*       the same for blocks past the LDS kernels, across workgroups: one launch per
//                  column, then the multisection (CLRSDP_EIG_BLK=1, instead of eigmin_batched).
#pragma once
#include "kernels.h"

namespace clrsdp {

// chol_lookahead's per-column timestamps (tools/micro/potrf_blk_bench.hip; compiled out in the
// library): [block][wave][column][point]
#ifdef CLRSDP_LA_TRACE
__device__ unsigned long long g_la_trace[64 * 16 * 128 * 4];
#define LA_STAMP(q) do { if (lane == 0 && w < 16 && j < 128 && blockIdx.x < 64 && blockIdx.y == 0) \
  g_la_trace[((blockIdx.x * 16 + w) * 128 + j) * 4 + (q)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define LA_STAMP(q)
#endif
// a - b c in the factorisations' trailing updates: mw::fms_fast at double-double (its bound and
// the reason it suffices there are in mwfloat.h), the plain expression otherwise.
// CLRSDP_FMS_EXACT (compile time) keeps the accurate form everywhere.
template <class T>
__device__ __forceinline__ T fms_upd(const T& a, const T& b, const T& c) { return a - b * c; }
#ifndef CLRSDP_FMS_EXACT
template <>
__device__ __forceinline__ mw::dd fms_upd<mw::dd>(const mw::dd& a, const mw::dd& b, const mw::dd& c) {
  return mw::fms_fast(a, b, c);
}
#endif

// A workgroup barrier that orders LDS only: the waves' outstanding global stores (final L / L^-1
// entries, read by no wave of the launch before a full barrier) are not waited for, as
// __syncthreads' release fence would (s_waitcnt vmcnt(0) on every column's or panel's critical
// path)
__device__ __forceinline__ void lds_barrier() {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// ------------------------------------------------------------------------------------------
// chol_lookahead: the multi-word potrf (A = L L^T in place, INV = false) of chol_packed with a
// one-column look-ahead, so the serial pivot chain no longer waits for the trailing update.
// 1024 threads: wave 0 is the CHAIN, waves 1..15 the BULK.  Phase j (one barrier each):
//   chain: column j+1 as the bulk published it (updated by columns 0..j-1) minus column j's
//          contribution, its pivot (LDL: d and 1/d by recip_fast; LL^T: sqrt and 1/sqrt by
//          pivot_sqrt), the scaled column j+1 -> LDS (buffer (j+1) & 1) and to the output;
//   bulk:  every element of columns >= j+2 minus column j's contribution (chol_packed's
//          liveness-packed slots, 15 waves), then the owners of column j+2 publish it.
// The chain's step (one multi-word FMA per lane, the pivot, one product per lane) and the bulk's
// update run side by side: a phase costs max(chain, bulk) + one barrier, where chol_packed's
// step costs chain + bulk + two barriers.  Every element sees its terms in the same order as in
// chol_packed (column j's term at step j); the factors agree with chol_packed's to the multi-word
// rounding, not bitwise: at double-double every update is fms_upd's one-two-sum form (round 6),
// and at quad-double with opts bit 1 (the default) the LDL pivot reciprocal takes one Newton
// step from the double-double one (~2^-208 relative instead of chol_packed's ~2^-212)
// (tests/test_gpu_parity.py::test_chol_lookahead_qd_one_newton_step).
// LDL (quad-double): A = U D U^T, then L = U D^1/2 with all n square roots side by side.
// MPMP.jl:1433-1442 / 1499-1505 (the factorisations of S_j and Q; the reference's approx_lu!).
// ------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T readlane0(const T& v) {
  T o;
  const double* s = reinterpret_cast<const double*>(&v);
  double* d = reinterpret_cast<double*>(&o);
#pragma unroll
  for (int q = 0; q < (int)(sizeof(T) / 8); ++q) d[q] = readlane_d(s[q], 0);
  return o;
}
// The body on one matrix d (in place when ol.A == d.A), callable from other kernels of
// 64 (NW + 1) threads (potrf_blk_update, round 6); returns the failure column + 1 or 0 to
// every thread.
template <class T, bool INV, bool LDL, int NMAX, int NW, bool SKIP0 = false>
__device__ __forceinline__ int chol_lookahead_body(const MatDesc<T>& d, const MatDesc<T>& oi,
                                                   const MatDesc<T>& ol, int opts) {
  // opts (A/B switches): bit 0 = the chain wave at raised issue priority (its SIMD also runs
  // three bulk waves); bit 1 = one Newton step for the pivot's reciprocal (from the
  // double-double one: ~2^-208 relative instead of ~2^-212)
  constexpr int NTH = 64 * (NW + 1);
  constexpr int SA = (NMAX * (NMAX + 1) / 2 + 63) / 64;  // 64-element slots of the triangle
  // SKIP0: the bulk waves on the chain's SIMD (w % 4 == 0) stay idle, the others take their
  // slots -- the chain then issues alone on its SIMD (quad-double: its pivot is thousands of
  // cycles of dependent work, and the three bulk waves beside it finished last)
  constexpr int NWB = SKIP0 ? NW - NW / 4 : NW;  // bulk waves with slots
  constexpr int KA = (SA + NWB - 1) / NWB;
  constexpr int SX = (NMAX / 8) * (NMAX / 8 + 1) / 2;    // 8 x 8 tiles of L^-1
  constexpr int KX = INV ? (SX + NWB - 1) / NWB : 1;
  constexpr int RC = (NMAX + 63) / 64;                   // chain rows per lane
  static_assert(!INV || NMAX <= 64, "the chain holds one row of L^-1 per lane");
  __shared__ T colb[2][NMAX];    // scaled column j (LDL: of U), by parity
  __shared__ T colub[LDL ? 2 : 1][LDL ? NMAX : 1];  // LDL: the unscaled column j
  __shared__ T nextc[2][NMAX];   // column j+1 as the bulk leaves it, by parity
  __shared__ T rowb[INV ? 2 : 1][INV ? NMAX : 1];   // row j of L^-1 (LDL: of U^-1), by parity
  __shared__ T nextr[INV ? 2 : 1][INV ? NMAX : 1];  // row j+1 of L^-1 as the bulk leaves it
  __shared__ T dgl[LDL ? NMAX : 1];
  __shared__ int fail;
  const int n = d.n, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const bool chain = w == 0;
  const bool idle = chain || (SKIP0 && (w & 3) == 0);
  const int wb = SKIP0 ? w - 1 - (w >> 2) : w - 1;  // rank among the bulk waves with slots
  auto wave_max = [](int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
  };
  // ---- bulk slots of A: slot wb + NW k, element e = 64 slot + lane of the column-major triangle
  T a[KA];
  int ar[KA], ac[KA], alo[KA], ahi[KA];
  const int ne = n * (n + 1) / 2;
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    const int e = 64 * (wb + NWB * k) + lane;
    int r = -1, c = -1;
    if (!idle && e < ne) {
      int rem = e;
      c = 0;
      while (rem >= n - c) {
        rem -= n - c;
        ++c;
      }
      r = c + rem;
    }
    ar[k] = r;
    ac[k] = c;
    a[k] = T(0.0);
    if (c >= 0) a[k] = d.A[r + (size_t)c * d.lda];
    ahi[k] = idle ? -1 : wave_max(c);
    alo[k] = idle ? NMAX : -wave_max(c >= 0 ? -c : -NMAX);
  }
  // ---- bulk tiles of L^-1 (chol_packed's 8 x 8 tiles, R >= C), identity to start
  T x[KX];
  int xr[KX], xc[KX], xR[KX], xC[KX];
  if constexpr (INV) {
    const int nt8 = (n + 7) / 8;
#pragma unroll
    for (int k = 0; k < KX; ++k) {
      int t = wb + NWB * k, C = 0;
      bool tv = !idle;
      if (tv) {
        while (C < nt8 && t >= nt8 - C) {
          t -= nt8 - C;
          ++C;
        }
        tv = C < nt8;
      }
      const int R = C + t;
      xR[k] = tv ? R : -1;
      xC[k] = tv ? C : 0;
      const int r = 8 * R + (lane & 7), c = 8 * C + (lane >> 3);
      const bool v = tv && r < n && c < n;
      xr[k] = v ? r : -1;
      xc[k] = v ? c : NMAX;
      x[k] = T((v && r == c) ? 1.0 : 0.0);
    }
  }
  // chain: the pivot of column c from the updated column cv (row c in lane 0), the scaled
  // column to colb / colub (buffer q) and to L
  T cv[RC];
  auto chain_column = [&](int c, int q) {
    const T dn = readlane0(cv[0]);
    T s, rs;
    if constexpr (LDL) {
      if constexpr (std::is_same<T, mw::qd>::value) {
        if (opts & 2) {
          rs = recip_qd_newton1(dn);
        } else {
          rs = recip_fast(dn);
        }
      } else {
        rs = recip_fast(dn);
      }
    } else {
      pivot_sqrt(dn, s, rs);
    }
#pragma unroll
    for (int u = 0; u < RC; ++u) {
      const int r = c + lane + 64 * u;
      if (r < n) {
        T o;
        if constexpr (LDL) {
          o = r == c ? dn : cv[u] * rs;
          colub[q][r] = cv[u];
        } else {
          o = r == c ? s : cv[u] * rs;
        }
        colb[q][r] = o;
        if (ol.A) ol.A[r + (size_t)c * ol.lda] = o;
      }
    }
    if (lane == 0) {
      if constexpr (LDL) dgl[c] = dn;
      if (!(dn > T(0.0))) fail = c + 1;
    }
    return rs;
  };
  // chain: row c of L^-1 (lane = column index <= c) scaled by the pivot's 1/sqrt (LL^T; U^-1 has
  // a unit diagonal) -> rowb (buffer q) and the output
  auto chain_row = [&](int c, int q, T xv, const T& rs) {
    if constexpr (INV) {
      if (lane <= c) {
        if constexpr (!LDL) xv = xv * rs;
        rowb[q][lane] = xv;
        oi.A[c + (size_t)lane * oi.lda] = xv;
      }
    }
  };
  // ---- phase -1: the chain factors column 0 (and row 0 of L^-1), the bulk publishes column 1
  // and row 1
  if (chain) {
    if (opts & 1) __builtin_amdgcn_s_setprio(3);
    if (lane == 0) fail = 0;
#pragma unroll
    for (int u = 0; u < RC; ++u) {
      const int r = lane + 64 * u;
      cv[u] = r < n ? d.A[r] : T(0.0);
    }
    const T rs = chain_column(0, 0);
    chain_row(0, 0, T(1.0), rs);
  } else {
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (alo[k] <= 1 && 1 <= ahi[k] && ac[k] == 1) nextc[1][ar[k]] = a[k];
    if constexpr (INV) {
#pragma unroll
      for (int k = 0; k < KX; ++k)
        if (xR[k] == 0 && xr[k] == 1) nextr[1][xc[k]] = x[k];
    }
  }
  lds_barrier();  // (the chain's L / L^-1 stores are read back only after the loop's full barrier)
  for (int j = 0; j + 1 < n; ++j) {
    LA_STAMP(0);
    if (fail) break;
    const int p = j & 1, p1 = (j + 1) & 1;
    if (chain) {
      // column j+1 (and row j+1 of L^-1): the published values minus step j's term, the pivot
      const int c = j + 1;
      const T cuj = LDL ? colub[p][c] : colb[p][c];
#pragma unroll
      for (int u = 0; u < RC; ++u) {
        const int r = c + lane + 64 * u;
        cv[u] = r < n ? fms_upd(nextc[p1][r], colb[p][r], cuj) : T(0.0);
      }
      T xv = T(0.0);
      if constexpr (INV) {
        if (lane <= c) xv = lane <= j ? fms_upd(nextr[p1][lane], colb[p][c], rowb[p][lane]) : T(1.0);
      }
      LA_STAMP(1);
      const T rs = chain_column(c, p1);
      LA_STAMP(2);
      chain_row(c, p1, xv, rs);
      LA_STAMP(3);
    } else {
      // columns >= j+2 (and rows >= j+2 of L^-1) minus step j's term; then the owners of
      // column j+2 (and of row j+2) publish it
#pragma unroll
      for (int k = 0; k < KA; ++k)
        if (ahi[k] >= j + 2 && ac[k] >= j + 2)
          a[k] = fms_upd(a[k], colb[p][ar[k]], (LDL ? colub[p] : colb[p])[ac[k]]);
      if constexpr (INV) {
#pragma unroll
        for (int k = 0; k < KX; ++k)
          if (xR[k] >= 0 && 8 * xC[k] <= j && j + 2 <= 8 * xR[k] + 7 && xr[k] >= j + 2 && xc[k] <= j)
            x[k] = fms_upd(x[k], colb[p][xr[k]], rowb[p][xc[k]]);
      }
      const int c2 = j + 2;
      if (c2 < n) {
#pragma unroll
        for (int k = 0; k < KA; ++k)
          if (alo[k] <= c2 && c2 <= ahi[k] && ac[k] == c2) nextc[p][ar[k]] = a[k];
        if constexpr (INV) {
#pragma unroll
          for (int k = 0; k < KX; ++k)
            if (xR[k] == (c2 >> 3) && xr[k] == c2) nextr[p][xc[k]] = x[k];
        }
      }
      LA_STAMP(3);
    }
    lds_barrier();
  }
  __syncthreads();
  const int failed = fail;
  if constexpr (LDL) {
    // L = U D^1/2 (column c times sqrt d_c, the diagonal sqrt d_c); L^-1 = D^-1/2 U^-1 (row r
    // times 1/sqrt d_r): the n square roots side by side
    if (!failed) {
      for (int c = tid; c < n; c += NTH) {
        T sq, rq;
        pivot_sqrt(dgl[c], sq, rq);
        colb[0][c] = sq;
        colb[1][c] = rq;
      }
    }
    __syncthreads();
    if (!failed)
      for (int e = tid; e < n * n; e += NTH) {
        const int r = e % n, c = e / n;
        if (ol.A) {
          if (r > c) ol.A[r + (size_t)c * ol.lda] = ol.A[r + (size_t)c * ol.lda] * colb[0][c];
          else if (r == c) ol.A[r + (size_t)c * ol.lda] = colb[0][c];
        }
        if constexpr (INV) {
          if (r >= c) oi.A[r + (size_t)c * oi.lda] = oi.A[r + (size_t)c * oi.lda] * colb[1][r];
        }
      }
  }
  for (int e = tid; e < n * n; e += NTH) {  // zeros above the diagonal
    const int r = e % n, c = e / n;
    if (c > r) {
      if (ol.A) ol.A[r + (size_t)c * ol.lda] = T(0.0);
      if constexpr (INV) oi.A[r + (size_t)c * oi.lda] = T(0.0);
    }
  }
  return failed;
}
template <class T, bool INV, bool LDL, int NMAX, int NW = 15, bool SKIP0 = false>  // NW bulk waves
__global__ __launch_bounds__(64 * (NW + 1)) void chol_lookahead(const MatDesc<T>* __restrict__ in,
                                                       const MatDesc<T>* __restrict__ out_inv,
                                                       const MatDesc<T>* __restrict__ out_l,
                                                       int* __restrict__ info, int opts = 0) {
  const MatDesc<T> d = in[blockIdx.x];
  const MatDesc<T> ol = out_l ? out_l[blockIdx.x] : MatDesc<T>{nullptr, 0, 0};
  const MatDesc<T> oi = INV ? out_inv[blockIdx.x] : MatDesc<T>{nullptr, 0, 0};
  const int f = chol_lookahead_body<T, INV, LDL, NMAX, NW, SKIP0>(d, oi, ol, opts);
  if (threadIdx.x == 0 && info) info[blockIdx.x] = f;
}

// ------------------------------------------------------------------------------------------
// Blocked multi-word potrf across workgroups (round 6).  chol_lookahead keeps a whole block on
// one CU: at C4 (16 Schur blocks of 127, double-double) 16 of 256 CUs run the ~n^3/6 trailing
// update and a column costs ~1.8 us (the bulk's multi-word FMAs, not the pivot chain).  Here
// the block is cut into NB-column panels k (k0 = NB k) and each panel costs three steps, the
// last two spread over many workgroups:
//   diag  (1 WG / matrix): L_kk and L_kk^-1 of the (updated) NB x NB diagonal block
//         (chol_lookahead_body, 256 threads);
//   trsm  (rows / 16 WGs): the panel below it, L_ik = A_ik L_kk^-T (a product with L_kk^-1 in
//         LDS, no serial chain), and zeros in the block row above the diagonal;
//   update(lower 16 x 16 tiles of the trailing matrix): A_ij -= L_ik L_jk^T; the workgroup 0 of
//         each matrix updates the next diagonal block itself and goes straight on to its diag
//         step, so one launch does both (update k + diag k+1).
// Launches for n = 127, NB = 32: diag, trsm, {update, diag} x 3 with trsm between = 7.  The
// factor is LL^T with every element's panel contributions summed panel by panel (a different
// order from chol_lookahead's column by column: agreement to the multi-word rounding, not bitwise).
// MPMP.jl:1433-1442 (the factorisation of S_j).
// ------------------------------------------------------------------------------------------
// *p where ok, else zero (p is not read then).  The quad-double form names the limbs: the
// conditional expression on the whole struct went through a 32-byte stack slot there.
template <class T>
__device__ __forceinline__ T load_or_zero(bool ok, const T* p) { return ok ? *p : T(0.0); }
template <>
__device__ __forceinline__ mw::qd load_or_zero<mw::qd>(bool ok, const mw::qd* p) {
  double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
  if (ok) { a = p->x[0]; b = p->x[1]; c = p->x[2]; d = p->x[3]; }
  return mw::qd(a, b, c, d);
}
template <class T>
struct BlkPotrfDesc {
  T* A;      // the matrix (column-major, lower triangle in, L out, zeros above)
  T* Linv;   // NB x NB scratch: L_kk^-1 of the current panel (ld NB)
  int n, lda;
};

// the diagonal step of panel k (k0 = NB k) on matrix m: L_kk, L_kk^-1; failure -> info[m]
template <class T, bool LDL, int NB>
__device__ __forceinline__ void potrf_blk_diag(const BlkPotrfDesc<T>& b, int k0, int* info, int m,
                                               int opts) {
  const int nb = min(NB, b.n - k0);
  const MatDesc<T> dk{b.A + k0 + (size_t)k0 * b.lda, nb, b.lda};
  const MatDesc<T> oi{b.Linv, nb, NB};
  const int f = chol_lookahead_body<T, true, LDL, NB, 3>(dk, oi, dk, opts);
  // (the first failure stays: the panels after it run on what it left and fail again)
  if (threadIdx.x == 0 && info && f && info[m] == 0) info[m] = k0 + f;
}

template <class T, bool LDL, int NB>
__global__ __launch_bounds__(256) void potrf_blk_first(const BlkPotrfDesc<T>* __restrict__ bd,
                                                       int* __restrict__ info, int opts) {
  const BlkPotrfDesc<T> b = bd[blockIdx.x];
  if (threadIdx.x == 0 && info) info[blockIdx.x] = 0;
  __syncthreads();
  potrf_blk_diag<T, LDL, NB>(b, 0, info, blockIdx.x, opts);
}

// trsm of panel k: blockIdx.y = matrix, blockIdx.x = 16-row chunk of rows k0 + NB .. n-1
// (chunk 0 also zeros the NB rows k0.. above the diagonal in the columns right of the panel)
template <class T, int NB>
__global__ __launch_bounds__(256) void potrf_blk_trsm(const BlkPotrfDesc<T>* __restrict__ bd, int k0) {
  const BlkPotrfDesc<T> b = bd[blockIdx.y];
  const int r0 = k0 + NB + 16 * blockIdx.x, tid = threadIdx.x;
  if (blockIdx.x == 0)
    for (int e = tid; e < NB * max(0, b.n - k0 - NB); e += 256) {
      const int r = k0 + e % NB, c = k0 + NB + e / NB;
      if (r < b.n) b.A[r + (size_t)c * b.lda] = T(0.0);
    }
  if (r0 >= b.n) return;
  __shared__ T li[NB][NB + 1];  // L_kk^-1, [c][t]
  __shared__ T ar[NB][17];      // the 16 rows of A_ik, [t][row]
  for (int e = tid; e < NB * NB; e += 256) {
    const int c = e % NB, t = e / NB;
    li[c][t] = b.Linv[c + (size_t)t * NB];
  }
  for (int e = tid; e < NB * 16; e += 256) {
    const int rr = e % 16, t = e / 16;
    ar[t][rr] = load_or_zero(r0 + rr < b.n, b.A + r0 + rr + (size_t)(k0 + t) * b.lda);
  }
  __syncthreads();
  const int rr = tid % 16;
  for (int c = tid / 16; c < NB; c += 16) {  // L_ik[r, c] = sum_{t <= c} A_ik[r, t] L_kk^-1[c, t]
    T acc = T(0.0);
    for (int t = 0; t <= c; ++t) acc = fms_upd(acc, -ar[t][rr], li[c][t]);
    if (r0 + rr < b.n && k0 + c < b.n) b.A[r0 + rr + (size_t)(k0 + c) * b.lda] = acc;
  }
}

// update of panel k (A_ij -= L_ik L_jk^T over the lower 16 x 16 tiles of rows / columns
// k1 = k0 + NB .. n-1) fused with the diagonal step of panel k+1: blockIdx.y = matrix,
// blockIdx.x = 0 updates the diagonal block k+1 and factors it, blockIdx.x >= 1 the other tiles
// (lower tiles (I, J), I >= J, of the trailing matrix, the ones inside the diagonal block skipped)
template <class T, bool LDL, int NB>
__global__ __launch_bounds__(256) void potrf_blk_update(const BlkPotrfDesc<T>* __restrict__ bd,
                                                        int k0, int* __restrict__ info, int opts) {
  const BlkPotrfDesc<T> b = bd[blockIdx.y];
  const int k1 = k0 + NB, tid = threadIdx.x;
  if (k1 >= b.n) return;
  __shared__ T lr[NB][17], lc[NB][17];  // rows of L_ik, L_jk: [t][row]
  const int ntr = (b.n - k1 + 15) / 16;  // 16-tiles of the trailing matrix
  constexpr int DT = NB / 16;            // 16-tiles per diagonal block
  auto upd_tile = [&](int I, int J) {    // tile (I, J) of the trailing matrix, I >= J
    const int ri = k1 + 16 * I, cj = k1 + 16 * J;
    for (int e = tid; e < NB * 16; e += 256) {
      const int rr = e % 16, t = e / 16;
      lr[t][rr] = load_or_zero(ri + rr < b.n, b.A + ri + rr + (size_t)(k0 + t) * b.lda);
      lc[t][rr] = load_or_zero(cj + rr < b.n, b.A + cj + rr + (size_t)(k0 + t) * b.lda);
    }
    __syncthreads();
    const int rr = tid % 16, cc = tid / 16, r = ri + rr, c = cj + cc;
    if (r < b.n && c < b.n && r >= c) {
      T acc = b.A[r + (size_t)c * b.lda];
#pragma unroll 8
      for (int t = 0; t < NB; ++t) acc = fms_upd(acc, lr[t][rr], lc[t][cc]);
      b.A[r + (size_t)c * b.lda] = acc;
    }
    __syncthreads();
  };
  if (blockIdx.x == 0) {
    for (int I = 0; I < DT && I < ntr; ++I)
      for (int J = 0; J <= I; ++J) upd_tile(I, J);
    potrf_blk_diag<T, LDL, NB>(b, k1, info, blockIdx.y, opts);
    return;
  }
  // tile index q = blockIdx.x - 1 over the lower tiles outside the diagonal block, row by row
  int q = blockIdx.x - 1, I = DT, J = 0;
  int before = DT * (DT + 1) / 2;  // tiles of rows < DT (all inside the diagonal block)
  // rows I >= DT hold I + 1 tiles each
  int rem = q;
  I = DT;
  while (I < ntr && rem >= I + 1) {
    rem -= I + 1;
    ++I;
  }
  (void)before;
  if (I >= ntr) return;
  J = rem;
  upd_tile(I, J);
}

// ------------------------------------------------------------------------------------------
// The fp64 chain (potrf64_*; CLRSDP_POTRF_BLK=1): the same three steps per NB-column panel, with
//   diag   one wave, lane = row of the NB x NB diagonal block, the row in registers: column j's
//          pivot and the l_cj of the rank-1 update come by v_readlane (no barrier, no LDS on the
//          serial chain); writes L_kk and the zeros above its diagonal;
//   trsm   (64-row chunks x matrices): one row of A_ik per thread, forward substitution against
//          L_kk in LDS (no explicit inverse, so the factor keeps the plain backward-error bound
//          of the Cholesky recurrence); chunk 0 zeros the block row right of the panel;
//   update (lower 64 x 64 tiles of the trailing matrix x matrices): A_ij -= L_ik L_jk^T on
//          v_mfma_f64_16x16x4f64, four waves of 32 x 32 outputs (2 x 2 MFMA tiles, NB / 4
//          k-steps each), the two NB-deep operand slabs in LDS at gemm_f64_tile's pitch (64 + 16
//          doubles: the four k-rows of a fragment read start 32 banks apart).  The product is
//          formed transposed (the MFMA's A operand is L_jk, negated; B is L_ik), which puts the 16
//          lanes of an accumulator register on 16 consecutive rows of one column of A: C is
//          loaded into the accumulators and stored from them in 128-byte runs, with no staging
//          of the output tile.  Workgroup 0 of each matrix updates the next diagonal block (VALU)
//          and factors it, the tile workgroups leave that block alone.
// A failed matrix (info[m] != 0) is left as it is by the launches after the failure.  (Workgroup 0
// may set info[m] while the tile workgroups of the same launch read it: they then update that
// matrix or not, and its contents are unspecified either way; no other matrix reads the flag.)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double readlane_f64(double x, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l),
                          __builtin_amdgcn_readlane(__double2loint(x), l));
}
// one wave: the nb x nb (nb <= NB) block Ds[r + c DP] (lower triangle) -> L at A (ld lda), zeros
// above the diagonal; the first pivot that is not positive -> info[m] = kbase + its column + 1
template <int NB>
__device__ __forceinline__ void potrf64_diag(const double* Ds, int DP, int nb, double* A, int lda,
                                             int kbase, int* info, int m) {
  static_assert(NB <= 64, "one lane per row");
  const int lane = threadIdx.x & 63;
  double row[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c)
    row[c] = (lane < nb && c <= lane) ? Ds[lane + c * DP] : (c == lane ? 1.0 : 0.0);
  int fail = 0;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const double p = readlane_f64(row[j], j);
    if (!fail && j < nb && !(p > 0.0)) fail = j + 1;
    if (!fail) {
      double s, rs;
      pivot_sqrt(p, s, rs);
      const double l = lane > j ? row[j] * rs : (lane == j ? s : 0.0);
      row[j] = l;
#pragma unroll
      for (int c = j + 1; c < NB; ++c) row[c] = row[c] - l * readlane_f64(l, c);
    }
  }
  if (fail) {
    if (lane == 0 && info && info[m] == 0) info[m] = kbase + fail;
    return;
  }
  if (lane < nb) {
#pragma unroll
    for (int c = 0; c < NB; ++c)
      if (c < nb) A[lane + (size_t)c * lda] = c <= lane ? row[c] : 0.0;
  }
}

template <int NB>
__global__ __launch_bounds__(256) void potrf64_first(const BlkPotrfDesc<double>* __restrict__ bd,
                                                     int* __restrict__ info) {
  constexpr int DP = NB + 1;
  __shared__ double Ds[NB * DP];
  const BlkPotrfDesc<double> b = bd[blockIdx.x];
  const int tid = threadIdx.x, nb = min(NB, b.n);
  if (tid == 0 && info) info[blockIdx.x] = 0;
  for (int e = tid; e < NB * NB; e += 256) {
    const int r = e % NB, c = e / NB;
    Ds[r + c * DP] = (r < nb && c <= r) ? b.A[r + (size_t)c * b.lda] : 0.0;
  }
  __syncthreads();
  if (tid < 64) potrf64_diag<NB>(Ds, DP, nb, b.A, b.lda, 0, info, blockIdx.x);
}

// trsm of panel k: blockIdx.y = matrix, blockIdx.x = 64-row chunk of rows k0 + NB .. n-1
template <int NB>
__global__ __launch_bounds__(64) void potrf64_trsm(const BlkPotrfDesc<double>* __restrict__ bd,
                                                   int k0, const int* __restrict__ info) {
  const BlkPotrfDesc<double> b = bd[blockIdx.y];
  const int k1 = k0 + NB, tid = threadIdx.x;
  if (k1 >= b.n) return;
  if (info && info[blockIdx.y]) return;
  if (blockIdx.x == 0)
    for (int e = tid; e < NB * (b.n - k1); e += 64) {
      const int r = k0 + e % NB, c = k1 + e / NB;
      b.A[r + (size_t)c * b.lda] = 0.0;
    }
  if (64 * (int)blockIdx.x >= b.n - k1) return;
  __shared__ double Ls[NB * NB];  // L_kk, [q + p NB]
  __shared__ double rd[NB];       // 1 / l_qq
  for (int e = tid; e < NB * NB; e += 64) {
    const int q = e % NB, p = e / NB;
    Ls[e] = q >= p ? b.A[(k0 + q) + (size_t)(k0 + p) * b.lda] : 0.0;
  }
  if (tid < NB) rd[tid] = 1.0 / b.A[(k0 + tid) + (size_t)(k0 + tid) * b.lda];
  __syncthreads();
  const int r = k1 + 64 * blockIdx.x + tid;
  if (r >= b.n) return;
  // (row[] in registers: every index is static, as in potrf_batched's panel)
  double row[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    double x = b.A[r + (size_t)(k0 + q) * b.lda];
#pragma unroll
    for (int p = 0; p < q; ++p) x = x - row[p] * Ls[q + p * NB];
    x = x * rd[q];
    row[q] = x;
    b.A[r + (size_t)(k0 + q) * b.lda] = x;
  }
}

// update of panel k fused with the diagonal step of panel k+1: blockIdx.y = matrix, blockIdx.x =
// 0 the next diagonal block, 1 + q the lower 64 x 64 tile q = I (I + 1) / 2 + J of the trailing
// matrix (rows / columns k1 = k0 + NB .. n-1)
template <int NB>
__global__ __launch_bounds__(256) void potrf64_update(const BlkPotrfDesc<double>* __restrict__ bd,
                                                      int k0, int* __restrict__ info) {
  constexpr int LM = 64 + 16, SZ = NB * LM, DP = NB + 1;
  static_assert(2 * NB * DP <= 2 * SZ && NB % 4 == 0, "LDS image");
  __shared__ double sm[2 * SZ];
  const BlkPotrfDesc<double> b = bd[blockIdx.y];
  const int k1 = k0 + NB, tid = threadIdx.x, n = b.n, lda = b.lda;
  if (k1 >= n) return;
  if (info && info[blockIdx.y]) return;
  double* A = b.A;
  if (blockIdx.x == 0) {
    const int nb = min(NB, n - k1);
    double* Ps = sm;            // rows k1 .. of panel k: Ps[r + t DP]
    double* Ds = sm + NB * DP;  // the updated diagonal block
    for (int e = tid; e < NB * NB; e += 256) {
      const int r = e % NB, t = e / NB;
      Ps[r + t * DP] = r < nb ? A[(k1 + r) + (size_t)(k0 + t) * lda] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < NB * NB; e += 256) {
      const int r = e % NB, c = e / NB;
      double v = 0.0;
      if (r < nb && c <= r) {
        v = A[(k1 + r) + (size_t)(k1 + c) * lda];
#pragma unroll 8
        for (int t = 0; t < NB; ++t) v = v - Ps[r + t * DP] * Ps[c + t * DP];
      }
      Ds[r + c * DP] = v;
    }
    __syncthreads();
    if (tid < 64) potrf64_diag<NB>(Ds, DP, nb, A + k1 + (size_t)k1 * lda, lda, k1, info, blockIdx.y);
    return;
  }
  const int q = blockIdx.x - 1;
  int I = (int)((sqrtf(8.0f * (float)q + 1.0f) - 1.0f) * 0.5f);
  while ((I + 1) * (I + 2) / 2 <= q) ++I;
  while (I * (I + 1) / 2 > q) --I;
  const int J = q - I * (I + 1) / 2;
  if (64 * I >= n - k1) return;
  const int i0 = k1 + 64 * I, j0 = k1 + 64 * J;
  double* Ri = sm;       // L_ik: element (row, t) at [t LM + row]
  double* Rj = sm + SZ;  // L_jk
  {
    const int i = tid & 63;
    const size_t gi = (size_t)min(i0 + i, n - 1), gj = (size_t)min(j0 + i, n - 1);
#pragma unroll
    for (int u = 0; u < NB / 4; ++u) {
      const int t = (tid >> 6) + 4 * u;
      Ri[t * LM + i] = gload(A + gi + (size_t)(k0 + t) * lda);
      Rj[t * LM + i] = gload(A + gj + (size_t)(k0 + t) * lda);
    }
  }
  const int lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, lr = lane & 15, lk = lane >> 4;
  // accumulator register r of (mj, ni): row i0 + 32 wm + 16 ni + lr, column j0 + 32 wn + 16 mj + lk + 4 r
  d4 acc[2][2];
#pragma unroll
  for (int mj = 0; mj < 2; ++mj)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = i0 + 32 * wm + 16 * ni + lr, c = j0 + 32 * wn + 16 * mj + lk + 4 * r;
        acc[mj][ni][r] = (rr < n && rr >= c) ? gload(A + rr + (size_t)c * lda) : 0.0;
      }
  __syncthreads();
#pragma unroll
  for (int kk = 0; kk < NB; kk += 4) {
    double af[2], bf[2];
#pragma unroll
    for (int mj = 0; mj < 2; ++mj) af[mj] = -Rj[(kk + lk) * LM + 32 * wn + 16 * mj + lr];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) bf[ni] = Ri[(kk + lk) * LM + 32 * wm + 16 * ni + lr];
#pragma unroll
    for (int mj = 0; mj < 2; ++mj)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mj][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[mj], bf[ni], acc[mj][ni], 0, 0, 0);
  }
#pragma unroll
  for (int mj = 0; mj < 2; ++mj)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = i0 + 32 * wm + 16 * ni + lr, c = j0 + 32 * wn + 16 * mj + lk + 4 * r;
        // (rr >= c: c < n; rows below k1 + NB with columns up to them are the next diagonal block)
        if (rr < n && rr >= c && rr >= k1 + NB) A[rr + (size_t)c * lda] = acc[mj][ni][r];
      }
}

// ------------------------------------------------------------------------------------------
// Double-double GEMM on the int8 matrix cores (Ozaki scheme; round 6, the Schur products of
// multi-word m = 1 blocks).  Every row of op(A) is scaled by 2^-E (|a| 2^-E < 1/2) and written as
// OZ_S base-2^7 digits d_p in [-64, 64], each the rounded leading part of the exact double-double
// remainder:  a = 2^E sum_{p < OZ_S} d_p 2^-7(p+1)  (every column of op(B) likewise, 2^F).  Then
//     (op(A) op(B))_ij = 2^(E_i + F_j) sum_L 2^-7(L+2) sum_{p+q=L} (D_p G_q)_ij ,
// every level-L sum of int8 products accumulates exactly in int32 (|.| <= 16 Kpad 64^2 < 2^31 for
// Kpad < 2^15) on v_mfma_i32_16x16x64_i8 and converts exactly to fp64; the OZ_S levels are summed
// in double-double, smallest first.  Levels L >= OZ_S are dropped: ~2^-7 OZ_S = 2^-112 relative
// to 2^(E_i + F_j) K -- a bound in the largest |a_ik| of row i times the largest |b_kj| of column
// j, where the VALU GEMM's is componentwise (sum_k |a_ik| |b_kj|).  The two differ by the spread of
// the operands along k: with V = D R, X^-1 = D^-1 M D^-1 and D = diag(2^(-g k)) -- the grading a
// monomial-type basis gives an interior-point iterate -- the largest a_ik and the largest b_kj sit
// at opposite ends of k and every product a_ik b_kj is smaller than the bound's scale by the span
// of D (2^44 at delta = 12, g = 4: 2^-68 instead of 2^-112 relative to the entry).  So the
// contraction index is equilibrated, exactly, before the split: element k of every vector is
// multiplied by 2^(ks kx[k]), kx[k] = the exponent of the largest |V_kj| of row k of V_b (set once
// from the uploaded V), ks = -1 for the columns of V_b and +1 for the rows of X^-1_b, Y_b and the
// columns of TX_b, TY_b; the products a_ik b_kj are unchanged and E, F are those of the scaled
// vectors.  After it the bound's scale is within a small factor of sum_k |a_ik| |b_kj| whenever
// the grading of the operands is the basis's (what is left is the spread of R and M themselves).
// 136 int8 MFMAs per 16 x 16 tile and 64-k chunk against 64 double-double FMAs per output and k
// on the VALU: 9.1 against 15.0 us for 16 products 64 x 64 @ 64 x 128, 15.1 against 43.0 us for
// 64 (tools/micro/ozaki_dd_bench.hip, same accuracy against a host double-double reference).
// Digit planes: D[(p * Rpad + v) * Kpad + k] (int8, zero-padded: the buffers are zeroed once and
// the split writes only v < nv, k < K).
// (Ozaki, Ogita, Oishi & Rump, Numer. Algorithms 59 (2012); integer slices as in Ootomo, Ozaki &
// Yokota, IJHPCA 38 (2024).)
// ------------------------------------------------------------------------------------------
constexpr int OZ_S = 16;
typedef int oz_v4i __attribute__((ext_vector_type(4)));
struct OzSplitDesc {
  const mw::dd* X;     // vector v, element k at X[v * sv + k * sk]
  long long sv, sk;
  signed char* D;      // digit planes, [OZ_S][Rpad][Kpad]
  int* E;              // per-vector exponent
  int nv, K, Rpad, Kpad;
  const int* kx;       // per-k equilibration exponents (K of them), element k scaled by 2^(ks kx[k])
  int ks, pad;
};
// one wave per vector (4 per workgroup); t2d: TileRef{desc, group of 4 vectors}
__global__ __launch_bounds__(256) void oz_split(const OzSplitDesc* __restrict__ descs,
                                                const TileRef* __restrict__ t2d) {
  const TileRef tr = t2d[blockIdx.x];
  const OzSplitDesc d = descs[tr.p];
  const int v = 4 * tr.t + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (v >= d.nv) return;
  const mw::dd* x = d.X + (size_t)v * d.sv;
  int ex = -1100;
  for (int k = lane; k < d.K; k += 64) {
    const double h = x[(size_t)k * d.sk].hi;
    if (h != 0.0) ex = max(ex, ilogb(h) + d.ks * d.kx[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ex = max(ex, __shfl_xor(ex, o));
  const int E = ex + 2;  // |x 2^(ks kx)| < 2^(ex+1) = 2^E / 2
  for (int k = lane; k < d.K; k += 64) {
    const mw::dd a = x[(size_t)k * d.sk];
    const int sh = d.ks * d.kx[k] - E;
    double h = ldexp(a.hi, sh), l = ldexp(a.lo, sh);
    signed char* out = d.D + (size_t)v * d.Kpad + k;
#pragma unroll
    for (int p = 0; p < OZ_S; ++p) {
      h *= 128.0;
      l *= 128.0;
      const double dg = rint(h);
      double e;
      h = mw::two_sum(h - dg, l, e);  // (h - dg is exact: |h - dg| <= 1/2 on h's grid)
      l = e;
      out[(size_t)p * d.Rpad * d.Kpad] = (signed char)(int)dg;
    }
  }
  if (lane == 0) d.E[v] = E;
}
struct OzGemmDesc {
  const signed char* DA;  // rows of op(A): [OZ_S][RpadA][Kpad]
  const int* EA;
  const signed char* DB;  // columns of op(B): [OZ_S][RpadB][Kpad]
  const int* EB;
  mw::dd* C;              // M x N, ld ldc:  C = op(A) op(B)
  int RpadA, RpadB, Kpad, ldc, M, N, tn, pad;
};
// one wave per 16 x 16 output tile (tile t: rows 16 (t / tn), columns 16 (t % tn)), 4 per
// workgroup; t2d: TileRef{desc, tile} by groups of 4 consecutive entries per workgroup
__global__ __launch_bounds__(256) void oz_gemm(const OzGemmDesc* __restrict__ descs,
                                               const TileRef* __restrict__ t2d, int ntiles) {
  const int wi = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (wi >= ntiles) return;
  const TileRef tr = t2d[wi];
  const OzGemmDesc d = descs[tr.p];
  const int r0 = 16 * (tr.t / d.tn), c0 = 16 * (tr.t % d.tn);
  const size_t pa = (size_t)d.RpadA * d.Kpad, pb = (size_t)d.RpadB * d.Kpad;
  const signed char* ra = d.DA + (size_t)(r0 + (l & 15)) * d.Kpad + 16 * (l >> 4);
  const signed char* rb = d.DB + (size_t)(c0 + (l & 15)) * d.Kpad + 16 * (l >> 4);
  oz_v4i acc[OZ_S];
#pragma unroll
  for (int L = 0; L < OZ_S; ++L) acc[L] = oz_v4i{0, 0, 0, 0};
  for (int k0 = 0; k0 < d.Kpad; k0 += 64) {
    oz_v4i a[OZ_S], b[OZ_S];
#pragma unroll
    for (int p = 0; p < OZ_S; ++p) {
      a[p] = *reinterpret_cast<const oz_v4i*>(ra + p * pa + k0);
      b[p] = *reinterpret_cast<const oz_v4i*>(rb + p * pb + k0);
    }
#pragma unroll
    for (int L = 0; L < OZ_S; ++L)
#pragma unroll
      for (int p = 0; p <= L; ++p) acc[L] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], b[L - p], acc[L], 0, 0, 0);
  }
  // C/D layout: column l & 15, row 4 (l >> 4) + r
  const int col = c0 + (l & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double hi = 0.0, lo = 0.0;
#pragma unroll
    for (int L = OZ_S - 1; L >= 0; --L) {  // smallest level first; every term exact in fp64
      double e;
      hi = mw::two_sum(hi, ldexp((double)acc[L][r], -7 * (L + 2)), e);
      lo += e;
    }
    const int row = r0 + 4 * (l >> 4) + r;
    if (row < d.M && col < d.N) {
      double e;
      const double h = mw::quick_two_sum(hi, lo, e);
      const int sc = d.EA[row] + d.EB[col];
      d.C[row + (size_t)col * d.ldc] = mw::dd(ldexp(h, sc), ldexp(e, sc));
    }
  }
}

// ------------------------------------------------------------------------------------------
// eigmin_lds: smallest eigenvalue of a symmetric matrix (n <= NMAX), 512 threads.  The matrix
// is symmetrised into LDS (ld = n), tridiagonalised by Householder reflections (full storage),
// then one wave runs a 64-point Sturm multisection.
// ------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------
// eigmin_reg (tools/micro/retired_kernels.h; eigmin_split below keeps its layout, scaling and
// multisection): lambda_min of a symmetric n <= 128 fp64 block with the matrix held in REGISTERS
// (replaces approx_eig_qr! in compute_step_length, MPMP.jl:1857-1860).  The input must be exactly
// symmetric (every caller's block comes from the symmetric GEMM epilogue).  512 threads; wave w
// owns row block rb(w) (rows 16 rb..16 rb+15, lane r = l & 15), lane class c = l >> 4 owns the column pairs
// j = 2c + 8s + {0,1}, s = 0..15 (fixed slots): 32 entries per thread.  Householder
// tridiagonalisation with ONE barrier per column k:
//   p_i = sum_j A_ij v_j in registers (+ 2 swaps across the column classes), per-wave v^T p to
//   LDS                                                                             -- barrier
//   w = beta p - K v; A -= v w^T + w v^T in registers; meanwhile every wave recomputes row k+1
//   of the updated matrix from the copy its owners published a step earlier (the owners' own
//   operations, so bitwise their registers) and builds the next reflector from it redundantly
//   (wave reduction, no barrier); the owners of row k+2 publish it for the step after next.
// The 16 lanes of a DPP row share a column class and so need the same 32 values of v and of p:
// lane t of the row reads only slot t and every FMA takes slot s from lane s by row_newbcast
// (v_fmac_f64_dpp).  Slots whose 8 columns are all <= k are skipped in groups of 4 by a uniform
// branch; the slots never move, so the loop carries no register copies.
// Then 512-way multisection with Sturm counts on the tridiagonal matrix.
// ------------------------------------------------------------------------------------------
// Compile-time loop (the DPP lane selector of row_newbcast is an instruction immediate).
template <int K, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (K < E) {
    f(std::integral_constant<int, K>{});
    static_for<K + 1, E>(f);
  }
}
// acc += src[lane J of this lane's 16-lane DPP row] * mul: one v_fmac_f64_dpp with
// row_newbcast (the f64 DPP form of CDNA3/4; the builtin route costs a copy + v_mov_b64_dpp +
// v_fma_f64 and serialises on the copy register).  A DPP source needs 2 wait states after a
// VALU write, which the compiler does not see inside inline asm: NOP = true puts an s_nop 1
// in front.  The statements are volatile, so they keep their program order among themselves.
template <int J, bool NOP>
__device__ __forceinline__ void fmac_bcast(double& acc, double src, double mul) {
  if constexpr (NOP)
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc) : "v"(src), "v"(mul), "n"(J));
  else
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc) : "v"(src), "v"(mul), "n"(J));
}

// Sturm count of the symmetric tridiagonal (dg, e2 = squared off-diagonals) below sigma, with a
// Newton-refined hardware reciprocal instead of the IEEE division (only signs are used) and
// the coefficients read two at a time.
__device__ inline int sturm_count_fast(const double* dg, const double* e2, int n, double sigma) {
  int cnt = 0;
  double q = dg[0] - sigma;
  cnt += q < 0.0;
  int i = 1;
  for (; i + 1 < n; i += 2) {
    const double d0 = dg[i], d1 = dg[i + 1], f0 = e2[i - 1], f1 = e2[i];
    q = q == 0.0 ? 1e-300 : q;
    double r = __builtin_amdgcn_rcp(q);
    r = fma(fma(-q, r, 1.0), r, r);
    r = fma(fma(-q, r, 1.0), r, r);
    q = (d0 - sigma) - f0 * r;
    cnt += q < 0.0;
    q = q == 0.0 ? 1e-300 : q;
    r = __builtin_amdgcn_rcp(q);
    r = fma(fma(-q, r, 1.0), r, r);
    r = fma(fma(-q, r, 1.0), r, r);
    q = (d1 - sigma) - f1 * r;
    cnt += q < 0.0;
  }
  for (; i < n; ++i) {
    q = q == 0.0 ? 1e-300 : q;
    double r = __builtin_amdgcn_rcp(q);
    r = fma(fma(-q, r, 1.0), r, r);
    r = fma(fma(-q, r, 1.0), r, r);
    q = (dg[i] - sigma) - e2[i - 1] * r;
    cnt += q < 0.0;
  }
  return cnt;
}

// Is lambda_min < sigma?  The multisection only needs "count >= 1", and with p_0 = 1 > 0 the
// Sturm sequence of leading principal minors has a sign change iff some minor is negative, so
// the count becomes an OR of sign bits: per row one FMA on the chain (e_{i-1} p_{i-2} is formed a
// row ahead), one subtraction, one multiplication and one integer OR; no compares, selects or
// branches.  sd/se are the padded arrays of eigmin_reg (nr a multiple of 8, se[i] = e2_{i-1} > 0
// inside the matrix, so a zero minor is followed by a nonzero one of the opposite sign of its
// predecessor and the sign test stays exact); (p_{i-1}, p_i) is rescaled by a power of two every
// 8 rows.
__device__ inline bool sturm_any_below(const double* __restrict__ sd, const double* __restrict__ se,
                                       int nr, double sigma) {
  double pm = 0.0, pc = 1.0;
  int acc = 0;
  for (int i0 = 0; i0 < nr; i0 += 8) {
    double dv[8], ev[8];
#pragma unroll
    for (int u = 0; u < 8; u += 2) {
      const double2 a = *reinterpret_cast<const double2*>(sd + i0 + u);
      const double2 b = *reinterpret_cast<const double2*>(se + i0 + u);
      dv[u] = a.x; dv[u + 1] = a.y;
      ev[u] = b.x; ev[u + 1] = b.y;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double pn = fma(dv[u] - sigma, pc, -(ev[u] * pm));
      acc |= __double2hiint(pn);
      pm = pc;
      pc = pn;
    }
    const int ex = __builtin_amdgcn_frexp_exp(pc);
    pc = __builtin_ldexp(pc, -ex);
    pm = __builtin_ldexp(pm, -ex);
  }
  return acc < 0;
}

// The same test with the chain split in two (round 4): leading principal minors p_i of rows
// [0, h) top-down and trailing minors q_i of rows [h, nr) bottom-up, two independent recurrences
// (the count is latency-bound: each row is one dependent FMA chain link), joined by
// det(T - sigma I) = p_{h-1} q_h - e2_{h-1} p_{h-2} q_{h+1}.  With the twisted factorisation
// N D N^T of T - sigma I at row h (Sylvester), lambda_min < sigma iff some p_i < 0 (i < h), some
// q_i < 0 (i >= h) or det < 0 (the twist pivot has the sign of det when p_{h-1}, q_h > 0).  Both
// chains rescale by powers of two every 8 rows; det's three terms carry one p and one q factor
// each, so the scales agree.
__device__ inline bool sturm_any_below2(const double* __restrict__ sd, const double* __restrict__ se,
                                        int nr, double sigma) {
  const int h = 8 * ((nr >> 3) >> 1);
  double pm = 0.0, pc = 1.0;  // p_{i-2}, p_{i-1}
  double qm = 0.0, qc = 1.0;  // q_{i+2}, q_{i+1}
  int acc = 0;
  const int nb = nr - h, nt = h;
  const int nmax = nb > nt ? nb : nt;
  for (int g = 0; g < nmax; g += 8) {
    double dt[8], et[8], db[8], eb[8];
    const bool top = g < nt;
    const int ib = nr - 8 - g;  // rows ib..ib+7 of the bottom chain, walked downwards
#pragma unroll
    for (int u = 0; u < 8; u += 2) {
      if (top) {
        const double2 a = *reinterpret_cast<const double2*>(sd + g + u);
        const double2 b = *reinterpret_cast<const double2*>(se + g + u);
        dt[u] = a.x; dt[u + 1] = a.y;
        et[u] = b.x; et[u + 1] = b.y;
      }
      const double2 c = *reinterpret_cast<const double2*>(sd + ib + u);
      // q_i couples to row i+1 through e2_i = se[i+1]
      const double2 e = *reinterpret_cast<const double2*>(se + ib + u);
      db[u] = c.x; db[u + 1] = c.y;
      eb[u] = e.y;
      eb[u + 1] = (u + 2 < 8) ? se[ib + u + 2] : (ib + 8 < nr + 0 ? se[ib + 8] : 0.0);
    }
    if (top) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double pn = fma(dt[u] - sigma, pc, -(et[u] * pm));
        acc |= __double2hiint(pn);
        pm = pc;
        pc = pn;
      }
      const int ex = __builtin_amdgcn_frexp_exp(pc);
      pc = __builtin_ldexp(pc, -ex);
      pm = __builtin_ldexp(pm, -ex);
    }
    if (g < nb) {
#pragma unroll
      for (int u = 7; u >= 0; --u) {
        const double qn = fma(db[u] - sigma, qc, -(eb[u] * qm));
        acc |= __double2hiint(qn);
        qm = qc;
        qc = qn;
      }
      const int ex = __builtin_amdgcn_frexp_exp(qc);
      qc = __builtin_ldexp(qc, -ex);
      qm = __builtin_ldexp(qm, -ex);
    }
  }
  // p_{h-1} = pc, p_{h-2} = pm; q_h = qc, q_{h+1} = qm; e2_{h-1} = se[h]
  const double det = fma(pc, qc, -(se[h] * pm * qm));
  acc |= __double2hiint(det);
  return acc < 0;
}

// ------------------------------------------------------------------------------------------
// eigmin_split (round 4): lambda_min of a symmetric fp64 block (n <= 128), the same Householder
// tridiagonalisation as eigmin_reg with the matrix in the registers of 8 "bulk" waves (same
// layout), but the reflector of each column is built ONCE, by a ninth "chain" wave at raised
// issue priority, instead of redundantly by every live wave: that redundancy made eigmin_reg
// VALU-issue bound (~300 instructions per column and wave against 96 useful FMAs, two waves per
// SIMD).  Two barriers per column k:
//   bulk:  p = A_k v_k in registers, per-wave v^T p, the rows of p to LDS          -- barrier 1
//   bulk:  w = beta p - K v; A_{k+1} = A_k - v w^T - w v^T in registers; the owners of row k+2
//          publish it (for step k+1)
//   chain: row k+1 of A_{k+1} from the copy its owners published a step earlier (their own
//          operations), the reflector v_{k+1} and beta_{k+1}, the tridiagonal entries -> LDS
//                                                                                   -- barrier 2
// The rank-2 update (two of the three FMAs per entry) runs under the chain's latency; per column
// only the matvec, two LDS round trips and the chain's ~40 dependent operations are serial.
// The chain lane (c, t16) holds the same column pair j0 = 2c + 8 t16 as a bulk lane, so its sums
// run in eigmin_reg's order.  Same scaling, Gershgorin bracket and multisection as eigmin_reg.
// ------------------------------------------------------------------------------------------
#ifdef CLRSDP_EIGSPLIT_STAMPS
__device__ unsigned long long g_eigsplit_stamps[8];
#endif
// DBG (timing experiments only): 1 = no update FMAs, 2 = no matvec FMAs, 4 = the chain wave
// skips the reflector (v_{k+1} = the published row), 8 = the old one-chain 256-way multisection,
// 128 / 256 = the column loop stops 32 / 64 columns early (what the tail columns cost)
// TAIL (round 5): the last TAIL columns (TAIL <= 32, n >= TAIL + 8) run on the chain wave alone:
// the trailing TAIL x TAIL matrix goes through LDS into its registers (row lane & 31 per lane,
// both half-waves alike) and every step is wave-local -- no barrier, no cross-wave exchange.
// The two-barrier skeleton costs ~0.8 us per column however small the trailing matrix is
// (the last 32 columns of a 128 block: 26 us of 145, tools/micro/eig_split_bench.hip).
template <int DBG = 0, int TAIL = 0>
__global__ __launch_bounds__(576) void eigmin_split(const MatDesc<double>* __restrict__ descs,
                                                     double* __restrict__ out) {
  static_assert(TAIL == 0 || (TAIL >= 8 && TAIL <= 32), "tail size");
  constexpr int NS = 16, NWB = 8, GS = (DBG & 16) ? 2 : 4;
#ifdef CLRSDP_EIGSPLIT_STAMPS
  // per column: chain lane 0 (slots 0-2: wait at barrier 1, reflector, wait at barrier 2) and
  // bulk wave 4 lane 0 (row block 7, live to the end; slots 3-6: matvec phase, wait at barrier
  // 1, update phase, wait at barrier 2); slot 7: multisection
  unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_prev = __builtin_amdgcn_s_memtime();
#define ES_STAMP(slot)                                            \
  {                                                               \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();   \
    st_acc[slot] += t_ - t_prev;                                  \
    t_prev = t_;                                                  \
  }
#else
#define ES_STAMP(slot)
#endif
  __shared__ __attribute__((aligned(16))) double rowb[2][128];
  __shared__ __attribute__((aligned(16))) double pb[2][128];
  __shared__ __attribute__((aligned(16))) double vb[2][128];
  __shared__ __attribute__((aligned(16))) double redw[2][NWB];
  __shared__ double betab[2];
  __shared__ double dg[128], e2[128];
  __shared__ __attribute__((aligned(16))) double sd[128], se[128];
  __shared__ double bnd[2];
  __shared__ unsigned long long masks[8];
  __shared__ double amaxw[NWB];
  const MatDesc<double> d = descs[blockIdx.x];
  const int n = d.n, lda = d.lda, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const bool chain = w == NWB;
  const int blk = w < 4 ? w : 11 - w;  // bulk row block (pairs 0/7, 1/6, 2/5, 3/4 per SIMD)
  const int c = lane >> 4, t16 = lane & 15;
  const int i = blk * 16 + t16;       // bulk: this lane's row
  const int j0 = 2 * c + 8 * t16;     // this lane's column pair (bulk: broadcast slot; chain: x_j)
  double a[NS][2];
#pragma unroll
  for (int s = 0; s < NS; ++s) a[s][0] = a[s][1] = 0.0;
  if (!chain) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int j = 2 * c + 8 * s + e;
        const int ic = min(i, n - 1), jc = min(j, n - 1);
        const double v = gload(d.A + ic + (size_t)jc * lda);
        a[s][e] = (i < n && j < n) ? v : 0.0;
      }
    double amax = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) amax = fmax(amax, fmax(fabs(a[s][0]), fabs(a[s][1])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
    if (lane == 0) amaxw[w] = amax;
  }
  __syncthreads();
  int ex0;
  {
    double amax = amaxw[0];
#pragma unroll
    for (int r = 1; r < NWB; ++r) amax = fmax(amax, amaxw[r]);
    ex0 = (amax > 0.0 && amax < INFINITY) ? __builtin_amdgcn_frexp_exp(amax) : 0;
  }
  if (!chain) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      a[s][0] = __builtin_ldexp(a[s][0], -ex0);
      a[s][1] = __builtin_ldexp(a[s][1], -ex0);
    }
  }
  auto publish_row = [&](int r, double* dst) {  // the owners of row r write its 128 entries
    if (!chain && blk == (r >> 4) && t16 == (r & 15)) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
        *reinterpret_cast<double2*>(dst + 2 * c + 8 * s) = make_double2(a[s][0], a[s][1]);
    }
  };
  // chain state: v of the current step at the lane's column pair, and beta
  double cx = 0.0, cy = 0.0, beta = 0.0, vi = 0.0;
  // the reflector of column r from x = row r of the current matrix (chain wave only):
  // v_j = 0 (j <= r), v0 (j = r+1), x_j (j > r+1), H = I - beta v v^T
  auto reflector = [&](int r, double xj0, double xj1, double xr, double x0) {
    double tl = (j0 >= r + 2 ? xj0 * xj0 : 0.0);
    tl = fma(j0 + 1 >= r + 2 ? xj1 : 0.0, xj1, tl);
    tl = xsum32(xsum16(row16_sum(tl)));  // sum_{j >= r+2} x_j^2
    double bt = 0.0, v0 = x0, e2r = x0 * x0;
    if (tl > 0.0) {
      const double ss = fma(x0, x0, tl);
      double nrm;
      if (ss > 0x1p-900) {  // Newton-refined hardware rsq / rcp (~1 ulp)
        double rs = __builtin_amdgcn_rsq(ss);
        rs = rs * fma(-0.5 * ss, rs * rs, 1.5);
        nrm = ss * rs;
        nrm = fma(fma(-nrm, nrm, ss), 0.5 * rs, nrm);
      } else {
        nrm = sqrt(ss);
      }
      const double alpha = x0 > 0.0 ? -nrm : nrm;
      v0 = x0 - alpha;
      const double q = fma(v0, v0, tl);
      double rc = __builtin_amdgcn_rcp(q);
      rc = fma(fma(-q, rc, 1.0), rc, rc);
      rc = fma(fma(-q, rc, 1.0), rc, rc);
      bt = 2.0 * rc;
      e2r = alpha * alpha;
    }
    cx = j0 <= r ? 0.0 : (j0 == r + 1 ? v0 : xj0);
    cy = j0 + 1 <= r ? 0.0 : (j0 + 1 == r + 1 ? v0 : xj1);
    beta = bt;
    *reinterpret_cast<double2*>(&vb[r & 1][j0]) = make_double2(cx, cy);
    if (lane == 0) {
      dg[r] = xr;
      e2[r] = e2r;
      betab[r & 1] = bt;
    }
  };
  publish_row(0, rowb[0]);
  if (n >= 2) publish_row(1, rowb[1]);
  __syncthreads();
  if (chain) {
    __builtin_amdgcn_s_setprio(3);
    if (n >= 2) {
      const double2 xr = *reinterpret_cast<const double2*>(&rowb[0][j0]);
      reflector(0, xr.x, xr.y, rowb[0][0], rowb[0][1]);
    } else if (lane == 0) {
      dg[0] = rowb[0][0];
    }
  }
  __syncthreads();
  if (!chain && n >= 2) {
    const double2 v2 = *reinterpret_cast<const double2*>(&vb[0][j0]);
    cx = v2.x;
    cy = v2.y;
    vi = vb[0][i];
    beta = betab[0];
  }
  constexpr int KSKIP = (DBG & 128) ? 32 : (DBG & 256) ? 64 : 0;
  // with the tail: the loop stops at iteration k0 = n - TAIL - 1 (A_{k0} in the registers, the
  // reflector v_{k0} in vb / betab), the chain wave does iterations k0 .. n - 3
  const bool tail = TAIL > 0 && n >= TAIL + 8;
  const int kend = tail ? n - TAIL - 1 + 2 : n;  // loop while k + 2 < kend
  for (int k = 0; k + 2 + KSKIP < kend; ++k) {
    const int lo = (k + 1) >> 3;  // slots s < lo hold columns <= k only
    const int r = k + 1;
    double pp = 0.0;
    if (!chain) {
      // ---- p = A_k v_k and this wave's part of v^T p (two FMA chains per column parity)
      const bool live = blk * 16 + 15 > k && blk * 16 < n;
      double pa[4] = {0.0, 0.0, 0.0, 0.0};
      if (live && !(DBG & 2)) {
        // slots in groups of GS behind one uniform branch each (pairs measured slower: a
        // branch and the DPP wait state per group)
        static_for<0, NS / GS>([&](auto G) {
          constexpr int g = decltype(G)::value;
          if (GS * g + GS - 1 >= lo) {
            static_for<GS * g, GS * g + GS>([&](auto S) {
              constexpr int s = decltype(S)::value;
              fmac_bcast<s, s == GS * g>(pa[2 * (s & 1)], cx, a[s][0]);
              fmac_bcast<s, false>(pa[2 * (s & 1) + 1], cy, a[s][1]);
            });
          }
        });
      }
      pp = xsum32(xsum16((pa[0] + pa[1]) + (pa[2] + pa[3])));
      double t = 0.0;
      if (c == 0) {
        pb[k & 1][i] = i > k ? pp : 0.0;
        t = vi * pp;
      }
      t = row16_sum(t);  // class-0 lanes carry the rows' v_i p_i
      if (lane == 0) redw[k & 1][w] = t;
      ES_STAMP(3)
    }
    __syncthreads();
    ES_STAMP(chain ? 0 : 4)
    if (chain) {
      // ---- row r of A_{k+1} and the reflector v_{k+1}
      double rw[NWB];
#pragma unroll
      for (int q = 0; q < NWB; q += 2) {
        const double2 v2 = *reinterpret_cast<const double2*>(&redw[k & 1][q]);
        rw[q] = v2.x;
        rw[q + 1] = v2.y;
      }
      const double* old = rowb[r & 1];
      const double2 pj = *reinterpret_cast<const double2*>(&pb[k & 1][j0]);
      const double2 o = *reinterpret_cast<const double2*>(old + j0);
      const double orr = old[r], or1 = old[r + 1];
      const double vr = vb[k & 1][r], vr1 = vb[k & 1][r + 1];
      const double pr = pb[k & 1][r], pr1 = pb[k & 1][r + 1];
      const double tot = ((rw[0] + rw[1]) + (rw[2] + rw[3])) + ((rw[4] + rw[5]) + (rw[6] + rw[7]));
      const double Kc = beta * beta * tot * 0.5;
      const double wr = fma(beta, pr, -(Kc * vr));
      const double gr = fma(Kc, vr, -wr), mhr = -(beta * vr);
      const double xj0 = fma(cx, gr, fma(pj.x, mhr, o.x));
      const double xj1 = fma(cy, gr, fma(pj.y, mhr, o.y));
      const double xr = fma(vr, gr, fma(pr, mhr, orr));
      const double x0 = fma(vr1, gr, fma(pr1, mhr, or1));
      if constexpr (DBG & 4) {
        cx = o.x;
        cy = o.y;
        *reinterpret_cast<double2*>(&vb[r & 1][j0]) = make_double2(cx, cy);
        if (lane == 0) { dg[r] = xr + xj0 + x0; e2[r] = 1.0; betab[r & 1] = 0.0; }
      } else {
        reflector(r, xj0, xj1, xr, x0);
      }
      ES_STAMP(1)
    } else if (blk * 16 + 15 > k + 1 && blk * 16 < n) {
      // ---- w = beta p - K v;  A -= v w^T + w v^T, i.e. a_ij += g_i v_j - h_i p_j
      double rw[NWB];
#pragma unroll
      for (int q = 0; q < NWB; q += 2) {
        const double2 v2 = *reinterpret_cast<const double2*>(&redw[k & 1][q]);
        rw[q] = v2.x;
        rw[q + 1] = v2.y;
      }
      const double2 pv = *reinterpret_cast<const double2*>(&pb[k & 1][j0]);
      const double tot = ((rw[0] + rw[1]) + (rw[2] + rw[3])) + ((rw[4] + rw[5]) + (rw[6] + rw[7]));
      const double Kc = beta * beta * tot * 0.5;
      const double wi = fma(beta, pp, -(Kc * vi));
      const double gi = fma(Kc, vi, -wi), mhi = -(beta * vi);
      // per group the p terms, then the v terms (a dependent pair is 8 issues apart); all p
      // terms ahead of all v terms measured slower
      if (!(DBG & 1)) static_for<0, NS / GS>([&](auto G) {
        constexpr int g = decltype(G)::value;
        if (GS * g + GS - 1 >= lo) {
          static_for<GS * g, GS * g + GS>([&](auto S) {
            constexpr int s = decltype(S)::value;
            fmac_bcast<s, s == GS * g>(a[s][0], pv.x, mhi);
            fmac_bcast<s, false>(a[s][1], pv.y, mhi);
          });
          static_for<GS * g, GS * g + GS>([&](auto S) {
            constexpr int s = decltype(S)::value;
            fmac_bcast<s, false>(a[s][0], cx, gi);
            fmac_bcast<s, false>(a[s][1], cy, gi);
          });
        }
      });
      publish_row(k + 2, rowb[k & 1]);
      ES_STAMP(5)
    }
    __syncthreads();
    ES_STAMP(chain ? 2 : 6)
    if (!chain) {
      const double2 v2 = *reinterpret_cast<const double2*>(&vb[r & 1][j0]);
      cx = v2.x;
      cy = v2.y;
      vi = vb[r & 1][i];
      beta = betab[r & 1];
    }
  }
  if (chain) __builtin_amdgcn_s_setprio(0);
  if constexpr (TAIL > 0) {
    if (tail) {
      constexpr int TT = TAIL;
      __shared__ double Mt[TT][TT + 1];
      __shared__ double ub[TT], pt[TT];
      const int k0 = n - TT - 1;
      // A_{k0}'s trailing block (rows and columns > k0) from the bulk registers, v_{k0} there
      if (!chain) {
#pragma unroll
        for (int sl = 0; sl < NS; ++sl)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int j = 2 * c + 8 * sl + e;
            if (i > k0 && j > k0 && i < n && j < n) Mt[i - k0 - 1][j - k0 - 1] = a[sl][e];
          }
      }
      if (tid < TT) ub[tid] = vb[k0 & 1][k0 + 1 + tid];
      __syncthreads();
      if (chain) {
        // lanes 0..TT-1 hold rows 0..TT-1; the others a dummy copy of row 0, masked out of
        // every sum and every LDS write
        const bool lo32 = lane < TT;
        const int t = lo32 ? lane : 0;
        double ar[TT];
#pragma unroll
        for (int j = 0; j < TT; ++j) ar[j] = Mt[t][j];
        double bt = betab[k0 & 1], ut = lo32 ? ub[t] : 0.0;
        static_for<0, TT - 1>([&](auto S) {
          constexpr int st = decltype(S)::value;  // global iteration k0 + st: apply v, then v'
          // p = A v over the live rows / columns (>= st), v^T p over the 32 lanes
          double p0 = 0.0, p1 = 0.0;
#pragma unroll
          for (int j = st; j < TT; ++j) {
            if ((j - st) & 1) p1 = fma(ar[j], ub[j], p1);
            else p0 = fma(ar[j], ub[j], p0);
          }
          const double p = (t >= st && lo32) ? p0 + p1 : 0.0;
          const double tot = xsum16(row16_sum(ut * p));
          const double Kc = bt * bt * tot * 0.5;
          const double wv = fma(bt, p, -(Kc * ut));
          const double g = fma(Kc, ut, -wv), mh = -(bt * ut);
          if (lo32) pt[t] = p;
          // A -= v w^T + w v^T: a_tj += mh p_j + g v_j (the p terms, then the v terms; the
          // broadcast reads phase by phase, not all hoisted: register pressure)
          asm volatile("" ::: "memory");
#pragma unroll
          for (int j = st; j < TT; ++j) ar[j] = fma(pt[j], mh, ar[j]);
          asm volatile("" ::: "memory");
#pragma unroll
          for (int j = st; j < TT; ++j) ar[j] = fma(ub[j], g, ar[j]);
          asm volatile("" ::: "memory");
          // the next reflector from column st of the updated matrix (global row r = k0 + 1 + st)
          const double xr = readlane_d(ar[st], st), x0 = readlane_d(ar[st], st + 1);
          const double tl = xsum16(row16_sum((t >= st + 2 && lo32) ? ar[st] * ar[st] : 0.0));
          double b2 = 0.0, v0 = x0, e2r = x0 * x0;
          if (tl > 0.0) {
            const double ss = fma(x0, x0, tl);
            double nrm;
            if (ss > 0x1p-900) {
              double rs = __builtin_amdgcn_rsq(ss);
              rs = rs * fma(-0.5 * ss, rs * rs, 1.5);
              nrm = ss * rs;
              nrm = fma(fma(-nrm, nrm, ss), 0.5 * rs, nrm);
            } else {
              nrm = sqrt(ss);
            }
            const double alpha = x0 > 0.0 ? -nrm : nrm;
            v0 = x0 - alpha;
            const double q = fma(v0, v0, tl);
            double rc = __builtin_amdgcn_rcp(q);
            rc = fma(fma(-q, rc, 1.0), rc, rc);
            rc = fma(fma(-q, rc, 1.0), rc, rc);
            b2 = 2.0 * rc;
            e2r = alpha * alpha;
          }
          ut = (t <= st || !lo32) ? 0.0 : (t == st + 1 ? v0 : ar[st]);
          bt = b2;
          if (lo32) ub[t] = ut;
          if (lane == 0) {
            dg[k0 + 1 + st] = xr;
            e2[k0 + 1 + st] = e2r;
          }
        });
        if (lane == TT - 1) dg[n - 1] = ar[TT - 1];  // (the last reflector only flips its sign)
      }
    } else if (tid == 0 && n >= 2) {
      dg[n - 1] = rowb[(n - 1) & 1][n - 1];
    }
  } else {
    // the last diagonal entry: row n-1 as its owners published it at the last step (or at the start)
    if (tid == 0 && n >= 2) dg[n - 1] = rowb[(n - 1) & 1][n - 1];
  }
  __syncthreads();
  // Gershgorin interval, scaling and 256-way multisection: as eigmin_reg
  int bnd_ex = 0;
  {
    double lo = INFINITY, hi = -INFINITY;
    if (tid < n) {
      double rr = 0.0;
      if (tid > 0) rr += sqrt(e2[tid - 1]);
      if (tid + 1 < n) rr += sqrt(e2[tid]);
      lo = dg[tid] - rr;
      hi = dg[tid] + rr;
    }
    if (w < 2) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o));
        hi = fmax(hi, __shfl_xor(hi, o));
      }
      if (lane == 0) {
        reinterpret_cast<double*>(masks)[2 * w] = lo;
        reinterpret_cast<double*>(masks)[2 * w + 1] = hi;
      }
    }
    __syncthreads();
    const double* m = reinterpret_cast<const double*>(masks);
    const double l = fmin(m[0], m[2]), h = fmax(m[1], m[3]);
    const double mag = fmax(fabs(l), fabs(h));
    const int ex = (mag > 0.0 && mag < INFINITY) ? __builtin_amdgcn_frexp_exp(mag) : 0;
    bnd_ex = ex;
    if (tid < 128) {
      sd[tid] = tid < n ? __builtin_ldexp(dg[tid], -ex) : 4.0;
      se[tid] = (tid >= 1 && tid < n) ? fmax(__builtin_ldexp(e2[tid - 1], -2 * ex), 0x1p-900) : 0.0;
    }
    if (tid == 0) {
      const double ls = __builtin_ldexp(l, -ex), hs = __builtin_ldexp(h, -ex);
      const double span = hs - ls;
      bnd[0] = ls - span * 1e-3 - 1e-300;
      bnd[1] = hs + span * 1e-3 + 1e-300;
    }
  }
  __syncthreads();
  double lo = bnd[0], hi = bnd[1];
  const int nr = (n + 7) & ~7;
  // 512-way on the 8 bulk waves (two per SIMD: the count is a latency-bound chain, so the second
  // wave per SIMD costs little), 6 rounds of 9 bits (2^-54 of the span): 3 us less than 256-way
  // on 4 waves in 7 rounds (DBG 64 keeps that, DBG 8 the two-ended count)
  constexpr int NCW = (DBG & 64) ? 4 : NWB;        // counting waves
  constexpr double NSIG = 64.0 * NCW + 1.0;
  for (int it = 0; it < ((DBG & 64) ? 7 : 6); ++it) {
    const double width = hi - lo;
    if (w < NCW) {
      const double sigma = lo + width * ((double)(tid + 1) / NSIG);
      const bool below = (DBG & 8) ? sturm_any_below2(sd, se, nr, sigma) : sturm_any_below(sd, se, nr, sigma);
      const unsigned long long mk = __ballot(below);
      if (lane == 0) masks[w] = mk;
    }
    __syncthreads();
    int f = -1;
    for (int q = 0; q < NCW && f < 0; ++q)
      if (masks[q]) f = q * 64 + __ffsll((long long)masks[q]) - 1;
    __syncthreads();
    if (f < 0) {
      lo = lo + width * ((NSIG - 1.0) / NSIG);
    } else {
      hi = lo + width * ((double)(f + 1) / NSIG);
      if (f > 0) lo = lo + width * ((double)f / NSIG);
    }
  }
  if (tid == 0) out[blockIdx.x] = __builtin_ldexp((lo + hi) * 0.5, bnd_ex + ex0);
#ifdef CLRSDP_EIGSPLIT_STAMPS
  ES_STAMP(7)
  if (lane == 0 && (chain || w == 4))
    for (int q = 0; q < 8; ++q)
      if ((chain && q < 3) || (!chain && q >= 3)) atomicAdd(&g_eigsplit_stamps[q], st_acc[q]);
#endif
#undef ES_STAMP
}

#ifdef CLRSDP_EIG_STAMPS
__device__ unsigned long long g_eig_stamps[8];
#define EIG_STAMP(slot)                                                     \
  if (tid == 0) {                                                           \
    unsigned long long t_ = __builtin_amdgcn_s_memtime();                   \
    atomicAdd(&g_eig_stamps[slot], t_ - t_prev);                           \
    t_prev = t_;                                                            \
  }
#else
#define EIG_STAMP(slot)
#endif
// Wave sum of a (multi-word) value by DPP and permlane swaps, limb by limb, with the word
// type's own addition at every step (commutative, so partner lanes agree): against the
// ds_bpermute butterfly of wave_sum, whose six dependent LDS-unit round trips per limb set the
// reflector's critical path in eigmin_lds.
template <int CTRL, class T>
__device__ inline T dpp_mw(const T& v) {
  T o;
  const double* a = reinterpret_cast<const double*>(&v);
  double* b = reinterpret_cast<double*>(&o);
#pragma unroll
  for (int q = 0; q < (int)(sizeof(T) / 8); ++q) b[q] = dpp_d<CTRL>(a[q]);
  return o;
}
__device__ inline double swap32_d(double x) {  // value of lane ^ 32
  const auto rl = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(x), false, false);
  const auto rh = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(x), false, false);
  const bool low = __lane_id() < 32;
  return low ? __hiloint2double(rh[1], rl[1]) : __hiloint2double(rh[0], rl[0]);
}
template <int SW, class T>
__device__ inline T swap_mw(const T& v) {
  T o;
  const double* a = reinterpret_cast<const double*>(&v);
  double* b = reinterpret_cast<double*>(&o);
#pragma unroll
  for (int q = 0; q < (int)(sizeof(T) / 8); ++q) b[q] = SW == 16 ? swap16_d(a[q]) : swap32_d(a[q]);
  return o;
}
template <class T>
__device__ inline T wave_sum_mw(T v) {
  v = v + dpp_mw<0xB1>(v);   // quad_perm [1,0,3,2]
  v = v + dpp_mw<0x4E>(v);   // quad_perm [2,3,0,1]
  v = v + dpp_mw<0x141>(v);  // row_half_mirror
  v = v + dpp_mw<0x140>(v);  // row_mirror
  v = v + swap_mw<16>(v);
  v = v + swap_mw<32>(v);
  return v;
}
// The same butterfly when only lane 0 needs the sum and only lanes 0..m-1 hold nonzero values:
// after level L lane 0 holds the sum of lanes 0..2^L - 1, so the levels past ceil(log2 m) would
// only add zeros (uniform branches on m).  eigmin_lds2's v^T p partials live on lanes 0-7 and
// its reflector norms on the first m = n - c - 1 lanes: half of the multi-word additions of
// those two sums are dropped from the per-column chain.
template <class T>
__device__ inline T lane0_sum_mw(T v, int m) {
  if (m > 1) v = v + dpp_mw<0xB1>(v);
  if (m > 2) v = v + dpp_mw<0x4E>(v);
  if (m > 4) v = v + dpp_mw<0x141>(v);
  if (m > 8) v = v + dpp_mw<0x140>(v);
  if (m > 16) v = v + swap_mw<16>(v);
  if (m > 32) v = v + swap_mw<32>(v);
  return v;
}

// (scale2, the exact power-of-two scaling of every limb: kernels.h)
// pow2_exp of a block from every thread's largest loaded magnitude (NW waves; red: NW doubles
// of LDS).  Its barrier also orders the load of the image before the reads that follow.
template <int NW>
__device__ __forceinline__ int load_scale_exp(double amax, double* __restrict__ red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  double mx = red[0];
#pragma unroll
  for (int q = 1; q < NW; ++q) mx = fmax(mx, red[q]);
  return pow2_exp(mx);
}
// The half-width word of a multi-word type and the rounding to it (the leading words of the
// non-overlapping representation).
template <class T> struct HalfWord;
template <> struct HalfWord<double> {
  using type = double;
  __device__ static double half(double v) { return v; }
};
template <> struct HalfWord<mw::dd> {
  using type = double;
  __device__ static double half(const mw::dd& v) { return v.hi; }
};
template <> struct HalfWord<mw::qd> {
  using type = mw::dd;
  __device__ static mw::dd half(const mw::qd& v) { return mw::dd(v.x[0], v.x[1]); }
};
// Multi-word "count >= 1" of the Sturm sequence (some eigenvalue of the tridiagonal below sigma),
// division-free as sturm_any_below: with p_0 = 1 the count is >= 1 iff some leading principal
// minor p_i = (d_i - sigma) p_{i-1} - e2_{i-1} p_{i-2} is negative (a zero minor is followed by a
// nonzero one of the sign opposite to its predecessor's, as the pivot form's q = 0 -> +tiny
// convention counts it; a zero last minor is not counted there either).  (p_{i-1}, p_i) is
// rescaled by the power of two of the larger every 4 rows (exact), so no minor overflows.  Per
// row two multi-word products and two differences, against a multi-word division in the pivot
// form (sturm_count), whose fp64 division sequences made the multi-word rounds of the
// multisection 56 % of eigmin_lds<dd>.
template <class T>
__device__ __forceinline__ bool sturm_any_below_mw(const T* __restrict__ dg, const T* __restrict__ e2, int n,
                                   const T& sigma) {
  T pm = T(0.0), pc = T(1.0);
  bool neg = false;
  // groups of 4 rows: the group's coefficients are read and d_i - sigma formed ahead of the
  // chain (LDS latency and the differences off the dependent path), then one rescale
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    T dv[4], fv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dv[u] = dg[i + u] - sigma;
      fv[u] = sel(i + u > 0, e2[i + u > 0 ? i + u - 1 : 0], T(0.0));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      T pn = dv[u] * pc - fv[u] * pm;
      // a zero minor followed by e2_i = 0 (a decoupled tridiagonal) would keep the recurrence
      // at zero and hide every later sign change: count it as negative (LAPACK's -pivmin),
      // as the fp64 count floors e2 at 2^-900
      if (Num<T>::hi(pn) == 0.0) pn = T(-__builtin_ldexp(fabs(Num<T>::hi(pc)), -300));
      neg = neg || (pn < T(0.0));
      pm = pc;
      pc = pn;
    }
    const double mx = fmax(fabs(Num<T>::hi(pc)), fabs(Num<T>::hi(pm)));
    if (mx > 0.0 && mx < INFINITY) {
      const int ex = __builtin_amdgcn_frexp_exp(mx);
      pc = scale2(pc, -ex);
      pm = scale2(pm, -ex);
    }
  }
  for (; i < n; ++i) {
    T pn = (dg[i] - sigma) * pc - sel(i > 0, e2[i > 0 ? i - 1 : 0], T(0.0)) * pm;
    if (Num<T>::hi(pn) == 0.0) pn = T(-__builtin_ldexp(fabs(Num<T>::hi(pc)), -300));
    neg = neg || (pn < T(0.0));
    pm = pc;
    pc = pn;
  }
  return neg;
}

// the multi-word count >= 1 tests (CLRSDP_EIG_PIVOT_COUNT: the pivot form, for A/B timing)
#ifdef CLRSDP_EIG_PIVOT_COUNT
#define ANY_BELOW(sg) (sturm_count(dg, e2, n, (sg)) >= 1)
#else
#define ANY_BELOW(sg) sturm_any_below_mw(dg, e2, n, (sg))
#endif
// The multisection phase of eigmin_lds / eigmin_lds2 (512 threads): lambda_min of the
// tridiagonal (dg, e2 = squared off-diagonals) in LDS to the word's precision, into
// out[blockIdx.x], times 2^ex (the input scaling of the caller, pow2_exp).  A is LDS scratch
// (>= 2n + 14 doubles), Wv one word of LDS scratch.
template <class T, bool NEWTON>
__device__ __forceinline__ void eig_multisection(const T* __restrict__ dg, const T* __restrict__ e2, int n,
                                 T* __restrict__ A, T* __restrict__ Wv, T* __restrict__ out, int ex) {
  constexpr int NT = 512, NW = 8;
  const int tid = threadIdx.x;
  if (n == 1) {
    if (tid == 0) out[blockIdx.x] = scale2(dg[0], ex);
    return;
  }
  // ---- multisection, 256-way on waves 0-3 (8 bits per round), in two phases:
  //  (1) fp64 on the leading limbs of the tridiagonal: Gershgorin bracket, 8 rounds;
  //  (2) multi-word, started from the fp64 eigenvalue +- delta, where delta bounds the effect of
  //      the rounding to fp64 (Weyl: |dlambda| <= ||dT|| <= ~3 eps64 ||T||) and of the fp64 Sturm
  //      counts (exact for a matrix perturbed by a few eps64 relative), with a wide margin.  The
  //      bracket is checked with two multi-word counts (no eigenvalue below it, one below its top)
  //      and replaced by the Gershgorin bracket if the check fails.  About half the multi-word
  //      rounds of a multisection from the Gershgorin bracket.
  // The matrix image in LDS is no longer needed: it holds the fp64 copy and the round masks.
  double* dgh = reinterpret_cast<double*>(A);
  double* e2h = dgh + n;
  double* bnd = e2h + n;  // [0,1] Gershgorin bracket, [2,3] multi-word start bracket, [4] ok
  unsigned long long* masks = reinterpret_cast<unsigned long long*>(bnd + 6);
  for (int i = tid; i < n; i += NT) {
    dgh[i] = Num<T>::hi(dg[i]);
    e2h[i] = Num<T>::hi(e2[i]);
  }
  __syncthreads();
  if (tid == 0) {
    double glo = 0.0, ghi = 0.0;
    for (int i = 0; i < n; ++i) {
      double r = 0.0;
      if (i > 0) r += sqrt(e2h[i - 1]);
      if (i + 1 < n) r += sqrt(e2h[i]);
      const double a = dgh[i] - r, b = dgh[i] + r;
      if (i == 0 || a < glo) glo = a;
      if (i == 0 || b > ghi) ghi = b;
    }
    // the leading limbs and the fp64 sqrt differ from the exact bounds by ~eps64 relative
    const double span = ghi - glo, mag = fmax(fabs(glo), fabs(ghi));
    bnd[0] = glo - span * 1e-3 - mag * 1e-12 - 1e-300;
    bnd[1] = ghi + span * 1e-3 + mag * 1e-12 + 1e-300;
  }
  __syncthreads();
  const int w = tid >> 6, lane = tid & 63;
  // one 512-way round: the first of the 512 interior points with a count >= 1 (every thread
  // gets the same answer); returns its index, or -1 if none
  auto first_hit = [&](bool hit) -> int {
    const unsigned long long mk = __ballot(hit);
    if (lane == 0) masks[w] = mk;
    __syncthreads();
    int f = -1;
    for (int q = 0; q < NW && f < 0; ++q)
      if (masks[q]) f = q * 64 + __ffsll((long long)masks[q]) - 1;
    __syncthreads();
    return f;
  };
  {
    // 8 rounds of 256 division-free counts on waves 0-3 (64 bits of the Gershgorin span)
    double lo = bnd[0], hi = bnd[1];
    for (int it = 0; it < 8; ++it) {
      const double width = hi - lo;
      bool hit = false;
      if (tid < 256) hit = sturm_any_below_mw(dgh, e2h, n, lo + width * ((double)(tid + 1) / 257.0));
      const int f = first_hit(hit);
      if (f < 0) {
        lo = lo + width * (256.0 / 257.0);
      } else {
        hi = lo + width * ((double)(f + 1) / 257.0);
        if (f > 0) lo = lo + width * ((double)f / 257.0);
      }
    }
    if (tid == 0) {
      const double c = 0.5 * (lo + hi);
      const double mag = fmax(fabs(bnd[0]), fabs(bnd[1]));
      const double delta = 64.0 * (double)n * 2.3e-16 * mag + (hi - lo) + 1e-300;
      bnd[2] = c - delta;
      bnd[3] = c + delta;
    }
  }
  __syncthreads();
  if constexpr (NEWTON && Num<T>::BITS > 60) {  // (multi-word words only)
    // (2') Newton on det(T - sigma I) from the fp64 centre.  (Before round 3 only at qd: at dd the
    // 11 parallel multisection rounds were as fast as the sequential chain of divisions.)  With the pivots of
    // T - sigma I = L D L^T, q_i = (d_i - sigma) - e2_{i-1} / q_{i-1}, and s_i = dq_i/dsigma =
    // -1 + e2_{i-1} s_{i-1} / q_{i-1}^2, the Newton step is 1 / sum_i s_i / q_i.  It converges
    // quadratically from the fp64 estimate (3 steps for a simple eigenvalue, a 4th confirms).
    // The result is accepted only if it converged AND two multi-word Sturm counts bracket it
    // (no eigenvalue below sigma - delta, one at most sigma + delta, delta = 2^(12-BITS)
    // magnitudes); otherwise the multisection below runs as before.
    // Division-free (round 3): the step is p_n / p_n' with the three-term recurrence of the
    // leading principal minors and of their derivatives, p_i = (d_i - s) p_{i-1} - e2_{i-1}
    // p_{i-2}, p_i' = (d_i - s) p_{i-1}' - p_{i-1} - e2_{i-1} p_{i-2}', the four values rescaled
    // by one power of two per row (exact, the ratio is unchanged): four multi-word products per
    // row and one division per step, against a division and three products per row.  A step
    // below 2^(-BITS/2 - 24) of the magnitude is the last one (quadratic convergence puts the
    // next correction far below the word); the two Sturm counts below accept the result.
    // Mixed precision (round 3, late): the derivative recurrence runs in the half-width word H
    // (dd for qd, fp64 for dd).  The step p/p' is a correction of the current error e, so a
    // relative error eta of p' only adds eta * e to the next error (quadratic convergence becomes
    // e^2 + eta e); p itself stays at full width.  At qd the first steps run entirely at dd
    // (from the fp64 centre to ~2^-100 of the magnitude), so only the last two steps carry qd
    // products, two per row instead of four.  The two Sturm counts below still decide.
    using H = typename HalfWord<T>::type;
    T* nres = Wv;  // free after the reduction: [0] = sigma
    const double mag = fmax(fabs(bnd[0]), fabs(bnd[1]));
    if (tid == 0) {
      T s = T(0.5 * (bnd[2] + bnd[3]));
      if constexpr (Num<T>::BITS > 150) {  // qd: dd pre-iterations on the dd-rounded tridiagonal
        H sh = H(0.5 * (bnd[2] + bnd[3]));
        const double tolh = ldexp(mag, -(Num<H>::BITS / 2 + 24)) + 1e-300;
        for (int it = 0; it < 3; ++it) {
          H pm = H(1.0), pc = HalfWord<T>::half(dg[0]) - sh, dm = H(0.0), dc = H(-1.0);
          for (int i = 1; i < n; ++i) {
            const H t = HalfWord<T>::half(dg[i]) - sh, e = HalfWord<T>::half(e2[i - 1]);
            const H pn = t * pc - e * pm;
            const H dn = (t * dc - pc) - e * dm;
            pm = pc;
            pc = pn;
            dm = dc;
            dc = dn;
            const double mx = fmax(fmax(fabs(Num<H>::hi(pc)), fabs(Num<H>::hi(pm))),
                                   fmax(fabs(Num<H>::hi(dc)), fabs(Num<H>::hi(dm))));
            if (mx > 0.0 && mx < INFINITY) {
              const int ex = __builtin_amdgcn_frexp_exp(mx);
              pc = scale2(pc, -ex);
              pm = scale2(pm, -ex);
              dc = scale2(dc, -ex);
              dm = scale2(dm, -ex);
            }
          }
          if (Num<H>::hi(dc) == 0.0) break;
          const H step = pc / dc;
          const double as = fabs(Num<H>::hi(step));
          if (!(as == as)) break;  // NaN: keep the last finite estimate
          sh = sh - step;
          if (as <= tolh) break;
        }
        s = T(sh);
      }
      const double tol = ldexp(mag, -(Num<T>::BITS / 2 + 24)) + 1e-300;
      int conv = 0;
      for (int it = 0; it < 4; ++it) {
        T pm = T(1.0), pc = dg[0] - s;
        H dm = H(0.0), dc = H(-1.0);
        for (int i = 1; i < n; ++i) {
          const T t = dg[i] - s;
          const T pn = t * pc - e2[i - 1] * pm;
          const H dn = (HalfWord<T>::half(t) * dc - HalfWord<T>::half(pc)) -
                       HalfWord<T>::half(e2[i - 1]) * dm;
          pm = pc;
          pc = pn;
          dm = dc;
          dc = dn;
          const double mx = fmax(fmax(fabs(Num<T>::hi(pc)), fabs(Num<T>::hi(pm))),
                                 fmax(fabs(Num<H>::hi(dc)), fabs(Num<H>::hi(dm))));
          if (mx > 0.0 && mx < INFINITY) {
            const int ex = __builtin_amdgcn_frexp_exp(mx);
            pc = scale2(pc, -ex);
            pm = scale2(pm, -ex);
            dc = scale2(dc, -ex);
            dm = scale2(dm, -ex);
          }
        }
        if (Num<H>::hi(dc) == 0.0) break;
        const T step = pc / T(dc);
        s = s - step;
        const double as = fabs(Num<T>::hi(step));
        if (!(as == as)) break;  // NaN: leave conv = 0
        if (as <= tol) { conv = 1; break; }
      }
      nres[0] = s;
      masks[2] = (unsigned long long)conv;
    }
    __syncthreads();
    const T s = nres[0];
    const T dl = T(ldexp(mag, 12 - Num<T>::BITS) + 1e-300);
    int c = 0;
    if (tid == 0) c = masks[2] && !ANY_BELOW(s - dl);
    if (tid == 64) c = ANY_BELOW(s + dl);
    __syncthreads();
    if (tid == 0 || tid == 64) masks[tid >> 6] = (unsigned long long)c;
    __syncthreads();
    const bool ok = masks[0] && masks[1];
    __syncthreads();
    if (ok) {
      if (tid == 0) out[blockIdx.x] = scale2(s, ex);
      return;
    }
  }
  T lo = T(bnd[2]), hi = T(bnd[3]);
  // check the start bracket at full width: count(lo) == 0 and count(hi) >= 1
  {
    int c = 0;
    if (tid == 0) c = !ANY_BELOW(lo);
    if (tid == 64) c = ANY_BELOW(hi);
    if (tid == 0 || tid == 64) masks[tid >> 6] = (unsigned long long)c;
    __syncthreads();
    const bool ok = masks[0] && masks[1];
    __syncthreads();
    if (!ok) {
      lo = T(bnd[0]);
      hi = T(bnd[1]);
    }
    // rounds to shrink the bracket to ~2^-BITS of the spectrum's magnitude.  The multi-word
    // counts are VALU-issue bound, so they run 256-way on waves 0-3 (one wave per SIMD: 8 bits
    // per round) rather than 512-way on two waves per SIMD (9 bits per round at twice the issue)
#ifdef CLRSDP_EIG_MW512
    constexpr int MS = 512, MB = 9;
#else
    constexpr int MS = 256, MB = 8;
#endif
    constexpr double MD = MS + 1.0;
    // rounds to take the bracket below 2^-(BITS+2) of the magnitude (from its actual width:
    // the checked fp64 start bracket is ~64 n eps64 wide, so about 40 of the bits are known)
    int rounds = Num<T>::BITS / MB + 3;
    {
      const double wd = Num<T>::hi(hi - lo);
      const double mag = fmax(fabs(bnd[0]), fabs(bnd[1]));
      const double tgt = ldexp(mag, -(Num<T>::BITS + 2)) + 1e-300;
      if (wd > 0.0 && wd < INFINITY)
        rounds = min(rounds, max(1, (int)ceil(log2(wd / tgt) / (double)MB) + 1));
    }
    for (int it = 0; it < rounds; ++it) {
      const T width = hi - lo;
      bool hit = false;
      if (tid < MS) {  // wave-uniform
        const T sigma = lo + width * T((double)(tid + 1) / MD);
        hit = ANY_BELOW(sigma);
      }
      const int f = first_hit(hit);
      if (f < 0) {
        lo = lo + width * T((double)MS / MD);
      } else {
        hi = lo + width * T((double)(f + 1) / MD);
        if (f > 0) lo = lo + width * T((double)f / MD);
      }
    }
  }
  if (tid == 0) out[blockIdx.x] = scale2((lo + hi) * T(0.5), ex);
}

template <class T, bool NEWTON = true>
__global__ __launch_bounds__(512) void eigmin_lds(const MatDesc<T>* __restrict__ descs,
                                                  T* __restrict__ out) {
#ifdef CLRSDP_EIG_STAMPS
  unsigned long long t_prev = __builtin_amdgcn_s_memtime();
#endif
  constexpr int NT = 512, NW = 8;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const MatDesc<T> d = descs[blockIdx.x];
  const int n = d.n, tid = threadIdx.x;
  // rows per pass and column classes of the matrix-vector product and the rank-2 update: every
  // wave holds rows when n <= 64 (64 rows x 8 classes), else 128 rows x 4 classes
  const int RW = n <= 64 ? 64 : 128, NC = NT / RW;
  T* A = reinterpret_cast<T*>(smem_raw);  // n x n
  T* v = A + (size_t)n * n;               // n
  T* p = v + n;                            // NC * n partials (eig_lds_bytes)
  T* dg = p + NC * n;                      // n
  T* e2 = dg + n;                          // n
  T* Wv = e2 + n;        // w vector (n)            -- carved after e2
  T* scal = Wv + n;      // [0] = beta, [1] = tail flag
  T* redw = scal + 4;    // NW partials of v^T A' v
  // coalesced load, then symmetrise and scale in LDS: A = (A + A^T) / 2^(ex + 1) (pow2_exp)
  double amax = 0.0;
  for (int j = tid >> 6; j < n; j += NT / 64)
    for (int i = tid & 63; i < n; i += 64) {
      // (the leading limb read back from the image: a local copy of the word kept a quad-double
      // in scratch)
      A[i + (size_t)j * n] = d.A[i + (size_t)j * d.lda];
      amax = fmax(amax, fabs(Num<T>::hi(A[i + (size_t)j * n])));
    }
  const int ex = load_scale_exp<NW>(amax, reinterpret_cast<double*>(redw));
  for (int j = tid >> 6; j < n; j += NT / 64)
    for (int i = tid & 63; i <= j; i += 64) {
      const T sv = (scale2(A[i + (size_t)j * n], -ex) + scale2(A[j + (size_t)i * n], -ex)) * T(0.5);
      A[i + (size_t)j * n] = sv;
      A[j + (size_t)i * n] = sv;
    }
  __syncthreads();
  for (int k = 0; k + 2 < n; ++k) {
    const int m = n - k - 1;
    T* Ak = A + (k + 1) + (size_t)(k + 1) * n;  // trailing m x m, ld n
    // ---- (A) wave 0: reflector of column k
    if (tid < 64) {
      T s = T(0.0);
      for (int i = tid; i < m; i += 64) {
        const T xi = A[(k + 1 + i) + (size_t)k * n];
        v[i] = xi;
        s += xi * xi;
      }
      s = wave_sum_mw(s);
      const T x0 = A[(k + 1) + (size_t)k * n];
      const T tail = s - x0 * x0;
      if (tid == 0) {
        dg[k] = A[k + (size_t)k * n];
        if (!(tail > T(0.0))) {
          e2[k] = x0 * x0;
          scal[0] = T(0.0);  // beta = 0: no reflection
        } else {
          T nrm, rnrm;
          pivot_sqrt(s, nrm, rnrm);  // (dd: off the IEEE sqrt/division sequences)
          const T alpha = sel(x0 > T(0.0), -nrm, nrm);
          const T v0 = x0 - alpha;
          e2[k] = alpha * alpha;
          v[0] = v0;
          scal[0] = recip_fast(tail + v0 * v0) * T(2.0);
        }
      }
    }
    __syncthreads();
    EIG_STAMP(0)
    const T beta = scal[0];
    if (beta == T(0.0)) continue;  // uniform: nothing to update
    // ---- (B) partial rows of A'v (NC column classes) and v^T A' v
    const int ri = tid & (RW - 1), cq = tid / RW;
    T vav = T(0.0);
    for (int ii = ri; ii < m; ii += RW) {
      T a0 = T(0.0), a1 = T(0.0), a2 = T(0.0), a3 = T(0.0);
      int j = cq;
      for (; j + 3 * NC < m; j += 4 * NC) {
        a0 += Ak[ii + (size_t)j * n] * v[j];
        a1 += Ak[ii + (size_t)(j + NC) * n] * v[j + NC];
        a2 += Ak[ii + (size_t)(j + 2 * NC) * n] * v[j + 2 * NC];
        a3 += Ak[ii + (size_t)(j + 3 * NC) * n] * v[j + 3 * NC];
      }
      for (; j < m; j += NC) a0 += Ak[ii + (size_t)j * n] * v[j];
      const T part = (a0 + a1) + (a2 + a3);
      p[cq * n + ii] = part;
      vav += part * v[ii];
    }
    EIG_STAMP(1)
    vav = wave_sum_mw(vav);
    if ((tid & 63) == 0) redw[tid >> 6] = vav;
    __syncthreads();
    EIG_STAMP(2)
    // ---- (C) w = beta A'v - K v,  K = beta^2 v^T A' v / 2
    {
      // pairwise (three dependent multi-word additions instead of seven)
      const T tot = ((redw[0] + redw[1]) + (redw[2] + redw[3])) + ((redw[4] + redw[5]) + (redw[6] + redw[7]));
      const T Kc = beta * beta * tot * T(0.5);
      for (int i = tid; i < m; i += NT) {
        T ps = (p[i] + p[n + i]) + (p[2 * n + i] + p[3 * n + i]);
        if (NC == 8) ps = ps + ((p[4 * n + i] + p[5 * n + i]) + (p[6 * n + i] + p[7 * n + i]));
        Wv[i] = ps * beta - Kc * v[i];
      }
    }
    __syncthreads();
    EIG_STAMP(3)
    // ---- (D) A' -= v w^T + w v^T
    for (int ii = ri; ii < m; ii += RW) {
      const T vi = v[ii], wi = Wv[ii];
      int j = cq;
      for (; j + 3 * NC < m; j += 4 * NC) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          T* a = Ak + ii + (size_t)(j + u * NC) * n;
          *a = *a - (vi * Wv[j + u * NC] + wi * v[j + u * NC]);
        }
      }
      for (; j < m; j += NC) {
        T* a = Ak + ii + (size_t)j * n;
        *a = *a - (vi * Wv[j] + wi * v[j]);
      }
    }
    __syncthreads();
    EIG_STAMP(4)
  }
  EIG_STAMP(5)
  if (tid == 0) {
    if (n >= 2) {
      dg[n - 2] = A[(n - 2) + (size_t)(n - 2) * n];
      dg[n - 1] = A[(n - 1) + (size_t)(n - 1) * n];
      const T e = A[(n - 1) + (size_t)(n - 2) * n];
      e2[n - 2] = e * e;
    } else {
      dg[0] = A[0];
    }
  }
  __syncthreads();
  eig_multisection<T, NEWTON>(dg, e2, n, A, Wv, out, ex);
  EIG_STAMP(6)
}

// ------------------------------------------------------------------------------------------
// eigmin_lds2: the Householder tridiagonalisation of eigmin_lds with two barriers per column
// instead of four, and the next reflector off the critical path.  The matrix is in LDS with a
// padded leading dimension (ld = 16 ceil(n/16) + 8, so the 16 lanes of an LDS pass hit distinct
// banks); thread (wave w, lane r + 8 c) owns row 64 q + 8 w + r (every pass q) and the column
// class j = c mod 8.  Per column k (trailing block k+1.., reflector v, beta):
//   (B) p_i = (A v)_i: the row's 8 class partials summed by DPP / permlane swaps inside the wave,
//       p -> LDS, the per-wave parts of v^T p -> LDS                              -- barrier
//   (D) with K = beta^2 v^T p / 2, g_i = beta p_i - 2K v_i and h_i = beta v_i (the row's own
//       values): a_ij -= h_i p_j + g_i v_j for every j > k of the thread's class (LDS reads of
//       p_j, v_j only; no w vector, no third barrier).  Column k+1 is skipped there: wave 0
//       forms its updated entries in registers and builds the next reflector from them (multi-
//       word norm, rsqrt pivot, reciprocal) while the other waves update     -- barrier
// The rows/columns <= k+1 are never read again, so column k+1 is not written back.
// ------------------------------------------------------------------------------------------
template <class T> __host__ __device__ constexpr int eig2_ld(int n) { return ((n + 15) / 16) * 16 + 8; }
template <class T> size_t eig2_lds_bytes(int n) {
  // A (n x ld), v (2 x ld), p (ld), dg, e2, scal (4), redw (2 x 8), + the tail's fp64 scratch
  return sizeof(T) * ((size_t)n * eig2_ld<T>(n) + 3 * (size_t)eig2_ld<T>(n) + 2 * (size_t)n + 4 + 16) + 64;
}
// The tridiagonalisation loop of eigmin_lds2 on the symmetric image A (n x ld in LDS, n >= 2,
// 512 threads): dg, e2 (and the last diagonal entry) when it returns.  KEEPV (fp64, eigmin_mx)
// also keeps every reflector: v_c in column c of V (n x n, rows c+1..n-1), beta_c in bet[c] and
// the signed off-diagonal T(c+1, c) in eo[c], so that A = Q T Q^T with Q = H_0 H_1 ... H_{n-2}.
template <class T, bool KEEPV>
__device__ __forceinline__ void tridiag_lds2(T* __restrict__ A, int ld, int n, T* __restrict__ vb,
                                             T* __restrict__ p, T* __restrict__ dg,
                                             T* __restrict__ e2, T* __restrict__ scal,
                                             T* __restrict__ redw, T* __restrict__ V,
                                             T* __restrict__ bet, T* __restrict__ eo) {
  // column slots per lane (j = cls + 8 t) and rows per lane in the reflector: a quad-double
  // image fits LDS only for n <= 64 (the launch checks it), so qd carries 8 slots and one row,
  // which keeps its per-lane words out of scratch
  constexpr int NSL = sizeof(T) > 16 ? 8 : 16, NH = sizeof(T) > 16 ? 1 : 2;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 7, cls = lane >> 3;
  const int npass = (n + 63) / 64;
  // reflector of column c from its entries x_i = col[i] (i > c; lane l holds rows c+1+l and
  // c+65+l), by wave 0: v into vb[c & 1], beta into scal[c & 1], dg[c] = diag, e2[c]
  auto reflector = [&](int c, const T (&x)[NH], const T& diag) {
    T s = T(0.0);
#pragma unroll
    for (int h = 0; h < NH; ++h) s += x[h] * x[h];
    s = lane0_sum_mw(s, n - c - 1);  // (only lane 0 uses s: beta, v0, e2[c])
    const T x0 = x[0];  // row c+1 (lane 0 is the only lane that uses x0, s and tail)
    const T tail = s - x0 * x0;
    T* v = vb + (c & 1) * ld;
    T beta = T(0.0), v0 = x0, e2c = x0 * x0, offd = x0;
    if (tail > T(0.0)) {
      T nrm, rnrm;
      if constexpr (std::is_same<T, double>::value) {  // (eigmin_mx) as eigmin_split's reflector
        if (s > 0x1p-900) {
          double rs = __builtin_amdgcn_rsq(s);
          rs = rs * fma(-0.5 * s, rs * rs, 1.5);
          nrm = s * rs;
          nrm = fma(fma(-nrm, nrm, s), 0.5 * rs, nrm);
        } else {
          nrm = sqrt(s);
        }
      } else {
        pivot_sqrt(s, nrm, rnrm);
      }
      const T alpha = sel(x0 > T(0.0), -nrm, nrm);
      v0 = x0 - alpha;
      e2c = alpha * alpha;
      offd = alpha;
      if constexpr (std::is_same<T, double>::value) {
        const double q = fma(v0, v0, tail);
        double rc = __builtin_amdgcn_rcp(q);
        rc = fma(fma(-q, rc, 1.0), rc, rc);
        rc = fma(fma(-q, rc, 1.0), rc, rc);
        beta = 2.0 * rc;
      } else {
        beta = recip_fast(tail + v0 * v0) * T(2.0);
      }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int i = c + 1 + lane + 64 * h;
      if (i < n) {
        const T vi = sel(i == c + 1, v0, x[h]);
        v[i] = vi;
        if constexpr (KEEPV) V[i + (size_t)c * n] = vi;
      }
    }
    if (lane < c + 1 && lane < ld) v[lane] = T(0.0);
    if (NH > 1 && lane + 64 < c + 1) v[lane + 64] = T(0.0);
    if (lane == 0) {
      dg[c] = diag;
      e2[c] = e2c;
      scal[c & 1] = beta;
      if constexpr (KEEPV) {
        bet[c] = beta;
        eo[c] = offd;
      }
    }
  };
  if (w == 0) {  // the reflector of column 0 from the input
    T x[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const int i = 1 + lane + 64 * h;
      x[h] = T(0.0);
      if (i < n) x[h] = A[i];
    }
    reflector(0, x, A[0]);
  }
  __syncthreads();
  for (int k = 0; k + 2 < n; ++k) {
    const T* v = vb + (k & 1) * ld;
    const T beta = scal[k & 1];
    // ---- (B) p = A' v on the trailing block (rows and columns > k)
    T vp = T(0.0);
    for (int q = 0; q < npass; ++q) {
      const int i = 64 * q + 8 * w + r;
      // the class's columns j = cls + 8 t > k, t < 16 (n <= 128): compile-time slots, so the
      // independent multi-word products interleave (a runtime loop serialised their chains)
      T acc[4] = {T(0.0), T(0.0), T(0.0), T(0.0)};
      if (i > k && i < n) {
#pragma unroll
        for (int t = 0; t < NSL; ++t) {
          const int j = cls + 8 * t;
          if (j > k && j < n) acc[t & 3] += A[i + (size_t)j * ld] * v[j];
        }
      }
      T pi = (acc[0] + acc[1]) + (acc[2] + acc[3]);
      pi = pi + dpp_mw<0x128>(pi);   // row_ror:8  -> classes c, c^1
      pi = pi + swap_mw<16>(pi);     // classes c ^ 2
      pi = pi + swap_mw<32>(pi);     // classes c ^ 4
      if (cls == 0 && i < n) {
        p[i] = sel(i > k, pi, T(0.0));
        if (i > k) vp += v[i] * pi;
      }
    }
    vp = lane0_sum_mw(vp, 8);  // (nonzero on the class-0 lanes 0-7 only)
    if (lane == 0) redw[(k & 1) * 8 + w] = vp;
    __syncthreads();
    // ---- (D) A' -= v w^T + w v^T on rows/columns > k+1; wave 0: column k+1 and its reflector
    const T* rw = redw + (k & 1) * 8;
    const T tot = ((rw[0] + rw[1]) + (rw[2] + rw[3])) + ((rw[4] + rw[5]) + (rw[6] + rw[7]));
    const T K2 = beta * beta * tot;  // 2K
    const int c1 = k + 1;
    const T pc = p[c1], vc = v[c1];
    if (w == 0) {  // column c1 (rows > c1) and its diagonal, updated in registers
      T x[NH];
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        const int i = c1 + 1 + lane + 64 * h;
        x[h] = T(0.0);
        if (i < n) {
          const T pi = p[i], vi = v[i];
          const T gi = beta * pi - K2 * vi, hi = beta * vi;
          x[h] = A[i + (size_t)c1 * ld] - (hi * pc + gi * vc);
        }
      }
      const T gc = beta * pc - K2 * vc, hc = beta * vc;
      const T diag = A[c1 + (size_t)c1 * ld] - (hc * pc + gc * vc);
      reflector(c1, x, diag);
    }
    for (int q = 0; q < npass; ++q) {
      const int i = 64 * q + 8 * w + r;
      if (i > c1 && i < n) {
        const T pi = p[i], vi = v[i];
        const T gi = beta * pi - K2 * vi, hi = beta * vi;
        // groups of 4 slots: all loads, then the 4 independent updates, then the stores (the
        // stores may alias later loads of the same LDS image, which would order every chain)
#pragma unroll
        for (int t0 = 0; t0 < NSL; t0 += 4) {
          if (cls + 8 * t0 >= n) break;  // (this lane has no live slot from t0 on)
          T av[4], pj[4], vj[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int j = cls + 8 * (t0 + u);
            const int jc = j < n ? j : n - 1;
            av[u] = A[i + (size_t)jc * ld];
            pj[u] = p[jc];
            vj[u] = v[jc];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) av[u] = av[u] - (hi * pj[u] + gi * vj[u]);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int j = cls + 8 * (t0 + u);
            if (j > c1 && j < n) A[i + (size_t)j * ld] = av[u];
          }
        }
      }
    }
    __syncthreads();
  }
  // the last diagonal entry (updated by the last step's (D))
  if (tid == 0) dg[n - 1] = A[(n - 1) + (size_t)(n - 1) * ld];
  __syncthreads();
}

// DBG (timing experiments, tools/micro/eig2_mw.hip): 1 = stop after the tridiagonalisation
template <class T, int DBG>
__device__ __forceinline__ void eigmin_lds2_dev(const MatDesc<T>& d, T* __restrict__ out,
                                                char* __restrict__ smem_raw) {
  constexpr int NT = 512;
  const int n = d.n, tid = threadIdx.x, lane = tid & 63;
  const int ld = eig2_ld<T>(n);
  T* A = reinterpret_cast<T*>(smem_raw);      // n x ld, column-major
  T* vb = A + (size_t)n * ld;                 // 2 x ld: v of step k in vb[(k & 1) * ld]
  T* p = vb + 2 * ld;                          // ld
  T* dg = p + ld;                              // n
  T* e2 = dg + n;                              // n
  T* scal = e2 + n;                            // [0..1] beta of the two v buffers
  T* redw = scal + 4;                          // 2 x 8 per-wave parts of v^T p
  // coalesced load, then symmetrise and scale: A = (A + A^T) / 2^(ex + 1) (pow2_exp)
  double amax = 0.0;
  for (int j = tid >> 6; j < n; j += NT / 64)
    for (int i = lane; i < n; i += 64) {
      A[i + (size_t)j * ld] = d.A[i + (size_t)j * d.lda];
      amax = fmax(amax, fabs(Num<T>::hi(A[i + (size_t)j * ld])));
    }
  const int ex = load_scale_exp<NT / 64>(amax, reinterpret_cast<double*>(redw));
  for (int j = tid >> 6; j < n; j += NT / 64)
    for (int i = lane; i <= j; i += 64) {
      const T sv = (scale2(A[i + (size_t)j * ld], -ex) + scale2(A[j + (size_t)i * ld], -ex)) * T(0.5);
      A[i + (size_t)j * ld] = sv;
      A[j + (size_t)i * ld] = sv;
    }
  __syncthreads();
  if (n == 1) {
    if (tid == 0) out[blockIdx.x] = scale2(A[0], ex);
    return;
  }
  tridiag_lds2<T, false>(A, ld, n, vb, p, dg, e2, scal, redw, nullptr, nullptr, nullptr);
  if constexpr (DBG == 1) {
    if (tid == 0) out[blockIdx.x] = dg[n - 1] + e2[0];
    return;
  }
  eig_multisection<T, true>(dg, e2, n, A, p, out, ex);
}

// redo (eigmin_mx's fallback launch): only the blocks with redo[block] != 0
template <class T, int DBG = 0>
__global__ __launch_bounds__(512) void eigmin_lds2(const MatDesc<T>* __restrict__ descs,
                                                   T* __restrict__ out,
                                                   const int* __restrict__ redo = nullptr) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  if (redo && redo[blockIdx.x] == 0) return;
  eigmin_lds2_dev<T, DBG>(descs[blockIdx.x], out, smem_raw);
}
#undef ANY_BELOW

// ------------------------------------------------------------------------------------------
// eigblk_*: lambda_min of blocks past the LDS kernels, tridiagonalised across workgroups
// (CLRSDP_EIG_BLK=1, in place of the one-CU eigmin_batched).  A right-looking Householder
// tridiagonalisation with one launch per column; nothing is handed over between workgroups
// inside a launch, everything crosses at kernel boundaries, and no sum uses an atomic.
//   eigblk_amax   per strip of R rows, the largest leading-limb magnitude (one partial each)
//   eigblk_sym    ex = pow2_exp(max of the partials); A = (A + A^T) / 2^(ex + 1); clears the
//                 state buffer that launch 0 reads
//   eigblk_col    launch k.  State on entry, in the per-matrix scratch (two buffers, ping-pong):
//                 v_{k-1}, p_{k-1} = beta A' v and beta_{k-1}; A is updated through reflector
//                 k - 2.  Every workgroup (one wave) forms, redundantly and by the same
//                 instruction sequence, w = p - (beta p^T v / 2) v, the true column k
//                 A[:, k] - v w_k - w v_k, and from it dg[k], e2[k], v_k and beta_k
//                 (eigmin_batched's tail > 0 rule: beta = 0, v = 0 for a column that is already
//                 tridiagonal).  Then it owns R rows of the trailing matrix and all their columns
//                 >= k + 1: one thread per row applies the pending rank-2 update, stores the entry
//                 and accumulates A' v_k in ascending column order, so p_k[i] is one thread's sum
//                 and lambda_min does not depend on R, on the grid or on the rest of the batch.
//                 Column k itself is outside the region the launch writes.
//   eigblk_sturm  one workgroup per matrix: the pending rank-2 update of the last 2 x 2, then the
//                 multisection phase of eigmin_lds / eigmin_lds2 on (dg, e2).
// A matrix with n <= k + 2 leaves launch k at once (batches mix sizes).
// Scratch per matrix, in words of T: [v (n), p (n), beta] twice, dg (n), e2 (n).
// ------------------------------------------------------------------------------------------
template <class T>
struct EigBlkDesc {
  T* A;          // n x n, leading dimension lda (destroyed)
  T* ws;         // eigblk_ws_words(n) words
  double* amax;  // one partial per strip of the prepass
  int n, lda;
};
constexpr size_t eigblk_ws_words(int n) { return 6 * (size_t)n + 2; }
template <class T>
__device__ __forceinline__ T* eigblk_state(const EigBlkDesc<T>& d, int q) {
  return d.ws + (size_t)q * (2 * (size_t)d.n + 1);
}
// eigblk_col's dynamic LDS: v_k and w, indexed by row
template <class T> constexpr size_t eigblk_col_lds(int n) { return 2 * sizeof(T) * (size_t)n; }
// eigblk_sturm's: the multisection's scratch (2n + 14 doubles), one word, and the tridiagonal
// when it is kept on chip
constexpr size_t eigblk_sturm_scr(int n) { return ((2 * (size_t)n + 14) * 8 + 31) / 32 * 32; }
template <class T> constexpr size_t eigblk_sturm_lds(int n, bool tri) {
  return eigblk_sturm_scr(n) + sizeof(T) * (1 + (tri ? 2 * (size_t)n : 0));
}

template <class T, int R>
__global__ __launch_bounds__(64) void eigblk_amax(const EigBlkDesc<T>* __restrict__ descs,
                                                  const int* __restrict__ redo = nullptr) {
  if (redo && redo[blockIdx.y] == 0) return;  // (a fallback launch: the flagged blocks only)
  const EigBlkDesc<T> d = descs[blockIdx.y];
  const int n = d.n, lane = threadIdx.x, i = blockIdx.x * R + lane;
  if ((int)blockIdx.x * R >= n) return;
  double amax = 0.0;
  if (lane < R && i < n)
    for (int j = 0; j < n; ++j) amax = fmax(amax, fabs(Num<T>::hi(d.A[i + (size_t)j * d.lda])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
  if (lane == 0) d.amax[blockIdx.x] = amax;
}

// pow2_exp of the block from the strip partials (a max: the order does not matter)
template <class T>
__device__ __forceinline__ int eigblk_exp(const EigBlkDesc<T>& d, int R) {
  double mx = 0.0;
  for (int s = 0; s * R < d.n; ++s) mx = fmax(mx, d.amax[s]);
  return pow2_exp(mx);
}

template <class T, int R>
__global__ __launch_bounds__(64) void eigblk_sym(const EigBlkDesc<T>* __restrict__ descs,
                                                 const int* __restrict__ redo = nullptr) {
  if (redo && redo[blockIdx.y] == 0) return;
  const EigBlkDesc<T> d = descs[blockIdx.y];
  const int n = d.n, lda = d.lda, lane = threadIdx.x, i = blockIdx.x * R + lane;
  if ((int)blockIdx.x * R >= n) return;
  const int ex = eigblk_exp(d, R);
  if (lane >= R || i >= n) return;
  // the thread of row i owns the pairs (i, j), (j, i) with j < i and the diagonal entry
  T* A = d.A;
  for (int j = 0; j < i; ++j) {
    const T s = (scale2(A[i + (size_t)j * lda], -ex) + scale2(A[j + (size_t)i * lda], -ex)) * T(0.5);
    A[i + (size_t)j * lda] = s;
    A[j + (size_t)i * lda] = s;
  }
  A[i + (size_t)i * lda] = scale2(A[i + (size_t)i * lda], -ex);
  // no reflector is pending when launch 0 (and the last launch of an n <= 2 block) reads buffer 0
  T* st = eigblk_state(d, 0);
  st[i] = T(0.0);
  st[n + i] = T(0.0);
  if (i == 0) st[2 * n] = T(0.0);
}

template <class T, int R>
__global__ __launch_bounds__(64) void eigblk_col(const EigBlkDesc<T>* __restrict__ descs, int k,
                                                 const int* __restrict__ redo = nullptr) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  if (redo && redo[blockIdx.y] == 0) return;
  const EigBlkDesc<T> d = descs[blockIdx.y];
  const int n = d.n, lda = d.lda, lane = threadIdx.x;
  if (n <= k + 2) return;
  const int i = k + 1 + (int)blockIdx.x * R + lane;  // the row of this thread
  if (i - lane >= n) return;
  T* vk = reinterpret_cast<T*>(smem_raw);  // n   reflector k, by row
  T* w = vk + n;                           // n   w of reflector k - 1, by row
  const T* __restrict__ vp = eigblk_state(d, k & 1);  // v_{k-1}, rows k .. n - 1
  const T* __restrict__ pp = vp + n;                   // p_{k-1}
  T* nx = eigblk_state(d, (k + 1) & 1);
  T* A = d.A;
  // ---- 1. w = p - (beta p^T v / 2) v, every workgroup alike
  const T betap = vp[2 * n];
  T pv = T(0.0);
  for (int r = k + lane; r < n; r += 64) pv += pp[r] * vp[r];
  pv = wave_sum_mw(pv);
  const T Kc = betap * pv * T(0.5);
  for (int r = k + lane; r < n; r += 64) w[r] = pp[r] - Kc * vp[r];
  __syncthreads();
  // ---- 2. the true column k, its diagonal entry and reflector
  const T vpk = vp[k], wk = w[k];
  T s = T(0.0);
  for (int r = k + 1 + lane; r < n; r += 64) {
    const T x = (A[r + (size_t)k * lda] - vp[r] * wk) - w[r] * vpk;
    vk[r] = x;
    s += x * x;
  }
  s = wave_sum_mw(s);
  __syncthreads();
  const T dk = (A[k + (size_t)k * lda] - vpk * wk) - wk * vpk;
  const T x0 = vk[k + 1];
  const T tail = s - x0 * x0;
  const bool refl = tail > T(0.0);  // (the same in every lane) else already tridiagonal here
  const T nrm = Num<T>::sqrt_(s);
  const T alpha = sel(x0 > T(0.0), -nrm, nrm);
  const T v0 = x0 - alpha;
  const T e2k = sel(refl, alpha * alpha, x0 * x0);
  const T beta = sel(refl, T(2.0) / (tail + v0 * v0), T(0.0));
  __syncthreads();
  if (refl) {
    if (lane == 0) vk[k + 1] = v0;
  } else {
    for (int r = k + 1 + lane; r < n; r += 64) vk[r] = T(0.0);
  }
  __syncthreads();
  // ---- 3. rows of this strip: pending rank-2 update, store, A' v_k in ascending columns
  if (lane < R && i < n) {
    constexpr int U = 128 / (int)sizeof(T);  // columns per batch, the next batch loaded ahead
    const T vi = vp[i], wi = w[i];
    T acc = T(0.0);
    T* a = A + i + (size_t)(k + 1) * lda;
    int j = k + 1;
    const int nfull = (n - j) / U;
    T ca[U], cv[U];
    if (nfull > 0) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ca[u] = a[(size_t)u * lda];
        cv[u] = vp[j + u];
      }
    }
    for (int b = 0; b < nfull; ++b) {
      const bool more = b + 1 < nfull;
      T na[U], nv[U];
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          na[u] = a[(size_t)(U + u) * lda];
          nv[u] = vp[j + U + u];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const T t = (ca[u] - vi * w[j + u]) - wi * cv[u];
        a[(size_t)u * lda] = t;
        acc += t * vk[j + u];
      }
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          ca[u] = na[u];
          cv[u] = nv[u];
        }
      }
      a += (size_t)U * lda;
      j += U;
    }
    for (; j < n; ++j, a += lda) {
      const T t = (*a - vi * w[j]) - wi * vp[j];
      *a = t;
      acc += t * vk[j];
    }
    // ---- 4. this strip's rows of the next state
    nx[i] = vk[i];
    if (refl) nx[n + i] = beta * acc;
    else nx[n + i] = T(0.0);
  }
  if (blockIdx.x == 0 && lane == 0) {
    T* dg = d.ws + 2 * (2 * (size_t)n + 1);
    dg[k] = dk;
    dg[n + k] = e2k;
    nx[2 * n] = beta;
  }
}

// TRI: the tridiagonal is copied into LDS; otherwise the multisection reads it from the scratch
// in global memory through the same pointers (2n words past the CU's LDS)
template <class T, bool TRI>
__global__ __launch_bounds__(512) void eigblk_sturm(const EigBlkDesc<T>* __restrict__ descs,
                                                    T* __restrict__ out, int R,
                                                    const int* __restrict__ redo = nullptr) {
  extern __shared__ __attribute__((aligned(32))) char smem_raw[];
  if (redo && redo[blockIdx.x] == 0) return;
  const EigBlkDesc<T> d = descs[blockIdx.x];
  const int n = d.n, lda = d.lda, tid = threadIdx.x;
  T* scr = reinterpret_cast<T*>(smem_raw);
  T* Wv = reinterpret_cast<T*>(smem_raw + eigblk_sturm_scr(n));
  T* dgg = d.ws + 2 * (2 * (size_t)n + 1);
  T* e2g = dgg + n;
  const int ex = eigblk_exp(d, R);
  if (tid == 0) {
    const T* A = d.A;
    if (n == 1) {
      dgg[0] = A[0];
    } else {
      // reflector n - 3 (none for n = 2: eigblk_sym cleared buffer 0) is pending on the last 2 x 2
      const T* vp = eigblk_state(d, (n - 2) & 1);
      const T* pp = vp + n;
      const int r0 = n - 2, r1 = n - 1;
      const T v0 = vp[r0], v1 = vp[r1];
      const T Kc = vp[2 * n] * (pp[r0] * v0 + pp[r1] * v1) * T(0.5);
      const T w0 = pp[r0] - Kc * v0, w1 = pp[r1] - Kc * v1;
      dgg[r0] = (A[r0 + (size_t)r0 * lda] - v0 * w0) - w0 * v0;
      dgg[r1] = (A[r1 + (size_t)r1 * lda] - v1 * w1) - w1 * v1;
      const T e = (A[r1 + (size_t)r0 * lda] - v1 * w0) - w1 * v0;
      e2g[r0] = e * e;
    }
  }
  __syncthreads();
  const T* dg = dgg;
  const T* e2 = e2g;
  if constexpr (TRI) {
    T* dl = Wv + 1;
    T* el = dl + n;
    for (int q = tid; q < n; q += 512) {
      dl[q] = dgg[q];
      if (q + 1 < n) el[q] = e2g[q];
    }
    __syncthreads();
    dg = dl;
    e2 = el;
  }
  eig_multisection<T, true>(dg, e2, n, scr, Wv, out, ex);
}

// ------------------------------------------------------------------------------------------
// eigmin_mx (round 4): multi-word lambda_min (n <= 64) from an fp64 eigenpair refined at the
// word's width, instead of a multi-word tridiagonalisation.  The reference computes lambda_min
// of L^-1 dM L^-T at BigFloat precision (compute_step_length, MPMP.jl:1857-1870); eigmin_lds2
// does so in double-double / quad-double arithmetic throughout, where every one of the n - 2
// columns is a chain of multi-word reductions, square roots and reciprocals (~5 us per column
// at dd).  Here:
//   1. A_h = the leading words of A_s = (A + A^T)/2, tridiagonalised in fp64 (tridiag_lds2,
//      keeping the reflectors): A_h = Q T Q^T.  T is rescaled by a power of two (|T| < 1).
//   2. fp64 lambda of T (512-way multisection) and a lower bound of its second eigenvalue: one
//      512-way round of full Sturm counts at lambda + span 2^(-t/8) (count <= 1 => lambda_2 >= ..).
//   3. z = its eigenvector (inverse iteration, tridiagonal LU with partial pivoting), x = Q z.
//   4. R refinement steps (1 at dd, 2 at qd): r = A_s x - rho x with rho = x^T A_s x / x^T x at
//      the full width (the only multi-word work: two or three n^2 matrix-vector products), then
//      the Newton correction (A - rho I) d = -r, d orthogonal to x, solved in fp64 through the
//      same Q and T: d = Q P (T - lambda I)^-1 P Q^T (-r), P = I - z z^T; x <- x + d (each step
//      multiplies the eigenvector error by ~eps64 ||A|| / gap).
//   5. rho of the final x.  Temple's bound: with ||r||^2 / ||x||^2 = eta and lambda_2 > rho,
//      rho - eta / (lambda_2 - rho) <= lambda_min <= rho.  rho is accepted when that width is
//      below 2^-(BITS+2) of the spectrum's magnitude; otherwise (a multiple or tightly
//      clustered lambda_min, or no separated lambda_2) the block is flagged and the launch
//      that follows (eigmin_lds2 with the flags) runs the multi-word path on it alone
//      (g_eigmx_fallbacks counts those).
// ------------------------------------------------------------------------------------------
__device__ unsigned int g_eigmx_fallbacks = 0;
template <class T> __host__ __device__ constexpr int eigmx_refine() { return 6; }
template <class T> size_t eigmx_own_bytes(int n) {
  const size_t ld = eig2_ld<double>(n), W = sizeof(T) / 8;
  return 8 * (128 + (size_t)n * ld + 3 * ld + 2 * (size_t)n + 4 + 16 + (size_t)n * n +
              2 * (size_t)n + 6 * (size_t)n + 64 + 8 + W * (size_t)n + 8 * W * (size_t)n) + 64;
}
// static LDS of split_tridiag_keepv (rowb, pb, vb, redw, betab, amaxw), on top of the dynamic size
constexpr size_t EIGMX_STATIC_LDS = 6400;
template <class T> size_t eigmx_lds_bytes(int n) { return eigmx_own_bytes<T>(n); }
// Sturm count of the (scaled, |T| < 1) tridiagonal in pivot form, pivots floored at 2^-900
__device__ __forceinline__ int sturm_count_piv(const double* __restrict__ dg,
                                               const double* __restrict__ e2, int n, double sigma) {
  constexpr double PIVMIN = 0x1p-900;
  int cnt = 0;
  double q = dg[0] - sigma;
  if (fabs(q) < PIVMIN) q = -PIVMIN;
  cnt += q < 0.0;
  for (int i = 1; i < n; ++i) {
    q = (dg[i] - sigma) - e2[i - 1] / q;
    if (fabs(q) < PIVMIN) q = -PIVMIN;
    cnt += q < 0.0;
  }
  return cnt;
}
// T - mu I = L D L^T for the (scaled) tridiagonal with mu just below lambda_1, so every pivot is
// positive in exact arithmetic (floored at 2^-900 against rounding): one thread, the pivot
// chain in registers, reciprocals by the hardware rcp and two Newton steps.  rd = 1 / D,
// ll = the subdiagonal of L.
__device__ __forceinline__ double rcp_nr(double q) {
  double r = __builtin_amdgcn_rcp(q);
  r = fma(fma(-q, r, 1.0), r, r);
  return fma(fma(-q, r, 1.0), r, r);
}
__device__ __forceinline__ void tri_ldl(const double* __restrict__ dg, const double* __restrict__ eo,
                                        int n, double mu, double* __restrict__ rd,
                                        double* __restrict__ ll) {
  constexpr double PIVMIN = 0x1p-900;
  double dcur = dg[0] - mu;
#pragma unroll 8
  for (int i = 0; i + 1 < n; ++i) {
    const double e = eo[i], an = dg[i + 1] - mu;
    const double r = rcp_nr(fmax(dcur, PIVMIN)), l = e * r;
    rd[i] = r;
    ll[i] = l;
    dcur = fma(-l, e, an);
  }
  rd[n - 1] = rcp_nr(fmax(dcur, PIVMIN));
}
// b <- (L D L^T)^-1 b, one thread
__device__ __forceinline__ void tri_ldl_solve(const double* __restrict__ rd,
                                              const double* __restrict__ ll, int n,
                                              double* __restrict__ b) {
  double y = b[0];
#pragma unroll 8
  for (int i = 1; i < n; ++i) {
    y = fma(-ll[i - 1], y, b[i]);
    b[i] = y;
  }
  double x = y * rd[n - 1];
  b[n - 1] = x;
#pragma unroll 8
  for (int i = n - 2; i >= 0; --i) {
    x = fma(b[i], rd[i], -ll[i] * x);
    b[i] = x;
  }
}
// eigmin_split's register-resident tridiagonalisation (576 threads: 8 bulk waves holding the
// matrix, one chain wave building each reflector once) on the fp64 image Ah (n x ld in LDS,
// n <= 128), keeping the reflectors for eigmin_mx: v_r in column r of V (n x n), beta_r in
// bet[r], the signed coupling T(r+1, r) in eo[r] and the diagonal in dg.  The image is scaled by
// 2^-ex0 (its largest entry below 1, as eigmin_split) and T comes out scaled alike; returns ex0.
// The DBG knobs and stamps of eigmin_split are left out; the arithmetic is the same.
__device__ __forceinline__ int split_tridiag_keepv(const double* __restrict__ Ah, int ld, int n,
                                                   double* __restrict__ dg, double* __restrict__ V,
                                                   double* __restrict__ bet,
                                                   double* __restrict__ eo) {
  constexpr int NS = 16, NWB = 8, GS = 4;
  __shared__ __attribute__((aligned(16))) double rowb[2][128];
  __shared__ __attribute__((aligned(16))) double pb[2][128];
  __shared__ __attribute__((aligned(16))) double vb[2][128];
  __shared__ __attribute__((aligned(16))) double redw[2][NWB];
  __shared__ double betab[2];
  __shared__ double amaxw[NWB];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const bool chain = w == NWB;
  const int blk = w < 4 ? w : 11 - w;
  const int c = lane >> 4, t16 = lane & 15;
  const int i = blk * 16 + t16;
  const int j0 = 2 * c + 8 * t16;
  double a[NS][2];
#pragma unroll
  for (int s = 0; s < NS; ++s) a[s][0] = a[s][1] = 0.0;
  if (!chain) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int j = 2 * c + 8 * s + e;
        const int ic = min(i, n - 1), jc = min(j, n - 1);
        const double v = Ah[ic + (size_t)jc * ld];
        a[s][e] = (i < n && j < n) ? v : 0.0;
      }
    double amax = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) amax = fmax(amax, fmax(fabs(a[s][0]), fabs(a[s][1])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
    if (lane == 0) amaxw[w] = amax;
  }
  __syncthreads();
  int ex0;
  {
    double amax = amaxw[0];
#pragma unroll
    for (int r = 1; r < NWB; ++r) amax = fmax(amax, amaxw[r]);
    ex0 = (amax > 0.0 && amax < INFINITY) ? __builtin_amdgcn_frexp_exp(amax) : 0;
  }
  if (!chain) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      a[s][0] = __builtin_ldexp(a[s][0], -ex0);
      a[s][1] = __builtin_ldexp(a[s][1], -ex0);
    }
  }
  auto publish_row = [&](int r, double* dst) {
    if (!chain && blk == (r >> 4) && t16 == (r & 15)) {
#pragma unroll
      for (int s = 0; s < NS; ++s)
        *reinterpret_cast<double2*>(dst + 2 * c + 8 * s) = make_double2(a[s][0], a[s][1]);
    }
  };
  double cx = 0.0, cy = 0.0, beta = 0.0, vi = 0.0;
  auto reflector = [&](int r, double xj0, double xj1, double xr, double x0) {
    double tl = (j0 >= r + 2 ? xj0 * xj0 : 0.0);
    tl = fma(j0 + 1 >= r + 2 ? xj1 : 0.0, xj1, tl);
    tl = xsum32(xsum16(row16_sum(tl)));
    double bt = 0.0, v0 = x0, offd = x0;
    if (tl > 0.0) {
      const double ss = fma(x0, x0, tl);
      double nrm;
      if (ss > 0x1p-900) {
        double rs = __builtin_amdgcn_rsq(ss);
        rs = rs * fma(-0.5 * ss, rs * rs, 1.5);
        nrm = ss * rs;
        nrm = fma(fma(-nrm, nrm, ss), 0.5 * rs, nrm);
      } else {
        nrm = sqrt(ss);
      }
      const double alpha = x0 > 0.0 ? -nrm : nrm;
      v0 = x0 - alpha;
      const double q = fma(v0, v0, tl);
      double rc = __builtin_amdgcn_rcp(q);
      rc = fma(fma(-q, rc, 1.0), rc, rc);
      rc = fma(fma(-q, rc, 1.0), rc, rc);
      bt = 2.0 * rc;
      offd = alpha;
    }
    cx = j0 <= r ? 0.0 : (j0 == r + 1 ? v0 : xj0);
    cy = j0 + 1 <= r ? 0.0 : (j0 + 1 == r + 1 ? v0 : xj1);
    beta = bt;
    *reinterpret_cast<double2*>(&vb[r & 1][j0]) = make_double2(cx, cy);
    if (j0 < n) V[j0 + (size_t)r * n] = cx;
    if (j0 + 1 < n) V[j0 + 1 + (size_t)r * n] = cy;
    if (lane == 0) {
      dg[r] = xr;
      betab[r & 1] = bt;
      bet[r] = bt;
      eo[r] = offd;
    }
  };
  publish_row(0, rowb[0]);
  publish_row(1, rowb[1]);
  __syncthreads();
  if (chain) {
    __builtin_amdgcn_s_setprio(3);
    const double2 xr = *reinterpret_cast<const double2*>(&rowb[0][j0]);
    reflector(0, xr.x, xr.y, rowb[0][0], rowb[0][1]);
  }
  __syncthreads();
  if (!chain) {
    const double2 v2 = *reinterpret_cast<const double2*>(&vb[0][j0]);
    cx = v2.x;
    cy = v2.y;
    vi = vb[0][i];
    beta = betab[0];
  }
  for (int k = 0; k + 2 < n; ++k) {
    const int lo = (k + 1) >> 3;
    const int r = k + 1;
    double pp = 0.0;
    if (!chain) {
      const bool live = blk * 16 + 15 > k && blk * 16 < n;
      double pa[4] = {0.0, 0.0, 0.0, 0.0};
      if (live) {
        static_for<0, NS / GS>([&](auto G) {
          constexpr int g = decltype(G)::value;
          if (GS * g + GS - 1 >= lo) {
            static_for<GS * g, GS * g + GS>([&](auto S) {
              constexpr int s = decltype(S)::value;
              fmac_bcast<s, s == GS * g>(pa[2 * (s & 1)], cx, a[s][0]);
              fmac_bcast<s, false>(pa[2 * (s & 1) + 1], cy, a[s][1]);
            });
          }
        });
      }
      pp = xsum32(xsum16((pa[0] + pa[1]) + (pa[2] + pa[3])));
      double t = 0.0;
      if (c == 0) {
        pb[k & 1][i] = i > k ? pp : 0.0;
        t = vi * pp;
      }
      t = row16_sum(t);
      if (lane == 0) redw[k & 1][w] = t;
    }
    __syncthreads();
    if (chain) {
      double rw[NWB];
#pragma unroll
      for (int q = 0; q < NWB; q += 2) {
        const double2 v2 = *reinterpret_cast<const double2*>(&redw[k & 1][q]);
        rw[q] = v2.x;
        rw[q + 1] = v2.y;
      }
      const double* old = rowb[r & 1];
      const double2 pj = *reinterpret_cast<const double2*>(&pb[k & 1][j0]);
      const double2 o = *reinterpret_cast<const double2*>(old + j0);
      const double orr = old[r], or1 = old[r + 1];
      const double vr = vb[k & 1][r], vr1 = vb[k & 1][r + 1];
      const double pr = pb[k & 1][r], pr1 = pb[k & 1][r + 1];
      const double tot = ((rw[0] + rw[1]) + (rw[2] + rw[3])) + ((rw[4] + rw[5]) + (rw[6] + rw[7]));
      const double Kc = beta * beta * tot * 0.5;
      const double wr = fma(beta, pr, -(Kc * vr));
      const double gr = fma(Kc, vr, -wr), mhr = -(beta * vr);
      const double xj0 = fma(cx, gr, fma(pj.x, mhr, o.x));
      const double xj1 = fma(cy, gr, fma(pj.y, mhr, o.y));
      const double xr = fma(vr, gr, fma(pr, mhr, orr));
      const double x0 = fma(vr1, gr, fma(pr1, mhr, or1));
      reflector(r, xj0, xj1, xr, x0);
    } else if (blk * 16 + 15 > k + 1 && blk * 16 < n) {
      double rw[NWB];
#pragma unroll
      for (int q = 0; q < NWB; q += 2) {
        const double2 v2 = *reinterpret_cast<const double2*>(&redw[k & 1][q]);
        rw[q] = v2.x;
        rw[q + 1] = v2.y;
      }
      const double2 pv = *reinterpret_cast<const double2*>(&pb[k & 1][j0]);
      const double tot = ((rw[0] + rw[1]) + (rw[2] + rw[3])) + ((rw[4] + rw[5]) + (rw[6] + rw[7]));
      const double Kc = beta * beta * tot * 0.5;
      const double wi = fma(beta, pp, -(Kc * vi));
      const double gi = fma(Kc, vi, -wi), mhi = -(beta * vi);
      static_for<0, NS / GS>([&](auto G) {
        constexpr int g = decltype(G)::value;
        if (GS * g + GS - 1 >= lo) {
          static_for<GS * g, GS * g + GS>([&](auto S) {
            constexpr int s = decltype(S)::value;
            fmac_bcast<s, s == GS * g>(a[s][0], pv.x, mhi);
            fmac_bcast<s, false>(a[s][1], pv.y, mhi);
          });
          static_for<GS * g, GS * g + GS>([&](auto S) {
            constexpr int s = decltype(S)::value;
            fmac_bcast<s, false>(a[s][0], cx, gi);
            fmac_bcast<s, false>(a[s][1], cy, gi);
          });
        }
      });
      publish_row(k + 2, rowb[k & 1]);
    }
    __syncthreads();
    if (!chain) {
      const double2 v2 = *reinterpret_cast<const double2*>(&vb[r & 1][j0]);
      cx = v2.x;
      cy = v2.y;
      vi = vb[r & 1][i];
      beta = betab[r & 1];
    }
  }
  if (chain) __builtin_amdgcn_s_setprio(0);
  if (tid == 0) dg[n - 1] = rowb[(n - 1) & 1][n - 1];
  __syncthreads();
  return ex0;
}
// DBG: per-block diagnostics and phase stamps (s_memtime) in g_eigmx_dbg[block * 24 + slot]
__device__ double g_eigmx_dbg[256 * 24];
// DBG 2: block 0's fp64 data for a host check (V n x n, then dg, eo, bet, z, x, r, s, d', d by n)
__device__ double g_eigmx_dump[64 * 64 + 12 * 64];
// TRI = 1: the register-resident tridiagonalisation (split_tridiag_keepv, 576 threads; the
// ninth wave only builds reflectors), TRI = 0: tridiag_lds2 on 512 threads
template <class T, int DBG = 0, int TRI = 1>
__global__ __launch_bounds__(TRI ? 576 : 512) void eigmin_mx(const MatDesc<T>* __restrict__ descs,
                                                             T* __restrict__ out,
                                                             int* __restrict__ redo) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr int NT = 512, NW = 8, R = eigmx_refine<T>();
  const MatDesc<T> d = descs[blockIdx.x];
  const int n = d.n, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double* dbg = DBG ? g_eigmx_dbg + (size_t)(blockIdx.x & 255) * 24 : nullptr;
  unsigned long long t_prev = DBG ? __builtin_amdgcn_s_memtime() : 0ull;
  auto stamp = [&](int slot) {
    if constexpr (DBG != 0) {
      if (tid == 0 && slot < 16) {
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        dbg[slot] = (double)(t - t_prev);
        t_prev = t;
      }
    }
  };
  bool ok = n >= 3;
  if (ok) {
    const int ld = eig2_ld<double>(n);
    double* sd = reinterpret_cast<double*>(smem_raw);  // 64 padded diagonal for the counts
    double* se = sd + 64;                              // 64 padded squared couplings
    double* A = se + 64;                               // n x ld
    double* vb = A + (size_t)n * ld;                   // 2 x ld
    double* p = vb + 2 * ld;                           // ld
    double* dg = p + ld;                               // n
    double* e2 = dg + n;                               // n
    double* scal = e2 + n;                             // 4
    double* redw = scal + 4;                           // 16
    double* V = redw + 16;                             // n x n reflectors
    double* bet = V + (size_t)n * n;                   // n
    double* eo = bet + n;                              // n signed off-diagonal
    double* rd = eo + n;                               // n  1 / D of T - mu I = L D L^T
    double* ll = rd + n;                               // n  L's subdiagonal
    double* wv = ll + 4 * n;                           // n  right-hand side / solution
    double* sc = wv + n;                               // 64 scalars
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(sc + 64);  // 8
    T* xv = reinterpret_cast<T*>(masks + 8);           // n   the eigenvector estimate
    T* part = xv + n;                                  // 8 x n  row partials of A_s x
    // the symmetrised entries (row lane, columns j = w + NW u) of the lane, every load issued
    // before any is used (a loop over j waited on each strided load in turn, ~n / NW global
    // latencies per pass; n <= 64 so one row per lane and at most JM columns per wave)
    // (quad-double: in two halves of JH columns, registers)
    constexpr int JM = 64 / NW, JH = sizeof(T) > 16 ? JM / 2 : JM;
    auto load_sym = [&](T* sv, int u0) {
#pragma unroll
      for (int u = 0; u < JH; ++u) {
        const int j = w + NW * (u0 + u), jc = min(j, n - 1), ic = min(lane, n - 1);
        const T a1 = d.A[ic + (size_t)jc * d.lda], a2 = d.A[jc + (size_t)ic * d.lda];
        sv[u] = (a1 + a2) * T(0.5);
      }
    };
    // (1) leading words of the symmetrised block, then the fp64 tridiagonalisation
    if (w < NW && lane < n) {
#pragma unroll
      for (int u0 = 0; u0 < JM; u0 += JH) {
        T sv[JH];
        load_sym(sv, u0);
#pragma unroll
        for (int u = 0; u < JH; ++u) {
          const int j = w + NW * (u0 + u);
          if (j < n && lane >= j) {
            A[lane + (size_t)j * ld] = Num<T>::hi(sv[u]);
            A[j + (size_t)lane * ld] = Num<T>::hi(sv[u]);
          }
        }
      }
    }
    __syncthreads();
    stamp(0);
    int ex0 = 0;  // (TRI 1: T comes out scaled by 2^-ex0)
    if constexpr (TRI == 1) {
      ex0 = split_tridiag_keepv(A, ld, n, dg, V, bet, eo);
      for (int i = tid; i + 1 < n; i += NT) e2[i] = eo[i] * eo[i];
      __syncthreads();
    } else {
      tridiag_lds2<double, true>(A, ld, n, vb, p, dg, e2, scal, redw, V, bet, eo);
    }
    stamp(1);
    // Gershgorin bracket of T and the power of two that scales it below 1
    if (tid == 0) {
      double glo = 0.0, ghi = 0.0;
      for (int i = 0; i < n; ++i) {
        const double rr = (i > 0 ? fabs(eo[i - 1]) : 0.0) + (i + 1 < n ? fabs(eo[i]) : 0.0);
        const double a = dg[i] - rr, b = dg[i] + rr;
        if (i == 0 || a < glo) glo = a;
        if (i == 0 || b > ghi) ghi = b;
      }
      const double mag = fmax(fabs(glo), fabs(ghi));
      const bool fin = mag > 0.0 && mag < INFINITY;
      const int ex = fin ? __builtin_amdgcn_frexp_exp(mag) : 0;
      sc[0] = fin ? 1.0 : 0.0;
      sc[1] = (double)ex;
      sc[6] = (double)(ex + ex0);  // A's units -> the scaled T's
      const double span = ldexp(ghi - glo, -ex);
      sc[2] = ldexp(glo, -ex) - span * 1e-3 - 1e-300;
      sc[3] = ldexp(ghi, -ex) + span * 1e-3 + 1e-300;
    }
    __syncthreads();
    ok = sc[0] != 0.0;
    if (ok) {
      const int ex = (int)sc[1];
      for (int i = tid; i < n; i += NT) {
        dg[i] = ldexp(dg[i], -ex);
        e2[i] = ldexp(e2[i], -2 * ex);
        eo[i] = ldexp(eo[i], -ex);
      }
      __syncthreads();
      auto first_hit = [&](bool hit) -> int {
        const unsigned long long mk = __ballot(hit && tid < NT);
        if (lane == 0 && w < NW) masks[w] = mk;
        __syncthreads();
        int f = -1;
        for (int q = 0; q < NW && f < 0; ++q)
          if (masks[q]) f = q * 64 + __ffsll((long long)masks[q]) - 1;
        __syncthreads();
        return f;
      };
      // (2) lambda of T: eigmin_split's multisection (the padded fp64 arrays, 512-way on all 8
      // waves, 6 rounds of 9 bits = 2^-54 of the span)
      const int nr = (n + 7) & ~7;
      if (tid < nr) {
        sd[tid] = tid < n ? dg[tid] : 4.0;
        se[tid] = (tid >= 1 && tid < n) ? fmax(e2[tid - 1], 0x1p-900) : 0.0;
      }
      __syncthreads();
      double lo = sc[2], hi = sc[3];
      for (int it = 0; it < 6; ++it) {
        const double width = hi - lo;
        const bool hit = sturm_any_below(sd, se, nr, lo + width * ((double)(tid + 1) / 513.0));
        const int f = first_hit(hit);
        if (f < 0) {
          lo = lo + width * (512.0 / 513.0);
        } else {
          hi = lo + width * ((double)(f + 1) / 513.0);
          if (f > 0) lo = lo + width * ((double)f / 513.0);
        }
      }
      const double lam = 0.5 * (lo + hi), span = sc[3] - sc[2];
      // lower bound of lambda_2: the largest lam + span 2^(-t/4) (t < 256) with at most one
      // eigenvalue below it
      bool le1 = false;
      if (tid < 256) le1 = sturm_count_piv(dg, e2, n, lam + span * exp2(-(double)tid * 0.25)) <= 1;
      const int f2 = first_hit(le1);
      // the fp64 tridiagonal is within ~n eps64 |T| of A_s (backward stable, plus the rounding
      // of A_s to its leading words): a margin of 2^-40 of the scaled magnitude
      const double lam2 = f2 < 0 ? -INFINITY : lam + span * exp2(-(double)f2 * 0.25) - 0x1p-40;
      stamp(2);
      // (3) L D L^T of T - mu I, mu = lambda - 2^-48 span (below lambda_1: the bracket is 2^-54
      // span wide), and two inverse-iteration solves from the all-ones vector (thread 0; each
      // solve grows the vector by at most ~2^48, so no rescaling in between)
      const double mu = lam - span * 0x1p-48;
      if (tid == 0) {
        tri_ldl(dg, eo, n, mu, rd, ll);
        for (int i = 0; i < n; ++i) wv[i] = 1.0;
        tri_ldl_solve(rd, ll, n, wv);
        tri_ldl_solve(rd, ll, n, wv);
      }
      __syncthreads();
      stamp(3);
      // (3') wave 0: z = wv / ||wv||, x = Q z (reflectors n-3 .. 0), x / ||x||
      double zl = 0.0;  // (wave 0, lane l < n: z_l; kept in the register for the projections)
      // x <- Q x (H_{n-2} first) or Q^T x (H_0 first), lane l holding x_l: the next reflector's
      // entry is loaded ahead of the current one's wave sum.  (The last "reflector" H_{n-2} acts
      // on one entry: it is the identity unless the contracted tail s - x0^2 came out positive,
      // in which case it flips the sign of row n-1 and T's last coupling is -x0.)
      auto apply_q = [&](double xl, bool transpose) -> double {
        const int m = n - 1, dk = transpose ? 1 : -1;
        int k = transpose ? 0 : n - 2;
        double vk = lane > k && lane < n ? V[lane + (size_t)k * n] : 0.0, bk = bet[k];
        for (int s = 0; s < m; ++s) {
          const int kn = k + dk;
          double vn = 0.0, bn = 0.0;
          if (s + 1 < m) {
            vn = lane > kn && lane < n ? V[lane + (size_t)kn * n] : 0.0;
            bn = bet[kn];
          }
          const double t = wave_sum_mw<double>(vk * xl);
          xl -= (bk * t) * vk;
          vk = vn;
          bk = bn;
          k = kn;
        }
        return xl;
      };
      if (w == 0) {
        double zz = lane < n ? wv[lane] : 0.0;
        double mz = fabs(zz);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mz = fmax(mz, __shfl_xor(mz, o));
        zz = mz > 0.0 && mz < INFINITY ? zz / mz : 0.0;
        const double nz = sqrt(wave_sum_mw<double>(zz * zz));
        zl = nz > 0.0 ? zz / nz : 0.0;
        double xl = apply_q(zl, false);
        const double nx = sqrt(wave_sum_mw<double>(xl * xl));
        xl = nx > 0.0 ? xl / nx : 0.0;
        if (lane < n) xv[lane] = T(xl);
        if constexpr (DBG == 2) {
          if (blockIdx.x == 0 && lane < n) {
            double* dm = g_eigmx_dump + (size_t)n * n;
            dm[lane] = dg[lane];
            dm[n + lane] = eo[lane];
            dm[2 * n + lane] = bet[lane];
            dm[3 * n + lane] = zl;
            dm[4 * n + lane] = xl;
            for (int k = 0; k < n; ++k) g_eigmx_dump[lane + (size_t)k * n] = V[lane + (size_t)k * n];
            if (lane == 0) { dm[10 * n] = mu; dm[10 * n + 1] = sc[6]; }
          }
        }
        if (lane == 0) sc[4] = nz > 0.0 && nx > 0.0 ? 1.0 : 0.0;
      }
      __syncthreads();
      stamp(4);
      ok = sc[4] != 0.0;
      // (4)-(5) Rayleigh quotient and residual of x; accepted as soon as Temple's width is below
      // 2^-(BITS+2) of |T| < 1, else a refinement step (at most R = 6: a close lambda_2 slows
      // the refinement to ~2^-50 |T| / gap per step, and a few more steps of ~25 us are far
      // cheaper than the multi-word fallback)
      for (int it = 0; ok && it <= R; ++it) {
        // row partials of y = A_s x: row lane, columns j = w (mod 8)
        if (lane < n && w < NW) {
          T acc = T(0.0);
#pragma unroll
          for (int u0 = 0; u0 < JM; u0 += JH) {
            T sv[JH];
            load_sym(sv, u0);
#pragma unroll
            for (int u = 0; u < JH; ++u) {
              const int j = w + NW * (u0 + u);
              if (j < n) acc = acc + sv[u] * xv[j];
            }
          }
          part[w * n + lane] = acc;
        }
        __syncthreads();
        stamp(5 + 3 * it);
        if (w == 0) {
          T y = T(0.0), xl = T(0.0);
          if (lane < n) {
            xl = xv[lane];
            y = ((part[lane] + part[n + lane]) + (part[2 * n + lane] + part[3 * n + lane])) +
                ((part[4 * n + lane] + part[5 * n + lane]) + (part[6 * n + lane] + part[7 * n + lane]));
          }
          const T num = wave_sum_mw<T>(xl * y), den = wave_sum_mw<T>(xl * xl);
          const T rho = num / den;
          const T rr = y - rho * xl;
          const double rh = ldexp(Num<T>::hi(rr), -(int)sc[6]);  // scaled residual
          const double eta = wave_sum_mw<double>(rh * rh) / Num<T>::hi(den);
          if constexpr (DBG != 0) {
            if (lane == 0 && it < 4) dbg[16 + it] = eta;
          }
          const double rhs = ldexp(Num<T>::hi(rho), -(int)sc[6]);
          const double tw = lam2 > rhs ? eta / (lam2 - rhs) : INFINITY;
          const bool acc = tw <= 0x1p-3 * Num<T>::eps();  // 2^-(BITS+2) of |T| < 1
          if (lane == 0) {
            // accepted / rejected (the last step, or no lambda_2 bound above rho: Temple's bound
            // cannot hold however far x is refined) / refine
            sc[5] = acc ? 1.0 : ((it == R || !(lam2 > rhs)) ? -1.0 : 0.0);
            if (acc) out[blockIdx.x] = rho;
            if constexpr (DBG != 0) {
              dbg[20] = lam;
              dbg[21] = lam2;
              dbg[22] = rhs;
              dbg[23] = tw;
            }
          }
          if (!acc && it < R && lam2 > rhs) {
            // s = P Q^T (-r) in fp64 (scaled) -> wv for the solve
            double s = apply_q(-rh, true);
            s -= wave_sum_mw<double>(zl * s) * zl;
            if (lane < n) wv[lane] = s;
            if constexpr (DBG == 2) {
              if (blockIdx.x == 0 && it == 0 && lane < n) {
                double* dm = g_eigmx_dump + (size_t)n * n;
                dm[5 * n + lane] = rh;
                dm[6 * n + lane] = s;
              }
            }
          }
        }
        __syncthreads();
        if (sc[5] != 0.0) {
          ok = sc[5] > 0.0;
          break;
        }
        if (tid == 0) tri_ldl_solve(rd, ll, n, wv);  // (T - mu I) d' = s
        __syncthreads();
        stamp(6 + 3 * it);
        if (w == 0) {  // x += Q P d' (unscaled: the residual was scaled by 2^-ex)
          double dl = lane < n ? wv[lane] : 0.0;
          dl -= wave_sum_mw<double>(zl * dl) * zl;
          dl = apply_q(dl, false);
          if constexpr (DBG == 2) {
            if (blockIdx.x == 0 && it == 0 && lane < n) {
              double* dm = g_eigmx_dump + (size_t)n * n;
              dm[7 * n + lane] = wv[lane];
              dm[8 * n + lane] = dl;
            }
          }
          if (lane < n) xv[lane] = xv[lane] + T(dl);
        }
        __syncthreads();
        stamp(7 + 3 * it);
      }
    }
  }
  // redo[block] = 1: the multi-word path (eigmin_lds2, the next launch) takes this block (a
  // clustered lambda_min, or n < 3)
  if (tid == 0) {
    redo[blockIdx.x] = ok ? 0 : 1;
    if (!ok && n >= 3) atomicAdd(&g_eigmx_fallbacks, 1u);
  }
}

// ------------------------------------------------------------------------------------------
// mxblk_*: eigmin_mx's scheme for multi-word blocks past the LDS kernels (CLRSDP_EIG_MX_BLK=1,
// in place of eigmin_batched / the multi-word eigblk_* chain): the O(n^3) work is fp64 and
// spread over workgroups, the multi-word work is one n^2 matrix-vector product per refinement
// step.  No reflectors are kept (the fp64 eigblk_* chain forms only the tridiagonal), so the
// correction operator is the dense fp64 Cholesky factor of A_h - mu I with mu just below lambda.
// The multi-word block A is only read; every fp64 image lives in the plan's scratch.  Per batch:
//   mxblk_amax     per strip of R rows, the largest leading-limb magnitude of A (Inf for a strip
//                  that holds a NaN or Inf)
//   mxblk_image    ex = pow2_exp(max of the partials); two fp64 images of the leading limbs of
//                  A_s = (A + A^T) / 2^(ex + 1); a block with n < 3, all zeros or a non-finite
//                  entry is flagged here (its images are the identity)
//   eigblk_amax / _sym / _col<double>  on the first image: its tridiagonal
//   mxblk_sturm    the pending update of the last 2 x 2 and the multisection of eigblk_sturm for
//                  lambda; a lower bound lam2 of lambda_2 from one round of full Sturm counts at
//                  lambda + span 2^(-t/4) (t < 256), less 2^-40 of the Gershgorin magnitude
//                  (eigmin_mx's rule: it covers the n 2^-52 between T and A_s up to n = 4096);
//                  mu = lambda - max(2^-40, 16 n 2^-53) span, subtracted from the second image's
//                  diagonal; the starting right-hand side of the inverse iteration
//   potrf64_*      Cholesky of the second image (a failed block is flagged, not an error)
//   MXBLK_INVIT x [trsm forward, trsm transposed, mxblk_norm]: z by inverse iteration,
//                  normalised after every round; x = z at the word's width after the last
//   at most MXBLK_REFINE + 1 x [mxblk_matvec, mxblk_rayleigh, trsm, trsm, mxblk_update]:
//     matvec       y = A_s x at the word's width: 64 rows per workgroup, four waves with a fixed
//                  quarter of the columns each (ascending), combined as (q0 + q1) + (q2 + q3)
//     rayleigh     rho = x^T y / x^T x, r = y - rho x, eta = |r|^2 / |x|^2; Temple: rho is accepted
//                  when eta / (lam2 - rho) <= 2^-(BITS+2) of the magnitude, and out = rho 2^ex;
//                  flagged when no lam2 lies above rho or the last step was not accepted;
//                  otherwise the fp64 right-hand side P (-r 2^k), P = I - z z^T, k from max |r|
//     update       x += P d 2^-k at the word's width, d the solution of the two vector solves
//   mxblk_finish   redo[block] = 0 for an accepted block, 1 for a flagged one: the launch of
//                  the multi-word route that follows takes the flagged blocks only
// The state of a block (state[7]: 0 running, 1 accepted, 2 flagged) lives on the device, and a
// block that is no longer running leaves every mxblk launch at once (the vector solves run on
// its stale right-hand side, which nothing reads).  Every sum is one thread's ascending sum or a
// fixed tree over a fixed thread -> element map, one workgroup per block: lambda_min does not
// depend on the grid or on the rest of the batch.  Launch arguments are constant, nothing waits
// inside a launch and nothing is read back, so the sequence can be captured.
// ------------------------------------------------------------------------------------------
// refinement steps at most.  Started at 8; every certified block of tests/test_gpu_eig_mxblk.py
// took 1 (double-double) or 2 (quad-double), the CPU restatement of the scheme 3 at most (gap
// 2^-20 at 212 bits).  Every step's launches are enqueued whether or not a block still runs
// (nothing is read back), so the spare steps cost launches: 4 keeps one in hand.
constexpr int MXBLK_REFINE = 4;
constexpr int MXBLK_INVIT = 3;   // rounds of inverse iteration for z
constexpr int MXBLK_ST = 8;      // state words: lambda, lam2, mu, magnitude, ex, k, steps, state
__device__ unsigned int g_mxblk_steps = 0;  // most refinement steps of an accepted block so far
template <class T>
struct MxBlkDesc {
  const T* A;    // n x n, leading dimension lda (read only)
  double* Ah;    // n x n, ld n: the image the fp64 chain tridiagonalises (destroyed by it)
  double* Af;    // n x n, ld n: the image that becomes the factor of A_h - mu I
  double* amax;  // one partial per strip of the prepass
  double* z;     // n   the fp64 eigenvector
  double* b;     // n   right-hand side / solution of the vector solves
  T* x;          // n   the eigenvector estimate at the word's width
  T* y;          // n   A_s x
  double* st;    // MXBLK_ST words of state
  int n, lda;
};
constexpr size_t mxblk_sturm_lds(int n) { return eigblk_sturm_lds<double>(n, true) + 512 * sizeof(double); }

template <class T, int R>
__global__ __launch_bounds__(64) void mxblk_amax(const MxBlkDesc<T>* __restrict__ descs) {
  const MxBlkDesc<T> d = descs[blockIdx.y];
  const int n = d.n, lane = threadIdx.x, i = blockIdx.x * R + lane;
  if ((int)blockIdx.x * R >= n) return;
  double amax = 0.0;
  if (lane < R && i < n)
    for (int j = 0; j < n; ++j) {
      const double a = fabs(Num<T>::hi(d.A[i + (size_t)j * d.lda]));
      amax = a < INFINITY ? fmax(amax, a) : INFINITY;  // (NaN: not below Inf either)
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
  if (lane == 0) d.amax[blockIdx.x] = amax;
}

template <class T, int R>
__global__ __launch_bounds__(64) void mxblk_image(const MxBlkDesc<T>* __restrict__ descs) {
  const MxBlkDesc<T> d = descs[blockIdx.y];
  const int n = d.n, lda = d.lda, lane = threadIdx.x, i = blockIdx.x * R + lane;
  if ((int)blockIdx.x * R >= n) return;
  double mx = 0.0;
  for (int s = 0; s * R < n; ++s) mx = fmax(mx, d.amax[s]);
  const bool bad = !(mx > 0.0 && mx < INFINITY) || n < 3;
  const int ex = bad ? 0 : pow2_exp(mx);
  if (blockIdx.x == 0 && lane == 0) {
    d.st[4] = (double)ex;
    d.st[5] = 0.0;
    d.st[6] = 0.0;
    d.st[7] = bad ? 2.0 : 0.0;
  }
  if (lane >= R || i >= n) return;
  // the thread of row i owns the pairs (i, j), (j, i) with j <= i
  const T* A = d.A;
  for (int j = 0; j <= i; ++j) {
    double h = i == j ? 1.0 : 0.0;
    if (!bad) {
      const T a = scale2(A[i + (size_t)j * lda], -ex);
      h = Num<T>::hi(i == j ? a : (a + scale2(A[j + (size_t)i * lda], -ex)) * T(0.5));
    }
    d.Ah[i + (size_t)j * n] = h;
    d.Ah[j + (size_t)i * n] = h;
    d.Af[i + (size_t)j * n] = h;
    d.Af[j + (size_t)i * n] = h;
  }
}

template <class T>
__global__ __launch_bounds__(512) void mxblk_sturm(const EigBlkDesc<double>* __restrict__ edescs,
                                                   const MxBlkDesc<T>* __restrict__ mdescs,
                                                   double* __restrict__ lamv) {
  extern __shared__ __attribute__((aligned(32))) char smem_raw[];
  const EigBlkDesc<double> d = edescs[blockIdx.x];
  const MxBlkDesc<T> m = mdescs[blockIdx.x];
  const int n = d.n, lda = d.lda, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (m.st[7] != 0.0) return;  // flagged by the prepass (n >= 3 from here on)
  double* scr = reinterpret_cast<double*>(smem_raw);
  double* Wv = reinterpret_cast<double*>(smem_raw + eigblk_sturm_scr(n));
  double* dl = Wv + 1;
  double* el = dl + n;
  double* red = reinterpret_cast<double*>(smem_raw + eigblk_sturm_lds<double>(n, true));  // 512
  double* dgg = d.ws + 2 * (2 * (size_t)n + 1);
  double* e2g = dgg + n;
  if (tid == 0) {
    // reflector n - 3 is pending on the last 2 x 2 (eigblk_sturm)
    const double* A = d.A;
    const double* vp = eigblk_state(d, (n - 2) & 1);
    const double* pp = vp + n;
    const int r0 = n - 2, r1 = n - 1;
    const double v0 = vp[r0], v1 = vp[r1];
    const double Kc = vp[2 * n] * (pp[r0] * v0 + pp[r1] * v1) * 0.5;
    const double w0 = pp[r0] - Kc * v0, w1 = pp[r1] - Kc * v1;
    dgg[r0] = (A[r0 + (size_t)r0 * lda] - v0 * w0) - w0 * v0;
    dgg[r1] = (A[r1 + (size_t)r1 * lda] - v1 * w1) - w1 * v1;
    const double e = (A[r1 + (size_t)r0 * lda] - v1 * w0) - w1 * v0;
    e2g[r0] = e * e;
  }
  __syncthreads();
  for (int q = tid; q < n; q += 512) {
    dl[q] = dgg[q];
    el[q] = q + 1 < n ? e2g[q] : 0.0;
  }
  __syncthreads();
  eig_multisection<double, true>(dl, el, n, scr, Wv, lamv, 0);
  __syncthreads();
  const double lam = lamv[blockIdx.x];
  // Gershgorin bracket of the tridiagonal
  double glo = INFINITY, ghi = -INFINITY;
  for (int i = tid; i < n; i += 512) {
    const double rr = (i > 0 ? sqrt(el[i - 1]) : 0.0) + (i + 1 < n ? sqrt(el[i]) : 0.0);
    glo = fmin(glo, dl[i] - rr);
    ghi = fmax(ghi, dl[i] + rr);
  }
  glo = -block_max(-glo, red);
  ghi = block_max(ghi, red);
  const double span = ghi - glo, mag = fmax(fabs(glo), fabs(ghi));
  // lower bound of lambda_2: the largest lam + span 2^(-t/4) (t < 256) with at most one
  // eigenvalue of T below it
  unsigned long long* masks = reinterpret_cast<unsigned long long*>(red);
  bool le1 = false;
  if (tid < 256) le1 = sturm_count_piv(dl, el, n, lam + span * exp2(-(double)tid * 0.25)) <= 1;
  const unsigned long long mk = __ballot(le1);
  if (lane == 0) masks[w] = mk;
  __syncthreads();
  int f2 = -1;
  for (int q = 0; q < 4 && f2 < 0; ++q)
    if (masks[q]) f2 = q * 64 + __ffsll((long long)masks[q]) - 1;
  const bool fin = mag > 0.0 && mag < INFINITY && lam == lam;
  const double lam2 = f2 < 0 ? -INFINITY : lam + span * exp2(-(double)f2 * 0.25) - 0x1p-40 * mag;
  const double mu = lam - fmax(0x1p-40, 16.0 * (double)n * 0x1p-53) * span;
  for (int i = tid; i < n; i += 512) {
    m.Af[i + (size_t)i * n] -= mu;
    // a fixed start with no symmetry of its own (a vector of ones is orthogonal to the wanted
    // eigenvector of many structured blocks)
    const double g = (double)(i + 1) * 0.6180339887498949;
    m.b[i] = 0.5 + (g - floor(g));
  }
  if (tid == 0) {
    m.st[0] = lam;
    m.st[1] = lam2;
    m.st[2] = mu;
    m.st[3] = mag;
    if (!fin || f2 < 0) m.st[7] = 2.0;  // no lambda_2 bound: Temple's bound cannot hold
  }
}

// z = b / |b| after a round of inverse iteration, b = z for the next round; after the last
// round x = z at the word's width
template <class T>
__global__ __launch_bounds__(256) void mxblk_norm(const MxBlkDesc<T>* __restrict__ descs,
                                                  const int* __restrict__ info, int first, int last) {
  __shared__ double red[256];
  const MxBlkDesc<T> d = descs[blockIdx.x];
  const int n = d.n, tid = threadIdx.x;
  if (d.st[7] != 0.0) return;
  if (first && info[blockIdx.x] != 0) {  // A_h - mu I did not factor
    if (tid == 0) d.st[7] = 2.0;
    return;
  }
  double mx = 0.0;
  bool fin = true;
  for (int i = tid; i < n; i += 256) {
    const double a = fabs(d.b[i]);
    fin = fin && a < INFINITY;
    mx = fmax(mx, a);
  }
  mx = block_max(mx, red);
  const double nf = block_max(fin ? 0.0 : 1.0, red);
  if (nf != 0.0 || !(mx > 0.0)) {
    if (tid == 0) d.st[7] = 2.0;
    return;
  }
  double s = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double v = d.b[i] / mx;
    s += v * v;
  }
  const double nrm = sqrt(block_sum(s, red));
  for (int i = tid; i < n; i += 256) {
    const double v = (d.b[i] / mx) / nrm;
    d.z[i] = v;
    d.b[i] = v;
    if (last) d.x[i] = T(v);
  }
}

template <class T>
__global__ __launch_bounds__(256) void mxblk_matvec(const MxBlkDesc<T>* __restrict__ descs) {
  __shared__ T part[3 * 64];
  const MxBlkDesc<T> d = descs[blockIdx.y];
  const int n = d.n, lda = d.lda, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if ((int)blockIdx.x * 64 >= n) return;
  if (d.st[7] != 0.0) return;
  const int ex = (int)d.st[4];
  const int i = blockIdx.x * 64 + lane, ic = min(i, n - 1);
  const int cq = (n + 3) / 4, j0 = w * cq, j1 = min(n, j0 + cq);
  const T* __restrict__ A = d.A;
  const T* __restrict__ x = d.x;
  T acc = T(0.0);
#pragma unroll 2
  for (int j = j0; j < j1; ++j) {
    const T a1 = scale2(A[ic + (size_t)j * lda], -ex), a2 = scale2(A[j + (size_t)ic * lda], -ex);
    acc = acc + ((a1 + a2) * T(0.5)) * x[j];
  }
  if (w > 0) part[(w - 1) * 64 + lane] = acc;
  __syncthreads();
  if (w == 0 && i < n) d.y[i] = (acc + part[lane]) + (part[64 + lane] + part[128 + lane]);
}

template <class T>
__global__ __launch_bounds__(256) void mxblk_rayleigh(const MxBlkDesc<T>* __restrict__ descs,
                                                      T* __restrict__ out, int it, int last) {
  __shared__ T red[256];
  __shared__ double redd[256];
  const MxBlkDesc<T> d = descs[blockIdx.x];
  const int n = d.n, tid = threadIdx.x;
  if (d.st[7] != 0.0) return;
  T num = T(0.0), den = T(0.0);
  for (int i = tid; i < n; i += 256) {
    const T xi = d.x[i];
    num = num + xi * d.y[i];
    den = den + xi * xi;
  }
  num = block_sum(num, red);
  den = block_sum(den, red);
  const T rho = num / den;
  double e = 0.0, rm = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double rh = Num<T>::hi(d.y[i] - rho * d.x[i]);
    e += rh * rh;
    rm = fmax(rm, fabs(rh));
  }
  const double eta = block_sum(e, redd) / Num<T>::hi(den);
  rm = block_max(rm, redd);
  const double lam2 = d.st[1], mag = d.st[3], rhs = Num<T>::hi(rho);
  const double tw = lam2 > rhs ? eta / (lam2 - rhs) : INFINITY;
  const bool acc = tw <= ldexp(mag, -(Num<T>::BITS + 2));
  if (acc || last || !(lam2 > rhs)) {
    if (tid == 0) {
      if (acc) {
        out[blockIdx.x] = scale2(rho, (int)d.st[4]);
        d.st[6] = (double)it;
      }
      d.st[7] = acc ? 1.0 : 2.0;
    }
    return;
  }
  // the right-hand side of the correction: P (-r 2^k) in fp64
  const int k = -pow2_exp(rm);
  double c = 0.0;
  for (int i = tid; i < n; i += 256)
    c += d.z[i] * -ldexp(Num<T>::hi(d.y[i] - rho * d.x[i]), k);
  c = block_sum(c, redd);
  for (int i = tid; i < n; i += 256)
    d.b[i] = -ldexp(Num<T>::hi(d.y[i] - rho * d.x[i]), k) - c * d.z[i];
  if (tid == 0) d.st[5] = (double)k;
}

template <class T>
__global__ __launch_bounds__(256) void mxblk_update(const MxBlkDesc<T>* __restrict__ descs) {
  __shared__ double red[256];
  const MxBlkDesc<T> d = descs[blockIdx.x];
  const int n = d.n, tid = threadIdx.x;
  if (d.st[7] != 0.0) return;
  const int k = (int)d.st[5];
  double c = 0.0;
  for (int i = tid; i < n; i += 256) c += d.z[i] * d.b[i];
  c = block_sum(c, red);
  for (int i = tid; i < n; i += 256) d.x[i] = d.x[i] + T(ldexp(d.b[i] - c * d.z[i], -k));
}

template <class T>
__global__ __launch_bounds__(256) void mxblk_finish(const MxBlkDesc<T>* __restrict__ descs, int nm,
                                                    int* __restrict__ redo) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nm) return;
  const bool ok = descs[q].st[7] == 1.0;
  redo[q] = ok ? 0 : 1;
  if (ok) atomicMax(&g_mxblk_steps, (unsigned int)descs[q].st[6]);
  else if (descs[q].n >= 3) atomicAdd(&g_eigmx_fallbacks, 1u);
}

}  // namespace clrsdp

namespace clrsdp {

// ------------------------------------------------------------------------------------------
// Cholesky + inverse of one fp64 block on chip with MFMA (chol_inv_tiles, below) and its
// diagonal-tile step.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ d4 mfma64(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// One wave: Cholesky factor and inverse of the 16x16 diagonal tile at (k0, k0) of the LDS image,
// with no LDS round trip inside the column chain.  Lane l holds row i = l & 15 of A (-> L) and
// of X (-> L^-1) in full (each of the four 16-lane DPP rows is a replica).  Per column j the
// pivot comes by v_readlane and every l_k / x_jm by row_newbcast from the lane that owns it, so
// a column costs ~50 VALU instructions and one dependent chain (broadcast -> fma -> readlane ->
// rsq).  Writes L_kk back into the image and L_kk^-1 column-major into Dinv; a non-positive
// pivot sets *flag = k0 + 1.
// IDX(i, j) = offset of tile element (i, j) in the image (only i >= j is read and written).
template <class IDX>
__device__ inline void chol_diag16_bc(double* __restrict__ A, IDX idx, int k0,
                                     double* __restrict__ Dinv, int* flag, int lane) {
  const int i = lane & 15;
  double a[16], x[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {  // symmetric tile from its lower triangle
    a[k] = A[idx(max(i, k), min(i, k))];
    x[k] = (k == i) ? 1.0 : 0.0;
  }
  // X = diag(r) Y: the rows of Y are left unscaled (y_i -= l_ij r_j y_j), and each lane
  // scales its own row by its pivot's 1/l_ii at the end
  int bad = 0;
  double rmine = 1.0;
  static_for<0, 16>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const double d = readlane_d(a[j], j);
    bad |= !(d > 0.0);
    double r = __builtin_amdgcn_rsq(d);
    r = r * (1.5 - 0.5 * d * r * r);  // Newton step: r = 1/sqrt(d) to ~1 ulp
    const double lv = a[j] * r;       // l_ij (row j: sqrt(d))
    const double nl = (i > j) ? -lv : 0.0;
    const double nlr = nl * r;
    rmine = (i == j) ? r : rmine;
    a[j] = lv;
    // a_ik -= l_i l_k (k > j; the next pivot column first).  Only the first reads lv right
    // after its VALU write; the y sources were last written a column ago.
    static_for<j + 1, 16>([&](auto K) {
      constexpr int k = decltype(K)::value;
      fmac_bcast<k, k == j + 1>(a[k], lv, nl);
    });
    static_for<0, j + 1>([&](auto M) {
      constexpr int m = decltype(M)::value;
      fmac_bcast<j, j == 15 && m == 0>(x[m], x[m], nlr);
    });
  });
#pragma unroll
  for (int k = 0; k < 16; ++k) x[k] *= rmine;
  if (lane < 16) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k <= i) A[idx(i, k)] = a[k];
      Dinv[k * 16 + i] = x[k];  // column-major L_kk^-1 (zero above the diagonal)
    }
    if (lane == 0 && bad) *flag = k0 + 1;
  }
}

// chol_diag16_bc software-pipelined (same arithmetic, bit for bit): each column's pivot chain
// (readlane -> rsq -> Newton -> l_j -> the next pivot column's update) is the critical path, and
// the rest of the previous column's rank-1 update is issued inside it, in four pieces between
// its dependent steps (in-order issue: those FMAs fill the chain's latency instead of following
// it).  The inverse rows are split over the four 16-lane DPP rows: register s of DPP row g holds
// column 4s + g of this lane's row of X, so a column's inverse update is ceil((j+1)/4) FMAs,
// not j+1.
// LD(i, k): element (i, k) of the symmetric input tile (default: the lower triangle of the image)
template <class IDX, class LD>
__device__ inline void chol_diag16_pipe(double* __restrict__ A, IDX idx, LD ld, int k0,
                                        double* __restrict__ Dinv, int* flag, int lane) {
  const int i = lane & 15, g = lane >> 4;
  double a[16], x[4];
#pragma unroll
  for (int k = 0; k < 16; ++k) a[k] = ld(i, k);
#pragma unroll
  for (int s = 0; s < 4; ++s) x[s] = (4 * s + g == i) ? 1.0 : 0.0;
  int bad = 0;
  double rmine = 1.0, lvp = 0.0, nlp = 0.0, nlrp = 0.0;  // column j-1's l, -l and -l r
  // piece C (of 4) of column JP's bulk: a[JP+2 ..] -= l l_k, then x[s] (4s <= JP)
  auto bulk = [&](auto JP, auto C, auto NOP) {
    constexpr int jp = decltype(JP)::value, c = decltype(C)::value;
    constexpr int NA = jp < 14 ? 14 - jp : 0, N = NA + jp / 4 + 1;
    static_for<c * N / 4, (c + 1) * N / 4>([&](auto T) {
      constexpr int t = decltype(T)::value;
      if constexpr (t < NA) fmac_bcast<jp + 2 + t, false>(a[jp + 2 + t], lvp, nlp);
      else fmac_bcast<jp, decltype(NOP)::value && t == c * N / 4>(x[t - NA], x[t - NA], nlrp);
    });
  };
  using F = std::false_type;
  static_for<0, 16>([&](auto J) {
    constexpr int j = decltype(J)::value;
    constexpr auto JP = std::integral_constant<int, (j > 0 ? j - 1 : 0)>{};
    const double d = readlane_d(a[j], j);
    bad |= !(d > 0.0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (j > 0) bulk(JP, std::integral_constant<int, 0>{}, F{});
    __builtin_amdgcn_sched_barrier(0);
    double r = __builtin_amdgcn_rsq(d);
    const double hd = 0.5 * d;
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (j > 0) bulk(JP, std::integral_constant<int, 1>{}, F{});
    __builtin_amdgcn_sched_barrier(0);
    const double t1 = hd * r;
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (j > 0) bulk(JP, std::integral_constant<int, 2>{}, F{});
    __builtin_amdgcn_sched_barrier(0);
    const double t2 = 1.5 - t1 * r;
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (j > 0) bulk(JP, std::integral_constant<int, 3>{}, F{});
    __builtin_amdgcn_sched_barrier(0);
    r = r * t2;
    const double lv = a[j] * r;
    const double nl = (i > j) ? -lv : 0.0;
    const double nlr = nl * r;
    rmine = (i == j) ? r : rmine;
    a[j] = lv;
    if constexpr (j < 15) fmac_bcast<j + 1, true>(a[j + 1], lv, nl);
    lvp = lv;
    nlp = nl;
    nlrp = nlr;
  });
  // column 15's bulk: the inverse update only
  static_for<0, 4>([&](auto C) { bulk(std::integral_constant<int, 15>{}, C, std::true_type{}); });
#pragma unroll
  for (int s = 0; s < 4; ++s) x[s] *= rmine;
  if (lane < 16) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k <= i) A[idx(i, k)] = a[k];
    if (lane == 0 && bad) *flag = k0 + 1;
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) Dinv[(4 * s + g) * 16 + i] = x[s];
}
template <class IDX>
__device__ inline void chol_diag16_pipe(double* __restrict__ A, IDX idx, int k0,
                                        double* __restrict__ Dinv, int* flag, int lane) {
  chol_diag16_pipe(A, idx, [&](int i, int k) { return A[idx(max(i, k), min(i, k))]; }, k0, Dinv, flag,
                   lane);
}

// ------------------------------------------------------------------------------------------
// chol_inv_tiles: A = L L^T and L^-1 for n <= NP (fp64), one 512-thread workgroup per matrix,
// with the off-diagonal 16x16 tiles resident in the worker waves' MFMA accumulators for the
// whole factorisation (no LDS round trip of the trailing matrix).  Tile (i, j), i > j, of the
// lower triangle belongs to worker (t mod 7), slot t / 7 (t = its row-major index); the slot
// holds A_ij^T in accumulator layout (register r of lane l = A_ij[l&15][(l>>4) + 4r]) until
// panel j turns it into L_ij, and X_ij = (L^-1)_ij (register r = X_ij[(l>>4) + 4r][l&15]) from
// then on.  Only the diagonal tiles, one 16-column panel of L, one 16-row block of X and the
// two diagonal inverses live in LDS (57 KB at NP = 128).  Per panel k:
//   (b) workers: L_ik^T = Linv_kk A_ik^T (the accumulator is exactly the B operand) -> LDS
//       panel; X_kj <- Linv_kk X_kj and X_kk = Linv_kk -> LDS row block;
//   (c) workers: A_ij^T -= L_jk L_ik^T, X_ij -= L_ik X_kj, diagonal tiles D_i -= L_ik L_ik^T;
//   wave 0, concurrently (look-ahead): as soon as L_{k+1,k} is in the panel, D_{k+1} -=
//       L L^T and its Cholesky + inverse (chol_diag16_bc, no LDS inside the column chain).
// The critical path per panel is one MFMA tile + the 16-column diagonal factorisation.
// ------------------------------------------------------------------------------------------
#ifdef CLRSDP_CHOL_TRACE
// [block][wave (up to 16)][point (up to 128)]
__device__ unsigned long long g_chol2_trace[256 * 16 * 128];
#define CT_TRACE() do { if ((threadIdx.x & 63) == 0 && tr_i < 128) g_chol2_trace[(blockIdx.x * 16 + (threadIdx.x >> 6)) * 128 + tr_i] = __builtin_amdgcn_s_memtime(); ++tr_i; } while (0)
#else
#define CT_TRACE()
#endif
#ifndef CLRSDP_CHOL256_NTH
#define CLRSDP_CHOL256_NTH 768
#endif
template <int NP>
struct CholTiles {
  // NTH threads: one chain wave and NWK workers (512 up to NP = 128; 768 at NP = 256).  Wave 4
  // (a worker) shares SIMD 0 with the chain wave, and its f64 MFMAs slow the chain's VALU
  // chain by half (tools/micro/diag16_bench.hip); measured and rejected: no tiles on it (the
  // MFMA work then has three SIMDs: 32.7 vs 31.3 us at n = 128) or its trailing update held
  // back until the chain's diagonal factor is done (35.0 vs 31.4 us)
  static constexpr int NTH = NP > 128 ? CLRSDP_CHOL256_NTH : 512;
  static constexpr int NT = NP / 16, NOFF = NT * (NT - 1) / 2, NWK = NTH / 64 - 1;
  static constexpr int SLOTS = (NOFF + NWK - 1) / NWK, DSLOTS = (NT + NWK - 1) / NWK;
  static constexpr int LDD = 18;        // diagonal tiles: column-major 16 x 18
  static constexpr int XLD = NP + 16;   // X row block: 16 x XLD row-major
  static constexpr int DT = 0, PN = DT + NT * 16 * LDD, XR = PN + NT * 256, DI = XR + 16 * XLD,
                       END = DI + 512;  // doubles; the int flags follow
  // flag[0], flag[3]: the failure slots by tile parity; flag[1]: look-ahead panels ready;
  // flag[2]: worker arrivals (chol_inv_tiles)
  static constexpr int NFLAGS = 4;
  static __device__ __forceinline__ void tile(int t, int& i, int& j) {  // row-major lower
    i = 1;
    while (i * (i + 1) / 2 <= t) ++i;
    j = t - i * (i - 1) / 2;
  }
  // The SPDINV form (chol_inv_tiles<NP, true>): the lower tiles of G = L^-T L^-1, diagonal ones
  // included, row-major over GWK workers (tile t: G worker t mod GWK, slot t / GWK).
  // CLRSDP_SPDINV_W4 = 0 keeps them off worker 3 (wave 4, which shares SIMD 0 with the chain
  // wave); DESIGN.md section 6 has both times.
#ifndef CLRSDP_SPDINV_W4
#define CLRSDP_SPDINV_W4 1
#endif
  static constexpr int NG = NT * (NT + 1) / 2, GWK = CLRSDP_SPDINV_W4 ? NWK : NWK - 1;
  static constexpr int GSLOTS = (NG + GWK - 1) / GWK;
  static __device__ __forceinline__ int gworker(int wk) {  // index among the G workers, or -1
    if (CLRSDP_SPDINV_W4) return wk;
    return wk == 3 ? -1 : wk - (wk > 3);
  }
  static __device__ __forceinline__ void gtile(int t, int& i, int& j) {  // row-major, j <= i
    i = 0;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    j = t - i * (i + 1) / 2;
  }
};
template <int NP>
size_t chol_inv_tiles_lds() { return sizeof(double) * CholTiles<NP>::END + sizeof(int) * CholTiles<NP>::NFLAGS; }

// SPDINV (NP <= 128): the workers also hold the lower tiles of G = A^-1 = L^-T L^-1 in GSLOTS more
// accumulator slots.  In (c) of panel k, behind the trailing update, G_ij += X_ki^T X_kj for
// i, j <= k, both operands read from the X row block in LDS (stable until the barrier that ends
// (c)): the products grow with k as the trailing update shrinks.  After the last panel each tile
// goes to out_g[block] with its mirror, so G is full and exactly symmetric; entries past n are
// not written, and nothing of G is written for a block that fails.  A block whose out_g (or
// out_g[block].A) is null runs the plain form's instructions on L and L^-1: those two come out
// the same bits either way.  G must not alias the input or L^-1.
template <int NP, bool SPDINV = false>
__global__ __launch_bounds__(CholTiles<NP>::NTH) void chol_inv_tiles(const MatDesc<double>* __restrict__ in,
                                                      const MatDesc<double>* __restrict__ out_inv,
                                                      int* __restrict__ info, int prio = 0,
                                                      const MatDesc<double>* __restrict__ out_g = nullptr) {
  static_assert(!SPDINV || NP <= 128, "chol_inv_tiles: A^-1 in the accumulators for NP <= 128 only");
  using CT = CholTiles<NP>;
  // prio: the diagonal chain (wave 0) at priority 3, the workers at 2, above co-resident waves
  // of other launches (which stay at 0)
  if (prio) {
    if (threadIdx.x < 64) __builtin_amdgcn_s_setprio(3);
    else __builtin_amdgcn_s_setprio(2);
  }
  constexpr int NT = CT::NT, NWK = CT::NWK, SLOTS = CT::SLOTS, DSLOTS = CT::DSLOTS;
  constexpr int LDD = CT::LDD, XLD = CT::XLD;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* Dt = reinterpret_cast<double*>(smem_raw) + CT::DT;  // diagonal tiles
  double* Pn = reinterpret_cast<double*>(smem_raw) + CT::PN;  // panel: L_ik column-major 16x16
  double* Xr = reinterpret_cast<double*>(smem_raw) + CT::XR;  // X row block k
  double* Di = reinterpret_cast<double*>(smem_raw) + CT::DI;  // Linv_kk by parity, col-major
  int* flag = reinterpret_cast<int*>(reinterpret_cast<double*>(smem_raw) + CT::END);
  // The failure of diagonal tile t is published in FAIL(t), a slot chosen by the tile's parity.
  // The chain wave factors D_{k+1} during panel k, and every wave decides to leave at the top of
  // panel k from FAIL(k): written during panel k - 1 (D_0: the prologue), so before the barrier
  // that ended it, and all waves read the same value.  (One slot for every tile let a worker that
  // read it late in panel k leave while the others, having read 0, spun on its flag + 2 arrival.)
  // At most one slot is ever set: every wave leaves at the top of the panel after the failure.
  static_assert(CT::NFLAGS == 4, "flag[0..3] are used below");
  auto FAIL = [&](int t) { return flag + 3 * (t & 1); };
#ifdef CLRSDP_CHOL_TRACE
  int tr_i = 0;
#endif
  CT_TRACE();
  const MatDesc<double> d = in[blockIdx.x];
  // (the wave index through readfirstlane: the slot coordinates and every branch on them are
  // scalar, not per-lane registers)
  const int n = d.n, tid = threadIdx.x, lane = tid & 63,
            w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = (n + 15) / 16;
  const int lr = lane & 15, lk = lane >> 4;
  const int wk = w - 1;  // worker index, -1 for wave 0
  // The chain wave and the workers run separate copies of the panel loop (the same barriers in
  // the same order): the workers' accumulator slots are not live in the chain wave's code, so
  // the register allocation is the larger of the two paths, not their sum (NP = 256: 18 slots
  // per worker next to the chain's 32-register rows).
  const MatDesc<double> o = out_inv[blockIdx.x];
  // prologue: the diagonal tiles 1.. into LDS with identity padding (tile 0 is the chain wave's:
  // it factors D_0 straight from global memory while the other waves load); L^-1's tiles are
  // written as they become final (tile row k after panel k), so no store tail is left for the
  // end; the zero tiles above the diagonal first (never read: the input is read on and below the
  // diagonal only, so in place is safe).  All loads of the diagonal tiles are issued before the
  // first LDS store: one memory latency, not one per pass of the loop.
  constexpr int DPER = (NT * 256 + CT::NTH - 1) / CT::NTH;
  double dv[DPER];
  auto prologue_load = [&]() {
#pragma unroll
    for (int q = 0; q < DPER; ++q) {
      const int e = tid + q * CT::NTH;
      const int t = e >> 8, c = (e >> 4) & 15, r = e & 15;
      const int gi = min(16 * t + r, n - 1), gj = min(16 * t + c, n - 1);
      dv[q] = gload(d.A + gi + (size_t)gj * d.lda);
    }
    asm volatile("" ::: "memory");  // (the loads stay above: not sunk into the selects below)
  };
  auto prologue_store = [&]() {
#pragma unroll
    for (int q = 0; q < DPER; ++q) {
      const int e = tid + q * CT::NTH;
      if (e < 256 || e >= NT * 256) continue;
      const int t = e >> 8, c = (e >> 4) & 15, r = e & 15;
      const int gi = 16 * t + r, gj = 16 * t + c;
      double v = gi == gj ? 1.0 : 0.0;
      if (t < nt && gi < n && gj < n && r >= c) v = dv[q];
      Dt[t * 16 * LDD + c * LDD + r] = v;
    }
    for (int j = tid >> 4; j < n; j += CT::NTH / 16)
      for (int i = (tid & 15); i < (j & ~15); i += 16) o.A[i + (size_t)j * o.lda] = 0.0;
    lds_barrier();
    CT_TRACE();
  };
  if (wk < 0) {
    // ======================= the chain wave: the diagonal tiles, one panel ahead
    if (lane == 0) {  // (before D_0's factorisation, which may set flag[0])
      flag[0] = 0;  // first failing pivot + 1 of an even diagonal tile (FAIL above)
      flag[1] = 0;  // panels whose L_{k+1,k} is in the panel buffer
      flag[2] = 0;  // worker arrivals at the (b) -> (c) barrier
      flag[3] = 0;  // first failing pivot + 1 of an odd diagonal tile
    }
    prologue_load();
    chol_diag16_pipe(Dt, [](int i, int j) { return j * LDD + i; },
                     [&](int i, int k) {  // D_0 from global memory, identity-padded past n
                       const int r = max(i, k), c = min(i, k);
                       return r < n ? gload(d.A + r + (size_t)c * d.lda) : (i == k ? 1.0 : 0.0);
                     },
                     0, Di, flag, lane);
    prologue_store();
    lds_barrier();
    CT_TRACE();
    for (int k = 0; k < nt; ++k) {
      if (*FAIL(k)) break;
      if (k + 1 < nt) {
        // D_{k+1} -= L L^T (L = L_{k+1,k}) and its factorisation
        // (the flags order LDS data only: relaxed LDS atomics and compiler fences, so neither
        // side waits for the workers' outstanding global stores of final L^-1 tiles)
        while (__hip_atomic_load(flag + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) <= k)
          __builtin_amdgcn_s_sleep(1);
        __atomic_signal_fence(__ATOMIC_ACQUIRE);
        CT_TRACE();
        const double* P = Pn + 256 * (k + 1);
        double* D = Dt + (k + 1) * 16 * LDD;
        d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = D[lr * LDD + lk + 4 * r];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double f = P[(4 * r + lk) * 16 + lr];
          acc = mfma64(-f, f, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) D[lr * LDD + lk + 4 * r] = acc[r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        chol_diag16_pipe(D, [](int i, int j) { return j * LDD + i; }, 16 * (k + 1),
                         Di + 256 * ((k + 1) & 1), FAIL(k + 1), lane);
        CT_TRACE();
      }
      lds_barrier();
      CT_TRACE();
    }
  } else {
    // ======================= the workers
    // ---- tile coordinates of this worker's slots (wave-uniform)
    int TI[SLOTS], TJ[SLOTS];
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
      const int t = wk + NWK * q;
      int ti = NT, tj = 0;  // empty slot: row NT is never active
      if (t < CT::NOFF) CT::tile(t, ti, tj);
      TI[q] = ti;
      TJ[q] = tj;
    }
    // ---- off-diagonal tiles straight into the accumulators (A_ij^T layout, coalesced along rows)
    d4 T[SLOTS];
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = 16 * TI[q] + lr, gj = 16 * TJ[q] + lk + 4 * r;
        T[q][r] = (TI[q] < nt && gi < n && gj < n) ? gload(d.A + gi + (size_t)gj * d.lda) : 0.0;
      }
    }
    d4 XD[DSLOTS];
#pragma unroll
    for (int q = 0; q < DSLOTS; ++q) XD[q] = d4{0.0, 0.0, 0.0, 0.0};
    // ---- SPDINV: this worker's tiles of G (wave-uniform coordinates; row NT: an empty slot)
    constexpr int GSLOTS = SPDINV ? CT::GSLOTS : 1;
    double* gA = nullptr;
    int ldg = 0;
    if constexpr (SPDINV) {
      if (out_g) {
        gA = out_g[blockIdx.x].A;
        ldg = out_g[blockIdx.x].lda;
      }
    }
    int GI[GSLOTS], GJ[GSLOTS];
    d4 G[GSLOTS];
#pragma unroll
    for (int q = 0; q < GSLOTS; ++q) {
      int gi = NT, gj = 0;
      if constexpr (SPDINV) {
        const int gw = CT::gworker(wk);
        const int t = gw + CT::GWK * q;
        if (gA && gw >= 0 && t < CT::NG) CT::gtile(t, gi, gj);
      }
      GI[q] = gi;
      GJ[q] = gj;
      G[q] = d4{0.0, 0.0, 0.0, 0.0};
    }
    bool done = true;
    prologue_load();
    prologue_store();
    lds_barrier();  // (the chain wave's first diagonal factor)
    CT_TRACE();
    for (int k = 0; k < nt; ++k) {
      if (*FAIL(k)) {
        done = false;
        break;
      }
      // an opaque zero per panel: the per-slot LDS and store addresses below are formed where
      // they are used, not hoisted out of the loop (NP = 256: dozens of loop-invariant
      // addresses kept live across the panels spilled to scratch)
      int opq = 0;
      if constexpr (SLOTS > 6) asm volatile("" : "+s"(opq));
      double* const Pn_ = Pn + opq;
      double* const Xr_ = Xr + opq;
      double* const Dt_ = Dt + opq;
      double* const oA = o.A + opq;
      const double* Dk = Di + 256 * (k & 1);
      // ---------------- (b): Linv_kk as the A operand: a[r] = Linv[lr][4r+lk]
      double lopA[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) lopA[r] = Dk[(4 * r + lk) * 16 + lr];
      // the look-ahead tile L_{k+1,k} first (wave 0 waits for it)
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int q = 0; q < SLOTS; ++q) {
          if (TI[q] >= nt || TJ[q] != k) continue;
          if ((TI[q] == k + 1) != (pass == 0)) continue;
          d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int r = 0; r < 4; ++r) acc = mfma64(lopA[r], T[q][r], acc);  // L_ik^T
          double* P = Pn_ + 256 * TI[q];
#pragma unroll
          for (int r = 0; r < 4; ++r) P[(lk + 4 * r) * 16 + lr] = acc[r];  // L_ik[lr][lk+4r]
          if (pass == 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __atomic_signal_fence(__ATOMIC_RELEASE);
            if (lane == 0) __hip_atomic_store(flag + 1, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < SLOTS; ++q) {  // X row block: X_kj <- Linv_kk X_kj (j < k)
        if (TI[q] != k) continue;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = mfma64(lopA[r], T[q][r], acc);
        T[q] = acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          Xr_[(lk + 4 * r) * XLD + 16 * TJ[q] + lr] = acc[r];
          const int gi = 16 * k + lk + 4 * r, gj = 16 * TJ[q] + lr;  // final: (L^-1)_kj
          if (gi < n && gj < n) oA[gi + (size_t)gj * o.lda] = acc[r];
        }
      }
      if (wk == k % NWK) {  // X_kk = Linv_kk (accumulator layout: register r = Linv[lk+4r][lr])
#pragma unroll
        for (int q = 0; q < DSLOTS; ++q)
          if (q == k / NWK) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              XD[q][r] = Dk[lr * 16 + lk + 4 * r];
              Xr_[(lk + 4 * r) * XLD + 16 * k + lr] = XD[q][r];
              const int gi = 16 * k + lk + 4 * r, gj = 16 * k + lr;  // final: (L^-1)_kk
              if (gi < n && gj < n) oA[gi + (size_t)gj * o.lda] = XD[q][r];
            }
          }
      }
      CT_TRACE();
      // workers-only barrier (wave 0 is busy with the next diagonal tile)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __atomic_signal_fence(__ATOMIC_RELEASE);
      if (lane == 0) __hip_atomic_fetch_add(flag + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      while (__hip_atomic_load(flag + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < NWK * (k + 1))
        __builtin_amdgcn_s_sleep(1);
      __atomic_signal_fence(__ATOMIC_ACQUIRE);
      CT_TRACE();
      // ---------------- (c) trailing update of the rows below k
      const double* Pk = Pn_;
#pragma unroll
      for (int q = 0; q < SLOTS; ++q) {
        const int ti = TI[q], tj = TJ[q];
        if (ti >= nt || ti <= k) continue;
        const double* Pi = Pk + 256 * ti;
        if (tj > k) {  // A_ij^T -= L_jk L_ik^T
          const double* Pj = Pk + 256 * tj;
          d4 acc = T[q];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc = mfma64(-Pj[(4 * r + lk) * 16 + lr], Pi[(4 * r + lk) * 16 + lr], acc);
          T[q] = acc;
        } else {  // X_ij -= L_ik X_kj (tj == k: the slot turns from L_ik into X_ik = -L_ik X_kk)
          d4 acc = tj == k ? d4{0.0, 0.0, 0.0, 0.0} : T[q];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc = mfma64(-Pi[(4 * r + lk) * 16 + lr], Xr_[(4 * r + lk) * XLD + 16 * tj + lr], acc);
          T[q] = acc;
        }
      }
      // diagonal tiles below the look-ahead one: D_i -= L_ik L_ik^T (in LDS)
#pragma unroll
      for (int q = 0; q < DSLOTS; ++q) {
        const int di = wk + NWK * q;
        if (di >= nt || di <= k + 1) continue;
        const double* Pi = Pk + 256 * di;
        double* D = Dt_ + di * 16 * LDD;
        d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = D[lr * LDD + lk + 4 * r];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double f = Pi[(4 * r + lk) * 16 + lr];
          acc = mfma64(-f, f, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) D[lr * LDD + lk + 4 * r] = acc[r];
      }
      // SPDINV: G_ij += X_ki^T X_kj (i, j <= k), row block k of L^-1 as both MFMA operands
      if constexpr (SPDINV) {
#pragma unroll
        for (int q = 0; q < GSLOTS; ++q) {
          if (GI[q] > k) continue;
          d4 acc = G[q];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc = mfma64(Xr_[(4 * r + lk) * XLD + 16 * GI[q] + lr],
                         Xr_[(4 * r + lk) * XLD + 16 * GJ[q] + lr], acc);
          G[q] = acc;
        }
      }
      CT_TRACE();
      lds_barrier();
      CT_TRACE();
    }
    // SPDINV: register r of a G slot = G_ij[lk + 4r][lr], which is coalesced (16 lanes along a
    // column) where the mirror (j, i) goes.  The tile itself goes out transposed through a
    // 16 x 17 scratch of this worker's own in the panel / row-block buffers, which nobody reads
    // after the last panel's barrier (no barrier here: a wave reads what it wrote).  A diagonal
    // tile takes both halves from its lower one, so G is exactly symmetric.  Inside n x n only.
    if constexpr (SPDINV) {
      constexpr int GLD = 17;
      static_assert((CT::NG + 1 < NWK ? CT::NG + 1 : NWK) * 16 * GLD <= NT * 256 + 16 * XLD,
                    "chol_inv_tiles: the transposing scratch of the workers that hold G tiles");
      if (done) {
        double* S = Pn + wk * 16 * GLD;
#pragma unroll
        for (int q = 0; q < GSLOTS; ++q) {
          if (GI[q] >= nt) continue;
          double t[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) S[(lk + 4 * r) * GLD + lr] = G[q][r];
#pragma unroll
          for (int r = 0; r < 4; ++r) t[r] = S[lr * GLD + lk + 4 * r];  // G_ij[lr][lk + 4r]
          const bool diag = GI[q] == GJ[q];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = lk + 4 * r;
            const int gi = 16 * GI[q] + lr, gj = 16 * GJ[q] + c;  // (i, j): row lr, column c
            const int mi = 16 * GJ[q] + lr, mj = 16 * GI[q] + c;  // (j, i): row lr, column c
            if (diag) {
              if (gi < n && gj < n) gA[gi + (size_t)gj * ldg] = lr >= c ? t[r] : G[q][r];
            } else {
              if (gi < n) gA[gi + (size_t)gj * ldg] = t[r];
              if (mj < n) gA[mi + (size_t)mj * ldg] = G[q][r];
            }
          }
        }
      }
    }
  }
  if (tid == 0 && info) info[blockIdx.x] = flag[0] ? flag[0] : flag[3];
  CT_TRACE();
}
#undef CT_TRACE


// ------------------------------------------------------------------------------------------
// The cluster part of the block solve (MPMP.jl:1751-1768) at fp64 with the explicit inverses, as
// two launches around slab_qsolve instead of four batched GEMVs (q_t, p_Wt | q_Wdy, q_dx):
//   cl_solve_t:  t = L^-1 rhs and this row block's share of W^T t   (one partial slab per block)
//   cl_solve_dx: u = t + W dy and dx = L^-T u                        (one column block of dx)
// L^-1 is the lower triangle of S_j in place (chol_inv_tiles; 2x2-blocked with X21 or not): row
// i only uses columns <= i, so the stale S12 above the diagonal is never read.  64-row / 64-column
// blocks, 4 waves; sums in a fixed order (deterministic).
// ------------------------------------------------------------------------------------------
struct ClSolveDesc {
  const double* L;    // D x D, column-major, ld D: L^-1 in the lower triangle
  const double* W;    // D x n_y, ld D: W = L^-1 B
  const double* rhs;  // D
  double* t;          // D: t = L^-1 rhs
  double* dx;         // D: dx = L^-T (t + W dy)
  int D, pad;
};

// Sum over the 64 lanes of each of the N values every lane holds, transposed: log2(N) halving
// steps (lane bit 5, 4, ... picks the half a lane keeps and adds its partner's copy of) and plain
// butterfly steps after that, so lane l ends with the total of value l >> (6 - log2 N) in
// N - 1 + (6 - log2 N) shuffles instead of 6 N.  Fixed order.
template <int N>
__device__ __forceinline__ double xpose_sum(double (&v)[N], int lane) {
  static_for<0, 6>([&](auto Lv) {
    constexpr int lev = decltype(Lv)::value;
    constexpr int o = 32 >> lev;
    constexpr int H = N >> (lev + 1);
    if constexpr (H >= 1) {
      const bool hi = (lane & o) != 0;
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const double send = hi ? v[j] : v[j + H];
        const double keep = hi ? v[j + H] : v[j];
        v[j] = keep + __shfl_xor(send, o);
      }
    } else {
      v[0] = v[0] + __shfl_xor(v[0], o);
    }
  });
  return v[0];
}

// grid: clusters x nrb row blocks; slabs[(cluster * nrb + block) * ny + c] (zeros past D)
__global__ __launch_bounds__(256) void cl_solve_t(const ClSolveDesc* __restrict__ ds, int nrb,
                                                  int ny, double* __restrict__ slabs) {
  __shared__ double part[4][64];
  const int c = blockIdx.x / nrb, rb = blockIdx.x - c * nrb;
  const ClSolveDesc d = ds[c];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int D = d.D, r0 = 64 * rb, i = r0 + lane, ic = min(i, D - 1);
  double* out = slabs + (size_t)blockIdx.x * ny;
  if (r0 >= D) {  // (clusters of different sizes)
    for (int e = tid; e < ny; e += 256) out[e] = 0.0;
    return;
  }
  // (1) t_i = sum_{k <= i} L_ik rhs_k, wave w over k in [64 w, 64 w + 64)
  const int k0 = 64 * w, k1 = min(k0 + 64, min(r0 + 64, D));
  double acc = 0.0;
  for (int kb = k0; kb < k1; kb += 16) {
    double lv[16], rv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int k = min(kb + u, k1 - 1);
      lv[u] = d.L[ic + (size_t)k * D];
      rv[u] = d.rhs[k];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (kb + u < k1 && kb + u <= i) acc = fma(lv[u], rv[u], acc);
  }
  part[w][lane] = acc;
  __syncthreads();
  double t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
  if (i >= D) t = 0.0;
  else if (w == 0) d.t[i] = t;
  // (2) sum over this block's rows of W_ic t_i: wave w takes 32 of every 128 columns
  for (int cb = 32 * w; cb < ny; cb += 128) {
    double v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const double wv = d.W[ic + (size_t)min(cb + j, ny - 1) * D];
      v[j] = i < D ? wv * t : 0.0;
    }
    const double sm = xpose_sum<32>(v, lane);
    const int cc = cb + (lane >> 1);
    if ((lane & 1) == 0 && cc < ny) out[cc] = sm;
  }
}

// grid: clusters x nrb column blocks (64 columns of dx each, 16 per wave)
__global__ __launch_bounds__(256) void cl_solve_dx(const ClSolveDesc* __restrict__ ds, int nrb,
                                                   int ny, const double* __restrict__ dy) {
  __shared__ double part[4][64];
  const int c = blockIdx.x / nrb, cbk = blockIdx.x - c * nrb;
  const ClSolveDesc d = ds[c];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int D = d.D, j0 = 64 * cbk + 16 * w;
  if (64 * cbk >= D) return;
  const int cw0 = (int)((long long)ny * w / 4), cw1 = (int)((long long)ny * (w + 1) / 4);
  double accx = 0.0;
  for (int rb = cbk; 64 * rb < D; ++rb) {  // the rows i >= 64 cbk, in order
    const int i = 64 * rb + lane, ic = min(i, D - 1);
    // u_i = t_i + W_i dy (this wave's share of the columns; the four shares in order)
    double sm = 0.0;
    for (int cb = cw0; cb < cw1; cb += 16) {
      double wv[16], yv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int cc = min(cb + u, cw1 - 1);
        wv[u] = d.W[ic + (size_t)cc * D];
        yv[u] = dy[cc];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (cb + u < cw1) sm = fma(wv[u], yv[u], sm);
    }
    part[w][lane] = sm;
    __syncthreads();
    const double ui =
        i < D ? d.t[ic] + ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) : 0.0;
    __syncthreads();  // (part is rewritten for the next row block)
    // dx_j += sum over this block's rows i >= j of L_ij u_i, the wave's 16 columns
    double v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int j = j0 + q;
      const double l = d.L[ic + (size_t)min(j, D - 1) * D];
      v[q] = (i < D && j < D && i >= j) ? l * ui : 0.0;
    }
    accx += xpose_sum<16>(v, lane);  // lane l: column j0 + (l >> 2)
  }
  const int j = j0 + (lane >> 2);
  if ((lane & 3) == 0 && j < D) d.dx[j] = accx;
}

// The two launches and what they may be given, for the loop body (direction_solves) and the
// stand-alone entry (clrsdp_cl_solve) alike: ncl clusters of at most 256 rows, nrb = cdiv(max D,
// 64) <= 4 row blocks each, and a slab_qsolve behind them that re-forms r in every workgroup
// (its read count and LDS bound)
inline bool cl_solve_ok(long long ncl, int nrb, int max_D, long long ny) {
  return ncl > 0 && ny > 0 && max_D >= 1 && max_D <= 256 && nrb >= 1 && nrb <= 4 &&
         ((ny + 63) / 64) * (ncl * nrb) * ny <= (1LL << 20) &&
         ((size_t)ny + 256) * sizeof(double) <= 64 * 1024;
}
inline void launch_cl_solve_t(hipStream_t s, const ClSolveDesc* ds, int ncl, int nrb, int ny,
                              double* slabs) {
  cl_solve_t<<<(unsigned)(ncl * nrb), 256, 0, s>>>(ds, nrb, ny, slabs);
}
inline void launch_cl_solve_dx(hipStream_t s, const ClSolveDesc* ds, int ncl, int nrb, int ny,
                               const double* dy) {
  cl_solve_dx<<<(unsigned)(ncl * nrb), 256, 0, s>>>(ds, nrb, ny, dy);
}


}  // namespace clrsdp
