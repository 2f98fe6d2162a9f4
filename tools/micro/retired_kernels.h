// Kernels that lost their A/B and left the library (DESIGN.md section 12 has each measurement).
// No library path launches them; the microbenchmarks in this directory still do, so that the
// figures in DESIGN.md stay reproducible.  The device helpers they share with the library's
// kernels come from the library headers.
#pragma once
#include "../../clustered-low-rank-sdp-solver_amd/csrc/kernels.h"
#include "../../clustered-low-rank-sdp-solver_amd/csrc/kernels_dense.h"

namespace clrsdp {

// wave butterfly sum (tools/micro/lat_probe.hip)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int s = 32; s > 0; s >>= 1) {
    if constexpr (sizeof(T) == 8) {
      v += __shfl_xor(v, s);
    } else {
      T o;
      double* od = reinterpret_cast<double*>(&o);
      const double* vd = reinterpret_cast<const double*>(&v);
#pragma unroll
      for (int q = 0; q < (int)(sizeof(T) / 8); ++q) od[q] = __shfl_xor(vd[q], s);
      v += o;
    }
  }
  return v;
}

#ifdef CLRSDP_EIGREG_STAMPS
__device__ unsigned long long g_eigreg_stamps[8];
#endif

// ------------------------------------------------------------------------------------------
// GEMM on the VALU for multi-word T: 16x16 tile, 256 threads, one output per thread.
// ------------------------------------------------------------------------------------------
template <class T, bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_valu(const GemmDesc<T>* __restrict__ descs,
                                                 const TileRef* __restrict__ t2d, double alpha,
                                                 double beta) {
  // 16x16 output tile, one output per thread with two accumulation chains (even / odd k): the
  // multi-word FMA is a long dependent sequence, so the tile is small enough for a batch of
  // 64x64 blocks to put two workgroups on every CU (the 32x32 tile with 2x2 outputs per thread
  // left half the CUs idle at one wave per SIMD)
  constexpr int BM = 16, BN = 16, BK = 16;
  __shared__ T As[BK][BM + 1];
  __shared__ T Bs[BK][BN + 1];
  const TileRef tr = t2d[blockIdx.x];
  const GemmDesc<T> d = descs[tr.p];
  const int t = tr.t;
  const int m0 = (t / d.tn) * BM, n0 = (t % d.tn) * BN;
  const int tid = threadIdx.x;
  const int ti = tid & 15, tj = tid >> 4;
  T acc0 = T(0.0), acc1 = T(0.0);
  for (int k0 = 0; k0 < d.K; k0 += BK) {
    {  // A tile 16 x 16: i contiguous in memory unless TA
      const int i = TA ? (tid >> 4) : (tid & 15), k = TA ? (tid & 15) : (tid >> 4);
      const int gi = m0 + i, gk = k0 + k;
      // (an unconditional load from a clamped index and a component-wise select: a multi-word
      // value assigned under a branch stayed in scratch memory)
      const bool in = gi < d.M && gk < d.K;
      const size_t ia = in ? (TA ? gk + (size_t)gi * d.lda : gi + (size_t)gk * d.lda) : 0;
      As[k][i] = sel(in, d.A[ia], T(0.0));
    }
    {  // B tile 16 x 16: j contiguous in memory iff TB
      const int j = TB ? (tid & 15) : (tid >> 4), k = TB ? (tid >> 4) : (tid & 15);
      const int gj = n0 + j, gk = k0 + k;
      const bool in = gj < d.N && gk < d.K;
      const size_t ib = in ? (TB ? gj + (size_t)gk * d.ldb : gk + (size_t)gj * d.ldb) : 0;
      Bs[k][j] = sel(in, d.B[ib], T(0.0));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BK; k += 2) {
      acc0 += As[k][ti] * Bs[k][tj];
      acc1 += As[k + 1][ti] * Bs[k + 1][tj];
    }
    __syncthreads();
  }
  const int row = m0 + ti, col = n0 + tj;
  if (row < d.M && col < d.N) {
    T v = (acc0 + acc1) * T(alpha);
    if (beta != 0.0) v += d.Cin[row + (size_t)col * d.ldcin] * T(beta);
    d.C[row + (size_t)col * d.ldc] = v;
  }
}

// out[e] = sum_{i<cnt} in[i*stride + e]  (fixed order), e < n
// (optionally out[e] = cbase*base[e] + csum*sum, the two vector updates that follow a slab sum)
template <class T>
__global__ void slab_sum(const T* in, int cnt, long long stride, long long n, T* out,
                         const T* base = nullptr, double cbase = 0.0, double csum = 1.0) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  T acc = in[e];
  int i = 1;
  for (; i + 7 < cnt; i += 8) {  // 8 loads in flight, summed in slab order
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = in[(size_t)(i + u) * stride + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; i < cnt; ++i) acc += in[(size_t)i * stride + e];
  if (base) acc = base[e] * T(cbase) + acc * T(csum);
  out[e] = acc;
}

// ------------------------------------------------------------------------------------------
// chol_inv_reg: for each matrix b of the batch, read A_b (n x n, SPD, lower triangle used),
// write Linv_b = L^-1 (lower triangular, exact zeros above the diagonal) and optionally L_b.
// Thread t owns rows [tr*TR, tr*TR+TR) x cols [tc*TC, tc*TC+TC) with tr = t % GR, tc = t / GR.
// Right-looking: step j broadcasts column j of L and row j of L^-1 through LDS (2 barriers); the
// column is scaled by the reciprocal of the pivot, formed once by the pivot's owner.
// In-place safe (out == A): every thread reads its own tile before anything is written.
// ------------------------------------------------------------------------------------------
// INV = false: the Cholesky factor only (out_l, in place allowed; out_inv unused)
template <class T, int TR, int TC, int GR, int GC, bool INV = true>
__global__ __launch_bounds__(GR * GC) void chol_inv_reg(const MatDesc<T>* __restrict__ in,
                                                        const MatDesc<T>* __restrict__ out_inv,
                                                        const MatDesc<T>* __restrict__ out_l,
                                                        int* __restrict__ info) {
  constexpr int NMAX = TR * GR;
  static_assert(TR * GR == TC * GC, "square tile grid");
  __shared__ T col[NMAX];
  __shared__ T row[NMAX];
  __shared__ T sd, rsd;  // pivot and its reciprocal (one division per column, by its owner)
  __shared__ int fail;
  const MatDesc<T> d = in[blockIdx.x];
  const int n = d.n;
  const int t = threadIdx.x, tr = t % GR, tc = t / GR;
  const int r0 = tr * TR, c0 = tc * TC;
  T a[TR][TC], x[TR][TC];
#pragma unroll
  for (int i = 0; i < TR; ++i)
#pragma unroll
    for (int c = 0; c < TC; ++c) {
      const int gi = r0 + i, gc = c0 + c;
      a[i][c] = T(0.0);
      if (gi < n && gc < n && gc <= gi) a[i][c] = d.A[gi + (size_t)gc * d.lda];
      x[i][c] = T(gi == gc ? 1.0 : 0.0);
    }
  if (t == 0) {
    fail = 0;
    const T d0 = d.A[0];
    if (!(d0 > T(0.0))) fail = 1;
    pivot_sqrt(d0, sd, rsd);
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    if (fail) break;
    const T s = sd, rs = rsd;
    // phase B: column j of L -> col[], row j of L^-1 -> row[]  (static register indices only)
    const int jc = j % TC, jr = j % TR;
    if (tc == j / TC) {
#pragma unroll
      for (int c = 0; c < TC; ++c) {
        if (c == jc) {
#pragma unroll
          for (int i = 0; i < TR; ++i) {
            const int gi = r0 + i;
            if (gi >= j && gi < n) {
              const T l = (gi == j) ? s : a[i][c] * rs;
              a[i][c] = l;
              col[gi] = l;
            }
          }
        }
      }
    }
    if (INV && tr == j / TR) {
#pragma unroll
      for (int i = 0; i < TR; ++i) {
        if (i == jr) {
#pragma unroll
          for (int c = 0; c < TC; ++c) {
            x[i][c] = x[i][c] * rs;
            row[c0 + c] = x[i][c];
          }
        }
      }
    }
    __syncthreads();
    // phase C: trailing update of A and of L^-1
    if (r0 + TR - 1 > j) {
      T ci[TR];
#pragma unroll
      for (int i = 0; i < TR; ++i) {
        ci[i] = T(0.0);
        if (r0 + i > j && r0 + i < n) ci[i] = col[r0 + i];
      }
      if (c0 + TC - 1 > j && c0 <= r0 + TR - 1) {
#pragma unroll
        for (int c = 0; c < TC; ++c) {
          const int gc = c0 + c;
          if (gc > j && gc < n) {
            const T cc = col[gc];
#pragma unroll
            for (int i = 0; i < TR; ++i)
              if (gc <= r0 + i) a[i][c] = a[i][c] - ci[i] * cc;
          }
        }
      }
      if (INV && c0 <= j) {
#pragma unroll
        for (int c = 0; c < TC; ++c) {
          const T rc = row[c0 + c];
#pragma unroll
          for (int i = 0; i < TR; ++i) x[i][c] = x[i][c] - ci[i] * rc;
        }
      }
    }
    // next pivot, by the owner of (j+1, j+1)
    const int jn = j + 1;
    if (jn < n && tr == jn / TR && tc == jn / TC) {
      T dn = T(0.0);
#pragma unroll
      for (int i = 0; i < TR; ++i)
#pragma unroll
        for (int c = 0; c < TC; ++c)
          if (i == jn % TR && c == jn % TC) dn = a[i][c];
      if (!(dn > T(0.0))) fail = jn + 1;
      pivot_sqrt(dn, sd, rsd);
    }
    __syncthreads();
  }
  if (t == 0 && info) info[blockIdx.x] = fail;
  if (INV) {
    const MatDesc<T> o = out_inv[blockIdx.x];
#pragma unroll
    for (int i = 0; i < TR; ++i)
#pragma unroll
      for (int c = 0; c < TC; ++c) {
        const int gi = r0 + i, gc = c0 + c;
        if (gi < n && gc < n) o.A[gi + (size_t)gc * o.lda] = x[i][c];
      }
  }
  if (out_l) {
    const MatDesc<T> ol = out_l[blockIdx.x];
#pragma unroll
    for (int i = 0; i < TR; ++i)
#pragma unroll
      for (int c = 0; c < TC; ++c) {
        const int gi = r0 + i, gc = c0 + c;
        if (gi < n && gc < n) ol.A[gi + (size_t)gc * ol.lda] = sel(gc <= gi, a[i][c], T(0.0));
      }
  }
}

// ------------------------------------------------------------------------------------------
// chol_packed: the column steps of chol_inv_reg for multi-word blocks n <= 64, with the elements
// placed by the steps at which they are live instead of on a fixed tile grid.  The lower
// triangle of A is numbered column-major (element (r, c) is updated at the steps j < c) and cut
// into 64-element slots; L^-1 (element (r, c) updated at the steps c <= j < r) is cut into 8 x 8
// tiles on and below the diagonal.  Slot s is register s / NW of wave s % NW, and a wave skips a
// slot (uniform branch) outside its live steps.  The waves then issue about n^3/384 multi-word
// FMAs for A instead of the grid's ~n^2/2 (a grid wave stays busy while any of its 64 rows is
// live) -- at quad-double one FMA is ~225 fp64 instructions.  With LDL = false every element goes
// through the same operations in the same order as in chol_inv_reg, so L and L^-1 are bitwise
// the same.
// LDL = true (quad-double): the square-root-free form A = U D U^T (U unit lower), so that the
// serial chain per column carries one reciprocal 1/d_j (two quad-double products) instead of a
// square root and its reciprocal (five); L = U D^1/2 and L^-1 = D^-1/2 U^-1 follow at the end
// with all n square roots side by side.  The factors then differ from chol_inv_reg's in the
// last bits only.
// ------------------------------------------------------------------------------------------
// NMAX = 128 (round 3, late): the multi-word potrf of blocks up to 128 (the double-double S_j
// of config 4), 129 slots of A, nine registers per thread at 1024 threads.
template <class T, int NT, bool INV, bool LDL = false, int NMAX = 64>
__global__ __launch_bounds__(NT) void chol_packed(const MatDesc<T>* __restrict__ in,
                                                  const MatDesc<T>* __restrict__ out_inv,
                                                  const MatDesc<T>* __restrict__ out_l,
                                                  int* __restrict__ info) {
  constexpr int NW = NT / 64;
  constexpr int SA = (NMAX * (NMAX + 1) / 2 + 63) / 64;  // 33 slots of A at n = 64
  constexpr int SX = (NMAX / 8) * (NMAX / 8 + 1) / 2;     // 36 tiles of L^-1
  constexpr int KA = (SA + NW - 1) / NW, KX = INV ? (SX + NW - 1) / NW : 1;
  __shared__ T col[NMAX];   // column j of L (LDL: of U)
  __shared__ T row[NMAX];   // row j of L^-1 (LDL: of U^-1)
  __shared__ T colu[LDL ? NMAX : 1];  // LDL: column j of the trailing matrix, unscaled
  __shared__ T dgl[LDL ? NMAX : 1];   // LDL: the pivots d_j
  __shared__ T sd, rsd;
  __shared__ int fail;
  const MatDesc<T> d = in[blockIdx.x];
  const int n = d.n, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  auto wave_max = [](int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
  };
  // A: slot w + NW k, element e = 64 slot + lane of the column-major lower triangle
  T a[KA];
  int ar[KA], ac[KA], alo[KA], ahi[KA];  // (ar, ac) = -1: no element; [alo, ahi] slot columns
  const int ne = n * (n + 1) / 2;
#pragma unroll
  for (int k = 0; k < KA; ++k) {
    const int e = 64 * (w + NW * k) + lane;
    int r = -1, c = -1;
    if (e < ne) {
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
    ahi[k] = wave_max(c);
    alo[k] = -wave_max(c >= 0 ? -c : -NMAX);
  }
  // L^-1: tile w + NW k of the column-major 8 x 8 tiles (R >= C); lane (r, c) = (8R + l%8, 8C + l/8)
  T x[KX];
  int xr[KX], xc[KX], xR[KX], xC[KX];  // xR = -1: no tile
  if constexpr (INV) {
    const int nt8 = (n + 7) / 8;
#pragma unroll
    for (int k = 0; k < KX; ++k) {
      int t = w + NW * k, C = 0;
      while (C < nt8 && t >= nt8 - C) {
        t -= nt8 - C;
        ++C;
      }
      const bool tv = C < nt8;
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
  // the pivot of column jp from its (updated) diagonal entry dn: sd = sqrt, rsd = 1/sqrt (LDL:
  // dgl[jp] = dn, rsd = 1/dn)
  auto pivot = [&](int jp, const T& dn) {
    if (!(dn > T(0.0))) fail = jp + 1;
    if constexpr (LDL) {
      dgl[jp] = dn;
      rsd = recip_fast(dn);
    } else {
      pivot_sqrt(dn, sd, rsd);
    }
  };
  if (tid == 0) {
    fail = 0;
    pivot(0, d.A[0]);
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    if (fail) break;
    const T s = sd, rs = rsd;
    // column j of L -> col[] (LDL: of U, and the unscaled column -> colu[]), row j of L^-1 -> row[]
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (alo[k] <= j && j <= ahi[k] && ac[k] == j) {
        if constexpr (LDL) {
          if (ar[k] > j) {  // (the diagonal keeps d_j; dgl holds it)
            const T u = a[k];
            a[k] = u * rs;
            col[ar[k]] = a[k];
            colu[ar[k]] = u;
          }
        } else {
          const T l = (ar[k] == j) ? s : a[k] * rs;
          a[k] = l;
          col[ar[k]] = l;
        }
      }
    if constexpr (INV) {
#pragma unroll
      for (int k = 0; k < KX; ++k)
        if (xR[k] == (j >> 3) && xr[k] == j && xc[k] <= j) {
          if constexpr (!LDL) x[k] = x[k] * rs;  // (U^-1 has a unit diagonal)
          row[xc[k]] = x[k];
        }
    }
    __syncthreads();
    // trailing update of A and of L^-1
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (ahi[k] > j && ac[k] > j) a[k] = a[k] - col[ar[k]] * (LDL ? colu : col)[ac[k]];
    if constexpr (INV) {
#pragma unroll
      for (int k = 0; k < KX; ++k)
        if (xR[k] >= 0 && 8 * xC[k] <= j && j < 8 * xR[k] + 7 && xr[k] > j && xc[k] <= j)
          x[k] = x[k] - col[xr[k]] * row[xc[k]];
    }
    // next pivot, by the owner of (j+1, j+1)
    const int jn = j + 1;
    if (jn < n) {
#pragma unroll
      for (int k = 0; k < KA; ++k)
        if (alo[k] <= jn && jn <= ahi[k] && ar[k] == jn && ac[k] == jn) pivot(jn, a[k]);
    }
    __syncthreads();
  }
  if (tid == 0 && info) info[blockIdx.x] = fail;
  if constexpr (LDL) {
    // L = U D^1/2 (column c times sqrt d_c, the diagonal sqrt d_c), L^-1 = D^-1/2 U^-1 (row r
    // times 1/sqrt d_r): the n square roots side by side, into col (sqrt) and row (1/sqrt)
    if (!fail) {
      for (int c = tid; c < n; c += NT) pivot_sqrt(dgl[c], col[c], row[c]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (ac[k] >= 0) a[k] = (ar[k] == ac[k]) ? col[ac[k]] : a[k] * col[ac[k]];
    if constexpr (INV) {
#pragma unroll
      for (int k = 0; k < KX; ++k)
        if (xr[k] >= 0) x[k] = x[k] * row[xr[k]];
    }
  }
  if constexpr (INV) {
    const MatDesc<T> o = out_inv[blockIdx.x];
#pragma unroll
    for (int k = 0; k < KX; ++k)
      if (xr[k] >= 0) o.A[xr[k] + (size_t)xc[k] * o.lda] = x[k];
    for (int e = tid; e < n * n; e += NT) {  // zeros above the diagonal tiles
      const int r = e % n, c = e / n;
      if ((c >> 3) > (r >> 3)) o.A[r + (size_t)c * o.lda] = T(0.0);
    }
  }
  if (out_l) {
    const MatDesc<T> ol = out_l[blockIdx.x];
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (ac[k] >= 0) ol.A[ar[k] + (size_t)ac[k] * ol.lda] = a[k];
    for (int e = tid; e < n * n; e += NT) {
      const int r = e % n, c = e / n;
      if (c > r) ol.A[r + (size_t)c * ol.lda] = T(0.0);
    }
  }
}

// NWV waves (8: one row block per wave, two waves per SIMD; 4: two row blocks per lane, one wave
// per SIMD, so the redundant per-column reflector chain costs each SIMD half the issue slots).
template <int DBG = 0, int NWV = 8>  // DBG (timing experiments only): 1 = no update FMAs, 2 = no matvec FMAs
__global__ __launch_bounds__(64 * NWV) void eigmin_reg(const MatDesc<double>* __restrict__ descs,
                                                        double* __restrict__ out) {
  constexpr int NS = 16, RPL = 8 / NWV;
#ifdef CLRSDP_EIGREG_STAMPS
  unsigned long long t_prev = __builtin_amdgcn_s_memtime();
  unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define ER_STAMP(slot) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[slot] += t_ - t_prev; t_prev = t_; }
#else
#define ER_STAMP(slot)
#endif
  // rowb[r&1] = row r of the matrix before the step that reflects column r-1 (published by the
  // lanes that own it); pb[k&1] = p = A'v of step k (inactive rows zero); vb[k&1] = v of step k;
  // redw[k&1] = the per-wave parts of v^T p.  Every buffer alternates between two copies, so one
  // barrier per column separates each write from the reads of the copy it replaces.
  __shared__ __attribute__((aligned(16))) double rowb[2][128];
  __shared__ __attribute__((aligned(16))) double pb[2][128];
  __shared__ __attribute__((aligned(16))) double vb[2][128];
  __shared__ __attribute__((aligned(16))) double redw[2][8];
  __shared__ double dg[128], e2[128];
  __shared__ __attribute__((aligned(16))) double sd[128], se[128];
  __shared__ double bnd[2];
  __shared__ unsigned long long masks[8];
  const MatDesc<double> d = descs[blockIdx.x];
  const int n = d.n, lda = d.lda, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  // row blocks of the lanes of wave w, paired so that every SIMD carries blocks that go idle
  // early and late (0/7, 1/6, 2/5, 3/4): NWV = 8, waves w and w+4 share a SIMD; NWV = 4, one
  // wave holds both blocks
  int blk[RPL];
  if constexpr (RPL == 1) {
    blk[0] = w < 4 ? w : 11 - w;
  } else {
    blk[0] = w;
    blk[1] = 7 - w;
  }
  const int c = lane >> 4, t16 = lane & 15;
  // the wave that holds the block of row n-1 (live to the last column) writes v, the diagonal
  // and the off-diagonal of every step; a wave with no row in (k+1, n) skips the reflector and
  // the update of step k (its rows are never read again, or are padding)
  bool writer = false;
#pragma unroll
  for (int h = 0; h < RPL; ++h) writer = writer || blk[h] == ((n - 1) >> 4);
  int i[RPL];
#pragma unroll
  for (int h = 0; h < RPL; ++h) i[h] = blk[h] * 16 + t16;
  // a[h][s][e] = A(i_h, 2c + 8s + e).  The input is exactly symmetric (the step-length product
  // is written by the symmetric GEMM epilogue), so only coalesced A(i, j) loads are needed.
  double a[RPL][NS][2];
#pragma unroll
  for (int h = 0; h < RPL; ++h)
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int j = 2 * c + 8 * s + e;
        const int ic = min(i[h], n - 1), jc = min(j, n - 1);  // unconditional loads, masked after
        const double v = gload(d.A + ic + (size_t)jc * lda);
        a[h][s][e] = (i[h] < n && j < n) ? v : 0.0;
      }
  // scale the block by 2^-ex0 so that its largest entry lies in [0.5, 1): the column norms of the
  // Householder reduction neither overflow nor underflow for any block norm in fp64 range (exact,
  // undone on the result)
  int ex0 = 0;
  {
    double amax = 0.0;
#pragma unroll
    for (int h = 0; h < RPL; ++h)
#pragma unroll
      for (int s = 0; s < NS; ++s) amax = fmax(amax, fmax(fabs(a[h][s][0]), fabs(a[h][s][1])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
    if (lane == 0) redw[0][w] = amax;
    __syncthreads();
    amax = redw[0][0];
#pragma unroll
    for (int r = 1; r < NWV; ++r) amax = fmax(amax, redw[0][r]);
    ex0 = (amax > 0.0 && amax < INFINITY) ? __builtin_amdgcn_frexp_exp(amax) : 0;
#pragma unroll
    for (int h = 0; h < RPL; ++h)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        a[h][s][0] = __builtin_ldexp(a[h][s][0], -ex0);
        a[h][s][1] = __builtin_ldexp(a[h][s][1], -ex0);
      }
  }
  // the owners of row r (lane r & 15 of every class, in the wave holding block r >> 4) write all
  // 32 entries
  auto publish_row = [&](int r, double* dst) {
#pragma unroll
    for (int h = 0; h < RPL; ++h)
      if (blk[h] == (r >> 4) && t16 == (r & 15)) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
          *reinterpret_cast<double2*>(dst + 2 * c + 8 * s) = make_double2(a[h][s][0], a[h][s][1]);
      }
  };
  const int j0 = 2 * c + 8 * t16;  // this lane's column pair (its slot of the v/p broadcasts)
  double cx = 0.0, cy = 0.0, beta = 0.0, v0 = 0.0, vi[RPL];
#pragma unroll
  for (int h = 0; h < RPL; ++h) vi[h] = 0.0;
  // the update of one group of 4 slots of row set h: a_ij += g_i v_j - h_i p_j (mhi = -h_i)
  // (the p terms of the 8 entries first, then the v terms: a dependent pair is 8 issues apart)
  auto upd_group = [&](auto G, auto H, double px, double py, double gi, double mhi) {
    constexpr int g = decltype(G)::value, h = decltype(H)::value;
    static_for<4 * g, 4 * g + 4>([&](auto S) {
      constexpr int s = decltype(S)::value;
      fmac_bcast<s, s == 4 * g>(a[h][s][0], px, mhi);
      fmac_bcast<s, false>(a[h][s][1], py, mhi);
    });
    static_for<4 * g, 4 * g + 4>([&](auto S) {
      constexpr int s = decltype(S)::value;
      fmac_bcast<s, false>(a[h][s][0], cx, gi);
      fmac_bcast<s, false>(a[h][s][1], cy, gi);
    });
  };
  // Reflector of column r from x = row r of the current matrix (at j0, j0+1, the lane's rows,
  // r and r+1), every wave redundantly: v_j = 0 (j <= r), v0 (j = r+1), x_j (j > r+1);
  // H = I - beta v v^T.  The sum of squares is a wave reduction whose six steps are interleaved
  // (sched_barrier) with the slot groups of the pending update `upd(g)` (in-order issue: the
  // update's FMAs fill the reduction's latency).
  auto reflector = [&](int r, double xj0, double xj1, const double* xi, double xr, double x0,
                       auto&& upd) {
    double tl = (j0 >= r + 2 ? xj0 * xj0 : 0.0);
    tl = fma(j0 + 1 >= r + 2 ? xj1 : 0.0, xj1, tl);
    tl += dpp_d<0xB1>(tl);
    __builtin_amdgcn_sched_barrier(0);
    upd(std::integral_constant<int, 0>{});
    __builtin_amdgcn_sched_barrier(0);
    tl += dpp_d<0x4E>(tl);
    __builtin_amdgcn_sched_barrier(0);
    upd(std::integral_constant<int, 1>{});
    __builtin_amdgcn_sched_barrier(0);
    tl += dpp_d<0x141>(tl);
    __builtin_amdgcn_sched_barrier(0);
    upd(std::integral_constant<int, 2>{});
    __builtin_amdgcn_sched_barrier(0);
    tl += dpp_d<0x140>(tl);
    __builtin_amdgcn_sched_barrier(0);
    upd(std::integral_constant<int, 3>{});
    __builtin_amdgcn_sched_barrier(0);
    tl = xsum32(xsum16(tl));  // sum_{j >= r+2} x_j^2 over the wave
    beta = 0.0;
    v0 = x0;
    double e2r = x0 * x0;
    if (tl > 0.0) {
      const double ss = fma(x0, x0, tl);
      double nrm;
      if (ss > 0x1p-900) {  // Newton-refined hardware rsq / rcp (~1 ulp), no IEEE sqrt/div chain
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
      beta = 2.0 * rc;
      e2r = alpha * alpha;
    }
    if (writer && lane == 0) {
      dg[r] = xr;
      e2[r] = e2r;
    }
    cx = j0 <= r ? 0.0 : (j0 == r + 1 ? v0 : xj0);
    cy = j0 + 1 <= r ? 0.0 : (j0 + 1 == r + 1 ? v0 : xj1);
#pragma unroll
    for (int h = 0; h < RPL; ++h) vi[h] = i[h] > r ? (i[h] == r + 1 ? v0 : xi[h]) : 0.0;
    if (writer) *reinterpret_cast<double2*>(&vb[r & 1][j0]) = make_double2(cx, cy);
  };
  publish_row(0, rowb[0]);
  if (n >= 2) publish_row(1, rowb[1]);
  __syncthreads();
  if (n >= 2) {
    const double2 xr = *reinterpret_cast<const double2*>(&rowb[0][j0]);
    double xi0[RPL];
#pragma unroll
    for (int h = 0; h < RPL; ++h) xi0[h] = rowb[0][i[h]];
    reflector(0, xr.x, xr.y, xi0, rowb[0][0], rowb[0][1], [](auto) {});
  } else if (tid == 0) {
    dg[0] = rowb[0][0];
  }
  ER_STAMP(0)
  for (int k = 0; k + 2 < n; ++k) {
    const int lo = (k + 1) >> 3;  // slots s < lo hold columns <= k only
    bool live[RPL];               // wave-uniform: some row of row set h is active
#pragma unroll
    for (int h = 0; h < RPL; ++h) live[h] = blk[h] * 16 + 15 > k && blk[h] * 16 < n;
    // ---- p = A' v (registers) and this wave's part of v^T p; two FMA chains per row set
    double pp[RPL];
    double t = 0.0;
    static_for<0, RPL>([&](auto H) {
      constexpr int h = decltype(H)::value;
      double pa[4] = {0.0, 0.0, 0.0, 0.0};
      // slots in groups of 4 behind one uniform branch each (a per-slot condition gets
      // if-converted into computing everything plus selects)
      if (live[h] && !(DBG & 2)) {
        static_for<0, NS / 4>([&](auto G) {
          constexpr int g = decltype(G)::value;
          if (4 * g + 3 >= lo) {
            static_for<4 * g, 4 * g + 4>([&](auto S) {
              constexpr int s = decltype(S)::value;
              // cx/cy were written by VALU selects: wait states before the first DPP read
              fmac_bcast<s, s == 4 * g>(pa[2 * (s & 1)], cx, a[h][s][0]);
              fmac_bcast<s, false>(pa[2 * (s & 1) + 1], cy, a[h][s][1]);
            });
          }
        });
      }
      pp[h] = (pa[0] + pa[1]) + (pa[2] + pa[3]);
    });
    ER_STAMP(1)
#pragma unroll
    for (int h = 0; h < RPL; ++h) {
      pp[h] = xsum32(xsum16(pp[h]));
      if (c == 0) {
        pb[k & 1][i[h]] = i[h] > k ? pp[h] : 0.0;
        t = fma(vi[h], pp[h], t);
      }
    }
    t = row16_sum(t);  // only lanes 0..15 (class 0) carry the rows' v_i p_i
    if (lane == 0) redw[k & 1][w] = t;
    ER_STAMP(2)
    __syncthreads();
    ER_STAMP(3)
    bool need = false;  // wave-uniform: some row of this wave lies beyond k+1
#pragma unroll
    for (int h = 0; h < RPL; ++h) need = need || (blk[h] * 16 + 15 > k + 1 && blk[h] * 16 < n);
    if (!need) continue;  // (the barrier of the next step is at its top, after the matvec)
    // ---- every LDS read of the step at once
    const int r = k + 1;
    const double* old = rowb[r & 1];
    double rw[NWV];
#pragma unroll
    for (int q = 0; q < NWV; q += 2) {
      const double2 v2 = *reinterpret_cast<const double2*>(&redw[k & 1][q]);
      rw[q] = v2.x;
      rw[q + 1] = v2.y;
    }
    const double2 pvr = *reinterpret_cast<const double2*>(&pb[k & 1][j0]);
    const double2 o = *reinterpret_cast<const double2*>(old + j0);
    double oi[RPL];
#pragma unroll
    for (int h = 0; h < RPL; ++h) oi[h] = old[i[h]];
    const double orr = old[r], or1 = old[r + 1];
    const double vr = vb[k & 1][r], vr1 = vb[k & 1][r + 1];
    const double pr = pb[k & 1][r], pr1 = pb[k & 1][r + 1];
    // ---- w = beta p - K v;  A' -= v w^T + w v^T, i.e. a_ij += g_i v_j - h_i p_j with
    // g_i = K v_i - w_i, h_i = beta v_i
    double tot;
    if constexpr (NWV == 8)
      tot = ((rw[0] + rw[1]) + (rw[2] + rw[3])) + ((rw[4] + rw[5]) + (rw[6] + rw[7]));
    else
      tot = (rw[0] + rw[1]) + (rw[2] + rw[3]);
    const double Kc = beta * beta * tot * 0.5;
    double gi[RPL], mhi[RPL];
#pragma unroll
    for (int h = 0; h < RPL; ++h) {
      const double wi = beta * pp[h] - Kc * vi[h];
      gi[h] = Kc * vi[h] - wi;
      mhi[h] = -(beta * vi[h]);
    }
    // row r = k+1 after this update, recomputed by every lane from the published row with the
    // owners' own operations (bitwise their registers): x_j = a_rj + g_r v_j - h_r p_j
    const double wr = beta * pr - Kc * vr;
    const double gr = Kc * vr - wr, mhr = -(beta * vr);
    const double xj0 = fma(cx, gr, fma(pvr.x, mhr, o.x));
    const double xj1 = fma(cy, gr, fma(pvr.y, mhr, o.y));
    double xi[RPL];
#pragma unroll
    for (int h = 0; h < RPL; ++h) xi[h] = fma(vi[h], gr, fma(pp[h], mhr, oi[h]));
    const double xr = fma(vr, gr, fma(pr, mhr, orr));
    const double x0 = fma(vr1, gr, fma(pr1, mhr, or1));
    ER_STAMP(4)
    // the pending update (old v in cx/cy) runs inside the reflector's reduction
    const double pxu = pvr.x, pyu = pvr.y;
    reflector(r, xj0, xj1, xi, xr, x0, [&](auto G) {
      constexpr int g = decltype(G)::value;
      static_for<0, RPL>([&](auto H) {
        constexpr int h = decltype(H)::value;
        if (blk[h] * 16 + 15 > k + 1 && blk[h] * 16 < n && !(DBG & 1) && 4 * g + 3 >= lo)
          upd_group(G, H, pxu, pyu, gi[h], mhi[h]);
      });
    });
    ER_STAMP(5)
    // the owners of row k+2 publish it (after their update) for the step after next; rowb[k&1]
    // was last read before this step's barrier
    publish_row(k + 2, rowb[k & 1]);
    ER_STAMP(6)
  }
  // the last diagonal entry: row n-1 as its owners published it at the last step (or at the start)
  __syncthreads();
  if (tid == 0 && n >= 2) dg[n - 1] = rowb[(n - 1) & 1][n - 1];
  __syncthreads();
  // Gershgorin interval of the tridiagonal: row r in thread r (waves 0-1), wave min/max, then
  // the two wave results through LDS (the masks words are free until the multisection)
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
    // every thread forms the interval; the tridiagonal is then scaled by 2^-ex so that the
    // interval lies in [-1, 1]: every |d_i - sigma| <= 2 and e_i <= 1, so 8 rows of minors grow
    // by at most 3^8 and sturm_any_below cannot overflow whatever the norm of the block (a
    // power-of-two scaling is exact and leaves every Sturm count unchanged)
    const double* m = reinterpret_cast<const double*>(masks);
    const double l = fmin(m[0], m[2]), h = fmax(m[1], m[3]);
    const double mag = fmax(fabs(l), fabs(h));
    const int ex = (mag > 0.0 && mag < INFINITY) ? __builtin_amdgcn_frexp_exp(mag) : 0;
    bnd_ex = ex;
    // the scaled, padded copy the counts read: rows n..127 get d = 4 (above every sigma, which
    // lies in [-1.002, 1.002]) and no coupling, so they add no negative minor; se[i] = e2_{i-1}
    // (se[0] = 0) floored at 2^-900, so that a zero minor is always followed by a nonzero one
    // (p_{i+1} = -e2_i p_{i-1}) and the recurrence never stalls at zero
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
  // ---- 256-way multisection on waves 0-3 (one per SIMD: a count is a 128-row chain of ~5 VALU
  // instructions per row, so a second wave per SIMD would double the round's issue time for one
  // more bit): 7 rounds of 8 bits bracket lambda_min to 2^-56 of the Gershgorin span, below the
  // Sturm count's own backward error (~n eps ||T||)
  double lo = bnd[0], hi = bnd[1];
  const int nr = (n + 7) & ~7;
  for (int it = 0; it < 7; ++it) {
    const double width = hi - lo;
    if (w < 4) {
      const double sigma = lo + width * ((double)(tid + 1) / 257.0);
      const unsigned long long mk = __ballot(sturm_any_below(sd, se, nr, sigma));
      if (lane == 0) masks[w] = mk;
    }
    __syncthreads();
    int f = -1;
    for (int q = 0; q < 4 && f < 0; ++q)
      if (masks[q]) f = q * 64 + __ffsll((long long)masks[q]) - 1;
    __syncthreads();
    if (f < 0) {
      lo = lo + width * (256.0 / 257.0);
    } else {
      hi = lo + width * ((double)(f + 1) / 257.0);
      if (f > 0) lo = lo + width * ((double)f / 257.0);
    }
  }
  ER_STAMP(7)
#ifdef CLRSDP_EIGREG_STAMPS
  if (tid == 0)
    for (int q = 0; q < 8; ++q) atomicAdd(&g_eigreg_stamps[q], st_acc[q]);
#endif
  if (tid == 0) out[blockIdx.x] = __builtin_ldexp((lo + hi) * 0.5, bnd_ex + ex0);
#undef ER_STAMP
}

// ------------------------------------------------------------------------------------------
// eigmin_onebar (round 6): eigmin_split with ONE barrier per column.  eigmin_split runs per
// column k: the bulk's p = A_k v_k and its reductions -- barrier -- the chain wave's reflector
// v_{k+1} beside the bulk's rank-2 update -- barrier; the matrix-vector product and its
// reductions sit between the two barriers on the critical path.  Here they move under the
// chain's reflector: v_{k+1} = x~ + v0 e_{k+2}, where x~ = row k+1 of A_{k+1} beyond column
// k+2 is known as soon as K_k is (x_j = o_j - beta v_r p_j + g_r v_j, the chain's own formula on
// the same operands, so the bulk's copy has the chain's bits), and only the scalar v0 = x_{k+2}
// - alpha waits for the reflector.  So after the barrier of column k the bulk waves apply the
// rank-2 update of column k and at once form, with the updated registers,
//     q = A_{k+1} x~,   c = A_{k+1} e_{k+2}   (per row, in LDS)
//     S1 = x~^T q,      S2 = x~^T c           (per-wave partials)
// while the chain wave builds v0 and beta_{k+1} from the same row.  After the next barrier
//     p_{k+1} = q + v0 c,   v_{k+1}^T p_{k+1} = S1 + v0 S2 + v0 p_{k+1}[k+2]
// come out of LDS with no further cross-wave exchange.  Chain and bulk form p, K, w_r, g_r and
// x~ by identical expressions from identical LDS operands, so v_{k+1} is one vector everywhere.
// Same layout, scaling, Gershgorin bracket and 512-way multisection as eigmin_split.
// ------------------------------------------------------------------------------------------
template <int DBG = 0>
__global__ __launch_bounds__(576) void eigmin_onebar(const MatDesc<double>* __restrict__ descs,
                                                      double* __restrict__ out) {
  constexpr int NS = 16, NWB = 8, GS = 4;
  __shared__ __attribute__((aligned(16))) double rowb[2][128];
  __shared__ __attribute__((aligned(16))) double qb[2][128];
  __shared__ __attribute__((aligned(16))) double cb[2][128];
  __shared__ __attribute__((aligned(16))) double redw[2][2 * NWB];  // (S1, S2) of each bulk wave
  __shared__ __attribute__((aligned(16))) double scal[2][2];         // v0, beta of the reflector
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
  // chain: v of the current step at the lane's column pair
  double cx = 0.0, cy = 0.0;
  // the reflector of row r from x = row r of the current matrix (chain wave only): v_j = 0
  // (j <= r), v0 (j = r+1), x_j (j > r+1), H = I - beta v v^T; v0 and beta go to scal[r & 1]
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
    if (lane == 0) {
      *reinterpret_cast<double2*>(scal[r & 1]) = make_double2(v0, bt);
      dg[r] = xr;
      e2[r] = e2r;
    }
  };
  // bulk state carried from step to step: x~ at the column pair and at the own row, and the
  // own row's q and c (full sums, in every lane of the row)
  double xt0 = 0.0, xt1 = 0.0, xti = 0.0, qi = 0.0, ci = 0.0;
  // the bulk's product with the freshly updated registers: q = A x~ (x~ at the pair in xt0/xt1,
  // zero at columns < r + 2), c = column r + 1, the partials S1 = x~^T q, S2 = x~^T c; to LDS
  // buffer r & 1 (read by the step that applies reflector r)
  auto product = [&](int r, int lo, bool live) {
    double pa[4] = {0.0, 0.0, 0.0, 0.0};
    double cp = 0.0;
    const int sc = (r + 1) >> 3;
    // (the column's entry picked by weights, not by a select of a[s][0] / a[s][1]: a runtime
    // choice between them became an address select and put a[][] in scratch)
    const double m1 = ((r + 1) & 1) ? 1.0 : 0.0, m0 = 1.0 - m1;
    if (live && !(DBG & 2)) {
      static_for<0, NS / GS>([&](auto G) {
        constexpr int g = decltype(G)::value;
        if (GS * g + GS - 1 >= lo) {
          static_for<GS * g, GS * g + GS>([&](auto S) {
            constexpr int s = decltype(S)::value;
            fmac_bcast<s, s == GS * g>(pa[2 * (s & 1)], xt0, a[s][0]);
            fmac_bcast<s, false>(pa[2 * (s & 1) + 1], xt1, a[s][1]);
            if (s == sc) cp = fma(a[s][1], m1, a[s][0] * m0);
          });
        }
      });
    }
    cp = (c == (((r + 1) >> 1) & 3)) ? cp : 0.0;
    const double qq = xsum32(xsum16((pa[0] + pa[1]) + (pa[2] + pa[3])));
    const double cc = xsum32(xsum16(cp));
    double t1 = 0.0, t2 = 0.0;
    if (c == 0) {
      qb[r & 1][i] = qq;
      cb[r & 1][i] = cc;
      t1 = xti * qq;
      t2 = xti * cc;
    }
    t1 = row16_sum(t1);
    t2 = row16_sum(t2);
    if (lane == 0) *reinterpret_cast<double2*>(&redw[r & 1][2 * w]) = make_double2(t1, t2);
    qi = qq;
    ci = cc;
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
  } else if (n >= 2) {
    // x~_0 = row 0 beyond column 1; q = A_0 x~_0, c = A_0 e_1
    const double2 o2 = *reinterpret_cast<const double2*>(&rowb[0][j0]);
    xt0 = j0 >= 2 ? o2.x : 0.0;
    xt1 = j0 + 1 >= 2 ? o2.y : 0.0;
    xti = i >= 2 ? rowb[0][i] : 0.0;
    product(0, 0, blk * 16 < n);
  }
  __syncthreads();
  for (int k = 0; k + 2 < n; ++k) {
    const int r = k + 1, par = k & 1, rp = r & 1;
    const int lo = (k + 1) >> 3;  // slots s < lo hold columns <= k only
    // ---- scalars of step k, identical in every wave: v0, beta, p_r, v^T p, K, w_r, g_r
    const double2 sv = *reinterpret_cast<const double2*>(scal[par]);
    const double v0 = sv.x, bk = sv.y;
    double rw[2 * NWB];
#pragma unroll
    for (int q = 0; q < 2 * NWB; q += 2) {
      const double2 v2 = *reinterpret_cast<const double2*>(&redw[par][q]);
      rw[q] = v2.x;
      rw[q + 1] = v2.y;
    }
    const double pr = fma(v0, cb[par][r], qb[par][r]);
    const double2 q2 = *reinterpret_cast<const double2*>(&qb[par][j0]);
    const double2 c2 = *reinterpret_cast<const double2*>(&cb[par][j0]);
    const double2 o = *reinterpret_cast<const double2*>(&rowb[rp][j0]);
    const double s1t = ((rw[0] + rw[2]) + (rw[4] + rw[6])) + ((rw[8] + rw[10]) + (rw[12] + rw[14]));
    const double s2t = ((rw[1] + rw[3]) + (rw[5] + rw[7])) + ((rw[9] + rw[11]) + (rw[13] + rw[15]));
    const double tot = fma(v0, pr, fma(v0, s2t, s1t));
    const double Kc = bk * bk * tot * 0.5;
    const double vr = v0;
    const double wr = fma(bk, pr, -(Kc * vr));
    const double gr = fma(Kc, vr, -wr), mhr = -(bk * vr);
    // p_k at the column pair (zero at the dead columns <= k)
    const double px = j0 > k ? fma(v0, c2.x, q2.x) : 0.0;
    const double py = j0 + 1 > k ? fma(v0, c2.y, q2.y) : 0.0;
    if (chain) {
      // ---- row r of A_{k+1} and the reflector v_{k+1} (cx, cy: v_k at the pair)
      const double orr = rowb[rp][r], or1 = rowb[rp][r + 1];
      const double pr1 = fma(v0, cb[par][r + 1], qb[par][r + 1]);
      const int ix = r + 1;  // v_k[r + 1] from the lane holding that column pair
      const double vr1 = readlane_d((ix & 1) ? cy : cx, 16 * ((ix >> 1) & 3) + (ix >> 3));
      const double xj0 = fma(cx, gr, fma(px, mhr, o.x));
      const double xj1 = fma(cy, gr, fma(py, mhr, o.y));
      const double xr = fma(vr, gr, fma(pr, mhr, orr));
      const double x0 = fma(vr1, gr, fma(pr1, mhr, or1));
      if constexpr (DBG & 4) {  // (timing only: no reflector)
        cx = xj0;
        cy = xj1;
        if (lane == 0) {
          *reinterpret_cast<double2*>(scal[r & 1]) = make_double2(x0, 0.0);
          dg[r] = xr;
          e2[r] = 1.0;
        }
      } else {
        reflector(r, xj0, xj1, xr, x0);
      }
    } else {
      const bool live = blk * 16 + 15 >= k + 2 && blk * 16 < n;
      if (live) {
        // v_k at the pair and the own row; p_k at the own row; w_i, g_i, h_i
        const double vx = j0 == r ? v0 : xt0;
        const double vy = j0 + 1 == r ? v0 : xt1;
        const double vi = i == r ? v0 : xti;
        const double pi = fma(v0, ci, qi);
        const double wi = fma(bk, pi, -(Kc * vi));
        const double gi = fma(Kc, vi, -wi), mhi = -(bk * vi);
        // x~_{k+1} = row r of A_{k+1} beyond column r + 1 (the chain's formula)
        const double oi = rowb[rp][i];
        const double nx0 = fma(vx, gr, fma(px, mhr, o.x));
        const double nx1 = fma(vy, gr, fma(py, mhr, o.y));
        const double nxi = fma(vi, gr, fma(pi, mhr, oi));
        // ---- A_{k+1} = A_k - v w^T - w v^T: a_ij += h_i p_j + g_i v_j
        if (!(DBG & 1)) static_for<0, NS / GS>([&](auto G) {
          constexpr int g = decltype(G)::value;
          if (GS * g + GS - 1 >= lo) {
            static_for<GS * g, GS * g + GS>([&](auto S) {
              constexpr int s = decltype(S)::value;
              fmac_bcast<s, s == GS * g>(a[s][0], px, mhi);
              fmac_bcast<s, false>(a[s][1], py, mhi);
            });
            static_for<GS * g, GS * g + GS>([&](auto S) {
              constexpr int s = decltype(S)::value;
              fmac_bcast<s, false>(a[s][0], vx, gi);
              fmac_bcast<s, false>(a[s][1], vy, gi);
            });
          }
        });
        xt0 = j0 >= r + 2 ? nx0 : 0.0;
        xt1 = j0 + 1 >= r + 2 ? nx1 : 0.0;
        xti = i >= r + 2 ? nxi : 0.0;
        // ---- q = A_{k+1} x~, c = A_{k+1} e_{r+1} and the partials for step k + 1
        product(r, lo, true);
        publish_row(k + 2, rowb[par]);
      } else {
        // no row beyond k + 1 here: zero q, c and partials (rows >= n stay exactly zero)
        xt0 = xt1 = xti = 0.0;
        product(r, lo, false);
      }
    }
    __syncthreads();
  }
  if (chain) __builtin_amdgcn_s_setprio(0);
  // the last diagonal entry: row n-1 as its owners published it at the last step (or at the start)
  if (tid == 0 && n >= 2) dg[n - 1] = rowb[(n - 1) & 1][n - 1];
  __syncthreads();
  // Gershgorin interval, scaling and 512-way multisection: as eigmin_split
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
  constexpr double NSIG = 64.0 * NWB + 1.0;
  for (int it = 0; it < 6; ++it) {
    const double width = hi - lo;
    if (w < NWB) {
      const double sigma = lo + width * ((double)(tid + 1) / NSIG);
      const bool below = sturm_any_below(sd, se, nr, sigma);
      const unsigned long long mk = __ballot(below);
      if (lane == 0) masks[w] = mk;
    }
    __syncthreads();
    int f = -1;
    for (int q = 0; q < NWB && f < 0; ++q)
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
}

}  // namespace clrsdp
