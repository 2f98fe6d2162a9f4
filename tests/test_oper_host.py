"""clrsdp_apply_operator / clrsdp_cl_solve (include/clrsdp.h) and tests/oper_cases.py without a GPU:
  1. the symbols are exported and bound, the header constants match _lib.py, and every refusal is
     CLRSDP_E_ARG before any device work (device 1 << 20 exists nowhere, so a cl_solve call that
     passes the checks is CLRSDP_E_HIP);
  2. the references hold on their own: the integer restatements equal oracle.trace_A /
     compute_weighted_A / compute_residuals (at 256 bits on the uniform kind; through the oracle's
     fp64 arithmetic, which is exact on the exact class, on every kind); the caps of the exact
     class hold; the exact class through the host build of the dd / qd operators (mwfloat.h) in
     several orders is one value; the numpy restatement of each operator meets the generic bound
     at fp64;
  3. sensitivity: each way these kernels could be subtly wrong, applied to the restatement, is
     rejected by the very check the GPU tests use, at every width."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import gemm_cases as gc
import oper_cases as oc
import reduce_cases as rc
from oracle import mpmp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 1 << 20
WORDS = list(oc.WORDS)


# ---- 1. symbols and argument checks -------------------------------------------------------------
def test_symbols_are_exported_and_bound(pk):
    from clrsdp_amd import _lib as L
    for name in ("clrsdp_apply_operator", "clrsdp_cl_solve"):
        assert name in L.EXPORTS
        assert getattr(L.lib(), name).restype is C.c_int32
    assert callable(pk.cl_solve) and callable(pk.DeviceSolver.apply_operator)
    hdr = open(os.path.join(ROOT, "include", "clrsdp.h")).read()
    for k, name in enumerate(("RHS", "WEIGHTED", "SYM", "LIN")):
        assert f"#define CLRSDP_APPLY_{name} {k}" in hdr and getattr(L, "APPLY_" + name) == k
    for k, name in enumerate(("COPY", "SUB", "DIAG")):
        assert f"#define CLRSDP_LIN_{name} {k}" in hdr and getattr(L, "LIN_" + name) == k
    # clrsdp_operands: four pointers, a double, two 32-bit integers, two pointers
    assert C.sizeof(L.Operands) == 4 * 8 + 8 + 2 * 4 + 2 * 8
    assert [f[0] for f in L.Operands._fields_] == ["blocks", "blocks2", "tuples", "scalar", "mult", "mode",
                                                   "only_m", "blocks_out", "tuples_out"]


def _cl(L, D=(3, 5), ny=4, ncl=None, null=()):
    Dv = np.ascontiguousarray(D, dtype=np.int64)
    buf = {k: np.zeros(1 << 17) for k in ("Linv", "W", "rhs", "dy", "t", "slabs", "dx")}     # never read
    p = {k: (None if k in null else v.ctypes.data_as(L.P_f64)) for k, v in buf.items()}
    return L.lib().clrsdp_cl_solve(NO_DEVICE, len(Dv) if ncl is None else ncl,
                                   None if "D" in null else Dv.ctypes.data_as(L.P_i64), ny, p["Linv"],
                                   p["W"], p["rhs"], p["dy"], p["t"], p["slabs"], p["dx"])


def test_cl_solve_refusals(pk):
    from clrsdp_amd import _lib as L
    assert _cl(L) == L.E_HIP
    assert _cl(L, D=(1,), ny=1) == L.E_HIP
    assert _cl(L, D=(256, 1), ny=160) == L.E_HIP
    for k in ("D", "Linv", "W", "rhs", "dy", "t", "slabs", "dx"):
        assert _cl(L, null=(k,)) == L.E_ARG, k
    for D in ((0,), (3, 257), (-1, 4)):
        assert _cl(L, D=D) == L.E_ARG, D
    for ny in (0, -2):
        assert _cl(L, ny=ny) == L.E_ARG
    for ncl in (0, -1, 4097):
        assert _cl(L, D=(2,) * 4097, ncl=ncl) == L.E_ARG
    assert _cl(L, D=(2,) * 4096, ny=2) == L.E_HIP
    # the bounds of the slab_qsolve behind it: ceil(ny / 64) ncl nrb ny <= 2^20, ny + 256 doubles of LDS
    assert _cl(L, D=(2,) * 4096, ny=256) == L.E_ARG          # 4 * 4096 * 256 = 2^22
    assert _cl(L, D=(200,), ny=7936) == L.E_ARG              # 124 * 4 * 7936 > 2^20
    assert _cl(L, D=(2,), ny=7936) == L.E_HIP                # 124 * 7936 < 2^20, 64 KiB exactly
    assert _cl(L, D=(2,), ny=7937) == L.E_ARG                # (7937 + 256) * 8 > 64 KiB


def test_apply_operator_null_arguments(pk):
    from clrsdp_amd import _lib as L
    a = L.Operands()
    route = C.c_int32(0)
    assert L.lib().clrsdp_apply_operator(None, L.APPLY_RHS, C.byref(a), C.byref(route)) == L.E_ARG
    assert L.lib().clrsdp_apply_operator(None, 99, None, None) == L.E_ARG


# ---- 2. the references hold on their own --------------------------------------------------------
def _operands(inst):
    return inst.blocks(1), inst.tuples(2), inst.tuples(3, pairs=True), inst.blocks(4, cancel=False)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_instances_reach_the_edges(kind):
    lay = oc.layout(kind)
    deltas = {lay.blocks[q][2] for q in lay.order}
    Ks = {lay.blocks[q][3] % 4 for q in lay.order}
    if kind == "uniform":
        assert len(set(lay.sizes())) == 1 and 64 < lay.sizes()[0] <= 128 and len(lay.order) == 2
        return
    assert {1, 63, 64, 65, 129} <= deltas and Ks == {0, 1, 2, 3}
    assert any(lay.blocks[q][2] * lay.blocks[q][3] > 64 * 256 for q in lay.order)       # scale_cols strides
    if kind == "trivial":
        assert all(c["m"] == 1 and len(c["deltas"]) == 1 and set(c["ranks"][0]) == {1} for c in lay.spec)
        return
    assert {1, 31, 32, 33, 64, 65, 127, 128, 129} <= set(lay.sizes())
    ms = lay.m_of()
    first, last = min(i for i, m in enumerate(ms) if m > 1), max(i for i, m in enumerate(ms) if m > 1)
    assert 0 < first and last < len(ms) - 1 and all(m > 1 for m in ms[first:last + 1])
    assert {c["m"] for c in lay.spec} == {1, 2, 3} and {len(c["deltas"]) for c in lay.spec} == {1, 2, 3}
    assert len({c["N"] for c in lay.spec}) >= 4 and lay.n_x > 256 and 256 not in lay.x_off
    assert any(x < 256 < y for x, y in zip(lay.x_off, lay.x_off[1:] + [lay.n_x]))
    rk = [r for c in lay.spec for r in c["ranks"]]
    assert any(set(r) >= {0, 1, 2, 3} or (r[0] == 0 and r[-1] == 0 and max(r) == 3) for r in rk)
    assert any(r[0] == 0 and r[-1] == 0 for r in rk)
    big = max(lay.order, key=lambda q: lay.blocks[q][2] * lay.blocks[q][3])
    assert max(lay.spec[big[0]]["ranks"][big[1]]) > 1                                    # column != sample


@pytest.mark.parametrize("kind", oc.KINDS)
@pytest.mark.parametrize("words", WORDS)
def test_exact_class_caps(kind, words):
    inst = oc.instance(kind, "exact", words)
    assert oc.caps_ok(inst, *_operands(inst))
    assert any(np.any(inst.lam[q][0] < 0) for q in inst.lay.order)
    assert any(np.any(inst.lam[q][0] > 0) for q in inst.lay.order)


def _oracle_blocks(lay, vals, bi):
    return [[lay.block(vals, j, l) for l in range(bi.L[j])] for j in range(bi.J)]


@pytest.mark.parametrize("kind", oc.KINDS)
def test_restatements_equal_the_oracle_on_the_exact_class(kind):
    """the oracle's fp64 arithmetic is exact on the exact class (caps), so trace_A,
    compute_weighted_A and compute_residuals must give the integers of the restatements: values
    and index layout on every instance"""
    inst = oc.instance(kind, "exact", 1)
    lay = inst.lay
    cons = inst.clusters()
    bi = O.get_block_info(cons)
    assert [n for bj in bi.Y_blocksizes for n in bj] == lay.sizes() and sum(bi.dim_S) == lay.n_x
    ar = O.Fp64()
    Z, d, a, base = _operands(inst)
    tr = O.trace_A(ar, cons, _oracle_blocks(lay, Z[0], bi), bi)
    ref, _ = oc.rhs_eval(inst, Z, d)
    assert rc.value_equal((-d[0] - tr)[None], ref)
    WA = O.compute_weighted_A(ar, cons, a[0], bi)
    ref, _ = oc.weighted_eval(inst, a, np.zeros_like(base))
    got = np.concatenate([WA[j][l].reshape(-1, order="F") for (j, l) in lay.order])
    assert rc.value_equal(got[None], ref)
    # the residuals of a non-PD integer state: P = sum x_i A_i - X - C, d = c - B y - Tr(A_* Y)
    y = inst.b * 2.0
    C = _oracle_blocks(lay, base[0], bi)
    P, p, dres = O.compute_residuals(ar, cons, a[0], _oracle_blocks(lay, Z[0], bi), y,
                                     _oracle_blocks(lay, Z[0], bi), inst.b, C, bi, False)
    # (restated: weighted_eval on the base -X - C where the oracle subtracts after Symmetric(.),
    # which is the same thing on blocks with m = 1 only; so compare block by block with m = 1)
    ref, _ = oc.weighted_eval(inst, a, -(Z + base))
    for (j, l) in lay.order:
        if lay.blocks[(j, l)][4] == 1:
            off, n = lay.blocks[(j, l)][:2]
            assert rc.value_equal(P[j][l].reshape(-1, order="F")[None], (ref[0][off:off + n * n], ref[1]))
    cB = O.stack_c(cons) - O.stack_B(cons) @ y
    ref, _ = oc.rhs_eval(inst, Z, -cB[None])                      # -(-(c - B y)) - Tr(A_* Y)
    assert rc.value_equal(dres[None], ref)


@pytest.mark.parametrize("words", [2, 4])
def test_restatements_equal_the_oracle_at_256_bits(words):
    """generic class, full-width V and lambda, non-symmetric Z: the restatements against the
    oracle's own functions in 256-bit arithmetic, to 2^-240 of sum |terms|"""
    import mpmath
    inst = oc.instance("uniform", "generic", words)
    lay = inst.lay
    cons = inst.clusters()
    bi = O.get_block_info(cons)
    ar = O.Mp(256)
    Z, d, a, base = _operands(inst)
    mp = lambda x: gc.limb_sum(x.reshape(words, 1, -1))[0]
    tr = O.trace_A(ar, cons, _oracle_blocks(lay, mp(Z), bi), bi)
    ref, _ = oc.rhs_eval(inst, Z, np.zeros_like(d))
    WA = O.compute_weighted_A(ar, cons, mp(a), bi)
    refw, _ = oc.weighted_eval(inst, a, np.zeros_like(base))
    s1, s2 = oc.abs_sums(inst, Z, d, a, base)
    with mpmath.workprec(320):
        e1 = max(abs(x + y) for x, y in zip(tr, gc.to_mpf(*ref)))
        W = gc.to_mpf(*refw)
        e2 = max(abs(x) for (j, l) in lay.order for x in (WA[j][l] - lay.block(W, j, l)).reshape(-1))
        assert e1 <= s1 * mpmath.mpf(2) ** -240 and e2 <= s2 * mpmath.mpf(2) ** -240, (e1, e2)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_oracle_fp64_meets_the_generic_bound(kind):
    """the oracle in fp64 on the generic class (non-symmetric Z, cancelling columns) is within the
    a-priori bound of the exact restatement on every instance: the layout again, on data where
    (r, s) and (s, r) differ, and the cancellation the class promises"""
    inst = oc.instance(kind, "generic", 1)
    lay = inst.lay
    cons = inst.clusters()
    bi = O.get_block_info(cons)
    Z, d, a, base = _operands(inst)
    tr = O.trace_A(O.Fp64(), cons, _oracle_blocks(lay, Z[0], bi), bi)
    ref, bnd = oc.rhs_eval(inst, Z, d)
    ok, fig = oc.judge("generic", (-d[0] - tr)[None], ref, bnd)
    assert ok, fig
    # bound / u = sum over the terms of (ops + 2) |term| <= (2 * 129 + 13) sum |terms|
    rel = np.abs(tr) / (bnd / oc.EPS[1])
    print(f"{kind}: oracle fp64 error / bound {fig:.3e}; median |Tr| / sum (ops + 2) |terms| = {np.median(rel):.2e}")
    assert np.median(rel) < 1e-5


@pytest.mark.parametrize("kind", oc.KINDS)
def test_numpy_restatement_meets_the_generic_bound(kind):
    inst = oc.instance(kind, "generic", 1)
    Z, d, a, base = _operands(inst)
    ref, bnd = oc.rhs_eval(inst, Z, d)
    (got, _), _ = oc.rhs_eval(inst, Z, d, exact=False)
    ok1, f1 = oc.judge("generic", got[None], ref, bnd)
    for fused in (False, True):
        ref, bnd = oc.weighted_eval(inst, a, base, fused=fused)
        (got, _), _ = oc.weighted_eval(inst, a, base, exact=False)
        ok2, f2 = oc.judge("generic", got[None], ref, bnd)
        assert ok1 and ok2, (f1, f2)
    print(f"{kind}: fp64 restatement error / bound: RHS {f1:.3e}, WEIGHTED {f2:.3e}")


PROBE = r"""
#include "mwfloat.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace mw;
template <class T> T make(const double* l);
template <> double make<double>(const double* l) { return l[0]; }
template <> dd make<dd>(const double* l) { return dd(l[0], l[1]); }
template <> qd make<qd>(const double* l) { return qd(l[0], l[1], l[2], l[3]); }
template <class T> void pr(const T& v) {
  const double* d = reinterpret_cast<const double*>(&v);
  for (int q = 0; q < Num<T>::W; ++q) printf(" %a", d[q]);
  printf("\n");
}
template <class T> std::vector<T> rd(FILE* f, long n) {
  constexpr int W = Num<T>::W;
  std::vector<double> a(W * n);
  if (fread(a.data(), 8, a.size(), f) != a.size()) exit(2);
  std::vector<T> t(n);
  double l[4];
  for (long i = 0; i < n; ++i) {
    for (int q = 0; q < W; ++q) l[q] = a[q * n + i];
    t[i] = make<T>(l);
  }
  return t;
}
// one block with m = 1: rhs_p = -d_p - lam_p v_p^T Z v_p in four orders, then
// out = base + V diag(a lam) V^T in three
template <class T> void run(FILE* f, long n, long K) {
  const std::vector<T> Z = rd<T>(f, n * n), V = rd<T>(f, n * K), lam = rd<T>(f, K), d = rd<T>(f, K),
                       a = rd<T>(f, K), base = rd<T>(f, n * n);
  for (int order = 0; order < 4; ++order)
    for (long p = 0; p < K; ++p) {
      T acc = T(0.0);
      if (order == 0) {          // U = Z V by ascending j, the dot by ascending i
        for (long i = 0; i < n; ++i) {
          T u = T(0.0);
          for (long j = 0; j < n; ++j) u += Z[i + j * n] * V[j + p * n];
          acc += u * V[i + p * n];
        }
      } else if (order == 1) {   // both descending
        for (long i = n - 1; i >= 0; --i) {
          T u = T(0.0);
          for (long j = n - 1; j >= 0; --j) u += Z[i + j * n] * V[j + p * n];
          acc += V[i + p * n] * u;
        }
      } else if (order == 2) {   // 64 strided lanes and the xor butterfly
        std::vector<T> ln(64, T(0.0));
        for (long i = 0; i < n; ++i) {
          T u = T(0.0);
          for (long j = 0; j < n; ++j) u += Z[i + j * n] * V[j + p * n];
          ln[i % 64] += u * V[i + p * n];
        }
        for (int o = 32; o > 0; o >>= 1) {
          std::vector<T> nx(ln);
          for (int l = 0; l < 64; ++l) nx[l] = ln[l] + ln[l ^ o];
          ln = nx;
        }
        acc = ln[0];
      } else {                   // v^T Z first
        for (long j = 0; j < n; ++j) {
          T w = T(0.0);
          for (long i = 0; i < n; ++i) w += V[i + p * n] * Z[i + j * n];
          acc += w * V[j + p * n];
        }
      }
      pr(lam[p] * acc * T(-1.0) + d[p] * T(-1.0));
    }
  for (int order = 0; order < 3; ++order)
    for (long j = 0; j < n; ++j)
      for (long i = 0; i < n; ++i) {
        T acc = order == 0 ? base[i + j * n] : T(0.0);
        if (order == 1) {
          for (long p = K - 1; p >= 0; --p) acc += V[i + p * n] * (a[p] * lam[p]) * V[j + p * n];
        } else {
          for (long p = 0; p < K; ++p) acc += (V[i + p * n] * (a[p] * lam[p] * T(1.0))) * V[j + p * n];
        }
        pr(order == 0 ? acc : acc + base[i + j * n]);
      }
}
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  long hdr[3];
  if (!f || fread(hdr, 8, 3, f) != 3) return 2;
  if (hdr[0] == 1) run<double>(f, hdr[1], hdr[2]);
  else if (hdr[0] == 2) run<dd>(f, hdr[1], hdr[2]);
  else run<qd>(f, hdr[1], hdr[2]);
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("oper_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    exe = d / "probe"
    inc = os.path.join(ROOT, "clustered-low-rank-sdp-solver_amd", "csrc")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + inc, str(src), "-o", str(exe)], check=True)

    def run(words, n, K, arrays):
        path = d / f"in_{words}.bin"
        with open(path, "wb") as f:
            f.write(np.array([words, n, K], dtype=np.int64).tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        out = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout
        return np.array([[float.fromhex(t) for t in ln.split()] for ln in out.strip().split("\n")])
    return run


@pytest.mark.parametrize("words", WORDS)
def test_exact_class_is_one_value_in_any_order(probe, words):
    """the delta = 65 block of the trivial kind through the host build of the operators: four
    orders of the trace and three of the weighted sum are bitwise one result, the exact integers --
    the claim the exact class rests on, shown without the kernels"""
    inst = oc.instance("trivial", "exact", words)
    lay = inst.lay
    q = (3, 0)
    off, n, dl, K, m = lay.blocks[q]
    assert (n, K, m) == (65, 8, 1)
    Z, d, a, base = _operands(inst)
    xo = lay.x_off[3]
    planes = lambda M: np.stack([M[w].reshape(-1, order="F") for w in range(words)])
    res = probe(words, n, K, [Z[:, off:off + n * n], planes(inst.V[q]), inst.lam[q], d[:, xo:xo + K],
                              a[:, xo:xo + K], base[:, off:off + n * n]])
    assert res.shape == (4 * K + 3 * n * n, words)
    ref, _ = oc.rhs_eval(inst, Z, d)
    for o in range(4):
        got = res[o * K:(o + 1) * K].T
        assert rc.value_equal(got, (ref[0][xo:xo + K], ref[1])), o
        assert rc.bitwise(got, res[:K].T)
    ref, _ = oc.weighted_eval(inst, a, base)
    for o in range(3):
        got = res[4 * K + o * n * n:4 * K + (o + 1) * n * n].T
        assert rc.value_equal(got, (ref[0][off:off + n * n], ref[1])), o
        assert rc.bitwise(got, res[4 * K:4 * K + n * n].T)


# ---- 3. sensitivity -----------------------------------------------------------------------------
RHS_MUTANTS = {"drop_last_col": oc.KINDS, "lane64": oc.KINDS, "swap_rs": ("general",),
               "ranksum_off": ("general",)}
WEIGHTED_MUTANTS = {"half": ("general",), "col_as_sample": ("general",)}


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("cls", oc.CLASSES)
@pytest.mark.parametrize("kind", oc.KINDS)
def test_a_wrong_operator_is_rejected(kind, cls, words):
    """the correctly rounded exact result passes the GPU tests' check; a dropped last column
    (K mod 4 != 0), lanes >= 64 never added, (r, s) read as (s, r), a rank-sum range off by one
    beside a rank-0 sample, the 1/2 dropped, the column index for the sample index do not"""
    inst = oc.instance(kind, cls, words)
    Z, d, a, base = _operands(inst)
    ref, bnd = oc.rhs_eval(inst, Z, d)
    ok, fig = oc.judge(cls, oc.ints_to_limbs(ref, words), ref, bnd)
    assert ok and fig <= 0.5
    for mut, kinds in RHS_MUTANTS.items():
        if kind in kinds:
            bad, _ = oc.rhs_eval(inst, Z, d, mut=mut)
            assert not oc.judge(cls, oc.ints_to_limbs(bad, words), ref, bnd)[0], mut
    ref, bnd = oc.weighted_eval(inst, a, base, fused=True)       # (the smaller of the two bounds)
    good = oc.ints_to_limbs(ref, words)
    ok, fig = oc.judge(cls, good, ref, bnd)
    assert ok and fig <= 0.5
    for mut, kinds in WEIGHTED_MUTANTS.items():
        if kind in kinds:
            bad, _ = oc.weighted_eval(inst, a, base, mut=mut)
            diff = bad[0] != ref[0]
            assert diff.any(), mut
            got = good.copy()
            got[:, diff] = oc.ints_to_limbs((bad[0][diff], bad[1]), words)
            assert not oc.judge(cls, got, ref, bnd)[0], mut
    if kind == "general":                                         # a block with m > 1 left unmirrored
        got = good.copy()
        off, n = inst.lay.blocks[(3, 0)][:2]
        got[0, off + 1] = np.nextafter(got[0, off + 1], 0.0)
        assert oc.mirrored_bitwise(inst.lay, good) and not oc.mirrored_bitwise(inst.lay, got)


def _tiles_sym(lay, X, broken):
    """blk_sym_tiles on fp64 blocks; `broken`: a block smaller than the handle's largest keeps its
    last, partial 32-tile row and column as they were"""
    out = X.copy()
    nmax = max(lay.sizes())
    for q in lay.order:
        off, n = lay.blocks[q][:2]
        B = X[off:off + n * n].reshape(n, n, order="F")
        S = (B + B.T) * 0.5
        S[np.diag_indices(n)] = np.diag(B)
        if broken and n < nmax and n % 32:
            lo = 32 * (n // 32)
            S[lo:, :], S[:, lo:] = B[lo:, :], B[:, lo:]
        out[off:off + n * n] = S.reshape(-1, order="F")
    return out


def test_a_wrong_symmetrisation_is_rejected():
    inst = oc.instance("general", "exact", 1)
    lay = inst.lay
    X = inst.blocks(5)
    _, ref, touched = oc.sym_expect(lay, X, 0, False, X)
    assert touched.all()
    good = _tiles_sym(lay, X[0], False)[None]
    assert oc.all_bitwise_symmetric(lay, good) and rc.value_equal(good, ref)
    bad = _tiles_sym(lay, X[0], True)[None]
    assert not oc.all_bitwise_symmetric(lay, bad) and not rc.value_equal(bad, ref)
    # mode 1 / 2 and the subset: a transposed read, a block outside the subset written
    for mode in (1, 2):
        exp, _, touched = oc.sym_expect(lay, X, mode, True, np.full_like(X, oc.NAN))
        assert not touched.all() and np.isnan(exp[0, ~touched]).all()
        wrong, _, _ = oc.sym_expect(lay, X, 3 - mode, True, np.full_like(X, oc.NAN))
        assert not rc.bitwise(exp, wrong)
        all_, _, _ = oc.sym_expect(lay, X, mode, False, np.full_like(X, oc.NAN))
        assert not rc.bitwise(exp, all_)


def test_an_uncopied_tail_is_rejected():
    """copy_guard2 moves 16 bytes at a time: with an odd count of doubles the last one is its
    8-byte tail; the keep-residuals test compares bitwise, which sees it"""
    src = rc.generic_vector(9, 1, 3)[0]
    dst = np.zeros(9)
    dst[:8] = src[:8]
    assert not rc.bitwise(dst, src)
    dst[8] = src[8]
    assert rc.bitwise(dst, src)


@pytest.mark.parametrize("cls", oc.CLASSES)
def test_a_wrong_cluster_solve_is_rejected(cls):
    """row 64 of a block skipped, W columns >= 128 dropped, u formed without t: each is rejected
    by cl_judge on the outputs it reaches; the rounded exact results pass"""
    Ds, ny = [63, 128, 193, 255], 129
    Ls, Ws, rs, dy = oc.cl_operands(Ds, ny, cls)
    good = oc.cl_eval(Ls, Ws, rs, dy)
    f64 = oc.cl_eval(Ls, Ws, rs, dy, exact=False)
    for (refs, bnds), (vals, _) in zip(good, f64):
        for ref, bnd, val in zip(refs, bnds, vals):
            ok, fig = oc.cl_judge(cls, val[0], ref, bnd)
            assert ok, fig
    hit = {"skip_row64": (1,), "w_col128": (1,), "no_t": (2,)}    # slabs, slabs, dx
    for mut, outs in hit.items():
        bad = oc.cl_eval(Ls, Ws, rs, dy, exact=False, mut=mut)
        seen = False
        for (refs, bnds), (vals, _) in zip(good, bad):
            for k in outs:
                seen = seen or not oc.cl_judge(cls, vals[k][0], refs[k], bnds[k])[0]
        assert seen, mut
    # NaN above the diagonal of L^-1 is part of the operands and must not be read
    assert all(np.isnan(L[np.triu_indices(L.shape[0], 1)]).all() for L in Ls if L.shape[0] > 1)
