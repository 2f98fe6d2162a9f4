"""clrsdp_reduce / clrsdp_slab_sum / clrsdp_update_state (include/clrsdp.h) without a GPU:
  1. the symbols are exported and bound, and every refusal of the header is CLRSDP_E_ARG before any
     device work (device 1 << 20 exists nowhere, so a call that passes the checks is CLRSDP_E_HIP);
  2. the references of tests/reduce_cases.py hold on their own: the exact class summed through the
     host build of the dd and qd operators (mwfloat.h) in 20 random orders and tree shapes is one
     value, the exact one; a left-to-right and a pairwise host sum of the generic class meet the
     bound; the generic class cancels as documented; the fold emulation agrees with its order;
  3. sensitivity: each way a kernel could be subtly wrong, applied to the reference, is rejected
     by the checks the GPU tests use, at every width."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import reduce_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 1 << 20
WORDS = list(rc.WORDS)


# ---- 1. symbols and argument checks -------------------------------------------------------------
def test_symbols_are_exported_and_bound(pk):
    from clrsdp_amd import _lib as L
    for name in ("clrsdp_reduce", "clrsdp_slab_sum", "clrsdp_update_state"):
        assert name in L.EXPORTS
        assert getattr(L.lib(), name).restype is C.c_int32
    assert callable(pk.reduce) and callable(pk.slab_sum) and callable(pk.update_state)
    assert C.sizeof(L.Fold) == 3 * 8 + 2 * 4
    hdr = open(os.path.join(ROOT, "include", "clrsdp.h")).read()
    assert f"#define CLRSDP_RED_G {L.RED_G}" in hdr and L.RED_G == rc.RED_G
    for k, name in enumerate(("DOT", "DOTSUM", "SUM", "MAX", "MIN", "MAXABS")):
        assert f"#define CLRSDP_OP_{name} {k}" in hdr and getattr(L, "OP_" + name) == k
    for k, name in enumerate(("FLAT_FOLD", "FLAT_TREE", "VEC", "FOLD", "ORDERED")):
        assert f"#define CLRSDP_RED_{name} {k}" in hdr and getattr(L, "RED_" + name) == k


def _reduce(L, kind, op, words=1, n=8, stride=1, null=(), folds=None, nfold=None, part=False, size=64):
    buf = {k: np.zeros(4 * size) for k in ("a", "b", "da", "db", "out", "part")}   # never read
    p = {k: (None if k in null else v.ctypes.data_as(L.P_f64)) for k, v in buf.items()}
    fl = None
    if folds is not None:
        fl = (L.Fold * len(folds))()
        for q, (cnt, st, off, o) in enumerate(folds):
            fl[q].cnt, fl[q].stride, fl[q].off, fl[q].op = cnt, st, off, o
    return L.lib().clrsdp_reduce(NO_DEVICE, words, kind, op, n, stride, p["a"], p["b"], p["da"], p["db"],
                                 (len(folds) if folds is not None else 0) if nfold is None else nfold,
                                 fl, p["out"], p["part"] if part else None)


def test_reduce_refusals(pk):
    from clrsdp_amd import _lib as L
    flat, tree, vec, fold, ordr = L.RED_FLAT_FOLD, L.RED_FLAT_TREE, L.RED_VEC, L.RED_FOLD, L.RED_ORDERED
    issued = {flat: (L.OP_DOT, L.OP_DOTSUM, L.OP_MAXABS), tree: (L.OP_DOT, L.OP_DOTSUM, L.OP_MAXABS),
              vec: (L.OP_DOT, L.OP_MAXABS), ordr: (L.OP_MIN,)}
    for words in WORDS:
        for kind, ops in issued.items():
            for op in range(-1, 7):
                want = L.E_HIP if op in ops else L.E_ARG
                assert _reduce(L, kind, op, words=words) == want, (kind, op, words)
    for words in (0, 3, 8):
        assert _reduce(L, vec, L.OP_DOT, words=words) == L.E_ARG
    for kind in (-1, 5):
        assert _reduce(L, kind, L.OP_DOT) == L.E_ARG
    for n in (0, -1, (1 << 28) + 1):
        assert _reduce(L, vec, L.OP_DOT, n=n) == L.E_ARG
    for kind in (flat, tree, vec):
        assert _reduce(L, kind, L.OP_DOT, stride=2) == L.E_ARG
        assert _reduce(L, kind, L.OP_DOT, null=("b",)) == L.E_ARG
        assert _reduce(L, kind, L.OP_MAXABS, null=("b", "da", "db")) == L.E_HIP
        for k in ("a", "out"):
            assert _reduce(L, kind, L.OP_DOT, null=(k,)) == L.E_ARG
    for kind in (flat, tree):
        for k in ("da", "db"):
            assert _reduce(L, kind, L.OP_DOTSUM, null=(k,)) == L.E_ARG
        assert _reduce(L, kind, L.OP_DOT, part=True) == L.E_HIP
    for kind in (vec, ordr):
        assert _reduce(L, kind, issued[kind][0], part=True) == L.E_ARG
    assert _reduce(L, vec, L.OP_DOT, folds=[(1, 1, 0, L.OP_SUM)]) == L.E_ARG     # folds: FOLD only
    assert _reduce(L, ordr, L.OP_MIN, stride=0) == L.E_ARG
    assert _reduce(L, ordr, L.OP_MIN, stride=3) == L.E_HIP
    assert _reduce(L, ordr, L.OP_MIN, n=1 << 20, stride=1 << 20) == L.E_ARG
    # FOLD: the call's op is ignored, every fold has its own
    good = [(8, 1, 0, L.OP_SUM), (3, 3, 1, L.OP_MAX), (1, 1, 7, L.OP_MIN), (4, 2, 1, L.OP_MAXABS)]
    assert _reduce(L, fold, -5, folds=good) == L.E_HIP
    assert _reduce(L, fold, 0, folds=good * 3) == L.E_HIP
    assert _reduce(L, fold, 0, folds=good * 3 + good[:1]) == L.E_ARG             # 13 folds
    assert _reduce(L, fold, 0, folds=[]) == L.E_ARG
    assert _reduce(L, fold, 0, folds=None, nfold=2) == L.E_ARG
    assert _reduce(L, fold, 0, folds=good, part=True) == L.E_ARG
    for bad in ((9, 1, 0, L.OP_SUM), (0, 1, 0, L.OP_SUM), (3, 4, 0, L.OP_SUM), (3, 3, 2, L.OP_SUM),
                (1, 1, 8, L.OP_SUM), (1, 1, -1, L.OP_SUM), (2, 0, 0, L.OP_SUM), (2, 1, 0, L.OP_DOT),
                (2, 1, 0, L.OP_DOTSUM), (2, 1, 0, 6)):
        assert _reduce(L, fold, 0, folds=good[:2] + [bad]) == L.E_ARG, bad       # not the first one
        for words in (2, 4):
            assert _reduce(L, fold, 0, words=words, folds=[bad]) == L.E_ARG, bad


def _slab(L, words=1, cnt=3, stride=10, n=8, null=(), q=False, ldq=8, out2=False, nout=12, off=2):
    buf = {k: np.zeros(4 * 4096) for k in ("in", "base", "Q", "out", "out2")}
    p = {k: (None if k in null else v.ctypes.data_as(L.P_f64)) for k, v in buf.items()}
    return L.lib().clrsdp_slab_sum(NO_DEVICE, words, cnt, stride, n, p["in"], p["base"], 1.0, -1.0,
                                   p["Q"] if q else None, ldq, p["out"], p["out2"] if out2 else None,
                                   nout, off)


def test_slab_sum_refusals(pk):
    from clrsdp_amd import _lib as L
    for words in WORDS:
        assert _slab(L, words=words) == L.E_HIP
        assert _slab(L, words=words, null=("base",), out2=True) == L.E_HIP
        for k in ("in", "out"):
            assert _slab(L, words=words, null=(k,)) == L.E_ARG
        for cnt in (0, -1, 65537):
            assert _slab(L, words=words, cnt=cnt) == L.E_ARG
        assert _slab(L, words=words, n=0) == L.E_ARG
        assert _slab(L, words=words, stride=7) == L.E_ARG                          # stride < n
        assert _slab(L, words=words, cnt=65536, stride=1 << 13) == L.E_ARG         # cnt stride > 2^28
        assert _slab(L, words=words, nout=9) == L.E_ARG                            # 2 + 8 > 9
        assert _slab(L, words=words, off=-1) == L.E_ARG
        assert _slab(L, words=words, nout=10) == L.E_HIP
    for words in (0, 3, 8):
        assert _slab(L, words=words) == L.E_ARG
    # slab_qsolve: fp64, 1 <= n <= 128, ldq >= n, no second output
    assert _slab(L, q=True) == L.E_HIP
    assert _slab(L, q=True, ldq=11) == L.E_HIP
    assert _slab(L, q=True, n=128, stride=128, ldq=128, nout=130) == L.E_HIP
    assert _slab(L, q=True, n=129, stride=129, ldq=129, nout=131) == L.E_ARG
    assert _slab(L, q=True, ldq=7) == L.E_ARG
    assert _slab(L, q=True, out2=True) == L.E_ARG
    for words in (2, 4):
        assert _slab(L, words=words, q=True) == L.E_ARG


def _update(L, words=1, nel=5, nx=3, ny=2, ninfo=4, nblk=0, null=(), pd=0, alpha=True, eig=False):
    names = ("X", "dX", "Y", "dY", "x", "dx", "c", "y", "dy", "b", "ap", "ad", "eX", "eY", "gm", "part",
             "step")
    buf = {k: np.zeros(4 * 1024) for k in names}
    p = {k: (None if k in null else v.ctypes.data_as(L.P_f64)) for k, v in buf.items()}
    info = np.zeros(64, dtype=np.int32)
    return L.lib().clrsdp_update_state(
        NO_DEVICE, words, nel, p["X"], p["dX"], p["Y"], p["dY"], nx, p["x"], p["dx"], p["c"], ny, p["y"],
        p["dy"], p["b"], ninfo, None if "info" in null else info.ctypes.data_as(L.P_i32),
        p["ap"] if alpha else None, p["ad"] if alpha else None, nblk, p["eX"] if eig else None,
        p["eY"] if eig else None, p["gm"] if eig else None, pd, p["part"], p["step"] if eig else None)


def test_update_state_refusals(pk):
    from clrsdp_amd import _lib as L
    fused = dict(nblk=3, alpha=False, eig=True)
    for words in WORDS:
        assert _update(L, words=words) == L.E_HIP
        assert _update(L, words=words, **fused) == L.E_HIP
        assert _update(L, words=words, pd=1, **fused) == L.E_HIP
        assert _update(L, words=words, nx=0, null=("x", "dx", "c")) == L.E_HIP     # a rank without clusters
        for k in ("X", "dX", "Y", "dY", "x", "dx", "c", "y", "dy", "b", "info", "part"):
            assert _update(L, words=words, null=(k,)) == L.E_ARG, k
        for kw in (dict(nel=0), dict(nx=-1), dict(ny=0), dict(ninfo=0), dict(nblk=-1)):
            assert _update(L, words=words, **kw) == L.E_ARG, kw
        # either path with the other's arguments, or without its own
        assert _update(L, words=words, alpha=False) == L.E_ARG
        assert _update(L, words=words, null=("ad",)) == L.E_ARG
        assert _update(L, words=words, eig=True) == L.E_ARG
        assert _update(L, words=words, nblk=3) == L.E_ARG
        assert _update(L, words=words, nblk=3, eig=True) == L.E_ARG                # alpha as well
        for k in ("eX", "eY", "gm", "step"):
            assert _update(L, words=words, null=(k,), **fused) == L.E_ARG, k
        for pd in (-1, 2):
            assert _update(L, words=words, pd=pd, **fused) == L.E_ARG
    for words in (0, 3, 8):
        assert _update(L, words=words) == L.E_ARG


def test_python_wrappers_reject_bad_shapes(pk):
    z = np.zeros
    with pytest.raises(ValueError):
        pk.reduce("sideways", z(4), z(4))
    with pytest.raises(ValueError):
        pk.reduce("vec", z(4), z(5))
    with pytest.raises(ValueError):
        pk.reduce("vec", z((2, 4)), z((2, 4)), precision_words=4)
    with pytest.raises(ValueError):
        pk.reduce("fold", z(4))
    with pytest.raises(ValueError):
        pk.reduce("fold", z(4), folds=[(2, 1, 0, "dot product")])
    with pytest.raises(ValueError):
        pk.slab_sum(z((3, 8)), 8, Q=z((7, 8)))
    with pytest.raises(ValueError):
        pk.update_state(*[z(3)] * 10, info=[0])
    with pytest.raises(ValueError):
        pk.update_state(*[z(3)] * 10, info=[0], alpha=(1.0, 1.0), eig=(z(2), z(2)))


# ---- 2. the references hold on their own --------------------------------------------------------
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
template <class T> T pairwise(const std::vector<T>& t, size_t lo, size_t hi) {
  if (hi - lo == 1) return t[lo];
  const size_t mid = lo + (hi - lo + 1) / 2;
  return pairwise(t, lo, mid) + pairwise(t, mid, hi);
}
// shape 0: left to right; 1: pairwise; 2: 64 strided lanes, then the xor butterfly; 3: chunks of
// `step`, each left to right, the chunk sums pairwise
template <class T> T total(const std::vector<T>& t, int shape, unsigned step) {
  const size_t n = t.size();
  if (shape == 0) {
    T s = t[0];
    for (size_t i = 1; i < n; ++i) s += t[i];
    return s;
  }
  if (shape == 1) return pairwise(t, 0, n);
  if (shape == 2) {
    std::vector<T> acc(64, T(0.0));
    for (size_t l = 0; l < 64 && l < n; ++l) {
      acc[l] = t[l];
      for (size_t i = l + 64; i < n; i += 64) acc[l] += t[i];
    }
    for (int o = 32; o > 0; o >>= 1) {
      std::vector<T> nx(acc);
      for (int l = 0; l < 64; ++l) nx[l] = acc[l] + acc[l ^ o];
      acc = nx;
    }
    return acc[0];
  }
  std::vector<T> part;
  for (size_t lo = 0; lo < n; lo += step) {
    T s = t[lo];
    for (size_t i = lo + 1; i < n && i < lo + step; ++i) s += t[i];
    part.push_back(s);
  }
  return pairwise(part, 0, part.size());
}
template <class T> void run(FILE* f, long n) {
  constexpr int W = Num<T>::W;
  std::vector<double> a(W * n), b(W * n);
  if (fread(a.data(), 8, a.size(), f) != a.size() || fread(b.data(), 8, b.size(), f) != b.size()) exit(2);
  std::vector<T> t(n);
  double l[4];
  for (long i = 0; i < n; ++i) {
    for (int q = 0; q < W; ++q) l[q] = a[q * n + i];
    const T x = make<T>(l);
    for (int q = 0; q < W; ++q) l[q] = b[q * n + i];
    t[i] = x * make<T>(l);
  }
  unsigned s = 12345u;
  for (int k = 0; k < 20; ++k) {
    if (k >= 2)   // (the first two: the given order, left to right and pairwise)
      for (long i = n - 1; i > 0; --i) {
        s = s * 1664525u + 1013904223u;
        std::swap(t[i], t[(s >> 8) % (unsigned)(i + 1)]);
      }
    s = s * 1664525u + 1013904223u;
    pr(total(t, k < 2 ? k : k % 4, 1 + (s >> 8) % 97));
  }
}
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  long hdr[2];
  if (!f || fread(hdr, 8, 2, f) != 2) return 2;
  if (hdr[0] == 1) run<double>(f, hdr[1]);
  else if (hdr[0] == 2) run<dd>(f, hdr[1]);
  else run<qd>(f, hdr[1]);
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("reduce_probe")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    exe = d / "probe"
    inc = os.path.join(ROOT, "clustered-low-rank-sdp-solver_amd", "csrc")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I" + inc, str(src), "-o", str(exe)], check=True)

    def run(a, b):
        words, n = a.shape
        path = d / f"in_{words}_{n}.bin"
        with open(path, "wb") as f:
            f.write(np.array([words, n], dtype=np.int64).tobytes())
            f.write(np.ascontiguousarray(a).tobytes())
            f.write(np.ascontiguousarray(b).tobytes())
        out = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout
        res = np.array([[float.fromhex(t) for t in ln.split()] for ln in out.strip().split("\n")])
        assert res.shape == (20, words)
        return res
    return run


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("n", [1, 2, 65, 1000, 4097])
def test_exact_class_is_one_value_in_any_order(probe, words, n):
    """20 orders and tree shapes through the host build of the operators: bitwise one result, the
    exact integer sum -- the claim the exact class rests on, shown without the kernels"""
    a, b = rc.exact_pair(n, words, seed=3)
    assert np.all(a[0] != 0) and np.all(np.abs(a[0]) < 2 ** 18) and n * np.max(np.abs(a[0])) ** 2 < 2 ** 50
    res = probe(a, b)
    ref = rc.dot_ints(a, b)
    for k in range(20):
        assert rc.value_equal(res[k], ref), (k, res[k])
        assert rc.bitwise(res[k], res[0]), (k, res[k], res[0])


def test_exact_class_at_its_largest_magnitudes(probe):
    """n amax^2 just below 2^50 at the longest vector the GPU tests use, with every sign equal in
    the leading limbs: the largest partial sums the class can produce are still exact"""
    n = 4 * 65536 + 1
    for words in WORDS:
        a, b = rc.exact_pair(n, words, seed=4)
        a[0], b[0] = np.abs(a[0]), np.abs(b[0])
        a[0, :] = b[0, :] = rc.amax(n)
        assert n * rc.amax(n) ** 2 < 2 ** 50 <= n * (rc.amax(n) + 1) ** 2 * 1.0001
        res = probe(a, b)
        ref = rc.dot_ints(a, b)
        for k in range(20):
            assert rc.value_equal(res[k], ref), (words, k)


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("n", [1, 2, 3, 257, 4097])
def test_host_sums_meet_the_bound(probe, words, n):
    """a faithful left-to-right and a pairwise host sum (and 18 shuffled ones) of the generic
    class are within (n + 2) u sum |a b| of the exact sum"""
    a, b = rc.generic_pair(n, words, seed=5)
    res = probe(a, b)
    ref, bnd = rc.dot_ints(a, b), rc.dot_bound(words, a, b)
    worst = max(rc.ratio(res[k], ref, bnd) for k in range(20))
    print(f"host sums words={words} n={n}: error / bound = {worst:.3e}")
    assert worst <= 1.0
    assert rc.judge("generic", res[0], ref, bnd)[0] and rc.judge("generic", res[1], ref, bnd)[0]


@pytest.mark.parametrize("words", WORDS)
def test_generic_class_cancels(words):
    import mpmath
    for n in (2, 257, 4096):
        a, b = rc.generic_pair(n, words, seed=6)
        assert np.all(a != 0.0) and np.all(b != 0.0)
        I, e = rc.dot_ints(a, b)
        with mpmath.workprec(320):
            s = abs(float(mpmath.ldexp(mpmath.mpf(int(I[0])), e)))
        t = float(np.sum(rc.lead(a) * rc.lead(b)))
        assert s <= 2.0 ** -19 * t, (n, s / t)
    for q in range(words - 1):                 # limbs do not overlap
        assert np.all(a[q] + a[q + 1] == a[q])


def test_fold_emulation_follows_the_documented_order():
    """lane l sums l, l + 64, ... then the butterfly: against an independent scalar loop"""
    r = rc.rng(7)
    for cnt in (1, 2, 63, 64, 65, 257, 513):
        v = r.uniform(-1, 1, cnt) * 2.0 ** r.integers(-30, 30, cnt)
        lanes = [0.0] * 64
        for i in range(cnt):
            lanes[i % 64] = v[i] if i < 64 else lanes[i % 64] + v[i]
        o = 32
        while o:
            lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
            o //= 2
        assert rc.fold_sum_f64(v) == lanes[0]
    # and it is order-sensitive: a reversed vector gives another fp64 sum somewhere
    v = r.uniform(-1, 1, 513) * 2.0 ** r.integers(-30, 30, 513)
    assert rc.fold_sum_f64(v) != rc.fold_sum_f64(v[::-1]) or rc.fold_sum_f64(v) != float(np.sum(v))


@pytest.mark.parametrize("words", WORDS)
def test_extreme_class_is_decided_by_the_last_limb(words):
    n = 300
    for op in ("max", "min", "maxabs"):
        for pos in rc.positions(n, words, chunk=rc.flat_chunk(n)):
            v, want = rc.extreme_vector(n, words, 8, pos, op)
            key = [tuple(v[:, i]) for i in range(n)]
            if op == "maxabs":
                key = [tuple(np.abs(v[0, i]) / v[0, i] * v[:, i]) for i in range(n)]
            best = (min if op == "min" else max)(range(n), key=lambda i: key[i])
            assert best == pos and rc.bitwise(np.array(key[best]), want)
            lead = sorted((k[0] for k in key), reverse=op != "min")
            if words > 1:
                assert lead[0] == lead[1], "a runner-up shares the leading limb"
            vn, wn = rc.extreme_vector(n, words, 8, pos, op, nan=True)
            assert np.isnan(vn[0, pos]) and np.isnan(wn[0]) and np.isnan(vn).sum() == 1


# ---- 3. sensitivity -----------------------------------------------------------------------------
N_SENS = 2 * 4 * 1024 + 1024 + 7          # beyond two sweeps of vec_reduce at every width, with a remainder
_sens = {}


def _sens_case(kind, words):
    if (kind, words) not in _sens:
        a, b = (rc.exact_pair if kind == "exact" else rc.generic_pair)(N_SENS, words, seed=9)
        _sens[(kind, words)] = (a, b, rc.dot_ints(a, b), rc.dot_bound(words, a, b))
    return _sens[(kind, words)]


def _mutated(name, a, b, words):
    n = a.shape[1]
    keep = np.ones(n, dtype=bool)
    if name == "drop_one":
        keep[n // 3] = False
    elif name == "chunk_last":
        keep[rc.flat_chunk(n) - 1] = False
    elif name == "remainder":
        keep[n - n % (rc.U[words] * rc.NT[words]):] = False
        assert not keep.all()
    elif name == "double_one":
        idx = np.concatenate([np.arange(n), [n // 3]])
        return rc.dot_ints(a[:, idx], b[:, idx])
    elif name == "trailing_limbs":
        a2 = a.copy()
        a2[1:] = 0.0
        return rc.dot_ints(a2, b)
    return rc.dot_ints(a[:, keep], b[:, keep])


MUTATIONS = [(name, words) for name in ("drop_one", "double_one", "chunk_last", "remainder", "trailing_limbs")
             for words in WORDS if not (name == "trailing_limbs" and words == 1)]   # (fp64 has none)


@pytest.mark.parametrize("name,words", MUTATIONS)
@pytest.mark.parametrize("kind", ["exact", "generic"])
def test_a_wrong_sum_is_rejected(kind, words, name):
    a, b, ref, bnd = _sens_case(kind, words)
    good = rc.to_limbs(ref, words)[:, 0]
    if kind == "exact":
        assert rc.judge(kind, good, ref, bnd)[0]
    else:   # the canonical limbs round the exact sum to the width: far inside the bound
        assert rc.judge(kind, good, ref, bnd)[1] < 1e-3
    bad = rc.to_limbs(_mutated(name, a, b, words), words)[:, 0]
    ok, fig = rc.judge(kind, bad, ref, bnd)
    assert not ok and fig > 1.0, (kind, words, name, fig)


@pytest.mark.parametrize("words", WORDS)
def test_max_in_place_of_max_abs_is_rejected(words):
    n = 300
    for pos in rc.positions(n, words, chunk=rc.flat_chunk(n)):
        v, want = rc.extreme_vector(n, words, 10, pos, "maxabs")
        i = max(range(n), key=lambda j: tuple(v[:, j]))            # max without the absolute value
        assert not rc.bitwise(v[:, i], want)
        # a comparison of the leading limbs alone stops at the first of the equal ones
        j = int(np.argmax(np.abs(v[0])))
        if words > 1 and j != pos:
            assert not rc.bitwise(np.abs(v[0, j]) / v[0, j] * v[:, j], want)
        # and a NaN that is dropped leaves a finite number where NaN is due
        vn, wn = rc.extreme_vector(n, words, 10, pos, "maxabs", nan=True)
        assert rc.is_nan(wn) and not rc.is_nan(np.nanmax(np.abs(vn[0])))


@pytest.mark.parametrize("words", WORDS)
def test_an_ignored_guard_is_rejected(words):
    """with a status word set the state must come back bitwise; the updated one does not"""
    import test_gpu_update_state as tu
    st = tu.exact_state(300, 5, 7, words, seed=11)
    new = tu.updated(st, 0.5, 0.25)
    for k in ("X", "Y", "x", "y"):
        assert not rc.bitwise(new[k], st[k]), k
    assert not rc.same(rc.dot_ints(new["X"], new["Y"]), rc.dot_ints(st["X"], st["Y"]))
