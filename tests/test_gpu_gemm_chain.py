"""GPU tests of chain_f64 on its own (clrsdp_gemm_chain / solver.gemm_chain, include/clrsdp.h):
the plain two-product chain with its dot epilogue, the SYM congruence with one and two pointer
sets, and the TRACE form, at block sizes around the 16-row wave tiles, the 32-column strips and
the 128-row limit, with 1 and 3 problems per launch.

Problem 0 is random, problem 1 graded (rows and columns scaled by 2^-(i mod 40), so the bound has
to be componentwise), problem 2 cancelling in the first product.  Every result is compared with
the exact value (integer arithmetic, tests/gemm_cases.py) in mpmath at 320 bits against the
a-priori bound: the product bound (n + 4) u |A||B| applied twice for the chain, once more for the
column dot of TRACE and for the dot epilogue.  O and rout start as a payload NaN, so an entry the
kernel did not write fails the NaN check.  Each test prints the largest ratio to its bound
(DESIGN.md section 3)."""
from fractions import Fraction

import numpy as np
import pytest

import gemm_cases as gc
from helpers import cw_err
from potrf_cases import dscale

pytestmark = pytest.mark.gpu

CHAIN_N = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 127, 128]
_cache = {}


def _problem(n, p):
    """A1, B1, C1, A2 and the dot operands DA, DdA, DB of problem p of size n"""
    key = ("chain", n, p)
    if key not in _cache:
        kind = ("random", "graded", "cancel")[p % 3]
        A1, B1 = gc.operands(kind, n, n, n, 1, seed=70 + p)
        C1 = gc.matrix(kind, n, n, 1, seed=70 + p)
        A2 = gc.matrix("random", n, n, 1, seed=70 + p, stream=55)
        d = dscale(n)
        if kind == "graded":                      # O_ij ~ 2^-(i mod 40) 2^-(j mod 40)
            A2 = A2 * (d[:, None] / d[None, :])[None]
        D = [gc.matrix(kind, n, n, 1, seed=70 + p, stream=56 + q)[0] for q in range(3)]
        mats = [A1[0], B1[0], C1[0], A2[0]] + D
        for m in mats:
            m.setflags(write=False)
        _cache[key] = tuple(mats) + (gc.product(A1, B1),)
    return _cache[key]


def _chain_ref(n, p, with_c1, neg):
    """(O exact, bound, |O| bound) of problem p for (a1, b1) = (1, -1), or negated (-1, 1)"""
    key = ("ref", n, p, with_c1)
    if key not in _cache:
        A1, B1, C1, A2, _, _, _, P = _problem(n, p)
        _cache[key] = gc.chain_reference(A1, B1, C1 if with_c1 else None, A2, 1.0, -1.0, P)
    (I, e), bnd, absO = _cache[key]
    return ((-I if neg else I), e), bnd, absO


@pytest.mark.parametrize("n", CHAIN_N)
def test_chain(pk, n):
    """O = A2 (a1 A1 B1 + b1 C1) in the Z form (1, -1) and the dY form (-1, 1), with and without
    C1, 3 problems and 1; the dY form again with the dot epilogue: O bitwise the same, and each
    problem's partials, summed exactly, within the dot bound of the exact <DA + DdA, DB + O>"""
    worst = wdot = 0.0
    for nprob in (3, 1):
        pr = [_problem(n, p) for p in range(nprob)]
        col = lambda q: [x[q] for x in pr]
        for with_c1 in (True, False):
            for a1, b1 in ((1.0, -1.0), (-1.0, 1.0)):
                O, part = pk.gemm_chain("chain", col(0), col(1), col(3), col(2) if with_c1 else None,
                                        a1=a1, b1=b1)
                assert part is None
                for p in range(nprob):
                    ref, bnd, _ = _chain_ref(n, p, with_c1, a1 < 0)
                    r = gc.ratio(O[p][None], ref, bnd)
                    assert r <= 1.0, (n, nprob, p, with_c1, a1, b1, r)
                    worst = max(worst, r)
        Od, part = pk.gemm_chain("chain", col(0), col(1), col(3), col(2), a1=-1.0, b1=1.0,
                                 dot=(col(4), col(5), col(6)))
        ns = -(-n // 32)
        assert part.shape == (nprob * ns,) and not np.isnan(part).any()
        O2, _ = pk.gemm_chain("chain", col(0), col(1), col(3), col(2), a1=-1.0, b1=1.0)
        for p in range(nprob):
            assert np.array_equal(Od[p], O2[p]), f"n={n} problem {p}: O changes with the dot epilogue"
            ref, bnd, absO = _chain_ref(n, p, True, True)
            dref, dbnd = gc.dot_reference(pr[p][4], pr[p][5], pr[p][6], ref, bnd, absO)
            # workgroup b = strip b // nprob of problem b % nprob; the strips' partials summed exactly
            Si, es = gc.ints(part[p::nprob][None, None, :])
            got = (np.array([[Si.sum()]], dtype=object), es)
            G = gc.to_mpf(*got)
            r = cw_err(G, gc.to_mpf(*dref), dbnd)
            assert r <= 1.0, (n, nprob, p, "dot", r)
            wdot = max(wdot, r)
    print(f"CHAIN n={n}: error / bound = {worst:.3e}, dot partials {wdot:.3e}")


def _exact_inverse_rounded(X):
    """the inverse of an integer matrix in rational arithmetic (Gauss-Jordan on Fractions), every
    entry rounded once to float64"""
    n = len(X)
    M = [[Fraction(int(X[i, j])) for j in range(n)] + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for k in range(n):
        piv = next(i for i in range(k, n) if M[i][k] != 0)
        M[k], M[piv] = M[piv], M[k]
        inv = 1 / M[k][k]
        M[k] = [v * inv for v in M[k]]
        for i in range(n):
            if i != k and M[i][k] != 0:
                f = M[i][k]
                M[i] = [a - f * b for a, b in zip(M[i], M[k])]
    return np.array([[float(M[i][n + j]) for j in range(n)] for i in range(n)])


@pytest.mark.parametrize("n", [17, 33])
def test_chain_z_from_an_exact_inverse(pk, n):
    """Z = X^-1 (P Y - R) as compute_search_direction forms it: X = G G^T + n I in integers, X^-1
    its exact rational inverse rounded once, P and Y symmetric, R = mu I - X Y rounded"""
    G = np.rint(4.0 * gc._uniform(90, 1, (n, n)))
    X = G @ G.T + n * np.eye(n)
    Xinv = _exact_inverse_rounded(X)
    Y, Pm = gc.sym_matrix(n, 91, graded=False), gc.sym_matrix(n, 92, graded=False)
    R = 0.25 * np.eye(n) - X @ Y
    O, _ = pk.gemm_chain("chain", [Pm], [Y], [Xinv], [R], a1=1.0, b1=-1.0)
    ref, bnd, _ = gc.chain_reference(Pm, Y, R, Xinv, 1.0, -1.0)
    r = gc.ratio(O[0][None], ref, bnd)
    print(f"CHAIN Z = X^-1 (P Y - R) n={n}: error / bound = {r:.3e}")
    assert r <= 1.0


def _sym_problem(n, q):
    key = ("sym", n, q)
    if key not in _cache:
        L, M = gc.known_lower(n, 100 + q), gc.sym_matrix(n, 100 + q)
        assert np.all(np.triu(L, 1) == 0.0) and np.array_equal(M, M.T)
        O, bnd, _ = gc.chain_reference(M, np.ascontiguousarray(L.T), None, L, 1.0, 0.0)
        _cache[key] = (L, M, O, bnd)
    return _cache[key]


@pytest.mark.parametrize("n", CHAIN_N)
def test_chain_sym(pk, n):
    """O = L (M L^T) with exact lower triangular L and symmetric M: one pointer set (3 problems
    and 1) and two sets with different data in each half (2 x 3 and 2 x 1): within the bound of
    the exact L M L^T and bitwise symmetric.  The same congruence through clrsdp_gemm (T = L M,
    then the SYM launch T L^T) meets the same bound; the two are not claimed to agree bitwise."""
    from clrsdp_amd import _lib as L_
    worst = wg = 0.0
    for halves, nprob in ((1, 3), (1, 1), (2, 3), (2, 1)):
        pr = [_sym_problem(n, q) for q in range(halves * nprob)]
        O, _ = pk.gemm_chain("sym", [x[1] for x in pr], [x[0] for x in pr], halves=halves)
        for q, (L, M, ref, bnd) in enumerate(pr):
            assert np.array_equal(O[q], O[q].T), f"n={n} halves={halves} problem {q}: not bitwise symmetric"
            r = gc.ratio(O[q][None], ref, bnd)
            assert r <= 1.0, (n, halves, nprob, q, r)
            worst = max(worst, r)
    pr = [_sym_problem(n, q) for q in range(3)]
    T = pk.gemm([x[0] for x in pr], [x[1] for x in pr], raw_limbs=True)
    S = pk.gemm([t[0] for t in T.C], [x[0] for x in pr], form="sym", transb=True, raw_limbs=True)
    assert S.untouched and T.untouched
    if n > 1:
        assert S.path in (L_.PATH_UNI32, L_.PATH_UNI64), L_.PATH_NAMES.get(S.path)
    for q, (L, M, ref, bnd) in enumerate(pr):
        assert np.array_equal(S.C[q][0], S.C[q][0].T)
        r = gc.ratio(S.C[q], ref, bnd)
        assert r <= 1.0, (n, q, "clrsdp_gemm SYM", r)
        wg = max(wg, r)
    print(f"CHAIN_SYM n={n}: error / bound = {worst:.3e}; through clrsdp_gemm SYM {wg:.3e}")


TRACE_NC = [1, 31, 32, 33, 100, 255]


def _trace_ncs(n):
    i = CHAIN_N.index(n)
    return TRACE_NC if n == 33 else [TRACE_NC[i % 6], TRACE_NC[(i + 3) % 6]]


@pytest.mark.parametrize("n", CHAIN_N)
def test_chain_trace(pk, n):
    """rout[t] = c_agg lam[t] ((Z V)[:, t] . V[:, t]) + c_in din[t], V with NC columns around the
    32-column strips (all six NC at n = 33, two of them at every other n), with and without din,
    3 problems and 1"""
    worst = 0.0
    for nc in _trace_ncs(n):
        data = []
        for p in range(3):
            kind = ("random", "graded", "cancel")[p]
            Z, V = gc.operands(kind, n, nc, n, 1, seed=120 + p)
            lam = 0.5 + np.abs(gc._uniform(120 + p, 3, (nc,)))
            din = gc._uniform(120 + p, 4, (nc,))
            data.append((Z[0], V[0], lam, din))
        for with_din in (True, False):
            refs = [gc.trace_reference(Z, V, lam, din if with_din else None, -1.0, -1.0) for Z, V, lam, din in data]
            for nprob in (3, 1):
                d = data[:nprob]
                rout, _ = pk.gemm_chain("trace", [x[0] for x in d], [x[1] for x in d], lam=[x[2] for x in d],
                                        din=[x[3] for x in d] if with_din else None, c_agg=-1.0, c_in=-1.0)
                for p in range(nprob):
                    r = gc.ratio(rout[p][None, None, :], refs[p][0], refs[p][1])
                    assert r <= 1.0, (n, nc, with_din, nprob, p, r)
                    worst = max(worst, r)
    print(f"CHAIN_TRACE n={n} NC={_trace_ncs(n)}: error / bound = {worst:.3e}")


@pytest.mark.parametrize("sc", [1.0, 2.0 ** 400, 2.0 ** -400], ids=["1", "2^400", "2^-400"])
def test_chain_exact_cases(pk, sc):
    """small integers times powers of two: every partial sum of all three forms is representable
    whatever the order, so the results equal the exact ones bitwise, also with A1 (and C1, din)
    scaled by 2^+-400"""
    n, nc = 33, 40
    ex = lambda i, j, p, st: gc.matrix("exact", i, j, 1, seed=140 + p, stream=st)[0]
    A1, B1, C1, A2 = ([ex(n, n, p, st) for p in range(3)] for st in (50, 51, 52, 53))
    As, Cs = [a * sc for a in A1], [c * sc for c in C1]
    O, _ = pk.gemm_chain("chain", As, B1, A2, Cs, a1=-1.0, b1=1.0)
    for p in range(3):
        assert np.array_equal(O[p], A2[p] @ (Cs[p] - As[p] @ B1[p])), p
    Ls = [np.tril(ex(n, n, p, 54)) for p in range(4)]
    Ms = [(np.tril(ex(n, n, p, 55)) + np.tril(ex(n, n, p, 55), -1).T) * sc for p in range(4)]
    O, _ = pk.gemm_chain("sym", Ms, Ls, halves=2)
    for p in range(4):
        assert np.array_equal(O[p], Ls[p] @ (Ms[p] @ Ls[p].T)), p
    V = [ex(n, nc, p, 56) for p in range(3)]
    lam = [ex(1, nc, p, 57)[0] for p in range(3)]
    din = [ex(1, nc, p, 58)[0] * sc for p in range(3)]
    rout, _ = pk.gemm_chain("trace", As, V, lam=lam, din=din, c_agg=-1.0, c_in=-1.0)
    for p in range(3):
        assert np.array_equal(rout[p], -lam[p] * np.einsum("it,it->t", As[p] @ V[p], V[p]) - din[p]), p
