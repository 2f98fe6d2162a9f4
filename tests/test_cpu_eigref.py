"""The eigenvalue references of the lambda_min tests (helpers.known_spectrum and
helpers.neg_pivots) against mpmath.eigsy at n = 18, where the eigen-solve is cheap."""
import mpmath
import numpy as np

from helpers import known_spectrum, neg_pivots

N = 18


def _eigs(A):
    with mpmath.workprec(320):
        return sorted(mpmath.eigsy(mpmath.matrix(A.tolist()), eigvals_only=True))


def _lam(n):
    with mpmath.workprec(320):
        return ([mpmath.mpf(-0.5), mpmath.mpf(-0.5) + mpmath.ldexp(1, -60)]
                + [mpmath.mpf(-0.4) + mpmath.mpf(0.8) * i / n for i in range(2, n)])


def test_known_spectrum_against_eigsy():
    """Exactly symmetric, and every eigenvalue (the clustered pair at 2^-60 included) as given,
    to 1e-90."""
    lam = _lam(N)
    A = known_spectrum(N, lam, np.random.default_rng(1))
    assert all(A[i, j] == A[j, i] for i in range(N) for j in range(i))
    assert max(abs(float(A[i, j])) for i in range(N) for j in range(i)) > 1e-3   # (dense)
    ev = _eigs(A)
    with mpmath.workprec(320):
        assert abs(ev[0] - min(lam)) <= mpmath.mpf(10) ** -90
        assert max(abs(a - b) for a, b in zip(ev, sorted(lam))) <= mpmath.mpf(10) ** -90


def test_known_spectrum_sizes_one_and_two():
    rng = np.random.default_rng(2)
    assert known_spectrum(1, [0.75], rng)[0, 0] == 0.75
    A = known_spectrum(2, [-1.0, 3.0], rng)
    ev = _eigs(A)
    assert abs(ev[0] + 1) <= 1e-90 and abs(ev[1] - 3) <= 1e-90


def test_neg_pivots_brackets_lambda_min():
    """neg_pivots(A - sigma I) is 0 just below lambda_min and 1 just above it (2 above the
    second eigenvalue of the clustered pair), and counts every eigenvalue below a shift."""
    lam = _lam(N)
    A = known_spectrum(N, lam, np.random.default_rng(3))
    ev = _eigs(A)
    with mpmath.workprec(320):
        eye = np.array([[mpmath.mpf(int(i == j)) for j in range(N)] for i in range(N)], dtype=object)
        d = mpmath.ldexp(1, -80)
        assert neg_pivots(A - (ev[0] - d) * eye) == 0
        assert neg_pivots(A - (ev[0] + d) * eye) == 1
        assert neg_pivots(A - (ev[1] + d) * eye) == 2
        for sigma in (-0.45, 0.0, 0.3):
            assert neg_pivots(A - mpmath.mpf(sigma) * eye) == sum(e < sigma for e in ev)


def test_neg_pivots_generalised_pair():
    """The same bracket for a pair (dM, M), M positive definite, against eigsy of
    L^-1 dM L^-T (L the 320-bit Cholesky factor of M)."""
    rng = np.random.default_rng(4)
    G = rng.standard_normal((N, N))
    Mf = G @ G.T / N + 0.5 * np.eye(N)
    Mf = (Mf + Mf.T) / 2
    with mpmath.workprec(320):
        dM = known_spectrum(N, _lam(N), rng)
        M = np.array([[mpmath.mpf(float(x)) for x in row] for row in Mf], dtype=object)
        L = mpmath.cholesky(mpmath.matrix(M.tolist()))
        Li = mpmath.inverse(L)
        T = Li * mpmath.matrix(dM.tolist()) * Li.T
        T = (T + T.T) / 2
        ev = sorted(mpmath.eigsy(T, eigvals_only=True))
        d = (ev[1] - ev[0]) / 4
        assert d > 0
        assert neg_pivots(dM - (ev[0] - d) * M) == 0
        assert neg_pivots(dM - (ev[0] + d) * M) == 1
        assert neg_pivots(dM - (ev[1] + d) * M) == 2
        tiny = mpmath.ldexp(1, -200) * abs(ev[0])
        assert neg_pivots(dM - (ev[0] - tiny) * M) == 0
        assert neg_pivots(dM - (ev[0] + tiny) * M) == 1
