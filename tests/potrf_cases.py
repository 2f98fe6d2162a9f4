"""Inputs of the Cholesky tests (test_potrf_host.py on the CPU, test_gpu_potrf.py on the GPU):
symmetric positive definite blocks as raw limbs of shape (words, n, n) -- the exact matrix is the
limb sum -- and the Cholesky recurrence in software arithmetic of a chosen width.

kind 0  G G^T + n I with G uniform in [-1, 1), symmetrised; at words > 1 plus symmetric terms at
        2^-53 and 2^-106, the exact sum split into the word's limbs (so every limb is filled)
kind 1  kind 0 scaled exactly, D A D with D = diag(2^-(i mod 40)): entries down to 2^-78
kind 2  a known factor: A_ij = min(i, j) + 1 scaled D A D with the same D, so L = D tril(ones)
        and L^-1 = (I - subdiagonal) D^-1 is bidiagonal, both exactly representable
kind 3  ill conditioned but exactly positive definite: G an n x (n // 2) integer matrix in
        [-8, 8], A = G G^T (exact integers, rank n // 2) + tau I with tau = 2^-10 / 2^-50 /
        2^-120 at words 1 / 2 / 4, placed in the next limb of the diagonal (words 1: added to
        the integer).  lambda_min(A) = tau, against entries of ~2^10: the factorisation needs
        the word's full width (test_potrf_host.py runs the recurrence one width lower: it fails).
"""
import mpmath
import numpy as np

EPS = {1: 2.0 ** -53, 2: 2.0 ** -104, 4: 2.0 ** -206}
BITS = {1: 53, 2: 104, 4: 206}
TAU = {1: 2.0 ** -10, 2: 2.0 ** -50, 4: 2.0 ** -120}
PREC = 320
_mpf = np.frompyfunc(mpmath.mpf, 1, 1)


def dscale(n):
    """the diagonal of D: 2^-(i mod 40)"""
    return 2.0 ** -(np.arange(n) % 40).astype(np.float64)


def _split(A, words):
    """symmetric object matrix of mpf -> (words, n, n) limbs (limb q = the nearest double of what
    the limbs before it leave over, exactly)"""
    n = A.shape[0]
    out = np.zeros((words, n, n))
    for i in range(n):
        for j in range(i + 1):
            r = A[i, j]
            for q in range(words):
                h = float(r)
                out[q, i, j] = out[q, j, i] = h
                r = mpmath.fsub(r, h, exact=True)
    return out


def spd_limbs(inst, n, words, kind, seed=11):
    """(words, n, n) float limbs of the block of the given kind (module docstring)"""
    d = dscale(n)
    if kind in (0, 1):
        G = inst.uniform(seed, 600, n * n).reshape(n, n)
        A0 = G @ G.T
        A0 = 0.5 * (A0 + A0.T) + n * np.eye(n)
        if words == 1:
            limbs = A0[None].copy()
        else:
            with mpmath.workprec(PREC):
                A = _mpf(A0)
                for t in (1, 2):
                    u = inst.uniform(seed, 600 + t, n * n).reshape(n, n)
                    A = A + _mpf(0.5 * (u + u.T) * 2.0 ** (-53 * t))
                limbs = _split(A, words)
        if kind == 1:
            limbs = limbs * (d[:, None] * d[None, :])[None]       # powers of two: exact
        return limbs
    limbs = np.zeros((words, n, n))
    if kind == 2:
        i = np.arange(n)
        limbs[0] = (np.minimum(i[:, None], i[None, :]) + 1.0) * (d[:, None] * d[None, :])
        return limbs
    if kind == 3:
        k = n // 2
        G = np.rint(8.0 * inst.uniform(seed, 700, n * max(k, 1))).astype(np.int64).reshape(n, max(k, 1))[:, :k]
        limbs[0] = (G @ G.T).astype(np.float64)                   # |.| <= 64 k: exact
        if words == 1:
            limbs[0] += TAU[1] * np.eye(n)                        # integers < 2^18 + 2^-10: exact
        else:
            limbs[1] = TAU[words] * np.eye(n)
            for i in np.flatnonzero(np.diag(limbs[0]) == 0.0):    # (a zero row of G: tau leads)
                limbs[0, i, i], limbs[1, i, i] = limbs[1, i, i], 0.0
        return limbs
    raise ValueError(kind)


def known_factor(n, inverse):
    """kind 2: L = D tril(ones), or L^-1 = (I - subdiagonal) D^-1 (floats, exact)"""
    d = dscale(n)
    if not inverse:
        return np.tril(np.ones((n, n))) * d[:, None]
    X = np.diag(1.0 / d)
    for i in range(1, n):
        X[i, i - 1] = -1.0 / d[i - 1]
    return X


def exact(limbs):
    """(words, ...) float limbs -> their exact sums as mpf objects (a float array at one word)"""
    if limbs.shape[0] == 1:
        return limbs[0]
    with mpmath.workprec(PREC):
        A = _mpf(limbs[0])
        for t in limbs[1:]:
            A = A + _mpf(t)
    return A


def cholesky_at(limbs, bits):
    """The right-looking Cholesky recurrence (pivot d_k = a_kk, l_ik = a_ik / sqrt(d_k),
    a_ij -= l_ik l_jk) on the exact limb sum, every operation rounded to ``bits`` bits (mpmath;
    IEEE doubles at 53, which round the same).  Returns (fail, min_pivot): fail = 0 or the
    1-based column of the first pivot that is not positive, min_pivot over the pivots met."""
    n = limbs.shape[1]
    if bits == 53:
        A = exact(limbs)
        A = A.astype(np.float64) if A.dtype == object else A.copy()   # the sum rounded to 53 bits
        pmin = np.inf
        for k in range(n):
            p = A[k, k]
            if not p > 0.0:
                return k + 1, pmin
            pmin = min(pmin, p)
            l = A[k + 1:, k] / np.sqrt(p)
            A[k + 1:, k + 1:] -= np.outer(l, l)                   # one product, one subtraction
        return 0, pmin
    with mpmath.workprec(bits):
        A = exact(limbs)
        A = _mpf(A) if A.dtype != object else +A                  # (unary plus: rounded to bits)
        pmin = mpmath.inf
        for k in range(n):
            p = A[k, k]
            if not p > 0:
                return k + 1, pmin
            pmin = min(pmin, p)
            l = A[k + 1:, k] / mpmath.sqrt(p)
            for j in range(k + 1, n):                             # the lower triangle only
                A[j:, j] = A[j:, j] - l[j - k - 1:] * l[j - k - 1]
        return 0, pmin
