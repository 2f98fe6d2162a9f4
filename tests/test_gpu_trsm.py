"""GPU tests of the stand-alone triangular solves (clrsdp_trsm / solver.trsm, include/clrsdp.h):
trsm_batched where its on-chip panel fits (fp64 n <= 1199, double-double 559, quad-double 239) and
the blocked chain across workgroups beyond (per super-block of KB rows: trsm_batched on the
sub-triangle, then trsm_blk_update on the rows not yet solved; forced at every size by
CLRSDP_TRSM_BLK=1, KB set by CLRSDP_TRSM_KB).

Inputs.  Modes 1 and 2: the L and U that solver.getrf returns for a random matrix (pivoted factors
have bounded growth; the factors of a double-double / quad-double factorisation fill all their
limbs).  Mode 0: numpy's Cholesky factor of G G^T + n I, at words > 1 plus limb terms scaled by
2^-53 and 2^-106.  Right-hand sides: random, with the same limb terms.  Matrices and right-hand
sides are handed over as limbs (normalised by error-free sums), so the exact T and b are the limb
sums.

Residual: r = b - T x in mpmath at 320 bits (fp64 with n >= 600: np.longdouble, whose own error
n 2^-64 |T||x| is 2^-14 of the bound) against the a-priori substitution bound with the margin of
the getrf tests: |r_i| <= 8 n eps (|T||x|)_i, eps = 2^-53 / 2^-104 / 2^-206.  Every test prints
the largest ratio to that bound (measured: DESIGN.md section 3).
"""
import mpmath
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = {1: 2.0 ** -53, 2: 2.0 ** -104, 4: 2.0 ** -206}
BOUND = {1: 1199, 2: 559, 4: 239}    # the largest n of the on-chip panel
PREC = 320
_mpf = np.frompyfunc(mpmath.mpf, 1, 1)
_cache = {}


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _limbs(terms, words):
    """(words, ...) normalised limbs of t0 + t1 + t2 (the leading `words` limbs of the exact sum;
    the value under test is the sum of these limbs)"""
    if words == 1:
        return terms[0][None].copy()
    s, e = _two_sum(terms[0], terms[1])
    e, f = _two_sum(e, terms[2])
    s, e = _two_sum(s, e)
    e, f = _two_sum(e, f)
    return np.stack([s, e, f, np.zeros_like(s)][:words])


def _rand(n, m, words, seed, stream):
    from clrsdp_amd import instance as inst
    return [(inst.uniform(seed, stream + t, n * m).reshape(n, m) - 0.5) * 2.0 ** (-53 * t)
            for t in range(1 if words == 1 else 3)]


def _factor(pk, n, words, mode, seed):
    """(words, n, n) limbs of the stored factor: mode 0 potrf's L, modes 1 / 2 getrf's L \\ U"""
    key = ("fac", n, words, min(mode, 1), seed)
    if key not in _cache:
        from clrsdp_amd import instance as inst
        if mode == 0:
            G = inst.uniform(seed, 300, n * n).reshape(n, n)
            t = _rand(n, n, words, seed, 310)
            t[0] = np.linalg.cholesky(G @ G.T + n * np.eye(n))
            _cache[key] = _limbs([np.tril(x) for x in t], words)
        else:
            A = inst.uniform(seed, 500, n * n).reshape(n, n)
            LU, perms, info = pk.getrf([A], precision_words=words, raw_limbs=True)
            assert info.tolist() == [0]
            _cache[key] = LU[0]
    return _cache[key]


def _system(F, mode, trans):
    """limbs of the matrix T that the call solves with, and whether T is lower triangular"""
    n = F.shape[1]
    if mode == 0:
        T = np.tril(F)
    elif mode == 1:
        T = np.tril(F, -1)
        T[0] += np.eye(n)
    else:                                      # U read transposed: forward U^T x = b
        T = np.triu(F).transpose(0, 2, 1)
    return (T.transpose(0, 2, 1), False) if trans else (T, True)


def _exact(limbs):
    A = _mpf(limbs[0])
    for t in limbs[1:]:
        A = A + _mpf(t)
    return A


def residual_ratio(T, lower, X, B, words, cols=None):
    """max over rows and the columns `cols` of |b - T x|_i / (8 n eps (|T||x|)_i)"""
    n = T.shape[1]
    cols = list(range(X.shape[2])) if cols is None else sorted(set(cols))
    bound = 8.0 * n * EPS[words] * (np.abs(T[0]) @ np.abs(X[0][:, cols]))
    assert np.all(bound > 0)
    if words == 1 and n >= 600:
        ld = np.longdouble
        r = np.abs(B[0][:, cols].astype(ld) - T[0].astype(ld) @ X[0][:, cols].astype(ld)).astype(float)
        return float(np.max(r / bound))
    with mpmath.workprec(PREC):
        Tm, Xm, Bm = _exact(T), _exact(X[:, :, cols]), _exact(B[:, :, cols])
        worst = 0.0
        for k in range(len(cols)):
            x = list(Xm[:, k])
            for i in range(n):
                lo, hi = (0, i + 1) if lower else (i, n)
                r = abs(Bm[i, k] - mpmath.fdot(Tm[i, lo:hi], x[lo:hi]))
                worst = max(worst, float(r) / bound[i, k])
    return worst


def _solve(pk, Fs, Bs, mode, trans, words):
    return pk.trsm(Fs, Bs, mode, trans, precision_words=words, raw_limbs=True)


def _batch(pk, sizes, nrhs, words, mode, seed=61):
    Fs = [_factor(pk, n, words, mode, seed + b) for b, n in enumerate(sizes)]
    Bs = [_limbs(_rand(n, r, words, seed + b, 700), words) for b, (n, r) in enumerate(zip(sizes, nrhs))]
    return Fs, Bs


MIXED = [1, 16, 31, 32, 33, 64, 65, 100]


@pytest.mark.parametrize("trans", [False, True], ids=["fwd", "trans"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("nrhs", [1, 8, 65])
@pytest.mark.parametrize("words", [1, 2, 4], ids=["fp64", "dd", "qd"])
def test_chain_against_the_on_chip_kernel(pk, monkeypatch, words, nrhs, mode, trans):
    """CLRSDP_TRSM_BLK=1 with CLRSDP_TRSM_KB=32 (up to four super-blocks, ragged tails, blocks
    that leave the chain early; nrhs = 65 = n for the n = 65 block) against the unset run:
    double-double and quad-double bitwise equal, fp64 equal to 1e-13 and within the bound.
    Multi-word mode 0 batches up to n = 128 take the one-wave vector kernels whatever the
    switch, so that case also runs with a block of 130, which brings trsm_batched in."""
    batches = [MIXED] + ([MIXED + [130]] if mode == 0 and words > 1 else [])
    for sizes in batches:
        Fs, Bs = _batch(pk, sizes, [nrhs] * len(sizes), words, mode)
        monkeypatch.delenv("CLRSDP_TRSM_BLK", raising=False)
        monkeypatch.delenv("CLRSDP_TRSM_KB", raising=False)
        X0 = _solve(pk, Fs, Bs, mode, trans, words)
        monkeypatch.setenv("CLRSDP_TRSM_BLK", "1")
        monkeypatch.setenv("CLRSDP_TRSM_KB", "32")
        X1 = _solve(pk, Fs, Bs, mode, trans, words)
        worst = 0.0
        for b, n in enumerate(sizes):
            assert X1[b].shape == (words, n, nrhs)
            T, lower = _system(Fs[b], mode, trans)
            if words > 1:
                assert np.array_equal(X0[b], X1[b]), (n, int(np.sum(X0[b] != X1[b])))
                cols = [0, nrhs // 2, nrhs - 1]   # (every column is bitwise the on-chip kernel's)
                worst = max(worst, residual_ratio(T, lower, X1[b], Bs[b], words, cols))
            else:
                d = np.max(np.abs(X1[b] - X0[b])) / np.max(np.abs(X0[b]))
                assert d <= 1e-13, (n, d)
                r0 = residual_ratio(T, lower, X0[b], Bs[b], words, [0, nrhs // 2, nrhs - 1])
                r1 = residual_ratio(T, lower, X1[b], Bs[b], words)
                assert r0 <= 1.0, (n, r0)
                worst = max(worst, r1)
        print(f"trsm chain KB=32 words={words} mode={mode} trans={trans} nrhs={nrhs} "
              f"sizes={sizes}: residual / bound = {worst:.3e}")
        assert worst <= 1.0


PAST = {1: [1209, 37], 2: [565, 37], 4: [245, 37]}


@pytest.mark.parametrize("trans", [False, True], ids=["fwd", "trans"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("nrhs", [1, 8])
@pytest.mark.parametrize("words", [1, 2, 4], ids=["fp64-1209", "dd-565", "qd-245"])
def test_past_the_panel(pk, monkeypatch, words, nrhs, mode, trans):
    """The first sizes beyond each bound with a ragged tail, with a small block in the same
    batch, default switches: the residual bound."""
    monkeypatch.delenv("CLRSDP_TRSM_BLK", raising=False)
    monkeypatch.delenv("CLRSDP_TRSM_KB", raising=False)
    sizes = PAST[words]
    assert sizes[0] > BOUND[words]
    Fs, Bs = _batch(pk, sizes, [nrhs] * 2, words, mode, seed=71)
    X = _solve(pk, Fs, Bs, mode, trans, words)
    for b, n in enumerate(sizes):
        T, lower = _system(Fs[b], mode, trans)
        ratio = residual_ratio(T, lower, X[b], Bs[b], words)
        print(f"trsm past the panel words={words} n={n} mode={mode} trans={trans} nrhs={nrhs}: "
              f"residual / bound = {ratio:.3e}")
        assert ratio <= 1.0


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("words", [1, 2, 4], ids=["fp64", "dd", "qd"])
def test_trsm_blk_0_keeps_the_on_chip_bound(pk, monkeypatch, words, mode):
    from clrsdp_amd import _lib as L
    monkeypatch.setenv("CLRSDP_TRSM_BLK", "0")
    n = BOUND[words] + 1
    with pytest.raises(L.ClrsdpError) as ei:
        pk.trsm([np.eye(n)], [np.ones(n)], mode, False, precision_words=words)
    assert ei.value.code == L.E_ARG
    X = pk.trsm([2.0 * np.eye(n - 1)], [np.ones(n - 1)], mode, False, precision_words=words,
                raw_limbs=True)
    assert np.array_equal(X[0][0, :, 0], np.full(n - 1, 1.0 if mode == 1 else 0.5))
